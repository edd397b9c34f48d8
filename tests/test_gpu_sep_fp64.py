"""GPU test of the fused SepConv halves (csrc/sepf.hip forward, csrc/sepb.hip backward) against the fp64 reference of their definition
(tests/_sep_ref.py), through the C ABI: 24 cases, K in {3, 5} x (C in 36 .. 80 on 2 x 13 x 37 at one row per wave, C in 36 .. 48 on 4 x 19 x 507 at two),
which reach the twelve instantiated variants of csrc/sep.h in both directions (tests/test_sep_ref.py shows that without a GPU).  Per case:

* forward, training form: the four source forms (a, b present or NULL, relu 0 or 1): y, t and the reduced statistics, with three slab rows beyond
  max(addk_sep_rows, addk_conv_rows) that must come back zero; once with t = NULL;
* forward with the fused finalize, twice in a row on one zeroed counter workspace: (a, b, mean, invstd, running_mean, running_var) against fp64 and bit
  for bit the same both times, the ticket counters back at zero, the slab rows beyond addk_sep_rows untouched (include/addk.h, stats_rows);
* forward, inference form (t = stats = NULL): the epilogues (nterm, ea) = (0, none), (0, set), (1, set), (2, none), (3, set), (4, set), the terms cycling
  through the four source forms, so that term 0 (staged through LDS) and the later terms (read from global memory) each meet a ReLU and a plain form;
* backward: the four source forms x {first touch, accumulate onto g0}: g, the reduced (dA, dB) and the workspace rows summed; g with dab = NULL;
  g = NULL with dab = NULL (the workspace alone is written); the first launch again, bit for bit;
* batches of three members under one key, forward (each member with its own fused finalize and counter workspace) and backward: at one row per wave the
  case, 3 x 5 x 16 and 1 x 1 x 1; at two the case, its shape again with another seed and wider strides, and 4 x 9 x 771 (392 workgroups).  The members'
  grids differ (workgroups beyond a member's own must leave), meta[2] is the largest; each member is held to fp64 with its own guards and is bit for bit
  its lone launch; the replayed batch is bit for bit the first run.

Every launch first asserts with addk_sep_*_config that it takes the variant its case names.  Every buffer is a slice of a wider one: x from channel 8
of rows of C + 12 floats, pw_w from column 8 of rows of C + 12, ldy = lddy = ldg = C + 12, ldt = C + 8, stats_ld = C + 4, term i in rows of C + 4 i + 4.
First-touch outputs start as FIRST_TOUCH_BITS, slabs as SLAB_BITS; ws is exactly rows x C x K^2 floats and dab exactly rows x C x 2 doubles between guard
bands.  After every launch the guard bands are intact, every element outside a slice kept its bits and every slab, ws and dab element inside was written.
Bound: TOL = 2e-5 of the reference's max-abs (tests/_wgrad_ref.py: fp32 products, fp32 accumulation; both kernels use mfma_f32_16x16x4f32 alone);
tests/test_sep_ref.py shows that it separates the right result from eleven subtly wrong ones by a factor of 1500 at least.  The errors measured on the
MI355X are in profiles/sep_fp64_errors.txt; every item appends its own to sep_fp64_errors.txt in the report directory (the environment variable
ADDK_TEST_REPORTS, else test_reports/ under the working directory)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _sep_ref as R

pytestmark = pytest.mark.gpu

TOL = R.TOL
LOG = os.path.join(os.environ.get('ADDK_TEST_REPORTS') or 'test_reports', 'sep_fp64_errors.txt')
FT, SB = R.FIRST_TOUCH_BITS, R.SLAB_BITS
IDS = [R.case_id(c) for c in R.CASES]
# one case per variant for the batches: the upper end of each padded stride
BATCH_CASES = [c for c in R.CASES if c.op.C in (40, 48, 72, 80)]
BATCH_IDS = [R.case_id(c) for c in BATCH_CASES]
SPARE = 3                       # slab rows nobody owns


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    lb = L.load()
    fast = lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(R.FAST_ALL)
    yield L
    lb.addk_set_fast_paths(fast)
    _MEM.clear()


def _env(L):
    lb = L.load()
    lb.addk_set_fast_paths(R.FAST_ALL)
    return lb, torch.device('cuda:0'), torch.cuda.current_stream().cuda_stream


def _log(lines):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'a') as f:
        f.write(''.join(v + '\n' for v in lines))


def _finish(tag, errs):
    """log every figure, then assert"""
    _log(['%s %s %.2e' % (tag, k, v) for k, v in errs.items()] + ['worst %s %.2e' % (tag, max(errs.values(), key=lambda v: (v != v, v)))])
    bad = ['%s %.2e' % kv for kv in errs.items() if not kv[1] <= TOL]
    assert not bad, '%s beyond %.0e of the fp64 reference: %s' % (tag, TOL, ', '.join(bad))


_MEM = {}


def _mem(op, dev):
    """the op's seeded inputs on the device (kept for the three members of a batch at the most) and the addresses of their slices"""
    if op not in _MEM:
        while len(_MEM) >= 3:
            _MEM.pop(next(iter(_MEM)))
        up = lambda v: torch.tensor(v).to(dev)
        d = {k: [up(u) for u in v] if isinstance(v, list) else up(v) for k, v in R.make_inputs(op).items()}
        at = lambda k, off=0: d[k].data_ptr() + 4 * off
        ptr = {'x': at('x', R.XOFF), 'a': at('a'), 'b': at('b'), 'dw_w': at('dw_w'), 'pw_w': at('pw_w', R.WOFF), 'dy': at('dy'), 'ea': at('ea'), 'eb': at('eb'),
               'term': [v.data_ptr() for v in d['term']], 'ta': [v.data_ptr() for v in d['ta']], 'tb': [v.data_ptr() for v in d['tb']]}
        _MEM[op] = (d, ptr)
    return _MEM[op]


def _words(g):
    """the int32 words of a guarded buffer's data, on the host"""
    return g.data.cpu().numpy().view(np.int32)


def _rows_of(g, rows, row):
    return g.data.cpu().numpy().reshape(rows, row)


def _slice_check(what, name, g, P, row, Cn, init_words):
    """a [P][row] output of which the launch owns the first Cn columns: the guard band is intact and the other columns kept their bits; returns the slice"""
    assert g.intact(), '%s: guard band of %s overwritten' % (what, name)
    got = _rows_of(g, P, row)
    assert np.array_equal(got.view(np.int32)[:, Cn:], init_words[:, Cn:]), '%s: a row of %s changed beyond its %d channels' % (what, name, Cn)
    return got[:, :Cn]


class _Fwd:
    """One forward launch on the device: y (and t) as slices of wider first-touch rows between guard bands; in the training form (train) a slab of
    max(addk_sep_rows, addk_conv_rows) + SPARE rows of SLAB_BITS; with the fused finalize (fin) its six outputs and a zeroed counter workspace of exactly
    addk_bn_fin_ws_bytes, each between guard bands; epilogue = j: the inference form EPILOGUES[j].  Asserts that the launch takes the variant `want`."""

    def __init__(self, L, lb, dev, op, want, what, form=0, t=True, train=True, fin=False, epilogue=None):
        self.L, self.lb, self.op, self.what, self.form, self.fin, self.epilogue = L, lb, op, what, form, fin, epilogue
        self.P, Cc = R.pixels(op), op.C
        d, ptr = _mem(op, dev)
        self.d, ptr = d, dict(ptr)
        train = train and epilogue is None
        self.y = R.Guarded(self.P * R.ld(op, 'y'), dev)
        self.t = R.Guarded(self.P * R.ld(op, 't'), dev) if t and epilogue is None else None
        ptr['y'], ptr['t'] = self.y.data.data_ptr(), self.t.data.data_ptr() if self.t is not None else None
        self.gx = int(lb.addk_sep_rows(C.byref(R.fwd_args(L, op, ptr, form))))
        assert self.gx > 0, what
        self.rows, self.slab, self.counter, self.outs = 0, None, None, []
        if train:
            self.rows = max(self.gx, int(lb.addk_conv_rows(self.P, Cc))) + SPARE
            self.slab = R.Guarded(self.rows * R.ld(op, 'stats') * 4, dev)
            ptr['stats'] = self.slab.data.data_ptr()
        if fin:
            nbytes = int(lb.addk_bn_fin_ws_bytes(self.gx, R.ld(op, 'stats')))
            assert nbytes > 0 and nbytes % 4 == 0
            self.counter = R.Guarded(nbytes // 4, dev).fill_bits(0)
            self.outs = [R.Guarded(Cc, dev) for _ in range(6)]                    # R.FIN_NAMES' order
            o = [g.data.data_ptr() for g in self.outs]
            ptr['fin'] = [d['gamma'].data_ptr(), d['beta'].data_ptr(), o[4], o[5], o[0], o[1], o[2], o[3]]
            ptr['counter'] = self.counter.data.data_ptr()
        self.args = R.fwd_args(L, op, ptr, form, t=self.t is not None, stats_rows=self.rows, epilogue=epilogue, fin=fin)
        cfg = R.config(L, lb, self.args)
        assert cfg[0] == 1 and tuple(cfg[1:5]) == want and cfg[5] == self.gx, '%s takes %s, its case names %s' % (what, cfg, want)
        self.key = cfg[7]
        self.reset()

    def reset(self):
        """the outputs as before the launch (the counter workspace stays as the launch before left it)"""
        self.y.fill_bits(FT)
        if self.t is not None:
            self.t.fill_bits(FT)
        if self.slab is not None:
            self.slab.fill_bits(SB)
        for i, g in enumerate(self.outs):
            if i < 4:
                g.fill_bits(FT)
            else:
                g.data.copy_(self.d['rm0' if i == 4 else 'rv0'])

    def run(self, st):
        self.L.check(self.lb.addk_sep_fwd(C.byref(self.args), st), self.what)
        torch.cuda.synchronize()
        return self

    def buffers(self):
        return [g for g in [self.y, self.t, self.slab, self.counter] + self.outs if g is not None]

    def bits(self):
        """everything the launch may have written, guards included"""
        return [g.raw.clone() for g in self.buffers()]

    def check(self):
        op, what, P, Cc = self.op, self.what, self.P, self.op.C
        inp = R.make_inputs(op)
        t_ref, y_ref = R.ref_forward(op, self.form)
        first = lambda row: np.full((P, row), FT, dtype=np.int32)
        if self.epilogue is not None:
            y_ref = R.epilogue_fp64(op, inp, y_ref, self.epilogue)
        errs = {'y': R.rel_err(_slice_check(what, 'y', self.y, P, R.ld(op, 'y'), Cc, first(R.ld(op, 'y'))), y_ref)}
        if self.t is not None:
            errs['t'] = R.rel_err(_slice_check(what, 't', self.t, P, R.ld(op, 't'), Cc, first(R.ld(op, 't'))), t_ref)
        if self.slab is not None:
            row = R.ld(op, 'stats')
            assert self.slab.intact(), '%s: guard band of the slab overwritten' % what
            words = _words(self.slab).reshape(self.rows, row, 4)
            assert (words[:, Cc:] == np.int32(SB)).all(), '%s: a slab row changed beyond its %d channels' % (what, Cc)
            sl = self.slab.data.view(torch.float64).cpu().numpy().reshape(self.rows, row, 2)[:, :Cc]
            assert np.isfinite(sl[:self.gx]).all(), '%s: %d slab elements of the launch\'s own rows are not written' % (what, int((~np.isfinite(sl[:self.gx])).sum()))
            if self.fin:
                assert (words[self.gx:, :Cc] == np.int32(SB)).all(), '%s: the fused finalize form wrote slab rows beyond addk_sep_rows' % what
                sl = sl[:self.gx]
            else:
                assert (words[self.gx:, :Cc] == 0).all(), '%s: slab rows no workgroup owns are not zero' % what
            errs['stats'] = R.rel_err(sl.sum(0), R.stats_fp64(op, y_ref))
        if self.fin:
            assert self.counter.intact(), '%s: guard band of the counter workspace overwritten' % what
            ncnt = 1 + (self.gx + 15) // 16
            assert not _words(self.counter)[:ncnt].any(), '%s: ticket counters not back at zero' % what
            for name, g, ref in zip(R.FIN_NAMES, self.outs, R.finalize_fp64(op, inp, y_ref)):
                assert g.intact(), '%s: guard band of fin.%s overwritten' % (what, name)
                errs['fin_' + name] = R.rel_err(g.data.cpu().numpy(), ref)
        return errs


class _Bwd:
    """One backward launch on the device: g as a slice of wider rows (first touch: FIRST_TOUCH_BITS, accumulate: the seeded g0), ws of exactly rows x C x
    K^2 first-touch floats and dab of exactly rows x C x 2 doubles of SLAB_BITS, rows = addk_sep_bwd_rows, all between guard bands.  g and dab exist
    also where the launch is not given them: they must then keep every bit."""

    def __init__(self, L, lb, dev, op, want, what, form=0, accumulate=0, g=True, dab=True):
        self.L, self.lb, self.op, self.what, self.form, self.accumulate, self.has_g, self.has_dab = L, lb, op, what, form, accumulate, g, dab
        self.P, Cc = R.pixels(op), op.C
        d, ptr = _mem(op, dev)
        self.d, ptr = d, dict(ptr)
        self.rows = int(lb.addk_sep_bwd_rows(C.byref(R.bwd_args(L, op, dict(ptr, ws=None), form, g=False, dab=False))))     # the shape alone
        assert self.rows > 0, what
        self.g = R.Guarded(self.P * R.ld(op, 'g'), dev)
        self.dab = R.Guarded(self.rows * Cc * 4, dev)
        self.ws = R.Guarded(self.rows * Cc * op.K * op.K, dev)
        ptr.update(g=self.g.data.data_ptr(), dab=self.dab.data.data_ptr(), ws=self.ws.data.data_ptr())
        self.args = R.bwd_args(L, op, ptr, form, accumulate, g=g, dab=dab)
        cfg = R.config(L, lb, self.args)
        assert cfg[0] == 1 and tuple(cfg[1:5]) == want and cfg[5] == cfg[6] == self.rows, '%s takes %s, its case names %s' % (what, cfg, want)
        self.key = cfg[7]
        assert self.key == int(lb.addk_sep_bwd_batch_key(C.byref(self.args))) >= 0
        self.reset()
        self.init_words = _words(self.g).reshape(self.P, R.ld(op, 'g')).copy()

    def reset(self):
        if self.accumulate:
            self.g.data.copy_(self.d['g0'].reshape(-1))
        else:
            self.g.fill_bits(FT)
        self.dab.fill_bits(SB)
        self.ws.fill_bits(FT)

    def run(self, st):
        self.L.check(self.lb.addk_sep_bwd(C.byref(self.args), st), self.what)
        torch.cuda.synchronize()
        return self

    def buffers(self):
        return [self.g, self.dab, self.ws]

    def bits(self):
        return [g.raw.clone() for g in self.buffers()]

    def check(self):
        op, what, P, Cc, row = self.op, self.what, self.P, self.op.C, R.ld(self.op, 'g')
        dx, dab, dW = R.ref_backward(op, self.form)
        errs = {}
        got = _slice_check(what, 'g', self.g, P, row, Cc if self.has_g else 0, self.init_words)
        if self.has_g:
            init = R.make_inputs(op)['g0'] if self.accumulate else np.zeros((P, row))
            errs['g'] = R.rel_err(got, R.widen(dx, init, row, self.accumulate)[:, :Cc])
        assert self.dab.intact(), '%s: guard band of dab overwritten' % what
        if self.has_dab:
            sl = self.dab.data.view(torch.float64).cpu().numpy().reshape(self.rows, Cc, 2)
            assert np.isfinite(sl).all(), '%s: %d of %d dab elements are not written' % (what, int((~np.isfinite(sl)).sum()), sl.size)
            errs['dab'] = R.rel_err(sl.sum(0), dab)
        else:
            assert (_words(self.dab) == np.int32(SB)).all(), '%s: dab written although the launch was given none' % what
        assert self.ws.intact(), '%s: guard band of ws overwritten' % what
        ws = self.ws.data.cpu().numpy().reshape(self.rows, Cc, op.K * op.K)
        assert not (ws.view(np.int32) == np.int32(FT)).any() and np.isfinite(ws).all(), '%s: workspace elements are not written' % what
        errs['dw'] = R.rel_err(ws.astype(np.float64).sum(0), dW)
        return errs


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def _tagged(name, errs):
    return {'%s/%s' % (name, k): v for k, v in errs.items()}


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_forward_training_form_matches_fp64_in_every_source_form(lib, case):
    """y, t and the reduced statistics in the four source forms; the slab rows no workgroup owns come back zero; once with t = NULL"""
    L = lib
    lb, dev, st = _env(L)
    errs = {}
    for form in range(4):
        la = _Fwd(L, lb, dev, case.op, case.variant, '%s fwd %s' % (R.case_id(case), R.FORM_NAMES[form]), form).run(st)
        errs.update(_tagged(R.FORM_NAMES[form], la.check()))
    la = _Fwd(L, lb, dev, case.op, case.variant, '%s fwd without t' % R.case_id(case), 0, t=False).run(st)
    errs.update(_tagged('ab_relu/no_t', la.check()))
    _finish('fwd %s' % R.case_id(case), errs)


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_forward_fused_finalize_matches_fp64_and_repeats_bit_for_bit(lib, case):
    """Two launches in a row on one counter workspace, zeroed once: the six finalize outputs, y, t and the slab against fp64, the second launch bit for
    bit the first, the counters back at zero both times, the slab rows beyond addk_sep_rows untouched."""
    L = lib
    lb, dev, st = _env(L)
    la = _Fwd(L, lb, dev, case.op, case.variant, '%s fwd fused finalize' % R.case_id(case), 0, fin=True).run(st)
    errs = la.check()
    first = la.bits()
    la.reset()
    again = la.run(st).check()
    _finish('fin %s' % R.case_id(case), errs)
    assert again == errs and _same(first, la.bits()), '%s: the second launch on the same counters differs from the first' % R.case_id(case)


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_forward_inference_epilogues_match_fp64(lib, case):
    """t = stats = NULL; the six epilogues of R.EPILOGUES, epilogue j on a source in form j % 4 with term i in form (i + j) % 4"""
    L = lib
    lb, dev, st = _env(L)
    errs = {}
    for j, (nterm, ea) in enumerate(R.EPILOGUES):
        name = '%dterms_%s' % (nterm, 'ea' if ea else 'noea')
        la = _Fwd(L, lb, dev, case.op, case.variant, '%s fwd %s' % (R.case_id(case), name), j % 4, epilogue=j).run(st)
        assert la.args.nterm == nterm and bool(la.args.ea) == ea and not la.args.t and not la.args.stats
        errs.update(_tagged(name, la.check()))
    _finish('infer %s' % R.case_id(case), errs)


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_backward_matches_fp64_in_every_source_form(lib, case):
    """g, the reduced (dA, dB) and the summed workspace in the four source forms x {first touch, accumulate}; g with dab = NULL; g = NULL with dab = NULL;
    the first launch again, bit for bit"""
    L = lib
    lb, dev, st = _env(L)
    errs, first = {}, None
    for form in range(4):
        for acc in (0, 1):
            name = '%s/%s' % (R.FORM_NAMES[form], 'acc' if acc else 'first')
            la = _Bwd(L, lb, dev, case.op, case.variant, '%s bwd %s' % (R.case_id(case), name), form, acc).run(st)
            errs.update(_tagged(name, la.check()))
            if first is None:
                first = (la, la.bits())
    la = _Bwd(L, lb, dev, case.op, case.variant, '%s bwd without dab' % R.case_id(case), 1, 1, dab=False).run(st)
    errs.update(_tagged('ab/acc/no_dab', la.check()))
    la = _Bwd(L, lb, dev, case.op, case.variant, '%s bwd without g and dab' % R.case_id(case), 0, 0, g=False, dab=False).run(st)
    errs.update(_tagged('ab_relu/no_g_no_dab', la.check()))
    la, bits = first
    la.reset()
    repeat = la.run(st).bits()
    _finish('bwd %s' % R.case_id(case), errs)
    assert _same(bits, repeat), '%s: the repeated backward launch differs bit for bit' % R.case_id(case)


def _batch(L, lb, dev, st, case, direction, las):
    """prepare, upload and run the batch of `las`, check every member against fp64, then bit for bit against its lone launch and against a replay"""
    n, tag = len(las), '%s batch %s' % (direction, R.case_id(case))
    prepare, run = ((lb.addk_sep_fwd_batch_prepare, lb.addk_sep_batch_run) if direction == 'fwd' else (lb.addk_sep_bwd_batch_prepare, lb.addk_sep_bwd_batch_run))
    arr = (type(las[0].args) * n)(*[la.args for la in las])
    meta = (C.c_int64 * 8)()
    size = prepare(arr, n, None, 0, meta)
    if size < 0:
        L.check(int(size), 'sep_%s_batch_prepare' % direction)
    host = (C.c_uint8 * size)()
    rc = prepare(arr, n, host, size, meta)
    if rc < 0:
        L.check(int(rc), 'sep_%s_batch_prepare' % direction)
    grids = [la.gx if direction == 'fwd' else la.rows for la in las]
    assert len(set(grids)) > 1 and list(meta[:4]) == [las[0].key, n, max(grids), 1], '%s: meta %s, grids %s' % (tag, list(meta[:4]), grids)
    assert all(la.key == las[0].key for la in las)
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    L.check(run(blob.data_ptr(), meta, st), 'sep_%s_batch_run' % direction)
    torch.cuda.synchronize()
    errs = {}
    for i, la in enumerate(las):
        errs.update(_tagged('member%d_%dx%dx%d_%s' % ((i,) + tuple(la.op[:3]) + (R.FORM_NAMES[la.form],)), la.check()))
    batched = [la.bits() for la in las]
    differ = []
    for i, la in enumerate(las):
        la.reset()
        if not _same(batched[i], la.run(st).bits()):
            differ.append('member %d differs from its lone launch' % i)
    for la in las:
        la.reset()
    L.check(run(blob.data_ptr(), meta, st), 'sep_%s_batch_run' % direction)
    torch.cuda.synchronize()
    differ += ['member %d differs in the replay' % i for i, la in enumerate(las) if not _same(batched[i], la.bits())]
    _finish(tag, errs)
    assert not differ, '%s: %s' % (tag, '; '.join(differ))


@pytest.mark.parametrize('case', BATCH_CASES, ids=BATCH_IDS)
def test_forward_batch_members_match_fp64_and_their_lone_launches(lib, case):
    """three members of different grids under one key, member i in source form i, each with t, a slab, its own fused finalize and counter workspace"""
    L = lib
    lb, dev, st = _env(L)
    las = [_Fwd(L, lb, dev, op, case.variant, '%s fwd batch member %d' % (R.case_id(case), i), i, fin=True) for i, op in enumerate(R.batch_members(case))]
    _batch(L, lb, dev, st, case, 'fwd', las)


@pytest.mark.parametrize('case', BATCH_CASES, ids=BATCH_IDS)
def test_backward_batch_members_match_fp64_and_their_lone_launches(lib, case):
    """three members of different grids under one key, member i in source form 3 - i, members 0 and 2 accumulating, member 1 a first touch"""
    L = lib
    lb, dev, st = _env(L)
    las = [_Bwd(L, lb, dev, op, case.variant, '%s bwd batch member %d' % (R.case_id(case), i), 3 - i, 1 - i % 2)
           for i, op in enumerate(R.batch_members(case))]
    _batch(L, lb, dev, st, case, 'bwd', las)
