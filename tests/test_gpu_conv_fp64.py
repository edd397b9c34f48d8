"""GPU test of the halo-patch forward / data-gradient convolution kernels (csrc/conv3.hip, conv3b_row / tr3 / tr5 / s2.hip, conv3n.hip) against the
fp64 reference of their definition (tests/_conv_ref.py), through the C ABI, one launch per instantiated kernel and per parity of the dilation it
admits (tests/_conv_cases.py: 110 variants; tests/test_conv_ref.py shows without a GPU that the list reaches exactly the instantiated ones):

* every forward variant in the four source forms (a, b present or null, relu 0 or 1) x {no bias, bias, bias_n}: y and the reduced statistics;
* every data-gradient variant in the four destination forms x {first touch, accumulate onto a seeded g0}: g and the reduced (dA, dB); once with
  dab = NULL; with 2 planes (f16x3) also a first touch with dy scaled by exactly 2^-30, far below fp16's range;
* three virtually concatenated sources of 24 + 16 + 8 channels in mixed forms, and every source's gradient of a three-source convolution with its own w_choff,
  per pack layout and plane count;
* the tail_x3 mode on either side of its 192-channel line;
* the hoisted weight pack (addk_conv_*_pack_desc, addk_conv_pack_batch, wpack_ready = 1): bit-identical to the self-packing launch, pack included, and
  again on a replay of the launch alone.

Every launch first asserts, with addk_conv_*_config, that it takes the variant its case names.  The weight is a slice (w_choff = 8, cin_total = C + 12,
ldw = taps * cin_total + 4) of a wider one; y and g are slices of wider rows (ldy = Cout + 12, ldg = C + 12) whose other elements must keep their
bits, as must the guard bands around y, g, the slabs and wpack (exactly addk_conv_*_pack_floats floats); a first-touch output starts as NaN; the
statistics slab (stats_ld = Cout + 4) and the (dA, dB) slab are exactly addk_conv_rows rows of NaN, every element of which inside the slice a launch must
write.  Bound: 2e-5 of the reference's max-abs (TOL of tests/_wgrad_ref.py, the figure of tests/test_gpu_fast_kernels.py); tests/test_conv_ref.py shows
that it separates the right result from ten subtly wrong ones by a factor of 50 at least.  The errors measured on the MI355X are in
profiles/conv_fp64_errors.txt; every item appends its own to conv_fp64_errors.txt in the report directory (the environment variable
ADDK_TEST_REPORTS, else test_reports/ under the working directory)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _conv_ref as R

pytestmark = pytest.mark.gpu

TOL = R.TOL
LOG = os.path.join(os.environ.get('ADDK_TEST_REPORTS') or 'test_reports', 'conv_fp64_errors.txt')
ALL = [R.case_of(e) for e in R.CASES]
FWD_CASES = [c for c in ALL if c.direction == 'fwd']
DGRAD_CASES = [c for c in ALL if c.direction == 'dgrad']
TINY_DY = 2.0 ** -30
FT = R.FIRST_TOUCH_BITS


LAYOUTS, TAIL = R.LAYOUTS, R.TAIL
LAYOUT_IDS = ['%s-%dplanes' % (f.lookup.replace('_variant', ''), R.variant_planes(f.lookup, f.args)) for f, _ in LAYOUTS]
_cn = R.out_channels


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    lb = L.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    lb.addk_set_split_min_channels(0)
    yield L
    lb.addk_set_split_min_channels(-1)
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


def _log(lines):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'a') as f:
        f.write(''.join(v + '\n' for v in lines))


def _finish(tag, errs):
    """log every figure, then assert"""
    _log(['%s %s %.2e' % (tag, k, v) for k, v in errs.items()] + ['worst %s %.2e' % (tag, max(errs.values(), key=lambda v: (v != v, v)))])
    bad = ['%s %.2e' % kv for kv in errs.items() if not kv[1] <= TOL]
    assert not bad, '%s beyond %.0e of the fp64 reference: %s' % (tag, TOL, ', '.join(bad))


def _setup(L, mode):
    lb = L.load()
    lb.addk_set_fast_paths(R.FAST_ALL)
    lb.addk_set_split_min_channels(0)
    L.check(lb.addk_set_conv_precision(R.MODES[mode]), 'set_conv_precision')
    return lb, torch.device('cuda:0'), torch.cuda.current_stream().cuda_stream


_DEV = [None, None]


def _device_inputs(op, dev):
    """the op's seeded inputs on the device, kept for the launches of one op"""
    if _DEV[0] != op:
        up = lambda v: torch.tensor(v).to(dev)
        _DEV[:] = [op, {k: [up(u) for u in v] if isinstance(v, list) else up(v) for k, v in R.make_inputs(op).items()}]
    return _DEV[1]


def _bits(t):
    return t.cpu().numpy().view(np.int32)


class _Launch:
    """One forward (i is None) or one data gradient of source i on the device: its guarded output as a slice of wider rows (NaN for a first touch, the
    seeded g0 for an accumulating gradient), its guarded slab of exactly addk_conv_rows rows of NaN (None: no slab) and its guarded NaN wpack of exactly
    addk_conv_*_pack_floats floats.  Asserts that the launch takes the variant `want` in the library's current mode `mode`."""

    def __init__(self, L, lb, dev, op, mode, want, what, forms, bias_form=0, i=None, accumulate=0, slab=True, dy_scale=1.0):
        self.L, self.lb, self.op, self.i, self.what, self.accumulate, self.dy_scale = L, lb, op, i, what, accumulate, dy_scale
        self.forms, self.bias_form = forms, bias_form
        d = _device_inputs(op, dev)
        fwd = i is None
        self.P, self.Cn, self.ld = (op.N * op.OH * op.OW, op.Cout, op.ldy) if fwd else (op.N * op.H * op.W, op.Cs[i], R.ldg(op, i))
        self.slab_ld = op.stats_ld if fwd else self.Cn
        self.rows = int(lb.addk_conv_rows(self.P, self.Cn))
        assert 0 < self.rows <= 1024
        self.out = R.Guarded(self.P * self.ld, dev)
        self.slab = R.Guarded(self.rows * self.slab_ld * 4, dev) if slab else None
        self.dy = d['dy'] if dy_scale == 1.0 else d['dy'] * dy_scale          # a power of two: exact
        ptr = {'w': d['w'].data_ptr(), 'wpack': R.PTR['wpack'], 'dab': self.slab.data.data_ptr() if slab else None}
        if fwd:
            ptr.update(x=[v.data_ptr() for v in d['x']], a=[v.data_ptr() for v in d['a']], b=[v.data_ptr() for v in d['b']], y=self.out.data.data_ptr(),
                       stats=ptr['dab'], bias=d['bias'].data_ptr(), bias_n=d['bias_n'].data_ptr())
            make = lambda n: R.fwd_args(L, op, forms, bias_form, ptr, n)
            self.fn, self.fn_floats, self.fn_desc = lb.addk_conv_fwd, lb.addk_conv_fwd_pack_floats, lb.addk_conv_fwd_pack_desc
        else:
            ptr.update(x=d['x'][i].data_ptr(), a=d['a'][i].data_ptr(), b=d['b'][i].data_ptr(), dy=self.dy.data_ptr(), g=self.out.data.data_ptr())
            make = lambda n: R.dgrad_args(L, op, i, forms, accumulate, ptr, n, dab=slab)
            self.fn, self.fn_floats, self.fn_desc = lb.addk_conv_dgrad, lb.addk_conv_dgrad_pack_floats, lb.addk_conv_dgrad_pack_desc
        self.npk = int(self.fn_floats(C.byref(make(R.WPACK_ANY))))
        assert self.npk > 0, '%s: no halo-patch kernel takes the launch' % what
        self.wp = R.Guarded(self.npk, dev)
        ptr['wpack'] = self.wp.data.data_ptr()
        self.args = make(self.npk)
        got = R.variant_of(R.config(L, lb, self.args), op, 'fwd' if fwd else 'dgrad', mode, i or 0)
        assert got == want, '%s takes %s, its case names %s' % (what, got, want)
        self.reset(pack=True)
        self.init_bits = _bits(self.out.data).reshape(self.P, self.ld).copy()

    def reset(self, pack=False):
        """the outputs (and the pack) as before the launch"""
        if self.accumulate:
            self.out.data.copy_(_DEV[1]['g0'][self.i].reshape(-1))
        else:
            self.out.fill_bits(FT)
        if self.slab is not None:
            self.slab.fill_bits(R.SLAB_BITS)
        if pack:
            self.wp.fill_bits(FT)

    def run(self, st):
        self.L.check(self.fn(C.byref(self.args), st), self.what)
        torch.cuda.synchronize()
        return self

    def bits(self):
        """everything the launch may have written, guards included"""
        return [self.out.raw.clone(), self.wp.raw.clone()] + ([self.slab.raw.clone()] if self.slab is not None else [])

    def check(self):
        """The guards and everything outside the slices kept their bits and every slab element inside the slice was written; returns the errors of the
        output and of the reduced slab, max|got - ref| / max|ref| each."""
        op, what, Cn = self.op, self.what, self.Cn
        assert self.out.intact(), '%s: guard band of the output overwritten' % what
        assert self.wp.intact(), '%s: guard band of wpack overwritten' % what
        got = self.out.data.cpu().numpy().reshape(self.P, self.ld)
        assert np.array_equal(got.view(np.int32)[:, Cn:], self.init_bits[:, Cn:]), '%s: the output row changed beyond its %d channels' % (what, Cn)
        inp = R.make_inputs(op)
        if self.i is None:
            ref = R.ref_forward(op, self.forms, self.bias_form)
            errs = {'y': R.rel_err(got[:, :Cn], ref)}
            red = R.stats_fp64(ref) if self.slab is not None else None
        else:
            g, red = R.ref_dgrad(op, self.i, self.forms, self.dy_scale)
            init = inp['g0'][self.i] if self.accumulate else np.zeros((self.P, self.ld))
            errs = {'g': R.rel_err(got[:, :Cn], R.widen(g, init, self.ld, self.accumulate)[:, :Cn])}
        if self.slab is not None:
            assert self.slab.intact(), '%s: guard band of the slab overwritten' % what
            words = _bits(self.slab.data).reshape(self.rows, self.slab_ld, 4)
            assert (words[:, Cn:] == np.int32(R.SLAB_BITS)).all(), '%s: the slab row changed beyond its %d channels' % (what, Cn)
            sl = self.slab.data.view(torch.float64).cpu().numpy().reshape(self.rows, self.slab_ld, 2)[:, :Cn]
            assert np.isfinite(sl).all(), '%s: %d of %d slab elements are not written' % (what, int((~np.isfinite(sl)).sum()), sl.size)
            errs['stats' if self.i is None else 'dab'] = R.rel_err(sl.sum(0), red)
        return errs


def _want(case):
    return case.lookup, case.args


@pytest.mark.parametrize('case', FWD_CASES, ids=[R.case_id(c) for c in FWD_CASES])
def test_forward_variant_matches_fp64_in_every_source_and_bias_form(lib, case):
    """The four source forms x {no bias, bias, bias_n} of one forward case: y and the reduced statistics (a bias enters both)."""
    L = lib
    lb, dev, st = _setup(L, case.mode)
    op, errs = R.case_op(case), {}
    for form in range(4):
        for bf in range(3):
            name = '%s/%s' % (R.FORM_NAMES[form], R.BIAS_FORMS[bf])
            la = _Launch(L, lb, dev, op, case.mode, _want(case), '%s %s' % (R.case_id(case), name), [form], bf).run(st)
            errs.update(('%s/%s' % (name, k), v) for k, v in la.check().items())
    _finish('fwd %s' % R.case_id(case), errs)


@pytest.mark.parametrize('case', DGRAD_CASES, ids=[R.case_id(c) for c in DGRAD_CASES])
def test_dgrad_variant_matches_fp64_in_every_destination_form(lib, case):
    """The four destination forms x {first touch, accumulate onto g0} of one data-gradient case: g and the reduced (dA, dB); once with dab = NULL (g
    alone, nothing else written); with 2 planes also a first touch with dy scaled by exactly 2^-30 (the reference scales exactly)."""
    L = lib
    lb, dev, st = _setup(L, case.mode)
    op, errs = R.case_op(case), {}
    for form in range(4):
        for acc in (0, 1):
            name = '%s/%s' % (R.FORM_NAMES[form], 'acc' if acc else 'first')
            la = _Launch(L, lb, dev, op, case.mode, _want(case), '%s %s' % (R.case_id(case), name), form, i=0, accumulate=acc).run(st)
            errs.update(('%s/%s' % (name, k), v) for k, v in la.check().items())
    la = _Launch(L, lb, dev, op, case.mode, _want(case), '%s without dab' % R.case_id(case), 1, i=0, accumulate=1, slab=False).run(st)
    errs['ab/acc/no_dab/g'] = la.check()['g']
    if R.variant_planes(case.lookup, case.args) == 2:
        la = _Launch(L, lb, dev, op, case.mode, _want(case), '%s tiny dy' % R.case_id(case), 0, i=0, dy_scale=TINY_DY).run(st)
        errs.update(('ab_relu/first/dy*2^-30/%s' % k, v) for k, v in la.check().items())
    _finish('dgrad %s' % R.case_id(case), errs)


@pytest.mark.parametrize('fwd,dgrad', LAYOUTS, ids=LAYOUT_IDS)
def test_several_sources_match_fp64(lib, fwd, dgrad):
    """The forward case of a pack layout with three sources of 24 + 16 + 8 channels instead of one (a tail chunk of 8 channels after the first source, a
    lone chunk of 8: conv3n's quad steps) in the forms (a, b) + ReLU | plain | ReLU alone, then (a, b) | ReLU alone | (a, b) + ReLU with bias_n, the
    weights a slice from channel 8 of 60 per tap; and the data-gradient case with three sources of its channel count C, each source's gradient with its
    own w_choff (8, 8 + C, 8 + 2 C of 3 C + 12 per tap), form and accumulate flag."""
    L = lib
    lb, dev, st = _setup(L, fwd.mode)
    errs = {}
    op = R.case_op(R.three_sources(fwd))
    assert (op.w_choff, op.cin_total) == (8, 60)
    for forms, bf in (((0, 3, 2), 0), ((1, 2, 0), 2)):
        name = '+'.join(R.FORM_NAMES[f] for f in forms) + '/' + R.BIAS_FORMS[bf]
        la = _Launch(L, lb, dev, op, fwd.mode, _want(fwd), 'three sources %s %s' % (R.case_id(fwd), name), list(forms), bf).run(st)
        errs.update(('fwd/%s/%s' % (name, k), v) for k, v in la.check().items())
    op = R.case_op(R.three_destinations(dgrad))
    assert [R.choff(op, i) for i in range(3)] == [8, 8 + dgrad.Cs[0], 8 + 2 * dgrad.Cs[0]]
    for i, (form, acc) in enumerate(((0, 0), (3, 1), (2, 0))):
        name = 'src%d/%s/%s' % (i, R.FORM_NAMES[form], 'acc' if acc else 'first')
        la = _Launch(L, lb, dev, op, dgrad.mode, _want(dgrad), 'three sources %s %s' % (R.case_id(dgrad), name), form, i=i, accumulate=acc).run(st)
        errs.update(('dgrad/%s/%s' % (name, k), v) for k, v in la.check().items())
    _finish('sources %s | %s' % (R.case_id(fwd), R.case_id(dgrad)), errs)


@pytest.mark.parametrize('case', TAIL, ids=[R.case_id(c) for c in TAIL])
def test_tail_x3_takes_two_planes_from_192_channels_on(lib, case):
    """tail_x3 (mode 3): the fp16 kernels (2 planes) at >= 192 output-side channels, the bf16 kernels (3 planes) below (conv3.hip c3_planes): the launch
    takes the variant of that plane count and holds the bound."""
    L = lib
    lb, dev, st = _setup(L, 'tail_x3')
    op, Cn = R.case_op(case), _cn(case)
    assert R.variant_planes(case.lookup, case.args) == R.planes_of('tail_x3', Cn) == (2 if Cn >= 192 else 3)
    if case.direction == 'fwd':
        la = _Launch(L, lb, dev, op, 'tail_x3', _want(case), '%s [tail_x3]' % R.case_id(case), [0], 1)
    else:
        la = _Launch(L, lb, dev, op, 'tail_x3', _want(case), '%s [tail_x3]' % R.case_id(case), 0, i=0)
    _finish('tail_x3 %s' % R.case_id(case), la.run(st).check())


HOISTED = [c for pair in LAYOUTS for c in pair]


@pytest.mark.parametrize('case', HOISTED, ids=[R.case_id(c) for c in HOISTED])
def test_hoisted_pack_is_bit_identical_to_the_self_packing_launch(lib, case):
    """As a plan runs every step: the pack descriptor of the launch filled on the host, uploaded, addk_conv_pack_batch, then the launch with
    wpack_ready = 1 into fresh NaN outputs and a fresh NaN pack buffer.  Output, slab and pack (guards included) are bit-identical to the launch that
    packs its own weights, and again when the launch alone is replayed."""
    L = lib
    lb, dev, st = _setup(L, case.mode)
    op = R.case_op(case)
    if case.direction == 'fwd':
        la = _Launch(L, lb, dev, op, case.mode, _want(case), '%s hoisted' % R.case_id(case), [0], 2)
    else:
        la = _Launch(L, lb, dev, op, case.mode, _want(case), '%s hoisted' % R.case_id(case), 0, i=0, accumulate=1)
    errs = la.run(st).check()
    own = la.bits()
    la.reset(pack=True)
    desc = (C.c_uint8 * int(lb.addk_conv_pack_desc_bytes()))()
    L.check(la.fn_desc(C.byref(la.args), desc), 'conv_pack_desc')
    table = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
    L.check(lb.addk_conv_pack_batch(table.data_ptr(), 1, st), 'conv_pack_batch')
    la.args.wpack_ready = 1
    hoisted = la.run(st).bits()
    la.reset()
    replay = la.run(st).bits()
    _finish('hoisted %s' % R.case_id(case), errs)
    names = ('output', 'wpack', 'slab')
    diff = ['%s (%s)' % (n, tag) for tag, got in (('hoisted', hoisted), ('replay', replay)) for n, a, b in zip(names, own, got) if not torch.equal(a, b)]
    assert not diff, '%s: not bit-identical to the self-packing launch: %s' % (R.case_id(case), ', '.join(diff))
