"""GPU test of the kernels of csrc/pw.hip against the fp64 reference of their definition (tests/_pw_ref.py), through the C ABI: one item per lone
instantiation (46: pw_kernel <CT, KG> forward plain / resampled and data gradient with fp64 / fp32 lane sums, pwk_kernel <CT> plain / resampled, stem0_kernel,
k1s_dgrad_kernel <20 | 32>), six more shapes of them (k1s with 132 channels, 32 and 1 dy channels; a map of 5 pixels for pw_kernel forward, data gradient
and k1s), and a mixed three-member batch for each of the 30 pw_batch_kernel instantiations.  tests/test_pw_ref.py shows without a GPU that the cases reach
exactly these variants.

* forward: the four source forms (a, b present or NULL, relu 0 / 1; several sources in mixed forms) x {no bias, bias}; once with stats = NULL; a resampled
  source from a map smaller and from one larger than the grid, with rs_y and with rs_y = NULL;
* data gradient: the four destination forms x {first touch, accumulate onto a seeded g0}; once with dab = NULL; once with dy scaled by exactly 2^-30;
* stem0 with ldy = 64 and 72;
* batches: members of one key that differ in pixel count, output width, reduction length, form, bias / accumulate, slab and rs_y presence and source map:
  every member within the bound and bit-identical, guards included, to its own lone launch, and again when the same device blob is replayed.

Every launch first asserts, with addk_conv_*_config, that it takes the variant its case names.  The weight is a slice (w_choff = 8 of cin_total = K + 12,
ldw = cin_total + 4); x, dy, y, g and rs_y are slices of rows 8 floats wider whose other elements must keep their bits (NaN in the inputs' padding and
in the weight rows' padding), as must the guard bands around y / g, the slab and rs_y; a first-touch output starts as NaN; the slab (stats_ld = Cout + 4)
is exactly addk_conv_rows rows of NaN, every element of which inside the slice a launch must write (outside the 5-pixel map and k1s there are fewer
workgroups than rows, so the zero-fill of unowned rows is checked too).  Bound: 2e-5 of the reference's max-abs (TOL of tests/_wgrad_ref.py) for y / g, the
slab summed over its rows, and rs_y; tests/test_pw_ref.py shows that it separates the right result from fourteen subtly wrong ones by a factor of 260 at
least and that fp32 numpy arithmetic stays a factor of 5 below it.  The errors measured on the MI355X are in profiles/pw_fp64_errors.txt; every item
appends its own to pw_fp64_errors.txt in the report directory (the environment variable ADDK_TEST_REPORTS, else test_reports/ under the working directory)."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _pw_ref as R

pytestmark = pytest.mark.gpu

TOL = R.TOL
LOG = os.path.join(os.environ.get('ADDK_TEST_REPORTS') or 'test_reports', 'pw_fp64_errors.txt')
FT = R.FIRST_TOUCH_BITS


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    lb = L.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(R.FAST_ALL)
    yield L
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)
    _DEV.clear()


def _log(lines):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'a') as f:
        f.write(''.join(v + '\n' for v in lines))


def _finish(tag, errs):
    """log every figure, then assert"""
    _log(['%s %s %.2e' % (tag, k, v) for k, v in errs.items()] + ['worst %s %.2e' % (tag, max(errs.values(), key=lambda v: (v != v, v)))])
    bad = ['%s %.2e' % kv for kv in errs.items() if not kv[1] <= TOL]
    assert not bad, '%s beyond %.0e of the fp64 reference: %s' % (tag, TOL, ', '.join(bad))


_DEV = OrderedDict()


def _device_inputs(op, dev):
    """the op's seeded inputs on the device, kept for the launches of the last few ops"""
    if op not in _DEV:
        while len(_DEV) >= 4:
            _DEV.popitem(last=False)
        up = lambda v: torch.tensor(v).to(dev)
        _DEV[op] = {k: [up(u) for u in v] if isinstance(v, list) else up(v) for k, v in R.make_inputs(op).items()}
    return _DEV[op]


def _bits(t):
    return t.cpu().numpy().view(np.int32)


class _Run:
    """One launch on the device: its guarded output as a slice of wider rows (NaN for a first touch, the seeded g0 for an accumulating gradient), its
    guarded slab of exactly addk_conv_rows rows of NaN and its guarded NaN rs_y (each None where the launch has none).  Asserts that the launch takes
    the variant and batch key `want`."""

    def __init__(self, L, lb, dev, la, want, what, ldy=None):
        self.L, self.lb, self.la, self.what = L, lb, la, what
        op, lay = la.op, R.layout(la.op, ldy)
        self.fwd = fwd = op.kind != 'dgrad'
        self.d = d = _device_inputs(op, dev)
        self.P, self.Cn, self.ld = R.pixels(op), (op.Cout if fwd else op.Cs[0]), (lay['ldy'] if fwd else lay['ldg'])
        self.slab_ld = lay['stats_ld'] if fwd else self.Cn
        self.rows = int(lb.addk_conv_rows(self.P, self.Cn))
        assert 0 < self.rows <= 1024
        self.out = R.Guarded(self.P * self.ld, dev)
        self.slab = R.Guarded(self.rows * self.slab_ld * 4, dev) if la.stats else None
        self.rs_ld = lay.get('rs_ldy', 0)
        self.rsy = R.Guarded(self.P * self.rs_ld, dev) if la.rs_y else None
        self.dy = None
        if not fwd:
            self.dy = d['dy'] if la.dy_scale == 1.0 else d['dy'] * la.dy_scale          # a power of two: exact
        ptr = {k: [v.data_ptr() for v in d[k]] for k in ('x', 'a', 'b')}
        ptr.update(w=d['w'].data_ptr(), bias=d['bias'].data_ptr(), y=self.out.data.data_ptr(), dy=self.dy.data_ptr() if self.dy is not None else None,
                   slab=self.slab.data.data_ptr() if self.slab else None, rs_y=self.rsy.data.data_ptr() if self.rsy else None)
        self.args = R.launch_args(L, la, ptr, ldy)
        self.fn = lb.addk_conv_fwd if fwd else lb.addk_conv_dgrad
        cfg, self.gx, self.gy, key = R.bits.config(lb, L, (None, 'fwd' if fwd else 'dgrad'), self.args)
        assert (cfg, key) == want, '%s takes %s with batch key %d, its case names %s' % (what, cfg, key, want)
        assert self.gx <= self.rows
        self.reset()
        self.init_bits = _bits(self.out.data).reshape(self.P, self.ld).copy()

    def reset(self):
        """the outputs as before the launch"""
        if self.la.accumulate:
            self.out.data.copy_(self.d['g0'].reshape(-1))
        else:
            self.out.fill_bits(FT)
        if self.slab is not None:
            self.slab.fill_bits(R.SLAB_BITS)
        if self.rsy is not None:
            self.rsy.fill_bits(FT)

    def run(self, st):
        self.L.check(self.fn(C.byref(self.args), st), self.what)
        torch.cuda.synchronize()
        return self

    def bits(self):
        """everything the launch may have written, guards included"""
        return [b.raw.clone() for b in (self.out, self.slab, self.rsy) if b is not None]

    def check(self):
        """The guards and everything outside the slices kept their bits and every slab element inside the slice was written; returns the errors of the
        output, of the slab summed over its rows and of rs_y, max|got - ref| / max|ref| each."""
        what, Cn = self.what, self.Cn
        ref = R.reference(self.la)
        assert self.out.intact(), '%s: guard band of the output overwritten' % what
        got = self.out.data.cpu().numpy().reshape(self.P, self.ld)
        assert np.array_equal(got.view(np.int32)[:, Cn:], self.init_bits[:, Cn:]), '%s: the output row changed beyond its %d channels' % (what, Cn)
        errs = {'y': R.rel_err(got[:, :Cn], ref['y'])} if self.fwd else {'g': R.rel_err(got[:, :Cn], ref['g'])}
        if self.slab is not None:
            assert self.slab.intact(), '%s: guard band of the slab overwritten' % what
            words = _bits(self.slab.data).reshape(self.rows, self.slab_ld, 4)
            assert (words[:, Cn:] == np.int32(R.SLAB_BITS)).all(), '%s: the slab row changed beyond its %d channels' % (what, Cn)
            sl = self.slab.data.view(torch.float64).cpu().numpy().reshape(self.rows, self.slab_ld, 2)[:, :Cn]
            assert np.isfinite(sl).all(), '%s: %d of %d slab elements are not written' % (what, int((~np.isfinite(sl)).sum()), sl.size)
            errs['stats' if self.fwd else 'dab'] = R.rel_err(sl.sum(0), ref['stats' if self.fwd else 'dab'])
        if self.rsy is not None:
            c0 = self.la.op.Cs[0]
            assert self.rsy.intact(), '%s: guard band of rs_y overwritten' % what
            r = self.rsy.data.cpu().numpy().reshape(self.P, self.rs_ld)
            assert (r.view(np.int32)[:, c0:] == np.int32(FT)).all(), '%s: the rs_y row changed beyond its %d channels' % (what, c0)
            errs['rs_y'] = R.rel_err(r[:, :c0], ref['rs_y'])
        return errs


def _setup(L):
    lb = L.load()
    lb.addk_set_fast_paths(R.FAST_ALL)
    return lb, torch.device('cuda:0'), torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_lone_variant_matches_fp64_at_its_full_contract(lib, case):
    """every launch of R.case_launches: the variant's forms, bias / accumulate, slab and rs_y presence, maps and output strides"""
    L = lib
    lb, dev, st = _setup(L)
    errs = {}
    for label, la, ldy in R.case_launches(case):
        run = _Run(L, lb, dev, la, (case.cfg, case.key), '%s %s' % (case.name, label), ldy).run(st)
        assert run.gx < run.rows or case.cfg[0] == R.K1S or run.P == 5, '%s: every slab row is owned (gx %d, rows %d)' % (case.name, run.gx, run.rows)
        errs.update(('%s/%s' % (label, k), v) for k, v in run.check().items())
    _finish(case.name, errs)


@pytest.mark.parametrize('v', R.BATCH_VARIANTS, ids=[R.batch_id(v) for v in R.BATCH_VARIANTS])
def test_mixed_batch_matches_fp64_and_its_lone_launches_bit_for_bit(lib, v):
    """Three unequal members of one key through addk_conv_*_batch_prepare / addk_conv_batch_run (R.batch_members): the grid is the largest member's, so
    the smaller members' surplus workgroups must leave without a trace.  Every member within the bound and bit-identical, guards included, to its own
    lone launch; again when the same device blob is replayed into fresh NaN buffers."""
    L = lib
    lb, dev, st = _setup(L)
    key = R.pw_key(*v)
    want = ([R.PW] + list(v[1:]), key)
    runs = [_Run(L, lb, dev, la, want, '%s member %d' % (R.batch_id(v), i)) for i, la in enumerate(R.batch_members(v))]
    errs, lone = {}, []
    for i, run in enumerate(runs):
        errs.update(('lone%d/%s' % (i, k), e) for k, e in run.run(st).check().items())
        lone.append(run.bits())
        run.reset()
    meta, host = R.batch_prepare(lb, L, [run.args for run in runs], blob=True)
    assert list(meta[:4]) == [key, 3, max(r.gx for r in runs), max(r.gy for r in runs)]
    assert len({r.gx for r in runs}) == 3
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    diff = []
    for tag in ('batch', 'replay'):
        L.check(lb.addk_conv_batch_run(blob.data_ptr(), meta, st), 'conv_batch_run')
        torch.cuda.synchronize()
        for i, run in enumerate(runs):
            errs.update(('%s%d/%s' % (tag, i, k), e) for k, e in run.check().items())
            diff += ['%s member %d buffer %d' % (tag, i, j) for j, (a, b) in enumerate(zip(lone[i], run.bits())) if not torch.equal(a, b)]
            run.reset()
    _finish('batch %s' % R.batch_id(v), errs)
    assert not diff, '%s: not bit-identical to the lone launches: %s' % (R.batch_id(v), ', '.join(diff))
