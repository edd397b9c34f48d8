"""GPU test of the dense weight gradient (csrc/wgrad.hip, wgrad_pix.hip, wgrad_h3.hip, wgrad_hk.hip, wgrad_rs.hip) against the fp64
reference of its definition (tests/_wgrad_ref.py), at the whole contract of addk_conv_wgrad_args and on the path the plan takes:

* lone launches: every (case, mode) of tests/tools/make_wgrad_bits.CASES under its pinned launch key, in all four source forms (a, b
  present or null, relu 0 or 1), first touch and accumulating, with the case's padded or unpadded strides; gradients of 2^-30 in f16x3 on
  the kinds that split into fp16; the tail_x3 mode on kinds 5, 7 and 9;
* mixed batches (tests/_wgrad_ref.BATCHES): convs of different sizes, taps, dilations, strides, source forms and accumulate flags under one
  key in one addk_conv_wgrad_batch_prepare / run, as plan.py launches every weight gradient, then the same blob replayed.

Every gradient is a slice (w_choff = 8, cin_total = C + 12, ldw = taps * cin_total + 4) of a wider weight whose other elements must keep
their bits; dw and the workspace (exactly addk_conv_wgrad_ws floats) lie between guard bands that must keep theirs; a first-touch dw starts
as NaN.  Bound: 2e-5 of the reference's max-abs, the bound tests/test_gpu_fast_kernels.py holds all three arithmetics to;
tests/test_wgrad_ref.py shows that it separates the right gradient from five subtly wrong ones by a factor of 50 at least.  A change to
wgrad*.hip that reorders sums is judged here; tests/test_gpu_wgrad_bits.py judges a pure refactoring.  The errors measured on the MI355X
are in profiles/wgrad_fp64_errors.txt; every item appends its own to wgrad_fp64_errors.txt in the report directory (the environment
variable ADDK_TEST_REPORTS, else test_reports/ under the working directory)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _wgrad_ref as R

pytestmark = pytest.mark.gpu

TOL = R.TOL
LOG = os.path.join(os.environ.get('ADDK_TEST_REPORTS') or 'test_reports', 'wgrad_fp64_errors.txt')
LONE = [(case, mode) for case in R.CASES for mode in R.MODES if mode in case[5]]
TAIL = [case for case in R.CASES if case[5]['f16x3'][0] in (5, 7, 9)]
BATCH = [(batch, mode) for batch in R.BATCHES for mode in R.MODES if mode in batch[2]]
TINY_DY = 2.0 ** -30


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    lb = L.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    yield L
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


def _log(lines):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'a') as f:
        f.write(''.join(v + '\n' for v in lines))


class _Launch:
    """One weight gradient on the device: its inputs, its guarded dw (NaN for a first touch, the seeded dw0 for an accumulating launch) and
    its guarded NaN workspace of exactly addk_conv_wgrad_ws floats."""

    def __init__(self, L, op, dev, dev_in=None, dy_scale=1.0):
        lb = L.load()
        self.op, self.dy_scale = op, dy_scale
        self.host = R.make_inputs(op)
        self.x, self.a, self.b, self.dy = dev_in or [torch.tensor(v).to(dev) for v in self.host[:4]]
        if dy_scale != 1.0:
            self.dy = self.dy * dy_scale        # a power of two: exact
        self.dw = R.Guarded(op.Cout * op.ldw, dev)
        self.ws_floats = int(lb.addk_conv_wgrad_ws(op.N * op.OH * op.OW, op.Cout, op.C, op.k * op.k))
        self.ws = R.Guarded(self.ws_floats, dev)
        self.reset()
        self.init_bits = self.dw.data.view(torch.int32).cpu().numpy().reshape(op.Cout, op.ldw).copy()
        self.args = R.wgrad_args(L, op, {'dy': self.dy.data_ptr(), 'x': self.x.data_ptr(), 'a': self.a.data_ptr(), 'b': self.b.data_ptr(),
                                         'dw': self.dw.data.data_ptr(), 'ws': self.ws.data.data_ptr()}, self.ws_floats)

    def inputs(self):
        return [self.x, self.a, self.b, self.dy]

    def reset(self):
        """dw and the workspace as before the launch"""
        if self.op.accumulate:
            self.dw.data.copy_(torch.tensor(self.host[4]).reshape(-1))
        else:
            self.dw.fill_bits(R.FIRST_TOUCH_BITS)
        self.ws.fill_bits(R.FIRST_TOUCH_BITS)

    def bits(self):
        """everything the launch may have written, guards included"""
        return self.dw.raw.clone(), self.ws.raw.clone()

    def check(self, what):
        """The guards and everything outside the weight slice kept their bits; returns max|got - ref| / max|ref| over the slice."""
        op = self.op
        assert self.dw.intact(), '%s: dw guard band overwritten' % what
        assert self.ws.intact(), '%s: workspace guard band overwritten' % what
        got = self.dw.data.cpu().numpy().reshape(op.Cout, op.ldw)
        m = R.slice_mask(op)
        assert np.array_equal(got.view(np.int32)[~m], self.init_bits[~m]), '%s: dw changed outside its channel slice' % what
        ref = R.expected(op, R.reference(op) * self.dy_scale, self.host[4] if op.accumulate else np.zeros_like(self.host[4]))
        return R.rel_err(got[m], ref[m])


def _setup(L, fast, mode):
    lb = L.load()
    lb.addk_set_fast_paths(fast)
    L.check(lb.addk_set_conv_precision(R.ALL_MODES[mode]), 'set_conv_precision')
    return lb, torch.device('cuda:0'), torch.cuda.current_stream().cuda_stream


def _key(L, lb, args):
    cfg = (C.c_int32 * 4)()
    L.check(lb.addk_conv_wgrad_config(C.byref(args), cfg), 'conv_wgrad_config')
    return tuple(int(v) for v in cfg[:3])


def _run_lone(L, lb, st, launch, what):
    L.check(lb.addk_conv_wgrad(C.byref(launch.args), st), 'conv_wgrad')
    torch.cuda.synchronize()
    return launch.check(what)


def _finish(tag, errs):
    """log every figure, then assert"""
    _log(['%s %s %.2e' % (tag, k, v) for k, v in errs.items()] + ['worst %s %.2e' % (tag, max(errs.values(), key=lambda v: (v != v, v)))])
    bad = ['%s %.2e' % kv for kv in errs.items() if not kv[1] <= TOL]
    assert not bad, '%s beyond %.0e of the fp64 reference: %s' % (tag, TOL, ', '.join(bad))


@pytest.mark.parametrize('case,mode', LONE, ids=['%s-%s' % (c[0], m) for c, m in LONE])
def test_lone_launch_matches_fp64_in_every_source_form(lib, case, mode):
    """All four source forms x {first touch, accumulate} of one case in one arithmetic mode, under the launch key the case pins; in f16x3 on
    kinds 5, 6, 7 and 9 also a first touch with dy scaled by exactly 2^-30 (far below fp16's range; the reference scales exactly)."""
    L = lib
    lb, dev, st = _setup(L, case[2], mode)
    key = case[5][mode]
    errs, dev_in = {}, None
    for form in range(4):
        for acc in (0, 1):
            la = _Launch(L, R.case_op(case, form, acc), dev, dev_in)
            dev_in = la.inputs()
            assert _key(L, lb, la.args) == key, '%s [%s] %s gets launch key %s, expected %s' % (case[0], mode, R.FORM_NAMES[form], _key(L, lb, la.args), key)
            errs['%s/%s' % (R.FORM_NAMES[form], 'acc' if acc else 'first')] = _run_lone(L, lb, st, la, '%s [%s] %s acc=%d' % (case[0], mode, R.FORM_NAMES[form], acc))
    if mode == 'f16x3' and key[0] in (5, 6, 7, 9):
        la = _Launch(L, R.case_op(case, 0, 0), dev, dev_in, TINY_DY)
        assert _key(L, lb, la.args) == key
        errs['ab_relu/first/dy*2^-30'] = _run_lone(L, lb, st, la, '%s [%s] tiny dy' % (case[0], mode))
    _finish('lone %s[%s]' % (case[0], mode), errs)


@pytest.mark.parametrize('case', TAIL, ids=[c[0] for c in TAIL])
def test_lone_launch_matches_fp64_in_tail_x3(lib, case):
    """tail_x3 (mode 3): the two-term kernels on the 128-channel blocks (cty = 8), the three-term kernels everywhere else (wg_np_of), under
    the split modes' launch key: one first-touch launch of kinds 5, 7 and 9."""
    L = lib
    lb, dev, st = _setup(L, case[2], 'tail_x3')
    la = _Launch(L, R.case_op(case, 0, 0), dev)
    assert _key(L, lb, la.args) == case[5]['f16x3'], (case[0], _key(L, lb, la.args))
    _finish('lone %s[tail_x3]' % case[0], {'ab_relu/first': _run_lone(L, lb, st, la, '%s [tail_x3]' % case[0])})


@pytest.mark.parametrize('batch,mode', BATCH, ids=['%s-%s' % (b[0], m) for b, m in BATCH])
def test_mixed_batch_matches_fp64_and_replays_bit_for_bit(lib, batch, mode):
    """One batched launch over convs that share only the key: member i in source form i mod 4, accumulate = i mod 2, padded strides when i is
    odd, each with its own dw, workspace and guards.  Then every dw is put back, every workspace refilled with NaN and the SAME blob run
    again: all outputs bit-identical, as the plan replays the blob step after step."""
    L = lib
    name, fast, keys, _ = batch
    lb, dev, st = _setup(L, fast, mode)
    las = [_Launch(L, op, dev) for op in R.batch_ops(batch)]
    n = len(las)
    arr = (L.ConvWgradArgs * n)(*[la.args for la in las])
    meta = (C.c_int64 * 8)()
    size = lb.addk_conv_wgrad_batch_prepare(arr, n, None, 0, meta)
    if size < 0:
        L.check(int(size), 'conv_wgrad_batch_prepare')
    host = (C.c_uint8 * size)()
    rc = lb.addk_conv_wgrad_batch_prepare(arr, n, host, size, meta)
    if rc < 0:
        L.check(int(rc), 'conv_wgrad_batch_prepare')
    assert tuple(meta[:3]) == keys[mode] and meta[3] == n, '%s [%s]: the batch carries key %s, expected %s' % (name, mode, list(meta[:3]), keys[mode])
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    L.check(lb.addk_conv_wgrad_batch_run(blob.data_ptr(), meta, st), 'conv_wgrad_batch_run')
    torch.cuda.synchronize()
    errs = {'op%d/%s/%s' % (i, R.FORM_NAMES[la.op.form], 'acc' if la.op.accumulate else 'first'): la.check('%s [%s] op %d' % (name, mode, i)) for i, la in enumerate(las)}
    first = [la.bits() for la in las]
    for la in las:
        la.reset()
    L.check(lb.addk_conv_wgrad_batch_run(blob.data_ptr(), meta, st), 'conv_wgrad_batch_run')
    torch.cuda.synchronize()
    diff = ['op%d %s' % (i, o) for i, la in enumerate(las) for o, a, b in zip(('dw', 'ws'), first[i], la.bits()) if not torch.equal(a, b)]
    _finish('batch %s[%s]' % (name, mode), errs)
    assert not diff, '%s [%s]: the replay of the same blob differs bit for bit in %s' % (name, mode, ', '.join(diff))
