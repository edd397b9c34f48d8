"""The fp64 reference of the dense weight gradient (tests/_wgrad_ref.py) checked without a GPU: against a direct evaluation of the
definition in include/addk.h, and for what tests/test_gpu_wgrad_fp64.py rests on: that its bound separates the right gradient from the
subtly wrong ones a kernel could compute."""
import numpy as np
import pytest

import _wgrad_ref as R

TINY = [('pix_tiny', (1, 9, 11, 20, 24, 3, 1, 1), False), ('strided', (2, 7, 10, 6, 5, 3, 2, 1), True), ('dilated', (2, 6, 7, 5, 4, 3, 1, 2), False),
        ('k5_s2_d2', (1, 11, 9, 3, 4, 5, 2, 2), True)]


def _direct(op, x, a, b, dy, dw_init):
    """dw[co][tap*cin_total + w_choff + ci] (+)= sum_{n,oy,ox} dy[n,oy,ox,co] * z[n, oy*s - pad + ky*d, ox*s - pad + kx*d, ci], tap by tap"""
    aff, relu = R.FORMS[op.form]
    z = x[:, :op.C].astype(np.float64).reshape(op.N, op.H, op.W, op.C)
    if aff:
        z = a.astype(np.float64) * z + b.astype(np.float64)
    if relu:
        z = np.maximum(z, 0.0)
    zp = np.zeros((op.N, op.H + 2 * op.pad, op.W + 2 * op.pad, op.C))
    zp[:, op.pad:op.pad + op.H, op.pad:op.pad + op.W] = z
    g = dy[:, :op.Cout].astype(np.float64).reshape(op.N, op.OH, op.OW, op.Cout)
    out = np.array(dw_init, dtype=np.float64)
    s, d = op.stride, op.dil
    for ky in range(op.k):
        for kx in range(op.k):
            win = zp[:, ky * d: ky * d + (op.OH - 1) * s + 1: s, kx * d: kx * d + (op.OW - 1) * s + 1: s]
            t = np.einsum('nyxo,nyxc->oc', g, win)
            c0 = (ky * op.k + kx) * op.cin_total + op.w_choff
            out[:, c0:c0 + op.C] = t + (out[:, c0:c0 + op.C] if op.accumulate else 0.0)
    return out


@pytest.mark.parametrize('form', range(4), ids=R.FORM_NAMES)
@pytest.mark.parametrize('name,shape,padded', TINY, ids=[t[0] for t in TINY])
def test_reference_equals_the_definition(name, shape, padded, form):
    """unfold + matmul against the tap-by-tap sum over explicitly zero-padded z, to fp64 rounding, in the layout the GPU test uses (w_choff = 8,
    cin_total = C + 12, ldw = taps * cin_total + 4), first touch and accumulating; nothing outside the slice moves."""
    Ci, Cout = shape[3], shape[4]
    for acc in (0, 1):
        op = R.make_op(shape, 77, Ci + 8 if padded else Ci, Cout + 4 if padded else Cout, form, acc)
        assert (op.w_choff, op.cin_total, op.ldw) == (8, Ci + 12, op.k * op.k * (Ci + 12) + 4)
        x, a, b, dy, dw0 = R.make_inputs(op)
        got = R.expected(op, R.reference(op), dw0)
        want = _direct(op, x, a, b, dy, dw0)
        assert R.rel_err(got, want) <= 1e-13, (name, acc, R.rel_err(got, want))
        m = R.slice_mask(op)
        assert m.sum() == op.Cout * op.k * op.k * op.C and np.array_equal(got[~m], dw0.astype(np.float64)[~m])


def test_guard_band_allocator():
    g = R.Guarded(100).fill_bits(R.FIRST_TOUCH_BITS)
    assert g.data.numel() == 100 and g.raw.numel() == 100 + 2 * R.GUARD and g.data.data_ptr() % 16 == 0
    assert bool(g.data.isnan().all()) and g.intact()
    g.data.fill_(1.0)
    assert g.intact()
    for i in (R.GUARD - 1, R.GUARD + 100):
        keep = int(g.raw[i])
        g.raw[i] = 0x7fc00000       # another NaN: the bits count, not the value
        assert not g.intact()
        g.raw[i] = keep
    assert g.intact()


@pytest.mark.parametrize('case', R.CASES, ids=[c[0] for c in R.CASES])
def test_bound_separates_right_from_subtly_wrong(case):
    """Each of five mistakes a kernel could make moves the reference by at least 50 x TOL in the GPU test's own error measure, on every
    case of make_wgrad_bits.CASES and every source form it applies to, so a kernel that makes one cannot pass.  (Measured over the 19
    cases: a dropped pixel >= 300 x TOL (stem0), padding before the affine >= 410 x TOL, no ReLU >= 4e4 x TOL.)"""
    floor = 50 * R.TOL
    worst = {}

    def hold(what, form, e):
        worst[what] = min(worst.get(what, e), e)
        assert e >= floor, '%s: %s in form %s moves the reference by %.2e only (< %.0e)' % (case[0], what, R.FORM_NAMES[form], e, floor)

    for form, (aff, relu) in enumerate(R.FORMS):
        op = R.case_op(case, form)
        x, a, b, dy, dw0 = R.make_inputs(op)
        ref = R.reference(op)
        # 1. the last output pixel of the last image is dropped
        hold('dropped pixel', form, R.rel_err(R.grad_fp64(op, x, a, b, dy, aff, relu, drop_last=True), ref))
        # 2. the affine (and ReLU) is applied to the zero padding instead of padding after it
        if aff and op.k > 1:
            hold('padding before the affine', form, R.rel_err(R.grad_fp64(op, x, a, b, dy, aff, relu, affine_on_padding=True), ref))
        # 3. the ReLU is omitted: the reference of the form without it
        if relu:
            hold('no ReLU', form, R.rel_err(R.reference(op._replace(form=form + 1)), ref))
        # 4. accumulate is ignored: the gradient alone where dw0 + gradient is due
        hold('accumulate ignored', form, R.rel_err(R.expected(op, ref, dw0, accumulate=0), R.expected(op, ref, dw0, accumulate=1)))
        # 5. the slice starts one channel late
        zero = np.zeros_like(dw0)
        hold('w_choff + 1', form, R.rel_err(R.expected(op, ref, zero, w_choff=op.w_choff + 1), R.expected(op, ref, zero)))
    print(case[0], ' '.join('%s %.1e' % kv for kv in sorted(worst.items())))
