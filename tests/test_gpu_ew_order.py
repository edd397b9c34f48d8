"""The pinned arithmetic of the elementwise links of a cell block (csrc/elementwise.hip), bit for bit, through the C ABI.

affine_sum_bwd: the fp64 (dA, dB) slab rows against a numpy float64 evaluation in the order the file header of elementwise.hip states
 1. a thread's pixels ascend from row * npl + pl in steps of rows * npl (rows = addk_ew_rows(P, C) workgroups; a 256-thread workgroup
    is npl = 256 // nq pixel lanes of nq = ceil(C / 4) channel quads),
 2. each thread adds its pixels' terms in that order to a double that starts at 0,
 3. the workgroup adds its lanes pl = 0 .. npl-1 in that order to a double that starts at 0,
with dm * x the product of two floats, exact in double: the host result is exact, so every slab entry has to match it in every bit.
Each g[i] is compared bit for bit with numpy float32 (dm * a, + the old g when accumulating).  A ReLU mask is decided by the sign of
fmaf(a, x, b); the host takes the sign of a*x + b in double (a*x is exact there, and the sum cannot round across zero).

affine_sum_fwd: the vector-aligned and the generic kernel give the same bits (the generic one is forced by one term's x starting one
float past a 16-byte boundary).  bn_bwd_apply, in place: single launch, batch table and generic kernel give the same bits.

Shapes are the smallest that reach every path: two workgroups with threads of 3 and 2 pixels and an odd last trip (131, 40), npl = 1
(C = 1024), npl = 256 (C = 4), the 64 KB reduction panel (4 terms at C = 4 and C = 1024), C = 36 through both kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import addk  # noqa: F401  (registers the package)
from addk import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _rows_of(t, P, Cc, ld, misalign=0):
    """The [P][Cc] host array `t` in a NaN-filled device buffer of row stride ld, starting `misalign` floats past a 16-byte boundary.
    Returns (buffer, view)."""
    buf = _nan(P * ld + 4)
    view = buf[misalign:misalign + P * ld].view(P, ld)[:, :Cc]
    view.copy_(_dev(t))
    return buf, view


def _src(view, a=None, b=None, relu=0):
    s = L.Src()
    s.x, s.a, s.b = view.data_ptr(), (a.data_ptr() if a is not None else None), (b.data_ptr() if b is not None else None)
    s.ld, s.C, s.relu, s.rs_hw = view.stride(0), view.shape[1], int(relu), 0
    return s


def _same_bits(what, got, ref):
    got = got.detach().cpu().contiguous().numpy() if isinstance(got, torch.Tensor) else np.ascontiguousarray(got)
    ref = np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, '%s: %s %s vs %s %s' % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    iv = np.int64 if got.dtype == np.float64 else np.int32
    bad = got.view(iv) != ref.view(iv)
    n = int(bad.sum())
    if n:
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError('%s: %d of %d elements differ in bits (first: flat index %d, got %r, expected %r)'
                             % (what, n, bad.size, k, got.reshape(-1)[k], ref.reshape(-1)[k]))


def _ew_map(Cc):
    nq = min(256, (Cc + 3) // 4)
    return nq, max(1, 256 // nq)


# ------------------------------------------------------------------------------------------------------------------------------------
# affine_sum_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
def _slab_in_order(dm, x, rows, npl):
    """[rows][C][2] float64: (sum dm*x, sum dm) of the float32 arrays dm, x [P][C] in the order of the module docstring."""
    P, Cc = dm.shape
    step = rows * npl
    trips = -(-P // step)
    t = np.zeros((trips * step, Cc, 2), np.float64)
    t[:P, :, 0] = dm.astype(np.float64) * x.astype(np.float64)
    t[:P, :, 1] = dm
    t = t.reshape(trips, rows, npl, Cc, 2)               # pixel = trip * step + row * npl + pl
    lane = np.zeros((rows, npl, Cc, 2), np.float64)
    for k in range(trips):                               # a pixel past P adds +0.0 to a sum that is never -0.0: no bit moves
        lane = lane + t[k]
    out = np.zeros((rows, Cc, 2), np.float64)
    for pl in range(npl):
        out = out + lane[:, pl]
    return out


# (term count, indices of the terms with ReLU, relu_out, per term: 'g' gradient, 'd' dab slab, 'a' accumulate into g)
BWD_CFGS = [
    (1, (), 0, ['gd']),
    (2, (1,), 1, ['gd', 'gda']),
    (3, (0,), 0, ['d', 'g', 'gd']),
    (4, (2,), 1, ['gd', 'gda', 'd', 'g']),
    (2, (), 0, ['', 'gd']),                              # a term nobody wants a gradient of
]
# (P, C, row stride of the terms' x: C = the vector kernel, C + 1 = the generic one)
BWD_SHAPES = [(131, 40, 40), (37, 160, 160), (5, 1024, 1024), (600, 4, 4), (23, 80, 80), (131, 36, 36), (131, 36, 37)]


@pytest.mark.parametrize('cfg', range(len(BWD_CFGS)))
@pytest.mark.parametrize('P,Cc,ldx', BWD_SHAPES)
def test_affine_sum_bwd_sums_in_the_pinned_order(lib, P, Cc, ldx, cfg):
    nterm, relu_terms, relu_out, spec = BWD_CFGS[cfg]
    rng = np.random.default_rng(1000 * cfg + P + Cc + ldx)
    f32 = np.float32
    rows = int(lib.addk_ew_rows(P, Cc))
    nq, npl = _ew_map(Cc)
    assert rows == min(1024, max(1, P // (2 * npl)))
    dout = rng.standard_normal((P, Cc)).astype(f32)
    fout = rng.standard_normal((P, Cc)).astype(f32)
    fout[rng.random((P, Cc)) < 0.1] = 0.0                # relu_out masks where !(out > 0): zeros count as masked
    keep = []
    _, dout_d = _rows_of(dout, P, Cc, Cc + 4)
    _, fout_d = _rows_of(fout, P, Cc, Cc)
    ba = L.AffineSumBwdArgs()
    expect = []
    d = np.where(fout > 0, dout, f32(0)) if relu_out else dout
    for i in range(nterm):
        x = (rng.standard_normal((P, Cc)) + 0.2).astype(f32)
        lazy = i != 1 or nterm == 1                      # the second term is a plain one (a = b = NULL)
        a = ((0.5 + rng.random(Cc)) * rng.choice([-1.0, 1.0], Cc)).astype(f32) if lazy else None
        b = (0.3 * rng.standard_normal(Cc)).astype(f32) if lazy else None
        relu = i in relu_terms
        a_d, b_d = (_dev(a), _dev(b)) if lazy else (None, None)
        xbuf, x_d = _rows_of(x, P, Cc, ldx)
        keep += [a_d, b_d, xbuf]
        ba.term[i] = _src(x_d, a_d, b_d, relu)
        dm = d
        if relu:
            z = (a.astype(np.float64) * x.astype(np.float64) + b.astype(np.float64)) if lazy else x.astype(np.float64)
            dm = np.where(z > 0, d, f32(0))
        g_d = gbuf = g_ref = dab_d = None
        if 'g' in spec[i]:
            g_ref = dm * a if lazy else dm * f32(1)
            if 'a' in spec[i]:
                old = rng.standard_normal((P, Cc)).astype(f32)
                gbuf, g_d = _rows_of(old, P, Cc, Cc + 4)
                g_ref = g_ref + old
            else:
                gbuf = _nan(P * (Cc + 4) + 4)
                g_d = gbuf[:P * (Cc + 4)].view(P, Cc + 4)[:, :Cc]
            ba.g[i], ba.ldg[i], ba.accumulate[i] = g_d.data_ptr(), g_d.stride(0), int('a' in spec[i])
        if 'd' in spec[i]:
            dab_d = _nan(rows, Cc, 2, dtype=torch.float64)
            ba.dab[i] = dab_d.data_ptr()
        expect.append((g_d, gbuf, g_ref, dab_d, _slab_in_order(dm, x, rows, npl) if dab_d is not None else None))
    ba.nterm, ba.P, ba.C, ba.dout, ba.lddo = nterm, P, Cc, dout_d.data_ptr(), dout_d.stride(0)
    ba.out, ba.ldo, ba.relu_out = fout_d.data_ptr(), fout_d.stride(0), int(relu_out)
    L.check(lib.addk_affine_sum_bwd(C.byref(ba), _st()), 'affine_sum_bwd')
    torch.cuda.synchronize()
    tag = 'P=%d C=%d ldx=%d nterm=%d relu_out=%d' % (P, Cc, ldx, nterm, relu_out)
    for i, (g_d, gbuf, g_ref, dab_d, dab_ref) in enumerate(expect):
        if g_d is not None:
            _same_bits('%s g[%d]' % (tag, i), g_d, g_ref.astype(f32))
            pad = gbuf[:P * (Cc + 4)].view(P, Cc + 4)[:, Cc:]
            if 'a' not in spec[i]:
                assert torch.isnan(pad).all(), '%s: g[%d] written past C' % (tag, i)
        if dab_d is not None:
            _same_bits('%s dab[%d] (%d rows)' % (tag, i, rows), dab_d, dab_ref)


# ------------------------------------------------------------------------------------------------------------------------------------
# affine_sum_fwd: vector-aligned form == generic form
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate,relu_out', [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('nterm', [1, 2, 3, 4])
@pytest.mark.parametrize('P,Cc', [(131, 40), (9, 160), (3, 1024)])
def test_affine_sum_fwd_vector_and_generic_kernels_agree(lib, P, Cc, nterm, accumulate, relu_out):
    rng = np.random.default_rng(7 * P + Cc + 100 * nterm + 10 * accumulate + relu_out)
    f32 = np.float32
    terms = []
    for i in range(nterm):
        lazy = i != 1
        terms.append(((rng.standard_normal((P, Cc)) + 0.2).astype(f32),
                      _dev(((0.5 + rng.random(Cc)) * rng.choice([-1.0, 1.0], Cc)).astype(f32)) if lazy else None,
                      _dev((0.3 * rng.standard_normal(Cc)).astype(f32)) if lazy else None, i % 2 == 0 and i > 0))
    old = rng.standard_normal((P, Cc)).astype(f32)
    outs = []
    for misalign in (0, 1):                              # 1: term 0 starts one float past a 16-byte boundary -> the generic kernel
        keep = []
        ar = L.AffineSumArgs()
        for i, (x, a, b, relu) in enumerate(terms):
            xbuf, x_d = _rows_of(x, P, Cc, Cc, misalign if i == 0 else 0)
            keep.append(xbuf)
            ar.term[i] = _src(x_d, a, b, relu)
        assert (ar.term[0].x % 16 != 0) == bool(misalign)
        ldo = 3 * Cc                                     # a slot of a concat buffer
        obuf = _nan(P, ldo)
        out = obuf[:, Cc:2 * Cc]
        if accumulate:
            out.copy_(_dev(old))
        ar.nterm, ar.P, ar.C, ar.out, ar.ldo, ar.relu_out, ar.accumulate = nterm, P, Cc, out.data_ptr(), ldo, relu_out, accumulate
        L.check(lib.addk_affine_sum_fwd(C.byref(ar), _st()), 'affine_sum_fwd')
        torch.cuda.synchronize()
        assert not torch.isnan(out).any(), 'affine_sum_fwd left elements unwritten'
        assert torch.isnan(obuf[:, :Cc]).all() and torch.isnan(obuf[:, 2 * Cc:]).all(), 'affine_sum_fwd wrote outside its slot'
        outs.append(out.cpu().numpy().copy())
    _same_bits('affine_sum_fwd generic == vector P=%d C=%d nterm=%d acc=%d relu_out=%d' % (P, Cc, nterm, accumulate, relu_out), outs[1], outs[0])


# ------------------------------------------------------------------------------------------------------------------------------------
# bn_bwd_apply, in place: single == batch == generic
# ------------------------------------------------------------------------------------------------------------------------------------
def _apply_case(rng, P, Cc):
    f32 = np.float32
    return dict(P=P, C=Cc, g=rng.standard_normal((P, Cc)).astype(f32), x=(rng.standard_normal((P, Cc)) + 0.5).astype(f32),
                mean=_dev(rng.standard_normal(Cc).astype(f32)), c1=_dev((0.5 * rng.standard_normal(Cc)).astype(f32)),
                c2=_dev((0.5 * rng.standard_normal(Cc)).astype(f32)))


def _apply_single(lib, c, ld):
    """In place on a copy of g with row stride ld (ld = C: the vector kernel; C + 1: the generic one)."""
    P, Cc = c['P'], c['C']
    gbuf, g_d = _rows_of(c['g'], P, Cc, ld)
    xbuf, x_d = _rows_of(c['x'], P, Cc, ld)
    it = L.BnApplyItem()
    it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = g_d.data_ptr(), x_d.data_ptr(), c['c1'].data_ptr(), c['c2'].data_ptr(), c['mean'].data_ptr(), g_d.data_ptr(), P
    it.ldg, it.ldx, it.ldo, it.C = ld, ld, ld, Cc
    L.check(lib.addk_bn_bwd_apply(C.byref(it), _st()), 'bn_bwd_apply')
    torch.cuda.synchronize()
    if ld > Cc:
        assert torch.isnan(gbuf[:P * ld].view(P, ld)[:, Cc:]).all(), 'bn_bwd_apply wrote past C'
    return g_d.cpu().numpy().copy()


def _apply_batch(lib, cases):
    items, keep = [], []
    for c in cases:
        P, Cc = c['P'], c['C']
        gbuf, g_d = _rows_of(c['g'], P, Cc, Cc)
        xbuf, x_d = _rows_of(c['x'], P, Cc, Cc)
        it = L.BnApplyItem()
        it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = g_d.data_ptr(), x_d.data_ptr(), c['c1'].data_ptr(), c['c2'].data_ptr(), c['mean'].data_ptr(), g_d.data_ptr(), P
        it.ldg, it.ldx, it.ldo, it.C = Cc, Cc, Cc, Cc
        items.append(it)
        keep.append((gbuf, xbuf, g_d))
    arr = (L.BnApplyItem * len(items))(*items)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    L.check(lib.addk_bn_bwd_apply_batch(tab.data_ptr(), len(items), max(c['P'] for c in cases), _st()), 'bn_bwd_apply_batch')
    torch.cuda.synchronize()
    return [k[2].cpu().numpy().copy() for k in keep]


def test_bn_bwd_apply_in_place_single_batch_and_generic_agree(lib):
    rng = np.random.default_rng(5)
    cases = [_apply_case(rng, P, Cc) for P, Cc in [(1, 4), (51, 40), (4099, 40), (13, 256)]]
    singles = [_apply_single(lib, c, c['C']) for c in cases]
    for c, s in zip(cases, singles):
        assert not np.isnan(s).any(), 'bn_bwd_apply left elements unwritten'
        _same_bits('bn_bwd_apply generic == vector P=%d C=%d' % (c['P'], c['C']), _apply_single(lib, c, c['C'] + 1), s)
    for c, s, b in zip(cases, singles, _apply_batch(lib, cases)):
        _same_bits('bn_bwd_apply batch == single P=%d C=%d' % (c['P'], c['C']), b, s)
    for c, s, b in zip(cases, singles, [_apply_batch(lib, [c])[0] for c in cases]):      # each alone: the grid sized by its own P
        _same_bits('bn_bwd_apply batch of one == single P=%d C=%d' % (c['P'], c['C']), b, s)


def test_bn_bwd_apply_batch_of_mixed_sizes(lib):
    """Items of P = 7 and P = 4099 and of C = 40 and C = 160 in one table (the grid is sized by the largest P)."""
    rng = np.random.default_rng(6)
    cases = [_apply_case(rng, P, Cc) for P, Cc in [(7, 40), (4099, 160), (4099, 40), (7, 160)]]
    for c, b in zip(cases, _apply_batch(lib, cases)):
        _same_bits('bn_bwd_apply mixed batch == single P=%d C=%d' % (c['P'], c['C']), b, _apply_single(lib, c, c['C']))
