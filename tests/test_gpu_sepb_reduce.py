"""GPU tests of the fused SepConv-half backward (csrc/sepb.hip) on the paths no other sep-backward test takes: ReLU off, the affine
absent, the (dA, dB) slab or the input gradient not asked for.  Every other test in the tree launches it with relu = 1 and a, b
present; the reductions of stage 2 (weight gradient over the 16 pixel lanes, fp64 (dA, dB) over the same lanes) and the masks they
feed on are shared by all of these paths.  Against fp64 autograd of y = pw(dw(act(a*x + b))) at the bound of
tests/test_gpu_fast_kernels.py, on the smallest maps that reach each tile form: R = 1 with a map smaller than a tile row, KG = 5, and
the smallest maps sep_choose puts on R = 2 (N * ceil(H/8) * ceil(W/16) >= 384: 12 x 32 tiles), with partial tiles on both edges."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5              # tests/test_gpu_fast_kernels.py: fp32 products with fp32 accumulation against the fp64 reference's max-abs
FAST_ALL = 31

SHAPES = [
    # name,        N,  H,   W,  C, k   variant <KS, KG, KP, R>
    ('c48_k5_r1',  1,  9,  11, 48, 5, [5, 3, 56, 1]),     # map smaller than a tile row
    ('c36_k3_r1',  1,  9,  11, 36, 3, [3, 3, 40, 1]),     # ... last group holds 4 of 16 channels
    ('c68_k5_kg5', 1, 33,  65, 68, 5, [5, 5, 72, 1]),     # KG = 5, last group 4 of 16
    ('c80_k3_kg5', 1, 33,  65, 80, 3, [3, 5, 88, 1]),
    ('c40_k5_r2',  1, 95, 509, 40, 5, [5, 3, 40, 2]),     # R = 2: 40-stride, last group 8 of 16
    ('c36_k3_r2',  1, 95, 509, 36, 3, [3, 3, 40, 2]),     # ... last group 4 of 16
    ('c44_k5_r2',  1, 95, 509, 44, 5, [5, 3, 56, 2]),     # ... 56-stride
]
MODES = [
    # name,           relu, affine, dab,   g
    ('relu_noaffine',    1, False,  True,  True),
    ('lin_affine',       0, True,   True,  True),
    ('lin_noaffine',     0, False,  True,  True),
    ('relu_affine_nodab', 1, True,  False, True),
    ('relu_affine_nog',  1, True,   True,  False),
]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    L.load().addk_set_fast_paths(FAST_ALL)
    yield L
    L.load().addk_set_fast_paths(FAST_ALL)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_sepb_reductions_match_fp64_autograd(lib, shape, mode):
    """dx (first touch and accumulate), the (dA, dB) sums and dw from the workspace rows against fp64 autograd; bit-identical run to
    run; the case runs the variant named."""
    L = lib
    lb = L.load()
    name, N, H, W, Cc, k, variant = shape
    mname, relu, affine, want_dab, want_g = mode
    dev = torch.device('cuda:0')
    gen = torch.Generator(device='cpu').manual_seed(23 + sum(map(ord, name + mname)))
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    P = N * H * W
    x, a, b = rnd(P, Cc), rnd(Cc), 0.3 * rnd(Cc)
    wdw, wpw, dy = 0.3 * rnd(Cc, k * k), 0.2 * rnd(Cc, Cc), rnd(P, Cc)
    g0 = rnd(P, Cc)
    # fp64 autograd; without the affine the kernel's (dA, dB) are the gradients at a = 1, b = 0
    xr = x.double().view(N, H, W, Cc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ar_ = (a.double() if affine else torch.ones(Cc, device=dev, dtype=torch.float64)).requires_grad_(True)
    br_ = (b.double() if affine else torch.zeros(Cc, device=dev, dtype=torch.float64)).requires_grad_(True)
    wd = wdw.double().view(Cc, 1, k, k).requires_grad_(True)
    z = ar_.view(1, -1, 1, 1) * xr + br_.view(1, -1, 1, 1)
    if relu:
        z = F.relu(z)
    y = F.conv2d(F.conv2d(z, wd, padding=k // 2, groups=Cc), wpw.double().view(Cc, Cc, 1, 1))
    y.backward(dy.double().view(N, H, W, Cc).permute(0, 3, 1, 2))
    flat = lambda v: v.permute(0, 2, 3, 1).reshape(P, Cc)
    ba = L.SepBwdArgs()
    ba.dy, ba.lddy, ba.N, ba.H, ba.W, ba.K = dy.data_ptr(), Cc, N, H, W, k
    ba.src.x, ba.src.ld, ba.src.C, ba.src.relu = x.data_ptr(), Cc, Cc, relu
    ba.src.a, ba.src.b = (a.data_ptr(), b.data_ptr()) if affine else (None, None)
    ba.Cout, ba.ldw, ba.dw_w, ba.pw_w = Cc, Cc, wdw.data_ptr(), wpw.data_ptr()
    rows = lb.addk_sep_bwd_rows(C.byref(ba))
    assert rows > 0
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for acc in (0, 1, 0):
        g = g0.clone() if acc else torch.full((P, Cc), float('nan'), device=dev)
        dab = torch.full((rows, Cc, 2), float('nan'), device=dev, dtype=torch.float64)
        ws = torch.full((rows, Cc, k * k), float('nan'), device=dev)
        ba.g, ba.ldg, ba.accumulate = (g.data_ptr() if want_g else None), Cc, acc
        ba.dab, ba.ws = (dab.data_ptr() if want_dab else None), ws.data_ptr()
        if not outs:
            cfg = (C.c_int32 * 8)()
            L.check(lb.addk_sep_bwd_config(C.byref(ba), cfg), 'sep_bwd_config')
            assert cfg[0] == 1 and [int(v) for v in cfg[1:5]] == variant, '%s runs %s, not %s' % (name, list(cfg[0:5]), variant)
        L.check(lb.addk_sep_bwd(C.byref(ba), st), 'sep_bwd')
        torch.cuda.synchronize()
        outs.append((g, dab, ws))
    bits = lambda v: v.view(torch.int64 if v.dtype == torch.float64 else torch.int32)      # a buffer not asked for stays NaN: compare bits
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(outs[0], outs[2])), 'not reproducible'
    gx = flat(xr.grad)
    errs = {'dw': _rel(outs[0][2].double().sum(0), wd.grad.view(Cc, k * k))}
    if want_g:
        errs['dx'] = _rel(outs[0][0], gx)
        errs['dx_acc'] = _rel(outs[1][0], gx + g0.double())
    else:                                    # no gradient asked for: the buffers of all three launches stay as they were
        assert bool(torch.isnan(outs[0][0]).all()) and torch.equal(outs[1][0], g0)
    if want_dab:
        errs['dab'] = _rel(outs[0][1].sum(0), torch.stack([ar_.grad, br_.grad], 1))
        errs['dab_acc'] = _rel(outs[1][1].sum(0), torch.stack([ar_.grad, br_.grad], 1))
    else:
        assert bool(torch.isnan(outs[0][1]).all())
    print(name, mname, ' '.join('%s %.2e' % kv for kv in errs.items()))
    bad = ['%s %.2e' % kv for kv in errs.items() if not kv[1] <= TOL]
    assert not bad, '%s %s beyond %.0e: %s' % (name, mname, TOL, ', '.join(bad))
