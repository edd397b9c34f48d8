"""GPU tests of online hard example mining in the fused loss head: addk_ohem_select (per-pixel loss map, exact radix select of tau, kept
counts and weight sum), addk_ce_upsample_ohem_fwd_bwd (the loss head that reads the kept set) and train.TrainStep(ohem=...)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle                                                   # noqa: E402
import _ohem_ref as R                                           # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor, rel_err   # noqa: E402

N, LD, NC = 2, 24, 19
SHAPES = {'x8': ((16, 32), (128, 256)), 'x3.8': ((17, 33), (65, 129)), 'x1': ((33, 65), (33, 65))}
# regimes of tau = min(-log theta, l_(min(K, n))): (thresh, K as a function of the valid count n).  With logits rand * 3 over 19 classes
# three quarters of the pixels have a target probability below 0.05, so `quarter` (thresh 0.05, K = n / 4) still ends on -log theta; `k`
# asks for more pixels than the threshold passes (K = 0.9 n) and ends on the K-th largest loss.
REGIMES = {'quarter': (0.05, lambda n: n // 4), 'k': (0.05, lambda n: 9 * n // 10), 'theta': (0.7, lambda n: 16), 'all': (0.05, lambda n: n + 1000)}
MASKED = {'k': (0.05, lambda n: 9 * n // 10), 'half': (0.01, lambda n: n // 2), 'theta': (0.05, lambda n: n // 4)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _inputs(lo_hw, hi_hw):
    x = rand_tensor(31, 'ohem_x', (N,) + lo_hw + (NC,)) * 3
    r = np.random.default_rng(9)
    t = torch.from_numpy(r.integers(0, NC, (N,) + hi_hw)).long()
    t[torch.from_numpy(r.random((N,) + hi_hw) < 0.05)] = 255
    return x, t


_CACHE = {}


def _case(name):
    """inputs of a shape and its fp64 / fp32 loss maps, computed once and left unchanged"""
    if name not in _CACHE:
        lo_hw, hi_hw = SHAPES[name]
        x, t = _inputs(lo_hw, hi_hw)
        l64 = R.reference(x, t, hi_hw, 1.0, 1, dtype=torch.float64)['l']
        l32 = R.reference(x, t, hi_hw, 1.0, 1, dtype=torch.float32)['l']
        valid = l64 >= 0
        e32 = float((l32.double() - l64)[valid].abs().max())
        bound = max(4 * e32, 1e-6 * float(l64.max()))
        _CACHE[name] = dict(x=x, t=t, lo_hw=lo_hw, hi_hw=hi_hw, l64=l64, valid=valid, e32=e32, bound=bound)
    return _CACHE[name]


def _padded(x, dev):
    xa = torch.zeros(x.shape[:3] + (LD,), device=dev)
    xa[..., :NC] = x.to(dev)
    return xa


def _select(dev, xa, ta, lo_hw, hi_hw, thresh, K, wa=None, ignore=255):
    """one addk_ohem_select launch sequence; returns (map, tau, wsum_kept, counts) on the device"""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = lo_hw, hi_hw
    assert lib.addk_ohem_select_supported(N, H, W, OH, OW, NC) == 1
    lmap = torch.full((N, OH, OW), float('nan'), device=dev)
    tau, wk = torch.full((1,), float('nan'), device=dev), torch.full((1,), float('nan'), device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    # the workspace starts dirty: the launch sequence clears what it needs itself
    ws = torch.full((int(lib.addk_ohem_select_ws_bytes(N, OH, OW)),), 0x5a, dtype=torch.uint8, device=dev)
    a = L.OhemSelectArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), LD, N, H, W, NC, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, ignore
    a.thresh, a.min_kept_total = thresh, K
    a.pix_loss, a.tau, a.wsum_kept, a.counts, a.ws = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr(), ws.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.addk_ohem_select(C.byref(a), st))
    L.check(lib.addk_ohem_select(C.byref(a), st))          # a second call on the used workspace leaves the same result
    torch.cuda.synchronize()
    return lmap, tau, wk, counts


def _head(dev, xa, ta, lo_hw, hi_hw, wa, g0, acc, scale, wsum, lmap=None, tau=None):
    """the plain loss head, or the mining head when (lmap, tau) are given; returns (loss, g) on the host"""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = lo_hw, hi_hw
    loss = torch.full((1,), 0.25, device=dev)
    g = g0.clone().to(dev)
    ws = torch.zeros(int(lib.addk_ce_upsample_ws_floats(N, H, W)), device=dev)
    b = L.CeUpsampleOhemArgs()
    a = b.ce
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), LD, N, H, W, NC, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.wsum, a.scale, a.loss_out = wsum.data_ptr(), scale, loss.data_ptr()
    a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), LD, acc, ws.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    if lmap is None:
        L.check(lib.addk_ce_upsample_fwd_bwd(C.byref(a), st))
    else:
        b.pix_loss, b.tau = lmap.data_ptr(), tau.data_ptr()
        L.check(lib.addk_ce_upsample_ohem_fwd_bwd(C.byref(b), st))
    torch.cuda.synchronize()
    return loss.cpu(), g.cpu()


@pytest.mark.parametrize('shape', list(SHAPES))
def test_loss_map_matches_fp64_reference(dev, shape):
    """1. the stored map against fp64: within 4 x the error of the fp32 torch reference (floor 1e-6 * max l); invalid pixels are exactly -1.
    Measured on the MI355X (device error / fp32 torch error): see DESIGN.md, 'Online hard example mining'."""
    c = _case(shape)
    lmap, _, _, _ = _select(dev, _padded(c['x'], dev), c['t'].to(dev), c['lo_hw'], c['hi_hw'], 0.7, 16)
    lm = lmap.cpu()
    assert torch.equal(lm[~c['valid']], torch.full_like(lm[~c['valid']], -1.0))
    err = float((lm.double() - c['l64'])[c['valid']].abs().max())
    print('ohem loss map %s: device error %.3e, fp32 torch error %.3e (ratio %.2f), bound %.3e' % (shape, err, c['e32'], err / c['e32'], c['bound']))
    assert float(lm[c['valid']].min()) >= 0.0
    assert err <= c['bound'], (err, c['bound'])


@pytest.mark.parametrize('ignored_image', [False, True], ids=['mixed', 'one_image_ignored'])
@pytest.mark.parametrize('regime', list(REGIMES))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_selection_is_exact(dev, shape, regime, ignored_image):
    """2. tau and the counts against torch.sort of the very floats the device stored: equal with ==."""
    c = _case(shape)
    t = c['t'].clone()
    if ignored_image:
        t[1] = 255
    nvalid = int((t != 255).sum())
    thresh, kf = REGIMES[regime]
    K = kf(nvalid)
    lmap, tau, wk, counts = _select(dev, _padded(c['x'], dev), t.to(dev), c['lo_hw'], c['hi_hw'], thresh, K)
    lm = lmap.cpu()
    vals = lm[lm >= 0]
    tau_h, kept_h = R.select_tau(vals, thresh, K)
    assert int(counts[0]) == nvalid == vals.numel()
    assert float(tau) == tau_h, (float(tau), tau_h)
    assert int(counts[1]) == kept_h
    assert kept_h >= min(K, nvalid)
    assert float(wk) == float(kept_h)                               # no class weights, below 2^24: the sum of ones is exact
    if regime == 'k':
        assert tau_h < R.tau_theta(thresh) and K <= kept_h < nvalid and tau_h == float(torch.sort(vals).values[nvalid - K])
    elif regime in ('theta', 'quarter'):
        assert tau_h == R.tau_theta(thresh) and K < kept_h < nvalid
    else:
        assert kept_h == nvalid and tau_h == float(vals.min())
    if ignored_image:
        assert torch.equal(lm[1], torch.full_like(lm[1], -1.0))


def test_selection_with_no_valid_pixel(dev):
    """n == 0: tau = -log theta, nothing kept, zero weight sum."""
    c = _case('x1')
    t = torch.full_like(c['t'], 255)
    lmap, tau, wk, counts = _select(dev, _padded(c['x'], dev), t.to(dev), c['lo_hw'], c['hi_hw'], 0.7, 100)
    assert float(tau) == R.tau_theta(0.7) and counts.tolist() == [0, 0] and float(wk) == 0.0
    assert torch.equal(lmap.cpu(), torch.full((N,) + c['hi_hw'], -1.0))


def test_ties_at_tau_are_all_kept(dev):
    """3. at x1 the interpolation weights are exactly 1 and 0: 500 copies of one pixel carry one bit pattern; with tau on it, all are kept."""
    c = _case('x1')
    OH, OW = c['hi_hw']
    x, t = c['x'].clone(), c['t'].clone()
    l0 = c['l64'].reshape(-1)
    src = int(torch.argsort(l0)[l0.numel() // 2])                    # a valid pixel of median loss (invalid ones carry -1: the low end)
    assert l0[src] >= 0 and l0[src] < R.tau_theta(0.001)
    pos = torch.from_numpy(np.random.default_rng(3).permutation(N * OH * OW)[:500])
    pos[0] = src
    x.reshape(-1, NC)[pos] = x.reshape(-1, NC)[src].clone()
    t.reshape(-1)[pos] = int(t.reshape(-1)[src])
    xa, ta = _padded(x, dev), t.to(dev)
    lm = _select(dev, xa, ta, c['lo_hw'], c['hi_hw'], 0.001, 1)[0].cpu().reshape(-1)
    v = lm[src]
    assert torch.equal(lm[pos], v.expand(500))
    above = int((lm > v).sum())
    K = above + 250
    lmap, tau, _, counts = _select(dev, xa, ta, c['lo_hw'], c['hi_hw'], 0.001, K)
    assert float(tau) == float(v)
    ties = int((lm == v).sum())
    assert ties >= 500 and int(counts[1]) == above + ties > K
    assert bool((lmap.cpu().reshape(-1)[pos] >= float(tau)).all())


@pytest.mark.parametrize('regime', list(MASKED))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_mask_against_fp64(dev, shape, regime):
    """4. device mask and fp64 mask differ only on pixels whose fp64 loss lies within the bound of (1) of the fp64 tau: at most 0.1 % of the
    valid pixels.  With these seeded inputs the fp32 torch reference's mask differs from the fp64 one on no pixel (CPU, the three shapes
    in all three regimes; at most 3 valid pixels lie within the bound of tau)."""
    c = _case(shape)
    nvalid = int(c['valid'].sum())
    thresh, K = MASKED[regime][0], MASKED[regime][1](nvalid)
    lmap, tau, _, _ = _select(dev, _padded(c['x'], dev), c['t'].to(dev), c['lo_hw'], c['hi_hw'], thresh, K)
    mdev = lmap.cpu() >= float(tau)
    r64 = R.reference(c['x'], c['t'], c['hi_hw'], thresh, K, dtype=torch.float64)
    diff = mdev != r64['mask']
    near = (c['l64'] - r64['tau']).abs() <= c['bound']
    print('ohem mask %s %s: %d of %d valid pixels differ from fp64' % (shape, regime, int(diff.sum()), nvalid))
    assert not bool((diff & ~near).any())
    assert int(diff.sum()) <= 1e-3 * nvalid


@pytest.mark.parametrize('shape', list(SHAPES))
def test_loss_and_gradient_with_device_mask(dev, shape):
    """5. loss and gradient of the mining head against the reference on the DEVICE's mask: the plain head's bounds (tests/test_gpu_train.py),
    with and without class weights, accumulate 0 / 1, padding channels untouched, two runs bit-equal."""
    c = _case(shape)
    lo_hw, hi_hw = c['lo_hw'], c['hi_hw']
    nvalid = int(c['valid'].sum())
    thresh, K = MASKED['half'][0], MASKED['half'][1](nvalid)          # tau is the median loss: half of the weights are zeroed
    w = torch.rand(NC, generator=torch.Generator().manual_seed(4)) + 0.5
    g0 = rand_tensor(32, 'ohem_g0', (N,) + lo_hw + (LD,))
    xa, ta = _padded(c['x'], dev), c['t'].to(dev)
    for weight, acc in ((None, 0), (w, 1)):
        wa = weight.to(dev) if weight is not None else None
        lmap, tau, wk, counts = _select(dev, xa, ta, lo_hw, hi_hw, thresh, K, wa)
        mask = lmap.cpu() >= float(tau)
        assert int(mask.sum()) == int(counts[1])
        r64 = R.reference(c['x'], c['t'], hi_hw, thresh, K, weight, dtype=torch.float64, mask=mask, scale=0.5)
        r32 = R.reference(c['x'], c['t'], hi_hw, thresh, K, weight, dtype=torch.float32, mask=mask, scale=0.5)
        wsum64 = float((weight.double()[c['t'][mask]] if weight is not None else torch.ones(int(mask.sum()), dtype=torch.float64)).sum())
        assert abs(float(wk) - wsum64) <= 2e-6 * wsum64
        res = [_head(dev, xa, ta, lo_hw, hi_hw, wa, g0, acc, 0.5, wk, lmap, tau) for _ in range(2)]
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])        # deterministic
        la, ga = res[0]
        assert abs(float(la) - 0.25 - r64['loss']) <= 2e-6 * abs(r64['loss']), (float(la) - 0.25, r64['loss'])
        base = g0[..., :NC].double() if acc else 0
        assert rel_err(ga[..., :NC].double(), r64['grad'] + base) <= 5e-5
        assert rel_err(ga[..., :NC].double(), r32['grad'].double() + base) <= 1e-5
        assert torch.equal(ga[..., NC:], g0[..., NC:])                                         # padding channels untouched


@pytest.mark.parametrize('shape', list(SHAPES))
def test_keep_all_equals_plain_head(dev, shape):
    """6. thresh = 1: tau = 0, every valid pixel is kept and the mining head is the plain head."""
    import addk._lib as L
    lib = L.load()
    c = _case(shape)
    lo_hw, hi_hw = c['lo_hw'], c['hi_hw']
    OH, OW = hi_hw
    w = torch.rand(NC, generator=torch.Generator().manual_seed(4)) + 0.5
    g0 = rand_tensor(32, 'ohem_g0', (N,) + lo_hw + (LD,))
    xa, ta = _padded(c['x'], dev), c['t'].to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for weight, acc in ((None, 0), (w, 1)):
        wa = weight.to(dev) if weight is not None else None
        wsum = torch.zeros(1, device=dev); ws1 = torch.zeros(int(lib.addk_ce_ws_floats(N, OH * OW)), device=dev)
        L.check(lib.addk_ce_count(ta.data_ptr(), N * OH * OW, wa.data_ptr() if wa is not None else None, 255, NC, wsum.data_ptr(), ws1.data_ptr(), st))
        lp, gp = _head(dev, xa, ta, lo_hw, hi_hw, wa, g0, acc, 0.5, wsum)
        lmap, tau, wk, counts = _select(dev, xa, ta, lo_hw, hi_hw, 1.0, 1, wa)
        assert float(tau) == 0.0 and int(counts[0]) == int(counts[1]) == int(c['valid'].sum())
        lo, go = _head(dev, xa, ta, lo_hw, hi_hw, wa, g0, acc, 0.5, wk, lmap, tau)
        assert abs(float(lo) - float(lp)) <= 2e-6 * abs(float(lp) - 0.25)
        assert rel_err(go[..., :NC], gp[..., :NC]) <= 1e-6
        assert torch.equal(go[..., NC:], g0[..., NC:])


def test_bad_arguments_are_refused_without_a_launch(dev):
    import addk._lib as L
    lib = L.load()
    c = _case('x1')
    (H, W), (OH, OW) = c['lo_hw'], c['hi_hw']
    xa, ta = _padded(c['x'], dev), c['t'].to(dev)
    lmap = torch.full((N, OH, OW), 7.0, device=dev)
    tau, wk = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.addk_ohem_select_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def args(**kw):
        a = L.OhemSelectArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), LD, N, H, W, NC, OH, OW
        a.target, a.class_w, a.ignore_index, a.thresh, a.min_kept_total = ta.data_ptr(), None, 255, 0.7, 16
        a.pix_loss, a.tau, a.wsum_kept, a.counts, a.ws = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr(), ws.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bad = [dict(thresh=0.0), dict(thresh=1.5), dict(thresh=float('nan')), dict(min_kept_total=0), dict(ld=18), dict(C=7), dict(logits=None),
           dict(target=None), dict(pix_loss=None), dict(tau=None), dict(wsum_kept=None), dict(counts=None), dict(ws=None)]
    for kw in bad:
        assert lib.addk_ohem_select(C.byref(args(**kw)), st) == -1, kw
    g = torch.full((N, H, W, LD), 7.0, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    hws = torch.zeros(int(lib.addk_ce_upsample_ws_floats(N, H, W)), device=dev)

    def hargs(**kw):
        b = L.CeUpsampleOhemArgs()
        a = b.ce
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), LD, N, H, W, NC, OH, OW
        a.target, a.class_w, a.ignore_index, a.wsum, a.scale, a.loss_out = ta.data_ptr(), None, 255, wk.data_ptr(), 0.5, loss.data_ptr()
        a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), LD, 0, hws.data_ptr()
        b.pix_loss, b.tau = lmap.data_ptr(), tau.data_ptr()
        for k, v in kw.items():
            setattr(b if k in ('pix_loss', 'tau') else a, k, v)
        return b
    for kw in (dict(pix_loss=None), dict(tau=None), dict(ld=18), dict(wsum=None), dict(g=None), dict(C=7)):
        assert lib.addk_ce_upsample_ohem_fwd_bwd(C.byref(hargs(**kw)), st) == -1, kw
    torch.cuda.synchronize()
    assert float(lmap.min()) == float(lmap.max()) == 7.0 and float(tau) == float(wk) == float(loss) == 7.0 and counts.tolist() == [-7, -7]
    assert float(g.min()) == float(g.max()) == 7.0
    assert lib.addk_ohem_select_supported(N, H, W, OH, OW, 7) == 0 and lib.addk_ohem_select_supported(N, H, W, OH, OW, NC) == 1


# ---- 7. the training step ------------------------------------------------------------------------------------------------------

def _model(dev, seed=600):
    from addk.modeling.ADD import ADD
    args = (ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), 0)
    mo = oracle.ADD(*args)
    fill_params(mo, seed)
    ma = ADD(*args)
    ma.load_state_dict(mo.state_dict())
    return ma.to(dev)


def _batch(hw, seed=5):
    x = rand_tensor(seed, 'ts_x', (2, 3) + hw)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, 19, (2,) + hw)).long()
    t[torch.from_numpy(r.random((2,) + hw) < 0.05)] = 255
    return x, t


SHAPE = (2, 3, 65, 129)


def _fwd_bwd(dev, ohem):
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:])
    ts = TrainStep(_model(dev), SHAPE, use_graph=False, ohem=ohem)
    ts.load_batch(x.to(dev), t.to(dev))
    ts.forward_backward_only()
    torch.cuda.synchronize()
    return ts, int((t != 255).sum())


@pytest.fixture(scope='module')
def plain_step(dev):
    ts, _ = _fwd_bwd(dev, None)
    return ts.loss.item(), ts.flat_g.clone()


def test_step_mines_hard_examples(dev, plain_step):
    ts, nvalid = _fwd_bwd(dev, (0.7, 2000))
    names = [c.name for c in ts.g.bwd]
    assert names.count('ohem_select') == names.count('ce_upsample_ohem') == 2 and 'ce_upsample' not in names
    stats = ts.ohem_stats()
    assert len(stats) == 2
    for tau, kept, valid in stats:
        assert valid == nvalid and min(2000 * 2, valid) <= kept <= valid and 0.0 <= tau <= R.tau_theta(0.7)
    assert ts.loss.item() >= plain_step[0]                        # the mean over a top subset is not below the mean
    assert torch.isfinite(ts.flat_g).all()


def test_step_keep_all_equals_plain_step(dev, plain_step):
    ts, nvalid = _fwd_bwd(dev, (1.0, 2000))
    assert all(kept == valid == nvalid and tau == 0.0 for tau, kept, valid in ts.ohem_stats())
    assert abs(ts.loss.item() - plain_step[0]) <= 2e-6 * abs(plain_step[0])
    assert rel_err(ts.flat_g, plain_step[1]) <= 2e-4


def test_step_replayed_graph_equals_eager(dev):
    """After enable_capture() the step is one hipGraph; three replayed steps give the loss and parameters of three eager steps, bit for bit."""
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:])
    res = {}
    for mode in ('eager', 'graph'):
        ts = TrainStep(_model(dev), SHAPE, use_graph=False, ohem=(0.7, 2000))
        ts.load_batch(x.to(dev), t.to(dev))
        if mode == 'graph':
            ts.enable_capture()
        ls = [ts.step().item() for _ in range(4)]                  # graph: one eager step that is then captured, three replays
        torch.cuda.synchronize()
        assert (ts.graph is not None) == (mode == 'graph')
        res[mode] = (ls, ts.flat_p.clone(), ts.ohem_stats())
        ts.close()
    assert res['graph'][0] == res['eager'][0], (res['graph'][0], res['eager'][0])
    assert torch.equal(res['graph'][1], res['eager'][1])
    assert res['graph'][2] == res['eager'][2]
