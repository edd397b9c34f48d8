"""GPU tests of self-distillation from the final exit in the fused loss head: addk_ce_upsample_kd_fwd_bwd (cross-entropy + KL divergence
from a teacher's low-resolution logits, straight from the low-resolution maps) and train.TrainStep(distill=...).

Bounds of the kernel tests: the plain head's (tests/test_gpu_train.py: loss 2e-6 relative to fp64; gradient rel_err 5e-5 against fp64 and
1e-5 against the fp32 torch reference), each widened to 4 x the fp32 torch reference's own error against fp64 on the same inputs where that
is larger (the `_case` convention of tests/test_gpu_ohem.py).  Measured errors: DESIGN.md section 20."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle                                                   # noqa: E402
import _distill_ref as R                                        # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor, rel_err   # noqa: E402

N, LD, LDT, NC = 2, 24, 20, 19
SHAPES = {'x8': ((16, 32), (128, 256)), 'x3.8': ((17, 33), (65, 129)), 'x1': ((33, 65), (33, 65))}
PARAMS = {'a0.5_T1': (0.5, 1.0), 'a2_T4': (2.0, 4.0)}
W19 = torch.rand(NC, generator=torch.Generator().manual_seed(4)) + 0.5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


_CACHE = {}


def _case(name):
    """student and teacher logits (different seeds) and the target of a shape, made once and left unchanged"""
    if name not in _CACHE:
        lo_hw, hi_hw = SHAPES[name]
        x = rand_tensor(31, 'kd_x', (N,) + lo_hw + (NC,)) * 3
        y = rand_tensor(33, 'kd_teacher', (N,) + lo_hw + (NC,)) * 3
        r = np.random.default_rng(9)
        t = torch.from_numpy(r.integers(0, NC, (N,) + hi_hw)).long()
        t[torch.from_numpy(r.random((N,) + hi_hw) < 0.05)] = 255
        g0 = rand_tensor(32, 'kd_g0', (N,) + lo_hw + (LD,))
        _CACHE[name] = dict(x=x, y=y, t=t, g0=g0, lo_hw=lo_hw, hi_hw=hi_hw)
    return _CACHE[name]


def _refs(x, y, t, hi_hw, alpha, T, weight, mask=None):
    return tuple(R.reference(x, y, t, hi_hw, alpha, T, weight, dtype=dt, mask=mask, scale=0.5) for dt in (torch.float64, torch.float32))


def _padded(x, dev, ld):
    xa = torch.zeros(x.shape[:3] + (ld,), device=dev)
    xa[..., :NC] = x.to(dev)
    return xa


def _count(dev, ta, wa):
    """addk_ce_count: the weight sum of the valid pixels (wa None: their number)"""
    import addk._lib as L
    lib = L.load()
    out = torch.zeros(1, device=dev)
    ws = torch.zeros(int(lib.addk_ce_ws_floats(N, ta[0].numel())), device=dev)
    L.check(lib.addk_ce_count(ta.data_ptr(), ta.numel(), wa.data_ptr() if wa is not None else None, 255, NC, out.data_ptr(), ws.data_ptr(),
                              torch.cuda.current_stream().cuda_stream))
    return out


def _kd_args(xa, ya, ta, lo_hw, hi_hw, wa, wsum, nvalid, alpha, T, loss, kd, g, ws, acc, lmap=None, tau=None):
    import addk._lib as L
    (H, W), (OH, OW) = lo_hw, hi_hw
    b = L.CeUpsampleKdArgs()
    a = b.ce
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, NC, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.wsum, a.scale, a.loss_out = wsum.data_ptr(), 0.5, loss.data_ptr()
    a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), LD, acc, ws.data_ptr()
    if lmap is not None:
        b.pix_loss, b.tau = lmap.data_ptr(), tau.data_ptr()
    b.teacher, b.ld_teacher, b.alpha, b.temperature = ya.data_ptr(), ya.shape[-1], alpha, T
    b.nvalid, b.kd_out = nvalid.data_ptr(), kd.data_ptr()
    return b


def _kd_head(dev, xa, ya, ta, lo_hw, hi_hw, wa, g0, acc, wsum, nvalid, alpha, T, lmap=None, tau=None):
    """one addk_ce_upsample_kd_fwd_bwd launch sequence on fresh outputs; returns (loss, kd, g) on the host.  loss starts at 0.25 (it is
    accumulated), kd_out at NaN (it is written), the workspace dirty."""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = lo_hw, hi_hw
    assert lib.addk_ce_upsample_kd_supported(N, H, W, OH, OW, NC) == 1
    loss, kd = torch.full((1,), 0.25, device=dev), torch.full((1,), float('nan'), device=dev)
    g = g0.clone().to(dev)
    ws = torch.full((int(lib.addk_ce_upsample_kd_ws_floats(N, H, W)),), 7.0, device=dev)
    b = _kd_args(xa, ya, ta, lo_hw, hi_hw, wa, wsum, nvalid, alpha, T, loss, kd, g, ws, acc, lmap, tau)
    L.check(lib.addk_ce_upsample_kd_fwd_bwd(C.byref(b), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return loss.cpu(), kd.cpu(), g.cpu()


def _plain_head(dev, xa, ta, lo_hw, hi_hw, wa, g0, acc, wsum):
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = lo_hw, hi_hw
    loss = torch.full((1,), 0.25, device=dev)
    g = g0.clone().to(dev)
    ws = torch.zeros(int(lib.addk_ce_upsample_ws_floats(N, H, W)), device=dev)
    a = L.CeUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, NC, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.wsum, a.scale, a.loss_out = wsum.data_ptr(), 0.5, loss.data_ptr()
    a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), LD, acc, ws.data_ptr()
    L.check(lib.addk_ce_upsample_fwd_bwd(C.byref(a), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return loss.cpu(), g.cpu()


def _check(tag, res, r64, r32, g0, acc):
    """(loss, kd, g) of the device against the fp64 and fp32 references at the bounds of the module docstring; prints what it measured"""
    la, ka, ga = res
    loss, kd = float(la) - 0.25, float(ka)
    e_loss, e_kd = abs(loss - r64['loss']), abs(kd - r64['kd'])
    b_loss = max(2e-6 * abs(r64['loss']), 4 * abs(r32['loss'] - r64['loss']))
    b_kd = max(2e-6 * abs(r64['kd']), 4 * abs(r32['kd'] - r64['kd']))
    base = g0[..., :NC].double() if acc else 0
    e64 = rel_err(ga[..., :NC].double(), r64['grad'] + base)
    e32 = rel_err(ga[..., :NC].double(), r32['grad'].double() + base)
    b64 = max(5e-5, 4 * rel_err(r32['grad'].double(), r64['grad']))
    print('distill %s: loss err %.2e rel (fp32 torch %.2e), kd err %.2e rel (fp32 torch %.2e), grad %.2e vs fp64 (fp32 torch %.2e), %.2e vs fp32'
          % (tag, e_loss / abs(r64['loss']), abs(r32['loss'] - r64['loss']) / abs(r64['loss']), e_kd / abs(r64['kd']),
             abs(r32['kd'] - r64['kd']) / abs(r64['kd']), e64, rel_err(r32['grad'].double(), r64['grad']), e32))
    assert np.isfinite(loss) and np.isfinite(kd) and bool(torch.isfinite(ga).all())
    assert e_loss <= b_loss, (loss, r64['loss'], b_loss)
    assert e_kd <= b_kd, (kd, r64['kd'], b_kd)
    assert e64 <= b64, (e64, b64)
    assert e32 <= 1e-5, e32
    assert torch.equal(ga[..., NC:], g0[..., NC:])                                            # padding channels untouched


@pytest.mark.parametrize('par', list(PARAMS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_loss_kd_and_gradient_match_reference(dev, shape, par):
    """1. without class weights into a fresh gradient and with class weights accumulated into an existing one; two runs bit-equal, the
    teacher's buffer bit-unchanged."""
    c = _case(shape)
    alpha, T = PARAMS[par]
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), c['t'].to(dev)
    ya[..., NC:] = 5.0                                               # the teacher's padding channel is never read into the result
    y0 = ya.clone()
    nvalid = _count(dev, ta, None)
    for weight, acc in ((None, 0), (W19, 1)):
        wa = weight.to(dev) if weight is not None else None
        wsum = _count(dev, ta, wa)
        r64, r32 = _refs(c['x'], c['y'], c['t'], c['hi_hw'], alpha, T, weight)
        res = [_kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc, wsum, nvalid, alpha, T) for _ in range(2)]
        assert all(torch.equal(p, q) for p, q in zip(res[0], res[1]))                       # deterministic
        _check('%s %s %s' % (shape, par, 'weighted+acc' if acc else 'plain'), res[0], r64, r32, c['g0'], acc)
        assert r64['kd'] > 0 and float(res[0][1]) > 0
    assert torch.equal(ya, y0)


@pytest.mark.parametrize('shape', list(SHAPES))
def test_teacher_equal_to_student_leaves_the_plain_head(dev, shape):
    """2. the student's values in another buffer (another stride) as the teacher: KL = 0, loss and gradient are the plain head's."""
    c = _case(shape)
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['x'], dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    for weight, acc in ((None, 0), (W19, 1)):
        wa = weight.to(dev) if weight is not None else None
        wsum = _count(dev, ta, wa)
        lp, gp = _plain_head(dev, xa, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc, wsum)
        lo, kd, go = _kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc, wsum, nvalid, 2.0, 4.0)
        assert abs(float(kd)) <= 1e-6, float(kd)
        assert abs(float(lo) - float(lp)) <= 2e-6 * abs(float(lp) - 0.25)
        assert rel_err(go[..., :NC], gp[..., :NC]) <= 1e-6
        assert torch.equal(go[..., NC:], c['g0'][..., NC:])


def _select(dev, xa, ta, lo_hw, hi_hw, thresh, K, wa):
    """addk_ohem_select; returns (map, tau, wsum_kept, counts) on the device"""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = lo_hw, hi_hw
    f = dict(device=dev)
    lmap, tau, wk = torch.zeros((N, OH, OW), **f), torch.zeros(1, **f), torch.zeros(1, **f)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.addk_ohem_select_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    a = L.OhemSelectArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, NC, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.thresh, a.min_kept_total = thresh, K
    a.pix_loss, a.tau, a.wsum_kept, a.counts, a.ws = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr(), ws.data_ptr()
    L.check(lib.addk_ohem_select(C.byref(a), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lmap, tau, wk, counts


@pytest.mark.parametrize('shape', list(SHAPES))
def test_with_a_kept_set(dev, shape):
    """3. mining (regime `half` of tests/test_gpu_ohem.py: tau is the median loss) filters the cross-entropy term only: the reference takes
    the DEVICE's mask for CE and every valid pixel for KD."""
    c = _case(shape)
    alpha, T = PARAMS['a2_T4']
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    nv = int(nvalid.item())
    assert nv == int((c['t'] != 255).sum())
    for weight, acc in ((None, 0), (W19, 1)):
        wa = weight.to(dev) if weight is not None else None
        lmap, tau, wk, counts = _select(dev, xa, ta, c['lo_hw'], c['hi_hw'], 0.01, nv // 2, wa)
        mask = lmap.cpu() >= float(tau)
        assert int(mask.sum()) == int(counts[1]) and nv // 2 <= int(counts[1]) < nv
        r64, r32 = _refs(c['x'], c['y'], c['t'], c['hi_hw'], alpha, T, weight, mask=mask)
        res = [_kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc, wk, nvalid, alpha, T, lmap, tau) for _ in range(2)]
        assert all(torch.equal(p, q) for p, q in zip(res[0], res[1]))
        _check('%s kept set %s' % (shape, 'weighted+acc' if acc else 'plain'), res[0], r64, r32, c['g0'], acc)
        # the KD term is the unfiltered head's, bit for bit: mining never touches it
        full = _kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc, _count(dev, ta, wa), nvalid, alpha, T)
        assert torch.equal(full[1], res[0][1])


@pytest.mark.parametrize('shape', list(SHAPES))
def test_large_logits_stay_finite(dev, shape):
    """4. logits x 30 (|z| up to ~90, probabilities down to exp(-180)) at T = 1: finite, inside the bounds of (1)."""
    c = _case(shape)
    x, y = c['x'] * 30, c['y'] * 30
    xa, ya, ta = _padded(x, dev, LD), _padded(y, dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    r64, r32 = _refs(x, y, c['t'], c['hi_hw'], 0.5, 1.0, None)
    res = _kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], None, c['g0'], 0, nvalid, nvalid, 0.5, 1.0)
    _check('%s x30' % shape, res, r64, r32, c['g0'], 0)


def test_one_image_fully_ignored(dev):
    """5."""
    c = _case('x3.8')
    t = c['t'].clone()
    t[1] = 255
    alpha, T = PARAMS['a2_T4']
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), t.to(dev)
    nvalid = _count(dev, ta, None)
    r64, r32 = _refs(c['x'], c['y'], t, c['hi_hw'], alpha, T, None)
    res = _kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], None, c['g0'], 0, nvalid, nvalid, alpha, T)
    _check('one image ignored', res, r64, r32, c['g0'], 0)
    assert float(res[2][1, ..., :NC].abs().max()) == 0.0             # no pixel of the ignored image sends a gradient


@pytest.mark.parametrize('acc', [0, 1])
def test_every_pixel_ignored(dev, acc):
    """6. n == 0: kd_out is exactly 0 and the term adds exactly nothing to the gradient.  The cross-entropy normaliser is a stand-in word
    (1.0) so that the plain head's own 0/0 does not hide the comparison: with it the plain head leaves g = 0 (or g0), bit for bit."""
    c = _case('x3.8')
    t = torch.full_like(c['t'], 255)
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), t.to(dev)
    nvalid = _count(dev, ta, None)
    assert float(nvalid) == 0.0
    one = torch.ones(1, device=dev)
    lp, gp = _plain_head(dev, xa, ta, c['lo_hw'], c['hi_hw'], None, c['g0'], acc, one)
    lo, kd, go = _kd_head(dev, xa, ya, ta, c['lo_hw'], c['hi_hw'], None, c['g0'], acc, one, nvalid, 2.0, 4.0)
    assert float(kd) == 0.0 and float(lo) == float(lp) == 0.25
    assert torch.equal(go.view(torch.int32), gp.view(torch.int32))
    assert torch.equal(go[..., :NC], c['g0'][..., :NC] if acc else torch.zeros_like(go[..., :NC]))


def test_bad_arguments_are_refused_without_a_launch(dev):
    """7."""
    import addk._lib as L
    lib = L.load()
    c = _case('x1')
    (H, W), (OH, OW) = c['lo_hw'], c['hi_hw']
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    f = dict(device=dev)
    g, loss, kd = torch.full((N, H, W, LD), 7.0, **f), torch.full((1,), 7.0, **f), torch.full((1,), 7.0, **f)
    ws = torch.full((int(lib.addk_ce_upsample_kd_ws_floats(N, H, W)),), 7.0, **f)
    lmap, tau = torch.zeros((N, OH, OW), **f), torch.zeros(1, **f)
    st = torch.cuda.current_stream().cuda_stream

    def args(**kw):
        b = _kd_args(xa, ya, ta, c['lo_hw'], c['hi_hw'], None, nvalid, nvalid, 1.0, 4.0, loss, kd, g, ws, 0)
        for k, v in kw.items():
            setattr(b if hasattr(type(b), k) and k != 'ce' else b.ce, k, v)
        return b
    assert lib.addk_ce_upsample_kd_fwd_bwd(C.byref(args()), st) == 0           # the block itself is good
    torch.cuda.synchronize()
    g.fill_(7.0); loss.fill_(7.0); kd.fill_(7.0); ws.fill_(7.0)
    inf, nan = float('inf'), float('nan')
    bad = [dict(teacher=None), dict(nvalid=None), dict(kd_out=None), dict(logits=None), dict(target=None), dict(wsum=None), dict(loss_out=None),
           dict(g=None), dict(ws=None), dict(teacher=xa.data_ptr()), dict(ld_teacher=18), dict(ld=18), dict(ldg=18), dict(C=7),
           dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf), dict(temperature=0.0), dict(temperature=-2.0),
           dict(temperature=nan), dict(temperature=inf), dict(pix_loss=lmap.data_ptr()), dict(tau=tau.data_ptr())]
    for kw in bad:
        assert lib.addk_ce_upsample_kd_fwd_bwd(C.byref(args(**kw)), st) == -1, kw
    assert lib.addk_ce_upsample_kd_fwd_bwd(None, st) == -1
    torch.cuda.synchronize()
    for v in (g, loss, kd, ws):
        assert float(v.min()) == float(v.max()) == 7.0


# ---- 8, 9. the training step ---------------------------------------------------------------------------------------------------

SHAPE = (2, 3, 65, 129)
ARGS = (ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), 0)


def _oracle(seed=600):
    mo = oracle.ADD(*ARGS)
    fill_params(mo, seed)
    return mo


def _model(dev, seed=600):
    from addk.modeling.ADD import ADD
    ma = ADD(*ARGS)
    ma.load_state_dict(_oracle(seed).state_dict())
    return ma.to(dev)


def _batch(hw, seed=5):
    x = rand_tensor(seed, 'ts_x', (2, 3) + hw)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, 19, (2,) + hw)).long()
    t[torch.from_numpy(r.random((2,) + hw) < 0.05)] = 255
    return x, t


def _fwd_bwd(dev, distill):
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:])
    ma = _model(dev)
    ts = TrainStep(ma, SHAPE, use_graph=False, distill=distill)
    ts.load_batch(x.to(dev), t.to(dev))
    ts.forward_backward_only()
    torch.cuda.synchronize()
    names = {p: k for k, p in ma.named_parameters()}
    return ts, {names[p]: g.double().cpu() for p, g in ts.grads().items() if g is not None}


def test_step_against_the_oracle(dev):
    """8. forward_backward_only with distill=(1.0, 4.0) against the oracle model in fp32 and fp64 with the same loss written in torch (the
    oracle's full-resolution outputs are the bilinear samples of its low-resolution logits; the teacher is detached): the bounds of
    tests/test_gpu_train.py::test_train_step_forward_backward_and_sgd.  The parameters only the last exit uses get the plain step's gradient."""
    alpha, T = 1.0, 4.0
    x, t = _batch(SHAPE[2:])
    valid = t != 255
    ts, ga = _fwd_bwd(dev, (alpha, T))
    names = [c.name for c in ts.g.bwd]
    assert names.count('ce_upsample_kd') == 1 and names.count('ce_upsample') == 1
    res, last_only = {}, None
    for name, dt in (('o32', torch.float32), ('o64', torch.float64)):
        m = _oracle().to(dt)
        m.train()
        ys = m(x.to(dt))
        assert len(ys) == 2
        if last_only is None:
            # parameters no student shares: the first exit's own loss does not reach them
            gs = torch.autograd.grad(oracle.cross_entropy_mean_exits(ys[:1], t), list(m.parameters()), allow_unused=True, retain_graph=True)
            last_only = [k for (k, _), g_ in zip(m.named_parameters(), gs) if g_ is None]
        kd = sum(R.kd_term(y, ys[-1], valid, alpha, T) for y in ys[:-1]) / len(ys)
        loss = oracle.cross_entropy_mean_exits(ys, t) + kd
        loss.backward()
        res[name] = (loss.item(), {k: p.grad.double() for k, p in m.named_parameters()}, kd.item())
    la = ts.loss.item()
    assert abs(la - res['o64'][0]) <= 3 * abs(res['o32'][0] - res['o64'][0]) + 1e-4 * abs(la), (la, res['o64'][0], res['o32'][0])
    g64 = res['o64'][1]

    def rel_l2(gx):
        return (sum(float(((gx[k] - g64[k]) ** 2).sum()) for k in g64) / sum(float((g64[k] ** 2).sum()) for k in g64)) ** 0.5
    assert set(ga) == set(g64)
    print('distill step: loss %.6f (fp64 %.6f, fp32 %.6f), rel_l2 %.2e (fp32 torch %.2e)' % (la, res['o64'][0], res['o32'][0], rel_l2(ga), rel_l2(res['o32'][1])))
    assert rel_l2(ga) <= 2.0 * rel_l2(res['o32'][1]) + 1e-3
    stats = ts.distill_stats()
    assert len(stats) == 1 and all(np.isfinite(v) and v > 0 for v in stats)
    print('distill step: kd %.6e (fp64 %.6e, fp32 %.6e)' % (stats[0], res['o64'][2], res['o32'][2]))
    # the teacher is detached: what only the last exit uses gets the gradient of a plain step
    _, gp = _fwd_bwd(dev, None)
    assert len(last_only) > 0 and set(last_only) < set(ga)
    a = torch.cat([ga[k].reshape(-1) for k in last_only])
    b = torch.cat([gp[k].reshape(-1) for k in last_only])
    assert float(b.abs().max()) > 0 and rel_err(a, b) <= 2e-4


@pytest.mark.parametrize('ohem', [None, (0.7, 2000)], ids=['distill', 'distill+ohem'])
def test_step_replayed_graph_equals_eager(dev, ohem):
    """9. after enable_capture() the step is one hipGraph; four steps give the loss, kd and parameters of four eager steps, bit for bit."""
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:])
    res = {}
    for mode in ('eager', 'graph'):
        ts = TrainStep(_model(dev), SHAPE, use_graph=False, distill=(1.0, 4.0), ohem=ohem)
        ts.load_batch(x.to(dev), t.to(dev))
        if mode == 'graph':
            ts.enable_capture()
        ls = []
        for _ in range(4):                                         # graph: one eager step that is then captured, three replays
            l = ts.step().item()
            ls.append((l, tuple(ts.distill_stats())))
        torch.cuda.synchronize()
        assert (ts.graph is not None) == (mode == 'graph')
        res[mode] = (ls, ts.flat_p.clone())
        ts.close()
    assert res['graph'][0] == res['eager'][0], (res['graph'][0], res['eager'][0])
    assert torch.equal(res['graph'][1], res['eager'][1])
    kds = [k[0] for _, k in res['eager'][0]]
    assert all(np.isfinite(v) and v > 0 for v in kds) and len(set(kds)) == 4          # kd_out is written every step, not accumulated
