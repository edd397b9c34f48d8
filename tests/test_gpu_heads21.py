"""GPU tests of the fused logits heads at 21 classes (Pascal VOC): every entry point of the training heads and the label head through
the C ABI against an fp64 CPU reference built the way that head's 19-class test builds it (F.interpolate(bilinear, align_corners=False),
then the head's arithmetic in float64), and the training step and the Segmenter end to end on an F = 4 model with 21 classes.  (The
scoring, profile, calibration, gate and multi-view heads are not covered here: they take 19 classes.)

Two geometries: [2,5,9,21] -> 33x65 crosses the 64-column and 32-row tile edges of scu_walk and the 31-column tile of ce_up_kernel;
[1,7,6,21] -> 50x41 is a non-integer ratio.  Each runs with pixel stride 21 (the scalar-load kernels) and 24 on a 16-byte-aligned base
(the 16-byte-load kernels).  The targets hold 255, class 20 and out-of-range values (21, -1 among them).

Every bound is the one the head's 19-class test uses; the file and line stand next to it.  Integers (the mining counts and tau's bits,
the Dice class counts) are compared exactly.  Every head runs twice and the bits are compared."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

import oracle                                                   # noqa: E402
import _dice_ref as RD                                          # noqa: E402
import _distill_ref as RK                                       # noqa: E402
import _ohem_ref as RO                                          # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor, rel_err   # noqa: E402

NC, LD = 21, 24
GEOMS = {'tiles': (2, (5, 9), (33, 65)), 'ratio': (1, (7, 6), (50, 41))}
LDS = {'vec_ld24': 24, 'scalar_ld21': 21}
NEAR_TIE_GAP, NEAR_TIE_SHARE = 1e-4, 0.005      # tests/test_gpu_validate.py:21-22
W21 = torch.rand(NC, generator=torch.Generator().manual_seed(4)) + 0.5
KD = (2.0, 4.0)                                 # alpha, T: tests/test_gpu_dice.py:24
SCALE = 0.5

cases = pytest.mark.parametrize('ldname', list(LDS))
geoms = pytest.mark.parametrize('geom', list(GEOMS))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    import addk._lib as L
    return L.load(), L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _targets(n, hw, seed=17):
    """labels in [0, 21) (class 20 among them), 5 % at 255, and twelve pixels outside the range (tests/test_gpu_validate.py:38-45)"""
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, NC, (n,) + hw)).long()
    t[torch.from_numpy(r.random((n,) + hw) < 0.05)] = 255
    flat = t.view(-1)
    pos = torch.from_numpy(r.choice(flat.numel(), 12, replace=False))
    flat[pos] = torch.tensor([21, 22, 254, 256, 1000, 2 ** 40, -1, -2, -255, -1000, -2 ** 40, 20])
    return t


@functools.lru_cache(maxsize=None)
def _case(geom):
    """Inputs and the CPU references every test of a geometry shares: computed once, never modified."""
    N, lo, hi = GEOMS[geom]
    x = rand_tensor(61, 'h21_x:' + geom, (N,) + lo + (NC,)) * 3
    y = rand_tensor(63, 'h21_teacher:' + geom, (N,) + lo + (NC,)) * 3
    t = _targets(N, hi)
    assert int((t == 20).sum()) > 0 and int((t == 21).sum()) > 0 and int((t == -1).sum()) > 0 and int((t == 255).sum()) > 0
    up64 = Fn.interpolate(x.double().permute(0, 3, 1, 2), size=hi, mode='bilinear', align_corners=False)
    up32 = Fn.interpolate(x.permute(0, 3, 1, 2), size=hi, mode='bilinear', align_corners=False)
    top = up32.topk(2, dim=1).values
    near_tie = (top[:, 0] - top[:, 1]) < NEAR_TIE_GAP * float(up32.abs().max())
    g0 = rand_tensor(62, 'h21_g0:' + geom, (N,) + lo + (LD,))
    return dict(geom=geom, N=N, lo=lo, hi=hi, shape=(N, lo, hi), x=x, y=y, t=t, up64=up64, up32=up32, near_tie=near_tie,
                pred32=up32.argmax(1), pred64=up64.argmax(1), valid=(t != 255) & (t >= 0) & (t < NC), inrange=(t >= 0) & (t < NC),
                g0=g0)


def _dev_logits(x, ld, dev, seed=1):
    """[N,H,W,21] on the device at pixel stride ld: 24 with finite garbage in the padding channels on a 16-byte-aligned base, or dense"""
    if ld == NC:
        return x.to(dev).contiguous()
    xa = (rand_tensor(seed, 'h21_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
    xa[..., :NC] = x.to(dev)
    xa = xa.contiguous()
    assert xa.data_ptr() % 16 == 0
    return xa


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _resize(xa, ld, shape):
    """addk_resize_fwd: the materialised fp32 full-resolution logits [N,21,OH,OW] (any class count)"""
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape
    y = torch.empty((N, NC, OH, OW), device=xa.device)
    ar = L.ResizeArgs()
    ar.src.x, ar.src.ld, ar.src.C = xa.data_ptr(), ld, NC
    ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    L.check(lib.addk_resize_fwd(C.byref(ar), _stream()), 'resize_fwd')
    torch.cuda.synchronize()
    return y


def _count(ta, wa):
    """addk_ce_count: the weight sum of the valid pixels (wa None: their number)"""
    lib, L = _lib()
    out = torch.zeros(1, device=ta.device)
    ws = torch.zeros(int(lib.addk_ce_ws_floats(ta.shape[0], ta[0].numel())), device=ta.device)
    L.check(lib.addk_ce_count(ta.data_ptr(), ta.numel(), wa.data_ptr() if wa is not None else None, 255, NC, out.data_ptr(), ws.data_ptr(), _stream()))
    return out


def _fill_up(a, xa, ld, shape):
    N, (H, W), (OH, OW) = shape
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, NC, OH, OW


def _check_map(tag, got, c):
    """a uint8 arg-max map against the fp32 CPU arg-max outside the near-ties (tests/test_gpu_validate.py:151-160)"""
    tie = c['near_tie']
    share = float(tie.float().mean())
    wrong = (got.long() != c['pred32']) & ~tie
    print('%s: near-tie share %.4f%%, mismatches outside near-ties %d, fp32-vs-fp64 reference arg-max disagreements %d'
          % (tag, 100 * share, int(wrong.sum()), int((c['pred32'] != c['pred64']).sum())))
    assert share <= NEAR_TIE_SHARE                                   # tests/test_gpu_validate.py:159
    assert int(wrong.sum()) == 0                                     # tests/test_gpu_validate.py:160
    assert len(got.unique()) > 4


# ------------------------------------------------------------------------------------------------------------------------
# the references alone (CPU arithmetic; runs with the GPU tests because it guards their seeds)
# ------------------------------------------------------------------------------------------------------------------------
@geoms
def test_references_stay_under_the_near_tie_caps(geom):
    """fp64 and fp32 CPU references of the chosen seeds: near-ties under the cap of the label and scoring tests, and the fp32 arg-max differs
    from the fp64 one only inside them"""
    c = _case(geom)
    share = float(c['near_tie'].float().mean())
    differ = c['pred32'] != c['pred64']
    print('%s: near-tie share %.4f%% (cap %.2f%%), fp32 vs fp64 arg-max differ on %d pixels' % (geom, 100 * share, 100 * NEAR_TIE_SHARE, int(differ.sum())))
    assert share <= NEAR_TIE_SHARE and not bool((differ & ~c['near_tie']).any())


# ------------------------------------------------------------------------------------------------------------------------
# training heads
# ------------------------------------------------------------------------------------------------------------------------
def _select(xa, ld, ta, shape, thresh, K, wa=None):
    """addk_ohem_select on a dirty workspace, twice -> (map, tau, wsum_kept, counts) on the device (tests/test_gpu_ohem.py:61-81)"""
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape
    dev = xa.device
    assert lib.addk_ohem_select_supported(N, H, W, OH, OW, NC) == 1
    res = []
    ws = torch.full((int(lib.addk_ohem_select_ws_bytes(N, OH, OW)),), 0x5a, dtype=torch.uint8, device=dev)
    for _ in range(2):
        lmap = torch.full((N, OH, OW), float('nan'), device=dev)
        tau, wk = torch.full((1,), float('nan'), device=dev), torch.full((1,), float('nan'), device=dev)
        counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
        a = L.OhemSelectArgs()
        _fill_up(a, xa, ld, shape)
        a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
        a.thresh, a.min_kept_total = thresh, K
        a.pix_loss, a.tau, a.wsum_kept, a.counts, a.ws = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr(), ws.data_ptr()
        L.check(lib.addk_ohem_select(C.byref(a), _stream()), 'ohem_select')
        torch.cuda.synchronize()
        res.append((lmap, tau, wk, counts))
    assert all(_bits(p, q) for p, q in zip(res[0], res[1]))          # the second call, on the used workspace: the same bits
    return res[0]


def _head(entry, c, xa, ld, ta, wa, acc, wsum, lmap=None, tau=None, ya=None, nvalid=None, coef=None, loss0=None):
    """one launch of a loss head ('plain', 'ohem', 'kd', 'dice') on fresh outputs, twice -> (loss, kd_out, g) on the host"""
    lib, L = _lib()
    dev = xa.device
    N, (H, W), _ = c['shape']
    res = []
    for _ in range(2):
        loss = torch.full((1,), 0.25, device=dev) if loss0 is None else loss0.clone()
        kd = torch.full((1,), float('nan'), device=dev)
        g = c['g0'].clone().to(dev)
        ws = torch.full((int(lib.addk_ce_upsample_kd_ws_floats(N, H, W)),), 7.0, device=dev)

        def fill_ce(a):
            _fill_up(a, xa, ld, c['shape'])
            a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
            a.wsum, a.scale, a.loss_out = wsum.data_ptr(), SCALE, loss.data_ptr()
            a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), LD, acc, ws.data_ptr()
        if entry == 'plain':
            b = L.CeUpsampleArgs()
            fill_ce(b)
            fn = lib.addk_ce_upsample_fwd_bwd
        elif entry == 'ohem':
            b = L.CeUpsampleOhemArgs()
            fill_ce(b.ce)
            b.pix_loss, b.tau = lmap.data_ptr(), tau.data_ptr()
            fn = lib.addk_ce_upsample_ohem_fwd_bwd
        else:
            b = L.CeUpsampleDiceArgs() if entry == 'dice' else L.CeUpsampleKdArgs()
            k = b.kd if entry == 'dice' else b
            fill_ce(k.ce)
            if lmap is not None:
                k.pix_loss, k.tau = lmap.data_ptr(), tau.data_ptr()
            if ya is not None:
                k.teacher, k.ld_teacher, k.alpha, k.temperature = ya.data_ptr(), ya.shape[-1], KD[0], KD[1]
                k.nvalid, k.kd_out = nvalid.data_ptr(), kd.data_ptr()
            if entry == 'dice':
                b.coef = coef.data_ptr()
            fn = lib.addk_ce_upsample_dice_fwd_bwd if entry == 'dice' else lib.addk_ce_upsample_kd_fwd_bwd
        L.check(fn(C.byref(b), _stream()), entry)
        torch.cuda.synchronize()
        res.append((loss.cpu(), kd.cpu(), g.cpu()))
    assert _bits(res[0][0], res[1][0]) and _bits(res[0][2], res[1][2])        # deterministic
    assert ya is None or _bits(res[0][1], res[1][1])
    return res[0]


def _check_head(tag, c, res, r64, r32, acc, term=None, loss0=0.25, fixed=False):
    """(loss, kd, g) against the fp64 and fp32 references.  fixed (the plain and mining heads): loss 2e-6 relative, gradient 5e-5 against fp64
    and 1e-5 against fp32 (tests/test_gpu_train.py:118-121, tests/test_gpu_ohem.py:229-232).  Otherwise (the distillation and Dice heads):
    loss and the second term 2e-6 relative or 4x the fp32 reference's own error, gradient 5e-5 against fp64 or 4x the fp32 reference's
    error, 1e-5 against fp32 (tests/test_gpu_distill.py:123-136, tests/test_gpu_dice.py:193-206).  Padding channels untouched"""
    la, ka, ga = res
    loss = float(la.double()) - loss0
    e_loss = abs(loss - r64['loss'])
    b_loss = 2e-6 * abs(r64['loss']) if fixed else max(2e-6 * abs(r64['loss']), 4 * abs(r32['loss'] - r64['loss']))
    base = c['g0'][..., :NC].double() if acc else 0
    e64 = rel_err(ga[..., :NC].double(), r64['grad'] + base)
    e32 = rel_err(ga[..., :NC].double(), r32['grad'].double() + base)
    b64 = 5e-5 if fixed else max(5e-5, 4 * rel_err(r32['grad'].double(), r64['grad']))
    print('%s: loss err %.2e rel (bound %.2e), grad %.2e vs fp64 (bound %.2e), %.2e vs fp32' % (tag, e_loss / abs(r64['loss']), b_loss / abs(r64['loss']), e64, b64, e32))
    assert np.isfinite(loss) and bool(torch.isfinite(ga).all())
    assert e_loss <= b_loss, (loss, r64['loss'], b_loss)
    assert e64 <= b64, (e64, b64)
    assert e32 <= 1e-5, e32
    if term is not None:
        got = float(ka)
        e, b = abs(got - r64[term]), max(2e-6 * abs(r64[term]), 4 * abs(r32[term] - r64[term]))
        print('%s: %s term err %.2e rel (bound %.2e)' % (tag, term, e / abs(r64[term]), b / abs(r64[term])))
        assert e <= b, (got, r64[term], b)
    assert torch.equal(ga[..., NC:], c['g0'][..., NC:])


@cases
@geoms
def test_ce_upsample(dev, geom, ldname):
    """addk_ce_upsample_fwd_bwd: plain and with class weights + accumulation"""
    lib, L = _lib()
    c, ld = _case(geom), LDS[ldname]
    N, (H, W), (OH, OW) = c['shape']
    assert lib.addk_ce_upsample_supported(N, H, W, OH, OW, NC) == 1
    xa, ta = _dev_logits(c['x'], ld, dev), c['t'].to(dev)
    for weight, acc in ((None, 0), (W21, 1)):
        wa = weight.to(dev) if weight is not None else None
        r64, r32 = (RO.reference(c['x'], c['t'], c['hi'], 1.0, 1, weight, dtype=dt, mask=c['valid'], scale=SCALE) for dt in (torch.float64, torch.float32))
        res = _head('plain', c, xa, ld, ta, wa, acc, _count(ta, wa))
        _check_head('ce_upsample %s %s w%d' % (geom, ldname, acc), c, res, r64, r32, acc, fixed=True)


@cases
@geoms
def test_ohem_select_and_head(dev, geom, ldname):
    """addk_ohem_select: the map against fp64 (tests/test_gpu_ohem.py:50,115-119), tau and the counts exactly against torch.sort of the
    stored floats (:136-140); addk_ce_upsample_ohem_fwd_bwd on the device's mask (:219-233)"""
    c, ld = _case(geom), LDS[ldname]
    xa, ta = _dev_logits(c['x'], ld, dev), c['t'].to(dev)
    nvalid = int(c['valid'].sum())
    l64 = RO.reference(c['x'], c['t'], c['hi'], 1.0, 1, dtype=torch.float64)['l']
    l32 = RO.reference(c['x'], c['t'], c['hi'], 1.0, 1, dtype=torch.float32)['l']
    e32 = float((l32.double() - l64)[c['valid']].abs().max())
    bound = max(4 * e32, 1e-6 * float(l64.max()))                    # tests/test_gpu_ohem.py:50
    thresh, K = 0.01, nvalid // 2                                    # 'half' of tests/test_gpu_ohem.py:21: tau is the median loss
    for weight, acc in ((None, 0), (W21, 1)):
        wa = weight.to(dev) if weight is not None else None
        lmap, tau, wk, counts = _select(xa, ld, ta, c['shape'], thresh, K, wa)
        lm = lmap.cpu()
        assert torch.equal(lm[~c['valid']], torch.full_like(lm[~c['valid']], -1.0))
        err = float((lm.double() - l64)[c['valid']].abs().max())
        print('ohem map %s %s: device error %.3e, fp32 torch error %.3e, bound %.3e' % (geom, ldname, err, e32, bound))
        assert float(lm[c['valid']].min()) >= 0.0 and err <= bound
        vals = lm[lm >= 0]
        tau_h, kept_h = RO.select_tau(vals, thresh, K)
        assert int(counts[0]) == nvalid == vals.numel()              # exact
        assert float(tau) == tau_h and int(counts[1]) == kept_h and K <= kept_h < nvalid
        mask = lm >= float(tau)
        wsum64 = float((weight.double()[c['t'][mask]] if weight is not None else torch.ones(kept_h, dtype=torch.float64)).sum())
        assert abs(float(wk) - wsum64) <= 2e-6 * wsum64              # tests/test_gpu_ohem.py:225
        r64, r32 = (RO.reference(c['x'], c['t'], c['hi'], thresh, K, weight, dtype=dt, mask=mask, scale=SCALE) for dt in (torch.float64, torch.float32))
        res = _head('ohem', c, xa, ld, ta, wa, acc, wk, lmap=lmap, tau=tau)
        _check_head('ce_upsample_ohem %s %s w%d' % (geom, ldname, acc), c, res, r64, r32, acc, fixed=True)


@cases
@geoms
def test_ce_upsample_kd(dev, geom, ldname):
    """addk_ce_upsample_kd_fwd_bwd, without and with mining; the teacher's stride follows the student's, so both teacher loaders run"""
    c, ld = _case(geom), LDS[ldname]
    xa, ya, ta = _dev_logits(c['x'], ld, dev), _dev_logits(c['y'], ld, dev, seed=3), c['t'].to(dev)
    nv = _count(ta, None)
    assert float(nv) == float(c['valid'].sum())
    for mining, weight, acc in ((False, None, 0), (True, W21, 1)):
        wa = weight.to(dev) if weight is not None else None
        mask, kw, wsum = None, {}, _count(ta, wa)
        if mining:
            lmap, tau, wsum, counts = _select(xa, ld, ta, c['shape'], 0.01, int(c['valid'].sum()) // 2, wa)
            mask, kw = lmap.cpu() >= float(tau), dict(lmap=lmap, tau=tau)
        r64, r32 = (RK.reference(c['x'], c['y'], c['t'], c['hi'], KD[0], KD[1], weight, dtype=dt, mask=mask, scale=SCALE)
                    for dt in (torch.float64, torch.float32))
        res = _head('kd', c, xa, ld, ta, wa, acc, wsum, ya=ya, nvalid=nv, **kw)
        _check_head('ce_upsample_kd %s %s mining%d' % (geom, ldname, mining), c, res, r64, r32, acc, term='kd')


def _vec_close(tag, got, r64, r32):
    """per class: |got - fp64| <= max(2e-6 |fp64|, 4 |fp32 torch - fp64|) (tests/test_gpu_dice.py:212-216)"""
    got, a, b = got.double(), r64.double(), r32.double()
    err, bound = (got - a).abs(), torch.maximum(2e-6 * a.abs(), 4 * (b - a).abs())
    assert bool((err <= bound).all()), (tag, got, a, bound)


def _stats(xa, ld, ta, shape, weight, smooth):
    """addk_dice_stats on NaN-preset outputs and a dirty workspace, twice -> (coef, dice_out, loss, workspace words) on the device"""
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape
    dev = xa.device
    assert lib.addk_dice_stats_supported(N, H, W, OH, OW, NC) == 1
    nb = int(lib.addk_dice_stats_ws_bytes_classes(N, OH, OW, NC))
    assert nb % 4 == 0 and nb > int(lib.addk_dice_stats_ws_bytes(N, OH, OW))
    res = []
    for _ in range(2):
        coef, dout = torch.full((2 * NC,), float('nan'), device=dev), torch.full((1 + NC,), float('nan'), device=dev)
        loss = torch.full((1,), 0.25, device=dev)
        ws = torch.full((nb // 4,), 0x7fc12345, dtype=torch.int32, device=dev)
        a = L.DiceStatsArgs()
        _fill_up(a, xa, ld, shape)
        a.target, a.ignore_index, a.weight, a.smooth, a.scale = ta.data_ptr(), 255, weight, smooth, SCALE
        a.coef, a.dice_out, a.loss_out, a.ws = coef.data_ptr(), dout.data_ptr(), loss.data_ptr(), ws.data_ptr()
        L.check(lib.addk_dice_stats(C.byref(a), _stream()), 'dice_stats')
        torch.cuda.synchronize()
        res.append((coef, dout, loss, ws))
    assert all(_bits(p, q) for p, q in zip(res[0], res[1]))          # deterministic, the whole workspace included
    return res[0]


@cases
@geoms
def test_dice_stats_and_head(dev, geom, ldname):
    """addk_dice_stats (tests/test_gpu_dice.py:221-251) with class 7 absent, and addk_ce_upsample_dice_fwd_bwd in its four forms: alone,
    with mining, with a teacher, with both"""
    c, ld = _case(geom), LDS[ldname]
    absent = 7
    t = c['t'].clone()
    t[t == absent] = 3
    valid = (t != 255) & (t >= 0) & (t < NC)
    xa, ya, ta = _dev_logits(c['x'], ld, dev), _dev_logits(c['y'], ld, dev, seed=3), t.to(dev)
    weight, smooth = 0.25, 1e-3                                      # 'w0.25_s1e-3' of tests/test_gpu_dice.py:23
    coef, dout, loss, ws = _stats(xa, ld, ta, c['shape'], weight, smooth)
    r64, r32 = (RD.reference(c['x'], t, c['hi'], weight, smooth, dtype=dt, scale=SCALE, ce=False) for dt in (torch.float64, torch.float32))
    wsh, ch, dh = ws.cpu(), coef.cpu(), dout.cpu()
    Y = wsh[:NC].long()
    assert torch.equal(Y, r64['Y'].long()) and int(Y[absent]) == 0 and int(Y[20]) > 0 and r64['m'] == NC - 1      # exact
    I, P = wsh[32:32 + NC].view(torch.float32), wsh[64:64 + NC].view(torch.float32)
    present = r64['present']
    _vec_close('I', I, r64['I'], r32['I'])
    _vec_close('P', P, r64['P'], r32['P'])
    _vec_close('D', dh[1:][present], r64['D'][present], r32['D'][present])
    _vec_close('A', ch[:NC], r64['A'], r32['A'])
    _vec_close('B', ch[NC:], r64['B'], r32['B'])
    assert float(dh[1 + absent]) == -1.0 and float(ch[absent]) == 0.0 and float(ch[NC + absent]) == 0.0
    e, b = abs(float(dh[0]) - r64['dice']), max(2e-6 * abs(r64['dice']), 4 * abs(r32['dice'] - r64['dice']))     # tests/test_gpu_dice.py:247
    print('dice_stats %s %s: term %.9g ref64 %.9g rel err %.2e (bound %.2e)' % (geom, ldname, float(dh[0]), r64['dice'], e / abs(r64['dice']), b / abs(r64['dice'])))
    assert e <= b
    assert float(loss) == float(torch.tensor(0.25) + dh[0])          # tests/test_gpu_dice.py:251
    nv = _count(ta, None)
    for mining, teacher, weight_c, acc in ((False, False, None, 0), (True, False, W21, 1), (False, True, W21, 0), (True, True, None, 1)):
        wa = weight_c.to(dev) if weight_c is not None else None
        mask, kw, wsum = None, {}, _count(ta, wa)
        if mining:
            lmap, tau, wsum, counts = _select(xa, ld, ta, c['shape'], 0.01, int(valid.sum()) // 2, wa)
            mask, kw = lmap.cpu() >= float(tau), dict(lmap=lmap, tau=tau)
        rkw = dict(class_w=weight_c, mask=mask, scale=SCALE)
        if teacher:
            kw.update(ya=ya, nvalid=nv)
            rkw.update(teacher=c['y'], alpha=KD[0], T=KD[1])
        h64, h32 = (RD.reference(c['x'], t, c['hi'], weight, smooth, dtype=dt, **rkw) for dt in (torch.float64, torch.float32))
        res = _head('dice', c, xa, ld, ta, wa, acc, wsum, coef=coef, loss0=loss, **kw)      # the loss word already holds 0.25 + the term
        _check_head('ce_upsample_dice %s %s mining%d teacher%d' % (geom, ldname, mining, teacher), c, res, h64, h32, acc)


# ------------------------------------------------------------------------------------------------------------------------
# inference heads
# ------------------------------------------------------------------------------------------------------------------------
def _label(xa, ld, c, lut=None):
    lib, L = _lib()
    N, (H, W), (OH, OW) = c['shape']
    assert lib.addk_label_upsample_supported(N, H, W, OH, OW, NC) == 1
    lab = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=xa.device)
    a = L.LabelUpsampleArgs()
    _fill_up(a, xa, ld, c['shape'])
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, lab.data_ptr()
    L.check(lib.addk_label_upsample(C.byref(a), _stream()), 'label_upsample')
    torch.cuda.synchronize()
    return lab.cpu()


def _argmax(y):
    lib, L = _lib()
    N, Cc, OH, OW = y.shape
    y = y.contiguous()
    am = torch.empty((N, OH, OW), dtype=torch.int64, device=y.device)
    L.check(lib.addk_argmax_nchw(y.data_ptr(), N, Cc, OH * OW, am.data_ptr(), _stream()), 'argmax_nchw')
    torch.cuda.synchronize()
    return am.to(torch.uint8).cpu()


@cases
@geoms
def test_label_upsample(dev, geom, ldname):
    """addk_label_upsample: the fp32 CPU arg-max outside the near-ties, the bytes of the materialised path (tests/test_gpu_labels.py:156),
    and through a table"""
    c, ld = _case(geom), LDS[ldname]
    xa = _dev_logits(c['x'], ld, dev)
    got = _label(xa, ld, c)
    assert torch.equal(got, _label(xa, ld, c))
    _check_map('label %s %s' % (geom, ldname), got, c)
    assert int((got == 20).sum()) > 0                                # the last class is somebody's arg-max
    assert torch.equal(got, _argmax(_resize(xa, ld, c['shape'])))
    lut = torch.arange(255, -1, -1, dtype=torch.uint8)
    assert torch.equal(_label(xa, ld, c, lut.to(dev)), lut[got.long()])


# ------------------------------------------------------------------------------------------------------------------------
# end to end: ADD, F = 4, 21 classes, (2,3,33,65)
# ------------------------------------------------------------------------------------------------------------------------
SHAPE = (2, 3, 33, 65)


def _model(dev, seed=600):
    """the F = 4 two-exit model with 21 classes and synthetic weights; the classifier is scaled as in tests/test_gpu_validate.py:204-209 so
    that loss and entropy are well-conditioned sums"""
    from addk.modeling.ADD import ADD
    args = (ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, NC, make_args(4), 0)
    mo = oracle.ADD(*args)
    fill_params(mo, seed)
    with torch.no_grad():
        mo.decoder._conv[7].weight.mul_(4e-5)
        mo.decoder._conv[7].bias.mul_(4e-5)
    ma = ADD(*args)
    ma.load_state_dict(mo.state_dict())
    return ma.to(dev)


def _batch(seed=5):
    x = rand_tensor(seed, 'h21_ts_x', SHAPE)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, NC, (SHAPE[0],) + SHAPE[2:])).long()
    t[torch.from_numpy(r.random((SHAPE[0],) + SHAPE[2:]) < 0.05)] = 255
    return x, t


def test_train_step_fused_head_equals_stand_alone_path(dev, monkeypatch):
    """TrainStep.forward_backward_only() with the fused head against ADDK_FUSE_CE=0 (resize, cross-entropy, resize backward: any class
    count): the loss and all parameter gradients at the bounds of tests/test_gpu_train.py:183-184"""
    from addk.train import TrainStep
    x, t = _batch()
    out = {}
    for fuse in ('0', '1'):
        monkeypatch.setenv('ADDK_FUSE_CE', fuse)
        ts = TrainStep(_model(dev), SHAPE, use_graph=False)
        names = [c.name for c in ts.g.bwd]
        assert ('ce_upsample' in names) == (fuse == '1') and ('resize_nchw_bwd' in names) == (fuse == '0')
        ts.load_batch(x.to(dev), t.to(dev))
        ts.forward_backward_only()
        torch.cuda.synchronize()
        out[fuse] = (ts.loss.item(), ts.flat_g.clone(), {k: g.clone() for k, g in ts.grads().items() if g is not None})
    d_loss, d_g = abs(out['0'][0] - out['1'][0]) / abs(out['0'][0]), rel_err(out['1'][1], out['0'][1])
    print('train 21 classes: loss %.9g fused vs %.9g, rel %.3g; gradients rel_err %.3g' % (out['1'][0], out['0'][0], d_loss, d_g))
    assert math.isfinite(out['1'][0]) and float(out['0'][1].abs().max()) > 0
    assert d_loss <= 2e-6                                            # tests/test_gpu_train.py:183
    assert d_g <= 2e-4                                               # tests/test_gpu_train.py:184
    assert len(out['0'][2]) == len(out['1'][2]) > 0 and all(bool(torch.isfinite(g).all()) for g in out['1'][2].values())


def test_segmenter_equals_the_argmax_of_forward(dev):
    """Segmenter's map against addk_argmax_nchw of the model's own logits, byte for byte (tests/test_gpu_labels.py:377)"""
    from addk.segment import Segmenter
    ma = _model(dev).eval()
    x = _batch(9)[0].to(dev)
    with torch.no_grad():
        want = _argmax(ma(x)[-1])
    seg = Segmenter(ma, SHAPE, use_graph=False)
    assert [c.name for c in seg.g.fwd][-1] == 'label_upsample' and 'resize_nchw' not in [c.name for c in seg.g.fwd]
    y = seg.step(x)
    torch.cuda.synchronize()
    assert y.dtype == torch.uint8 and tuple(y.shape) == (SHAPE[0],) + SHAPE[2:] and len(want.unique()) > 1
    assert torch.equal(y.cpu(), want), int((y.cpu() != want).sum())
    seg.close()
