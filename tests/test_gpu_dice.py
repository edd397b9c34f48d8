"""GPU tests of the soft-Dice region term in the fused loss head: addk_dice_stats (the per-class sums of the batch, the coefficient table and
the term), addk_ce_upsample_dice_fwd_bwd (the loss head with the term's gradient, alone, with a kept set, with a teacher, with both) and
train.TrainStep(dice=...).

Bounds of the kernel tests: the plain head's (tests/test_gpu_train.py: loss and term 2e-6 relative to fp64; gradient rel_err 5e-5 against
fp64 and 1e-5 against the fp32 torch reference), each widened to 4 x the fp32 torch reference's own error against fp64 on the same inputs
where that is larger (the `_case` convention of tests/test_gpu_ohem.py).  Measured errors: DESIGN.md section 21."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle                                                   # noqa: E402
import _dice_ref as R                                           # noqa: E402
import _distill_ref as RD                                       # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor, rel_err   # noqa: E402

N, LD, LDT, NC = 2, 24, 20, 19
SHAPES = {'x8': ((16, 32), (128, 256)), 'x3.8': ((17, 33), (65, 129)), 'x1': ((33, 65), (33, 65))}
PARAMS = {'w1_s1': (1.0, 1.0), 'w64_s0': (64.0, 0.0), 'w0.25_s1e-3': (0.25, 1e-3)}
KD = (2.0, 4.0)                                                  # alpha, T of the cases with a teacher
ABSENT = 7                                                       # relabelled to 3 in every target: the absent-class path runs
W19 = torch.rand(NC, generator=torch.Generator().manual_seed(4)) + 0.5
SCALE = 0.5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


_CACHE, _REFS = {}, {}


def _case(name):
    """the inputs of tests/test_gpu_distill.py (student and teacher logits of two seeds, 5 % ignored) with one class removed from the target;
    made once and left unchanged"""
    if name not in _CACHE:
        lo_hw, hi_hw = SHAPES[name]
        x = rand_tensor(31, 'kd_x', (N,) + lo_hw + (NC,)) * 3
        y = rand_tensor(33, 'kd_teacher', (N,) + lo_hw + (NC,)) * 3
        r = np.random.default_rng(9)
        t = torch.from_numpy(r.integers(0, NC, (N,) + hi_hw)).long()
        t[torch.from_numpy(r.random((N,) + hi_hw) < 0.05)] = 255
        t[t == ABSENT] = 3
        g0 = rand_tensor(32, 'kd_g0', (N,) + lo_hw + (LD,))
        _CACHE[name] = dict(x=x, y=y, t=t, g0=g0, lo_hw=lo_hw, hi_hw=hi_hw, name=name)
    return _CACHE[name]


def _refs(c, par, weighted=False, teacher=False, mask=None, ce=True, t=None):
    """(fp64, fp32) references of a case; without a mask they are computed once and shared"""
    key = (c['name'], par, weighted, teacher, ce) if mask is None and t is None else None
    if key is None or key not in _REFS:
        weight, smooth = PARAMS[par]
        kw = dict(class_w=W19 if weighted else None, mask=mask, scale=SCALE, ce=ce)
        if teacher:
            kw.update(teacher=c['y'], alpha=KD[0], T=KD[1])
        res = tuple(R.reference(c['x'], c['t'] if t is None else t, c['hi_hw'], weight, smooth, dtype=dt, **kw) for dt in (torch.float64, torch.float32))
        if key is None:
            return res
        _REFS[key] = res
    return _REFS[key]


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


def _stats_args(xa, ta, lo_hw, hi_hw, weight, smooth, coef, dout, loss, ws):
    import addk._lib as L
    (H, W), (OH, OW) = lo_hw, hi_hw
    a = L.DiceStatsArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, NC, OH, OW
    a.target, a.ignore_index, a.weight, a.smooth, a.scale = ta.data_ptr(), 255, weight, smooth, SCALE
    a.coef, a.dice_out, a.loss_out, a.ws = coef.data_ptr(), dout.data_ptr(), loss.data_ptr(), ws.data_ptr()
    return a


def _stats(dev, xa, ta, lo_hw, hi_hw, weight, smooth, loss=None):
    """one addk_dice_stats launch sequence on fresh outputs: the table and dice_out preset to NaN (they are written), the workspace dirty,
    loss at 0.25 unless handed in (it is accumulated).  Returns device tensors (coef, dice_out, loss, workspace as int32 words)."""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = lo_hw, hi_hw
    assert lib.addk_dice_stats_supported(N, H, W, OH, OW, NC) == 1
    coef, dout = torch.full((2 * NC,), float('nan'), device=dev), torch.full((1 + NC,), float('nan'), device=dev)
    if loss is None:
        loss = torch.full((1,), 0.25, device=dev)
    nb = int(lib.addk_dice_stats_ws_bytes(N, OH, OW))
    assert nb % 4 == 0
    ws = torch.full((nb // 4,), 0x7fc12345, dtype=torch.int32, device=dev)      # NaN patterns as floats, huge counts as integers
    a = _stats_args(xa, ta, lo_hw, hi_hw, weight, smooth, coef, dout, loss, ws)
    L.check(lib.addk_dice_stats(C.byref(a), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return coef, dout, loss, ws


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


def _fill_ce(a, xa, ta, lo_hw, hi_hw, wa, wsum, loss, g, ws, acc):
    (H, W), (OH, OW) = lo_hw, hi_hw
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, NC, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.wsum, a.scale, a.loss_out = wsum.data_ptr(), SCALE, loss.data_ptr()
    a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), LD, acc, ws.data_ptr()


def _head(dev, entry, xa, ta, lo_hw, hi_hw, wa, g0, acc, wsum, coef=None, lmap=None, tau=None, ya=None, nvalid=None, loss=None):
    """one launch sequence of a loss head on fresh outputs: entry 'dice' (addk_ce_upsample_dice_fwd_bwd), 'plain', 'ohem' or 'kd'.  Returns
    device tensors (loss, kd_out, g, workspace)."""
    import addk._lib as L
    lib = L.load()
    H, W = lo_hw
    if loss is None:
        loss = torch.full((1,), 0.25, device=dev)
    kd = torch.full((1,), float('nan'), device=dev)
    g = g0.clone().to(dev)
    ws = torch.full((int(lib.addk_ce_upsample_kd_ws_floats(N, H, W)),), 7.0, device=dev)
    if entry == 'plain':
        b = L.CeUpsampleArgs()
        _fill_ce(b, xa, ta, lo_hw, hi_hw, wa, wsum, loss, g, ws, acc)
        fn = lib.addk_ce_upsample_fwd_bwd
    elif entry == 'ohem':
        b = L.CeUpsampleOhemArgs()
        _fill_ce(b.ce, xa, ta, lo_hw, hi_hw, wa, wsum, loss, g, ws, acc)
        b.pix_loss, b.tau = lmap.data_ptr(), tau.data_ptr()
        fn = lib.addk_ce_upsample_ohem_fwd_bwd
    else:
        b = L.CeUpsampleDiceArgs() if entry == 'dice' else L.CeUpsampleKdArgs()
        k = b.kd if entry == 'dice' else b
        _fill_ce(k.ce, xa, ta, lo_hw, hi_hw, wa, wsum, loss, g, ws, acc)
        if lmap is not None:
            k.pix_loss, k.tau = lmap.data_ptr(), tau.data_ptr()
        if ya is not None:
            k.teacher, k.ld_teacher, k.alpha, k.temperature = ya.data_ptr(), ya.shape[-1], KD[0], KD[1]
            k.nvalid, k.kd_out = nvalid.data_ptr(), kd.data_ptr()
        if entry == 'dice':
            b.coef = coef.data_ptr()
        fn = lib.addk_ce_upsample_dice_fwd_bwd if entry == 'dice' else lib.addk_ce_upsample_kd_fwd_bwd
    L.check(fn(C.byref(b), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return loss, kd, g, ws


def _run(dev, c, par, xa, ta, wa, acc, wsum, **kw):
    """addk_dice_stats, then the head with its table, on one loss word that starts at 0.25; (loss, dice, g) on the host"""
    weight, smooth = PARAMS[par]
    coef, dout, loss, _ = _stats(dev, xa, ta, c['lo_hw'], c['hi_hw'], weight, smooth)
    loss, _, g, _ = _head(dev, 'dice', xa, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc, wsum, coef=coef, loss=loss, **kw)
    return loss.cpu(), dout[:1].cpu(), g.cpu()


def _check(tag, res, r64, r32, g0, acc):
    """(loss, dice, g) of the device against the fp64 and fp32 references at the bounds of the module docstring; prints what it measured"""
    la, da, ga = res
    loss, dice = float(la) - 0.25, float(da)
    e_loss, e_dice = abs(loss - r64['loss']), abs(dice - r64['dice'])
    b_loss = max(2e-6 * abs(r64['loss']), 4 * abs(r32['loss'] - r64['loss']))
    b_dice = max(2e-6 * abs(r64['dice']), 4 * abs(r32['dice'] - r64['dice']))
    base = g0[..., :NC].double() if acc else 0
    e64 = rel_err(ga[..., :NC].double(), r64['grad'] + base)
    e32 = rel_err(ga[..., :NC].double(), r32['grad'].double() + base)
    b64 = max(5e-5, 4 * rel_err(r32['grad'].double(), r64['grad']))
    print('dice %s: loss err %.2e rel (fp32 torch %.2e), term err %.2e rel (fp32 torch %.2e), grad %.2e vs fp64 (fp32 torch %.2e), %.2e vs fp32'
          % (tag, e_loss / abs(r64['loss']), abs(r32['loss'] - r64['loss']) / abs(r64['loss']), e_dice / abs(r64['dice']),
             abs(r32['dice'] - r64['dice']) / abs(r64['dice']), e64, rel_err(r32['grad'].double(), r64['grad']), e32))
    assert np.isfinite(loss) and np.isfinite(dice) and bool(torch.isfinite(ga).all())
    assert e_loss <= b_loss, (loss, r64['loss'], b_loss)
    assert e_dice <= b_dice, (dice, r64['dice'], b_dice)
    assert e64 <= b64, (e64, b64)
    assert e32 <= 1e-5, e32
    assert torch.equal(ga[..., NC:], g0[..., NC:])                                            # padding channels untouched


# ---- addk_dice_stats -------------------------------------------------------------------------------------------------------------

def _vec_close(tag, got, r64, r32):
    """per class: |got - fp64| <= max(2e-6 |fp64|, 4 |fp32 torch - fp64|); returns the largest relative error for the print"""
    got, a, b = got.double(), r64.double(), r32.double()
    err, bound = (got - a).abs(), torch.maximum(2e-6 * a.abs(), 4 * (b - a).abs())
    assert bool((err <= bound).all()), (tag, got, a, bound)
    nz = a.abs() > 0
    return float((err[nz] / a.abs()[nz]).max()) if bool(nz.any()) else 0.0, float(((b - a).abs()[nz] / a.abs()[nz]).max()) if bool(nz.any()) else 0.0


@pytest.mark.parametrize('ld', [24, 19], ids=['vec_ld24', 'scalar_ld19'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_dice_stats(dev, shape, ld):
    """1. Y_c exact; I_c, P_c, D_c, the table and the term against fp64 at the loss bound, for the three parameter pairs; both loaders; a
    dirty workspace and NaN-preset outputs; a second call gives equal bits; the absent class has D = -1 and a zero table row."""
    c = _case(shape)
    xa, ta = _padded(c['x'], dev, ld), c['t'].to(dev)
    assert (xa.data_ptr() % 16 == 0) and (ld % 4 == 0) == (ld == 24)
    for par, (weight, smooth) in PARAMS.items():
        r64, r32 = _refs(c, par, ce=False)
        out = [_stats(dev, xa, ta, c['lo_hw'], c['hi_hw'], weight, smooth) for _ in range(2)]
        for p, q in zip(out[0], out[1]):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32))                    # deterministic, whole workspace included
        coef, dout, loss, ws = (v.cpu() for v in out[0])
        Y = ws[:NC].long()
        assert torch.equal(Y, r64['Y'].long()) and int(Y[ABSENT]) == 0 and r64['m'] == NC - 1
        I, P = ws[32:32 + NC].view(torch.float32), ws[64:64 + NC].view(torch.float32)
        assert bool(torch.isfinite(coef).all()) and bool(torch.isfinite(dout).all())
        present = r64['present']
        eI = _vec_close('I', I, r64['I'], r32['I'])
        eP = _vec_close('P', P, r64['P'], r32['P'])
        eD = _vec_close('D', dout[1:][present], r64['D'][present], r32['D'][present])
        eA = _vec_close('A', coef[:NC], r64['A'], r32['A'])
        eB = _vec_close('B', coef[NC:], r64['B'], r32['B'])
        assert float(dout[1 + ABSENT]) == -1.0 and float(coef[ABSENT]) == 0.0 and float(coef[NC + ABSENT]) == 0.0
        dice = float(dout[0])
        e, b = abs(dice - r64['dice']), max(2e-6 * abs(r64['dice']), 4 * abs(r32['dice'] - r64['dice']))
        print('dice_stats %s ld%d %s: rel err device (fp32 torch) I %.1e (%.1e) P %.1e (%.1e) D %.1e (%.1e) A %.1e (%.1e) B %.1e (%.1e) term %.1e (%.1e)'
              % ((shape, ld, par) + eI + eP + eD + eA + eB + (e / abs(r64['dice']), abs(r32['dice'] - r64['dice']) / abs(r64['dice']))))
        assert e <= b, (dice, r64['dice'], b)
        assert float(loss) == float(torch.tensor(0.25) + dout[0])                            # the loss word accumulated the term, once


def test_dice_stats_every_pixel_ignored(dev):
    """2. m == 0: an all-zero table, dice == 0 exactly, -1 for every class, the loss word untouched."""
    c = _case('x3.8')
    xa, ta = _padded(c['x'], dev, LD), torch.full_like(c['t'], 255).to(dev)
    coef, dout, loss, ws = _stats(dev, xa, ta, c['lo_hw'], c['hi_hw'], 64.0, 0.0)
    assert torch.equal(coef.cpu(), torch.zeros(2 * NC)) and float(dout[0]) == 0.0 and float(loss) == 0.25
    assert torch.equal(dout[1:].cpu(), torch.full((NC,), -1.0)) and torch.equal(ws[:NC].cpu(), torch.zeros(NC, dtype=torch.int32))


def test_dice_stats_bad_arguments_are_refused_without_a_launch(dev):
    """3."""
    import addk._lib as L
    lib = L.load()
    c = _case('x1')
    xa, ta = _padded(c['x'], dev, LD), c['t'].to(dev)
    f = dict(device=dev)
    coef, dout, loss = torch.full((2 * NC,), 7.0, **f), torch.full((1 + NC,), 7.0, **f), torch.full((1,), 7.0, **f)
    ws = torch.full((int(lib.addk_dice_stats_ws_bytes(N, *c['hi_hw'])) // 4,), 7.0, **f)
    st = torch.cuda.current_stream().cuda_stream
    inf, nan = float('inf'), float('nan')
    bad = [dict(logits=None), dict(target=None), dict(coef=None), dict(dice_out=None), dict(loss_out=None), dict(ws=None), dict(ld=18), dict(C=7),
           dict(weight=0.0), dict(weight=-1.0), dict(weight=nan), dict(weight=inf), dict(smooth=-1e-3), dict(smooth=nan), dict(smooth=inf)]
    for kw in bad:
        a = _stats_args(xa, ta, c['lo_hw'], c['hi_hw'], 1.0, 1.0, coef, dout, loss, ws)
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.addk_dice_stats(C.byref(a), st) == -1, kw
    torch.cuda.synchronize()
    for v in (coef, dout, loss, ws):
        assert float(v.min()) == float(v.max()) == 7.0


# ---- the head: loss and gradient ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('par', list(PARAMS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_loss_term_and_gradient_match_reference(dev, shape, par):
    """4. without and with class weights into a fresh gradient, and with class weights accumulated into an existing one; two runs bit-equal.  At
    weight = 64 the Dice part of the fp64 reference's gradient is at least as large as the cross-entropy part (asserted): the gradient
    bound there is a bound on the new code."""
    c = _case(shape)
    xa, ta = _padded(c['x'], dev, LD), c['t'].to(dev)
    for weighted, acc in ((False, 0), (True, 0), (True, 1)):
        wa = W19.to(dev) if weighted else None
        wsum = _count(dev, ta, wa)
        r64, r32 = _refs(c, par, weighted)
        if par == 'w64_s0' and not acc:
            gd = _refs(c, par, ce=False)[0]['grad']
            nd, nc = float(gd.norm()), float((r64['grad'] - gd).norm())
            print('dice %s %s: |g_dice| %.3e, |g_ce| %.3e (fp64 reference)' % (shape, par, nd, nc))
            assert nd >= nc, (nd, nc)
        res = [_run(dev, c, par, xa, ta, wa, acc, wsum) for _ in range(2)]
        assert all(torch.equal(p, q) for p, q in zip(res[0], res[1]))                       # deterministic
        _check('%s %s %s' % (shape, par, 'weighted+acc' if acc else 'weighted' if weighted else 'plain'), res[0], r64, r32, c['g0'], acc)
        assert r64['dice'] > 0 and float(res[0][1]) > 0


@pytest.mark.parametrize('shape', list(SHAPES))
def test_with_a_kept_set(dev, shape):
    """5. mining (regime `half` of tests/test_gpu_ohem.py: tau is the median loss) filters the cross-entropy term only: the reference takes
    the DEVICE's mask for CE and every valid pixel for the Dice term, and the term is that of the unfiltered run, bit for bit."""
    c = _case(shape)
    par = 'w64_s0'
    xa, ta = _padded(c['x'], dev, LD), c['t'].to(dev)
    nv = int((c['t'] != 255).sum())
    for weighted, acc in ((False, 0), (True, 1)):
        wa = W19.to(dev) if weighted else None
        lmap, tau, wk, counts = _select(dev, xa, ta, c['lo_hw'], c['hi_hw'], 0.01, nv // 2, wa)
        mask = lmap.cpu() >= float(tau)
        assert int(mask.sum()) == int(counts[1]) and nv // 2 <= int(counts[1]) < nv
        r64, r32 = _refs(c, par, weighted, mask=mask)
        res = [_run(dev, c, par, xa, ta, wa, acc, wk, lmap=lmap, tau=tau) for _ in range(2)]
        assert all(torch.equal(p, q) for p, q in zip(res[0], res[1]))
        _check('%s kept set %s' % (shape, 'weighted+acc' if acc else 'plain'), res[0], r64, r32, c['g0'], acc)
        full = _run(dev, c, par, xa, ta, wa, acc, _count(dev, ta, wa))
        assert torch.equal(full[1], res[0][1])                                               # the term: mining never touches it
        assert not torch.equal(full[2], res[0][2])                                           # the gradient: its CE part did change


@pytest.mark.parametrize('mined', [False, True], ids=['teacher', 'teacher+kept_set'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_with_a_teacher(dev, shape, mined):
    """6. with the distillation term (teacher ld = 20), and with both the teacher and a kept set: cross-entropy + KL + Dice."""
    c = _case(shape)
    par = 'w64_s0'
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    nv = int(nvalid.item())
    for weighted, acc in ((False, 0), (True, 1)):
        wa = W19.to(dev) if weighted else None
        kw, mask, wsum = dict(ya=ya, nvalid=nvalid), None, _count(dev, ta, wa)
        if mined:
            lmap, tau, wsum, counts = _select(dev, xa, ta, c['lo_hw'], c['hi_hw'], 0.01, nv // 2, wa)
            mask = lmap.cpu() >= float(tau)
            kw.update(lmap=lmap, tau=tau)
        r64, r32 = _refs(c, par, weighted, teacher=True, mask=mask)
        res = [_run(dev, c, par, xa, ta, wa, acc, wsum, **kw) for _ in range(2)]
        assert all(torch.equal(p, q) for p, q in zip(res[0], res[1]))
        _check('%s teacher%s %s' % (shape, '+kept set' if mined else '', 'weighted+acc' if acc else 'plain'), res[0], r64, r32, c['g0'], acc)


# ---- wiring ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', list(SHAPES))
def test_zero_table_leaves_the_other_entry_points(dev, shape):
    """7. with an all-zero coefficient table the Dice entry point's g, loss and loss partials are the plain, the mining and the
    distillation entry point's, bit for bit."""
    c = _case(shape)
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    zero = torch.zeros(2 * NC, device=dev)
    nv = int(nvalid.item())
    for weighted, acc in ((False, 0), (True, 1)):
        wa = W19.to(dev) if weighted else None
        wsum = _count(dev, ta, wa)
        lmap, tau, wk, _ = _select(dev, xa, ta, c['lo_hw'], c['hi_hw'], 0.01, nv // 2, wa)
        args = (xa, ta, c['lo_hw'], c['hi_hw'], wa, c['g0'], acc)
        for entry, norm, kw in (('plain', wsum, {}), ('ohem', wk, dict(lmap=lmap, tau=tau)), ('kd', wsum, dict(ya=ya, nvalid=nvalid)),
                                ('kd', wk, dict(ya=ya, nvalid=nvalid, lmap=lmap, tau=tau))):
            ref = _head(dev, entry, *args, norm, **kw)
            got = _head(dev, 'dice', *args, norm, coef=zero, **kw)
            for p, q in zip(ref, got):
                assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (entry, sorted(kw))


def test_head_bad_arguments_are_refused_without_a_launch(dev):
    """8."""
    import addk._lib as L
    lib = L.load()
    c = _case('x1')
    H, W = c['lo_hw']
    xa, ya, ta = _padded(c['x'], dev, LD), _padded(c['y'], dev, LDT), c['t'].to(dev)
    nvalid = _count(dev, ta, None)
    f = dict(device=dev)
    g, loss, kd, coef = torch.full((N, H, W, LD), 7.0, **f), torch.full((1,), 7.0, **f), torch.full((1,), 7.0, **f), torch.zeros(2 * NC, **f)
    ws = torch.full((int(lib.addk_ce_upsample_kd_ws_floats(N, H, W)),), 7.0, **f)
    lmap, tau = torch.zeros((N,) + c['hi_hw'], **f), torch.zeros(1, **f)
    st = torch.cuda.current_stream().cuda_stream

    def args(student, **kw):
        b = L.CeUpsampleDiceArgs()
        _fill_ce(b.kd.ce, xa, ta, c['lo_hw'], c['hi_hw'], None, nvalid, loss, g, ws, 0)
        b.coef = coef.data_ptr()
        if student:
            b.kd.teacher, b.kd.ld_teacher, b.kd.alpha, b.kd.temperature = ya.data_ptr(), LDT, 1.0, 4.0
            b.kd.nvalid, b.kd.kd_out = nvalid.data_ptr(), kd.data_ptr()
        for k, v in kw.items():
            setattr(b if k == 'coef' else b.kd if hasattr(L.CeUpsampleKdArgs, k) and k != 'ce' else b.kd.ce, k, v)
        return b
    nan = float('nan')
    bad = [(0, dict(coef=None)), (0, dict(logits=None)), (0, dict(target=None)), (0, dict(wsum=None)), (0, dict(loss_out=None)), (0, dict(g=None)),
           (0, dict(ws=None)), (0, dict(ld=18)), (0, dict(ldg=18)), (0, dict(C=7)), (0, dict(pix_loss=lmap.data_ptr())), (0, dict(tau=tau.data_ptr())),
           (1, dict(coef=None)), (1, dict(nvalid=None)), (1, dict(kd_out=None)), (1, dict(teacher=xa.data_ptr())), (1, dict(ld_teacher=18)),
           (1, dict(alpha=0.0)), (1, dict(alpha=nan)), (1, dict(temperature=0.0)), (1, dict(temperature=float('inf')))]
    for student, kw in bad:
        assert lib.addk_ce_upsample_dice_fwd_bwd(C.byref(args(student, **kw)), st) == -1, (student, kw)
    torch.cuda.synchronize()
    for v in (g, loss, kd, ws):
        assert float(v.min()) == float(v.max()) == 7.0
    for student in (0, 1):                                           # the blocks themselves are good
        assert lib.addk_ce_upsample_dice_fwd_bwd(C.byref(args(student)), st) == 0
    torch.cuda.synchronize()


# ---- the training step -------------------------------------------------------------------------------------------------------------

SHAPE = (2, 3, 65, 129)
ARGS = (ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), 0)
DICE = (1.0, 1.0)


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
    t[t == ABSENT] = 3
    return x, t


def _fwd_bwd(dev, **kw):
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:])
    ma = _model(dev)
    ts = TrainStep(ma, SHAPE, use_graph=False, **kw)
    ts.load_batch(x.to(dev), t.to(dev))
    ts.forward_backward_only()
    torch.cuda.synchronize()
    names = {p: k for k, p in ma.named_parameters()}
    return ts, {names[p]: g.double().cpu() for p, g in ts.grads().items() if g is not None}


def _oracle_runs(t, dice, distill=None, masks=None):
    """the oracle model in fp32 and fp64 with the step's loss written in torch: per exit CE (over the kept mask of that exit, when given) +
    the distillation term for every exit but the last + the Dice term, averaged over the exits.  name -> (loss, grads, [term per exit], [D])"""
    import torch.nn.functional as Fn
    x, _ = _batch(SHAPE[2:])
    valid = t != 255
    tc = torch.where(valid, t, torch.zeros_like(t))
    res = {}
    for name, dt in (('o32', torch.float32), ('o64', torch.float64)):
        m = _oracle().to(dt)
        m.train()
        ys = m(x.to(dt))
        loss, terms, Ds = 0, [], []
        for i, y in enumerate(ys):
            if masks is None:
                ce = Fn.cross_entropy(y, t, ignore_index=255)
            else:
                nll = -torch.log_softmax(y, dim=1).gather(1, tc[:, None]).squeeze(1)
                w = masks[i].to(dt)
                ce = (w * nll).sum() / w.sum()
            d, (_, _, Y, D) = R.dice_term(y, t, valid, *dice)
            loss = loss + ce + d
            if distill is not None and i < len(ys) - 1:
                loss = loss + RD.kd_term(y, ys[-1], valid, *distill)
            terms.append(float(d.detach()) / len(ys))
            Ds.append([float(v) if float(n) > 0 else None for v, n in zip(D.detach(), Y)])
        loss = loss / len(ys)
        loss.backward()
        res[name] = (loss.item(), {k: p.grad.double() for k, p in m.named_parameters()}, terms, Ds)
    return res


def _check_step(tag, ts, ga, res):
    """loss and parameter gradients at the bounds of tests/test_gpu_train.py::test_train_step_forward_backward_and_sgd; dice_stats() at the
    bound of the loss (the term is a part of that loss, computed from the same logits): 3 x the fp32 oracle's own error + 1e-4 relative,
    and the same in absolute terms for the per-class scores, which lie in [0, 1]."""
    la = ts.loss.item()
    o64, o32 = res['o64'], res['o32']
    assert abs(la - o64[0]) <= 3 * abs(o32[0] - o64[0]) + 1e-4 * abs(la), (la, o64[0], o32[0])
    g64 = o64[1]

    def rel_l2(gx):
        return (sum(float(((gx[k] - g64[k]) ** 2).sum()) for k in g64) / sum(float((g64[k] ** 2).sum()) for k in g64)) ** 0.5
    assert set(ga) == set(g64)
    print('dice step %s: loss %.6f (fp64 %.6f, fp32 %.6f), rel_l2 %.2e (fp32 torch %.2e)' % (tag, la, o64[0], o32[0], rel_l2(ga), rel_l2(o32[1])))
    assert rel_l2(ga) <= 2.0 * rel_l2(o32[1]) + 1e-3
    stats = ts.dice_stats()
    assert len(stats) == len(o64[2])
    for i, (term, D) in enumerate(stats):
        print('dice step %s exit %d: term %.6e (fp64 %.6e, fp32 %.6e)' % (tag, i, term, o64[2][i], o32[2][i]))
        assert abs(term - o64[2][i]) <= 3 * abs(o32[2][i] - o64[2][i]) + 1e-4 * abs(term)
        assert [d is None for d in D] == [d is None for d in o64[3][i]] and D[ABSENT] is None and sum(d is None for d in D) == 1
        for d, d64, d32 in zip(D, o64[3][i], o32[3][i]):
            assert d is None or abs(d - d64) <= 3 * abs(d32 - d64) + 1e-4


def test_step_against_the_oracle(dev):
    """9. forward_backward_only with dice=(1, 1) against the oracle model in fp32 and fp64 with the same term added (the oracle's
    full-resolution outputs are the bilinear samples of its low-resolution logits); dice=None gives the loss bits of a step built without
    the keyword, and another loss than the step with the term."""
    _, t = _batch(SHAPE[2:])
    ts, ga = _fwd_bwd(dev, dice=DICE)
    names = [c.name for c in ts.g.bwd]
    assert names.count('dice_stats') == 2 and names.count('ce_upsample_dice') == 2 and names.count('ce_upsample') == 0
    _check_step('dice', ts, ga, _oracle_runs(t, DICE))
    t0, _ = _fwd_bwd(dev)
    t1, _ = _fwd_bwd(dev, dice=None)
    assert torch.equal(t0.loss.view(torch.int32), t1.loss.view(torch.int32)) and [c.name for c in t0.g.bwd] == [c.name for c in t1.g.bwd]
    assert float(ts.loss) > float(t0.loss)


def test_step_with_ohem_and_distill_against_the_oracle(dev):
    """10. dice with ohem and distill together: the oracle takes each exit's kept mask from the DEVICE's map and tau."""
    _, t = _batch(SHAPE[2:])
    distill = (1.0, 4.0)
    ts, ga = _fwd_bwd(dev, dice=DICE, ohem=(0.7, 2000), distill=distill)
    names = [c.name for c in ts.g.bwd]
    assert names.count('ohem_select') == 2 and names.count('dice_stats') == 2 and names.count('ce_upsample_dice') == 2
    masks = []
    for o in ts.outs:
        st = o.binding['ohem_state']
        masks.append(st['pix_loss'].cpu() >= float(st['tau']))
    _check_step('dice+ohem+distill', ts, ga, _oracle_runs(t, DICE, distill, masks))
    assert all(np.isfinite(v) and v > 0 for v in ts.distill_stats())


@pytest.mark.parametrize('more', [{}, dict(ohem=(0.7, 2000), distill=(1.0, 4.0))], ids=['dice', 'dice+ohem+distill'])
def test_step_replayed_graph_equals_eager(dev, more):
    """11. after enable_capture() the step is one hipGraph; four steps give the loss, the terms, the scores and the parameters of four eager
    steps, bit for bit; dice_out is written every step, not accumulated."""
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:])
    res = {}
    for mode in ('eager', 'graph'):
        ts = TrainStep(_model(dev), SHAPE, use_graph=False, dice=DICE, **more)
        ts.load_batch(x.to(dev), t.to(dev))
        if mode == 'graph':
            ts.enable_capture()
        ls = []
        for _ in range(4):                                         # graph: one eager step that is then captured, three replays
            l = ts.step().item()
            ls.append((l, ts.dice_stats()))
        torch.cuda.synchronize()
        assert (ts.graph is not None) == (mode == 'graph')
        res[mode] = (ls, ts.flat_p.clone())
        ts.close()
    assert res['graph'][0] == res['eager'][0], (res['graph'][0], res['eager'][0])
    assert torch.equal(res['graph'][1], res['eager'][1])
    terms = [st[0][0] for _, st in res['eager'][0]]
    assert all(np.isfinite(v) and 0 < v < 0.5 for v in terms) and len(set(terms)) == 4
