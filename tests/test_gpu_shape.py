"""GPU tests of the two per-pixel loss shapes of the fused loss head: addk_ce_upsample_shaped_fwd_bwd (focal loss and label-smoothed
cross-entropy; alone, with a kept set from addk_ohem_select, with the coefficient table of addk_dice_stats, with both; at 19 and 21 classes,
on the vector-load and the dense pixel stride) and train.TrainStep(focal=..., label_smoothing=...).

Bounds of the kernel tests, the form of tests/test_gpu_dice.py, nothing fixed ahead against the code under test: the loss within
max(2e-6 |fp64|, 4 |fp32 torch reference - fp64|), the gradient's rel_err against fp64 within max(5e-5, 4 rel_err(fp32 torch reference,
fp64)); the references are tests/_shape_ref.py on the same inputs.  Bounds of the step tests: those of
tests/test_gpu_dice.py::test_step_against_the_oracle.  Measured errors: DESIGN.md section 37."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle                                                   # noqa: E402
import _shape_ref as R                                          # noqa: E402
from _dice_ref import dice_term                                 # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor, rel_err   # noqa: E402

N, SCALE = 2, 0.5
SHAPES = {'x8': ((16, 32), (128, 256)), 'x3.8': ((17, 33), (65, 129)), 'x1': ((33, 65), (33, 65))}
STRIDES = {19: {'vec': 20, 'dense': 19}, 21: {'vec': 24, 'dense': 21}}
FOCAL, SMOOTH = (1.0, 2.0, 3.5), (0.1, 0.3)
KINDS = [('focal', g) for g in FOCAL] + [('smooth', e) for e in SMOOTH]
DICE = (64.0, 0.0)                                               # weight, smooth of the cases with a table: the Dice gradient is no small part
WEIGHTS = {nc: torch.rand(nc, generator=torch.Generator().manual_seed(4)) + 0.5 for nc in (19, 21)}
GEOM = [(s, nc, ld) for s in SHAPES for nc in (19, 21) for ld in ('vec', 'dense')]
GEOM_IDS = ['%s-%d-%s' % g for g in GEOM]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


_CACHE, _REFS = {}, {}


def _case(shape, nc, mul=1.0):
    """low-resolution logits (rand * 3, times `mul`), a target with 5 % ignored pixels and a gradient to accumulate onto; made once and
    left unchanged"""
    key = (shape, nc, mul)
    if key not in _CACHE:
        lo_hw, hi_hw = SHAPES[shape]
        x = rand_tensor(31, 'shape_x', (N,) + lo_hw + (nc,)) * 3 * mul
        r = np.random.default_rng(9)
        t = torch.from_numpy(r.integers(0, nc, (N,) + hi_hw)).long()
        t[torch.from_numpy(r.random((N,) + hi_hw) < 0.05)] = 255
        g0 = rand_tensor(32, 'shape_g0', (N,) + lo_hw + (24,))
        _CACHE[key] = dict(x=x, t=t, g0=g0, lo_hw=lo_hw, hi_hw=hi_hw, nc=nc, key=key)
    return _CACHE[key]


def _refs(c, kind, value, weighted=False, mask=None, dice=None, t=None):
    """(fp64, fp32) references of a case; without a mask they are computed once and shared (between the strides, and the two accumulate modes)"""
    key = (c['key'], kind, value, weighted, dice) if mask is None and t is None else None
    if key is None or key not in _REFS:
        kw = dict(class_w=WEIGHTS[c['nc']] if weighted else None, mask=mask, scale=SCALE, dice=dice)
        kw['focal' if kind == 'focal' else 'smooth'] = value
        res = tuple(R.reference(c['x'], c['t'] if t is None else t, c['hi_hw'], dtype=dt, **kw) for dt in (torch.float64, torch.float32))
        if key is None:
            return res
        _REFS[key] = res
    return _REFS[key]


def _padded(x, dev, ld):
    xa = torch.zeros(x.shape[:3] + (ld,), device=dev)
    xa[..., :x.shape[-1]] = x.to(dev)
    return xa


def _count(dev, ta, wa, nc):
    """addk_ce_count: the weight sum of the valid pixels (wa None: their number)"""
    import addk._lib as L
    lib = L.load()
    out = torch.zeros(1, device=dev)
    ws = torch.zeros(int(lib.addk_ce_ws_floats(N, ta[0].numel())), device=dev)
    L.check(lib.addk_ce_count(ta.data_ptr(), ta.numel(), wa.data_ptr() if wa is not None else None, 255, nc, out.data_ptr(), ws.data_ptr(),
                              torch.cuda.current_stream().cuda_stream))
    return out


def _select(dev, xa, ta, c, thresh, K, wa):
    """addk_ohem_select; returns (map, tau, wsum_kept, counts) on the device"""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = c['lo_hw'], c['hi_hw']
    f = dict(device=dev)
    lmap, tau, wk = torch.zeros((N, OH, OW), **f), torch.zeros(1, **f), torch.zeros(1, **f)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.addk_ohem_select_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    a = L.OhemSelectArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, c['nc'], OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.thresh, a.min_kept_total = thresh, K
    a.pix_loss, a.tau, a.wsum_kept, a.counts, a.ws = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr(), ws.data_ptr()
    L.check(lib.addk_ohem_select(C.byref(a), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lmap, tau, wk, counts


def _stats(dev, xa, ta, c, loss):
    """addk_dice_stats with DICE's parameters: the term is added to `loss`; returns (coefficient table, dice_out)"""
    import addk._lib as L
    lib = L.load()
    (H, W), (OH, OW) = c['lo_hw'], c['hi_hw']
    nc = c['nc']
    assert lib.addk_dice_stats_supported(N, H, W, OH, OW, nc) == 1
    coef, dout = torch.full((2 * nc,), float('nan'), device=dev), torch.full((1 + nc,), float('nan'), device=dev)
    ws = torch.zeros(int(lib.addk_dice_stats_ws_bytes_classes(N, OH, OW, nc)), dtype=torch.uint8, device=dev)
    a = L.DiceStatsArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, nc, OH, OW
    a.target, a.ignore_index, a.weight, a.smooth, a.scale = ta.data_ptr(), 255, DICE[0], DICE[1], SCALE
    a.coef, a.dice_out, a.loss_out, a.ws = coef.data_ptr(), dout.data_ptr(), loss.data_ptr(), ws.data_ptr()
    L.check(lib.addk_dice_stats(C.byref(a), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return coef, dout


def _fill_ce(a, xa, ta, c, wa, wsum, loss, g, ws, acc):
    (H, W), (OH, OW) = c['lo_hw'], c['hi_hw']
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), xa.shape[-1], N, H, W, c['nc'], OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.wsum, a.scale, a.loss_out = wsum.data_ptr(), SCALE, loss.data_ptr()
    a.g, a.ldg, a.accumulate, a.ws = g.data_ptr(), g.shape[-1], acc, ws.data_ptr()


def _shape_words(b, kind, value):
    import addk._lib as L
    b.shape = {'none': L.CE_SHAPE_NONE, 'focal': L.CE_SHAPE_FOCAL, 'smooth': L.CE_SHAPE_SMOOTH}[kind]
    b.gamma, b.eps = (value, 0.0) if kind == 'focal' else (0.0, value) if kind == 'smooth' else (float('nan'), float('nan'))


def _head(dev, entry, xa, ta, c, wa, acc, wsum, kind='none', value=None, coef=None, lmap=None, tau=None, loss=None):
    """one launch sequence of a loss head on fresh outputs: entry 'shaped' (addk_ce_upsample_shaped_fwd_bwd), 'plain', 'ohem' or 'dice'.  The
    gradient starts as the case's g0 (its first ld channels), the workspace dirty, the loss word at 0.25 unless handed in.  Returns device
    tensors (loss, g, workspace)."""
    import addk._lib as L
    lib = L.load()
    H, W = c['lo_hw']
    if loss is None:
        loss = torch.full((1,), 0.25, device=dev)
    g = c['g0'][..., :xa.shape[-1]].clone().to(dev)
    ws = torch.full((int(lib.addk_ce_upsample_ws_floats(N, H, W)),), 7.0, device=dev)
    if entry == 'plain':
        b = L.CeUpsampleArgs()
        _fill_ce(b, xa, ta, c, wa, wsum, loss, g, ws, acc)
        fn = lib.addk_ce_upsample_fwd_bwd
    elif entry == 'ohem':
        b = L.CeUpsampleOhemArgs()
        _fill_ce(b.ce, xa, ta, c, wa, wsum, loss, g, ws, acc)
        b.pix_loss, b.tau = lmap.data_ptr(), tau.data_ptr()
        fn = lib.addk_ce_upsample_ohem_fwd_bwd
    else:
        b = L.CeUpsampleShapedArgs() if entry == 'shaped' else L.CeUpsampleDiceArgs()
        d = b.dice if entry == 'shaped' else b
        _fill_ce(d.kd.ce, xa, ta, c, wa, wsum, loss, g, ws, acc)
        if lmap is not None:
            d.kd.pix_loss, d.kd.tau = lmap.data_ptr(), tau.data_ptr()
        if coef is not None:
            d.coef = coef.data_ptr()
        if entry == 'shaped':
            _shape_words(b, kind, value)
        fn = lib.addk_ce_upsample_shaped_fwd_bwd if entry == 'shaped' else lib.addk_ce_upsample_dice_fwd_bwd
    L.check(fn(C.byref(b), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return loss, g, ws


_WORST = {}


def _check(tag, kind, loss, ga, r64, r32, g0, acc, nc):
    """loss and gradient of the device against the fp64 and fp32 references at the bounds of the module docstring; prints what it measured"""
    loss = float(loss) - 0.25
    e_loss = abs(loss - r64['loss'])
    b_loss = max(2e-6 * abs(r64['loss']), 4 * abs(r32['loss'] - r64['loss']))
    ga = ga.cpu()
    base = g0[..., :nc].double() if acc else 0
    e64 = rel_err(ga[..., :nc].double(), r64['grad'] + base)
    r32e = rel_err(r32['grad'].double(), r64['grad'])
    b64 = max(5e-5, 4 * r32e)
    print('shape %s: loss err %.2e rel (fp32 torch %.2e), grad %.2e vs fp64 (fp32 torch %.2e)'
          % (tag, e_loss / abs(r64['loss']), abs(r32['loss'] - r64['loss']) / abs(r64['loss']), e64, r32e))
    w = _WORST.setdefault(kind, [0.0, 0.0])
    w[0], w[1] = max(w[0], e_loss / abs(r64['loss'])), max(w[1], e64)
    print('shape worst so far (%s): loss %.2e rel, grad %.2e' % (kind, w[0], w[1]))
    assert np.isfinite(loss) and bool(torch.isfinite(ga).all())
    assert e_loss <= b_loss, (loss, r64['loss'], r32['loss'], b_loss)
    assert e64 <= b64, (e64, b64)
    assert torch.equal(ga[..., nc:], g0[..., nc:ga.shape[-1]])                               # padding channels untouched


# ---- the head: loss and gradient ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,nc,ld', GEOM, ids=GEOM_IDS)
def test_loss_and_gradient_match_reference(dev, shape, nc, ld):
    """1. focal gamma 1, 2, 3.5 and smoothing eps 0.1, 0.3: without and with class weights into a fresh gradient, and with class weights
    accumulated onto an existing one; two runs bit-equal."""
    c = _case(shape, nc)
    xa, ta = _padded(c['x'], dev, STRIDES[nc][ld]), c['t'].to(dev)
    assert xa.data_ptr() % 16 == 0 and (xa.shape[-1] % 4 == 0) == (ld == 'vec')
    for kind, value in KINDS:
        for weighted, acc in ((False, 0), (True, 0), (True, 1)):
            wa = WEIGHTS[nc].to(dev) if weighted else None
            wsum = _count(dev, ta, wa, nc)
            r64, r32 = _refs(c, kind, value, weighted)
            res = [_head(dev, 'shaped', xa, ta, c, wa, acc, wsum, kind, value) for _ in range(2)]
            assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(res[0], res[1]))       # deterministic
            tag = '%s %d %s %s=%g %s' % (shape, nc, ld, kind, value, 'weighted+acc' if acc else 'weighted' if weighted else 'plain')
            _check(tag, kind + (' accumulated' if acc else ''), res[0][0], res[0][1], r64, r32, c['g0'], acc, nc)
    # the shapes are shapes: (1 - p_t)^2 < 1 makes the focal loss the smaller one, and eps moves the loss away from the plain head's
    wsum = _count(dev, ta, None, nc)
    plain = float(_head(dev, 'plain', xa, ta, c, None, 0, wsum)[0])
    assert float(_head(dev, 'shaped', xa, ta, c, None, 0, wsum, 'focal', 2.0)[0]) < plain
    assert float(_head(dev, 'shaped', xa, ta, c, None, 0, wsum, 'smooth', 0.3)[0]) != plain


@pytest.mark.parametrize('shape,nc,ld', GEOM, ids=GEOM_IDS)
def test_with_a_kept_set_a_dice_table_and_both(dev, shape, nc, ld):
    """2. mining (tau is the median plain per-pixel loss: addk_ohem_select chooses on the plain cross-entropy) filters the shaped term and its
    normaliser; the Dice term goes by the plain predicate.  The reference takes the DEVICE's mask; addk_dice_stats adds the term to the loss
    word the head then accumulates into.  Both shapes, each without and with class weights into a FRESH gradient — there the bound is a
    bound on what the kernel produced — and with class weights accumulated onto an existing one."""
    c = _case(shape, nc)
    xa, ta = _padded(c['x'], dev, STRIDES[nc][ld]), c['t'].to(dev)
    nv = int((c['t'] != 255).sum())
    for weighted in (False, True):
        wa = WEIGHTS[nc].to(dev) if weighted else None
        lmap, tau, wk, counts = _select(dev, xa, ta, c, 0.01, nv // 2, wa)
        mask = lmap.cpu() >= float(tau)
        assert int(mask.sum()) == int(counts[1]) and nv // 2 <= int(counts[1]) < nv
        wsum = _count(dev, ta, wa, nc)
        for kind, value in (('focal', 2.0), ('smooth', 0.1)):
            for mined, table in ((True, False), (False, True), (True, True)):
                r64, r32 = _refs(c, kind, value, weighted, mask=mask if mined else None, dice=DICE if table else None)
                for acc in (0, 1) if weighted else (0,):
                    res = []
                    for _ in range(2):
                        loss = torch.full((1,), 0.25, device=dev)
                        coef = _stats(dev, xa, ta, c, loss)[0] if table else None
                        kw = dict(lmap=lmap, tau=tau) if mined else {}
                        res.append(_head(dev, 'shaped', xa, ta, c, wa, acc, wk if mined else wsum, kind, value, coef=coef, loss=loss, **kw))
                    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(res[0], res[1]))
                    tag = '%s %d %s %s=%g%s%s %s' % (shape, nc, ld, kind, value, ' kept set' * mined, ' dice' * table,
                                                     'weighted+acc' if acc else 'weighted' if weighted else 'plain')
                    _check(tag, kind + (' with more, accumulated' if acc else ' with more, fresh'), res[0][0], res[0][1], r64, r32, c['g0'], acc, nc)


# ---- edge cases --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nc', [19, 21])
@pytest.mark.parametrize('kind,value', [('focal', 2.0), ('focal', 1.0), ('smooth', 0.1)])
def test_every_pixel_ignored(dev, kind, value, nc):
    """3. n == 0 (the count word of addk_ce_count is 0): the loss word gets exactly 0, g is 0 (or what it was, with accumulate), nothing is
    non-finite; alone, and with the all-zero table addk_dice_stats leaves for such a batch."""
    c = _case('x3.8', nc)
    t = torch.full_like(c['t'], 255)
    xa, ta = _padded(c['x'], dev, STRIDES[nc]['vec']), t.to(dev)
    for weighted in (False, True):
        wa = WEIGHTS[nc].to(dev) if weighted else None
        wsum = _count(dev, ta, wa, nc)
        assert float(wsum) == 0.0
        for acc in (0, 1):
            for table in (False, True):
                loss = torch.full((1,), 0.25, device=dev)
                coef = _stats(dev, xa, ta, c, loss)[0] if table else None
                assert coef is None or float(coef.abs().max()) == 0.0
                loss, g, ws = _head(dev, 'shaped', xa, ta, c, wa, acc, wsum, kind, value, coef=coef, loss=loss)
                assert float(loss) == 0.25 and bool(torch.isfinite(ws).all()) and float(ws.abs().max()) == 0.0
                want = c['g0'][..., :xa.shape[-1]].clone()
                if not acc:
                    want[..., :nc] = 0
                assert torch.equal(g.cpu(), want)


@pytest.mark.parametrize('nc', [19, 21])
@pytest.mark.parametrize('kind,value', [('focal', 1.0), ('focal', 2.0), ('focal', 3.5), ('smooth', 0.1), ('smooth', 0.3)])
def test_logits_scaled_by_30(dev, kind, value, nc):
    """4. logits of magnitude ~100: p_t reaches 1 and 0 in fp32 (asserted on the fp32 reference's softmax).  Everything finite, the same bounds."""
    c = _case('x3.8', nc, mul=30.0)
    xr, up = R.upsample(c['x'], c['hi_hw'], torch.float32)
    p = torch.softmax(up.detach(), 1)
    valid = c['t'] != 255
    pt = p.gather(1, torch.where(valid, c['t'], torch.zeros_like(c['t']))[:, None]).squeeze(1)[valid]
    assert float(pt.max()) == 1.0 and float(pt.min()) == 0.0
    xa, ta = _padded(c['x'], dev, STRIDES[nc]['vec']), c['t'].to(dev)
    for weighted, acc in ((False, 0), (True, 0), (True, 1)):
        wa = WEIGHTS[nc].to(dev) if weighted else None
        wsum = _count(dev, ta, wa, nc)
        r64, r32 = _refs(c, kind, value, weighted)
        loss, g, ws = _head(dev, 'shaped', xa, ta, c, wa, acc, wsum, kind, value)
        assert bool(torch.isfinite(ws).all())
        _check('x30 %d %s=%g %s' % (nc, kind, value, 'weighted+acc' if acc else 'weighted' if weighted else 'plain'),
               kind + ' x30' + (' accumulated' if acc else ''), loss, g, r64, r32, c['g0'], acc, nc)


@pytest.mark.parametrize('shape,nc,ld', GEOM, ids=GEOM_IDS)
def test_shape_none_leaves_the_other_entry_points(dev, shape, nc, ld):
    """5. ADDK_CE_SHAPE_NONE through the new entry point: g, loss and loss partials of the plain, the mining and the Dice entry point, bit for
    bit (gamma and eps are NaN: they are not read)."""
    c = _case(shape, nc)
    xa, ta = _padded(c['x'], dev, STRIDES[nc][ld]), c['t'].to(dev)
    nv = int((c['t'] != 255).sum())
    for weighted, acc in ((False, 0), (True, 1)):
        wa = WEIGHTS[nc].to(dev) if weighted else None
        wsum = _count(dev, ta, wa, nc)
        lmap, tau, wk, _ = _select(dev, xa, ta, c, 0.01, nv // 2, wa)
        coef = _stats(dev, xa, ta, c, torch.zeros(1, device=dev))[0]
        for entry, norm, kw in (('plain', wsum, {}), ('ohem', wk, dict(lmap=lmap, tau=tau)), ('dice', wsum, dict(coef=coef)),
                                ('dice', wk, dict(coef=coef, lmap=lmap, tau=tau))):
            ref = _head(dev, entry, xa, ta, c, wa, acc, norm, **kw)
            got = _head(dev, 'shaped', xa, ta, c, wa, acc, norm, 'none', **kw)
            for p, q in zip(ref, got):
                assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (entry, sorted(kw))
            assert float(ref[0]) != 0.25


def test_bad_arguments_are_refused_without_a_launch(dev):
    """6."""
    import addk._lib as L
    lib = L.load()
    c = _case('x1', 19)
    H, W = c['lo_hw']
    xa, ta = _padded(c['x'], dev, 20), c['t'].to(dev)
    wsum = _count(dev, ta, None, 19)
    f = dict(device=dev)
    g, loss, coef = torch.full((N, H, W, 20), 7.0, **f), torch.full((1,), 7.0, **f), torch.zeros(38, **f)
    ws = torch.full((int(lib.addk_ce_upsample_ws_floats(N, H, W)),), 7.0, **f)
    lmap, tau = torch.zeros((N,) + c['hi_hw'], **f), torch.zeros(1, **f)
    st = torch.cuda.current_stream().cuda_stream

    def args(kind, value, **kw):
        b = L.CeUpsampleShapedArgs()
        _fill_ce(b.dice.kd.ce, xa, ta, c, None, wsum, loss, g, ws, 0)
        _shape_words(b, kind, value)
        for k, v in kw.items():
            where = b if k in ('shape', 'gamma', 'eps') else b.dice if k == 'coef' else b.dice.kd if hasattr(L.CeUpsampleKdArgs, k) and k != 'ce' else b.dice.kd.ce
            setattr(where, k, v)
        return b
    nan, inf = float('nan'), float('inf')
    bad = [('focal', 0.999), ('focal', 0.0), ('focal', -2.0), ('focal', nan), ('focal', inf), ('focal', -inf),
           ('smooth', 0.0), ('smooth', 1.0), ('smooth', -0.1), ('smooth', 1.5), ('smooth', nan), ('smooth', inf)]
    for kind, value in bad:
        assert lib.addk_ce_upsample_shaped_fwd_bwd(C.byref(args(kind, value)), st) == -1, (kind, value)
    more = [dict(shape=3), dict(shape=-1), dict(C=7), dict(C=20), dict(C=22), dict(logits=None), dict(target=None), dict(wsum=None), dict(loss_out=None),
            dict(g=None), dict(ws=None), dict(ld=18), dict(ldg=18), dict(pix_loss=lmap.data_ptr()), dict(tau=tau.data_ptr()),
            dict(teacher=coef.data_ptr())]
    for kind, value in (('focal', 2.0), ('smooth', 0.1)):
        for kw in more:
            assert lib.addk_ce_upsample_shaped_fwd_bwd(C.byref(args(kind, value, **kw)), st) == -1, (kind, kw)
    torch.cuda.synchronize()
    for v in (g, loss, ws):
        assert float(v.min()) == float(v.max()) == 7.0
    for kind, value in (('focal', 1.0), ('focal', 2.0), ('smooth', 0.1)):         # the blocks themselves are good, gamma == 1 among them
        for kw in ({}, dict(coef=coef.data_ptr()), dict(pix_loss=lmap.data_ptr(), tau=tau.data_ptr())):
            assert lib.addk_ce_upsample_shaped_fwd_bwd(C.byref(args(kind, value, **kw)), st) == 0
    torch.cuda.synchronize()


# ---- the training step -------------------------------------------------------------------------------------------------------------

SHAPE = (2, 3, 65, 129)


def _args(ncls):
    return (ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, ncls, make_args(4), 0)


def _oracle(ncls, seed=600):
    mo = oracle.ADD(*_args(ncls))
    fill_params(mo, seed)
    return mo


def _model(dev, ncls, seed=600):
    from addk.modeling.ADD import ADD
    ma = ADD(*_args(ncls))
    ma.load_state_dict(_oracle(ncls, seed).state_dict())
    return ma.to(dev)


def _batch(hw, ncls, seed=5):
    x = rand_tensor(seed, 'ts_x', (2, 3) + hw)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, ncls, (2,) + hw)).long()
    t[torch.from_numpy(r.random((2,) + hw) < 0.05)] = 255
    return x, t


def _fwd_bwd(dev, ncls=19, **kw):
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:], ncls)
    ma = _model(dev, ncls)
    ts = TrainStep(ma, SHAPE, use_graph=False, **kw)
    ts.load_batch(x.to(dev), t.to(dev))
    ts.forward_backward_only()
    torch.cuda.synchronize()
    names = {p: k for k, p in ma.named_parameters()}
    return ts, {names[p]: g.double().cpu() for p, g in ts.grads().items() if g is not None}


def _oracle_runs(t, ncls, focal=None, smooth=None, class_w=None, dice=None, masks=None):
    """the oracle model in fp32 and fp64 with the step's loss written in torch (tests/_shape_ref.py on the oracle's full-resolution outputs,
    which are the bilinear samples of its low-resolution logits): per exit the shaped loss (over the kept mask of that exit, when given) +
    the Dice term, averaged over the exits.  name -> (loss, grads)"""
    x, _ = _batch(SHAPE[2:], ncls)
    valid = t != 255
    res = {}
    for name, dt in (('o32', torch.float32), ('o64', torch.float64)):
        m = _oracle(ncls).to(dt)
        m.train()
        ys = m(x.to(dt))
        loss = 0
        for i, y in enumerate(ys):
            kw = dict(class_w=class_w, mask=None if masks is None else masks[i])
            loss = loss + (R.focal_loss(y, t, focal, **kw) if focal is not None else R.smooth_loss(y, t, smooth, **kw))
            if dice is not None:
                loss = loss + dice_term(y, t, valid, *dice)[0]
        loss = loss / len(ys)
        loss.backward()
        res[name] = (loss.item(), {k: p.grad.double() for k, p in m.named_parameters()})
    return res


def _check_step(tag, ts, ga, res):
    """loss and parameter gradients at the bounds of tests/test_gpu_dice.py::test_step_against_the_oracle: the loss within 3 x the fp32
    oracle's own error + 1e-4 relative, the parameter gradients' rel_l2 within 2 x the fp32 oracle's + 1e-3"""
    la = ts.loss.item()
    o64, o32 = res['o64'], res['o32']
    g64 = o64[1]

    def rel_l2(gx):
        return (sum(float(((gx[k] - g64[k]) ** 2).sum()) for k in g64) / sum(float((g64[k] ** 2).sum()) for k in g64)) ** 0.5
    print('shape step %s: loss %.6f (fp64 %.6f, fp32 %.6f), rel_l2 %.2e (fp32 torch %.2e)' % (tag, la, o64[0], o32[0], rel_l2(ga), rel_l2(o32[1])))
    assert abs(la - o64[0]) <= 3 * abs(o32[0] - o64[0]) + 1e-4 * abs(la), (la, o64[0], o32[0])
    assert set(ga) == set(g64)
    assert rel_l2(ga) <= 2.0 * rel_l2(o32[1]) + 1e-3


def test_step_focal_against_the_oracle(dev):
    """7. forward_backward_only with focal=2 against the oracle model in fp32 and fp64 with the same loss; focal=None and
    label_smoothing=None give the loss bits and the launch names of a step built without the keywords."""
    _, t = _batch(SHAPE[2:], 19)
    ts, ga = _fwd_bwd(dev, focal=2.0)
    names = [c.name for c in ts.g.bwd]
    assert names.count('ce_upsample_shaped') == 2 and names.count('ce_upsample') == 0
    _check_step('focal=2', ts, ga, _oracle_runs(t, 19, focal=2.0))
    t0, _ = _fwd_bwd(dev)
    t1, _ = _fwd_bwd(dev, focal=None, label_smoothing=None)
    assert torch.equal(t0.loss.view(torch.int32), t1.loss.view(torch.int32)) and [c.name for c in t0.g.bwd] == [c.name for c in t1.g.bwd]
    assert float(ts.loss) < float(t0.loss)                         # (1 - p_t)^2 < 1


def test_step_label_smoothing_with_class_weights_against_the_oracle(dev):
    """8."""
    _, t = _batch(SHAPE[2:], 19)
    ts, ga = _fwd_bwd(dev, label_smoothing=0.1, class_weight=WEIGHTS[19])
    assert [c.name for c in ts.g.bwd].count('ce_upsample_shaped') == 2
    _check_step('label_smoothing=0.1 weighted', ts, ga, _oracle_runs(t, 19, smooth=0.1, class_w=WEIGHTS[19]))


def test_step_with_ohem_and_dice_against_the_oracle(dev):
    """9. focal with ohem and dice together: the oracle takes each exit's kept mask from the DEVICE's map and tau."""
    _, t = _batch(SHAPE[2:], 19)
    dice = (1.0, 1.0)
    ts, ga = _fwd_bwd(dev, focal=2.0, ohem=(0.7, 2000), dice=dice, class_weight=WEIGHTS[19])
    names = [c.name for c in ts.g.bwd]
    assert names.count('ohem_select') == 2 and names.count('dice_stats') == 2 and names.count('ce_upsample_shaped') == 2
    masks = []
    for o in ts.outs:
        st = o.binding['ohem_state']
        masks.append(st['pix_loss'].cpu() >= float(st['tau']))
    _check_step('focal=2+ohem+dice weighted', ts, ga, _oracle_runs(t, 19, focal=2.0, class_w=WEIGHTS[19], dice=dice, masks=masks))
    assert all(0 < kept <= valid for _, kept, valid in ts.ohem_stats())


def test_step_21_classes_against_the_oracle(dev):
    """10. label smoothing with ohem and dice at 21 classes."""
    _, t = _batch(SHAPE[2:], 21)
    dice = (1.0, 1.0)
    ts, ga = _fwd_bwd(dev, ncls=21, label_smoothing=0.1, ohem=(0.7, 2000), dice=dice)
    assert [c.name for c in ts.g.bwd].count('ce_upsample_shaped') == 2
    masks = []
    for o in ts.outs:
        st = o.binding['ohem_state']
        masks.append(st['pix_loss'].cpu() >= float(st['tau']))
    _check_step('21 classes label_smoothing=0.1+ohem+dice', ts, ga, _oracle_runs(t, 21, smooth=0.1, dice=dice, masks=masks))


@pytest.mark.parametrize('kw', [dict(focal=2.0), dict(label_smoothing=0.1, ohem=(0.7, 2000), dice=(1.0, 1.0))], ids=['focal', 'smooth+ohem+dice'])
def test_step_replayed_graph_equals_eager(dev, kw):
    """11. after enable_capture() the step is one hipGraph: one eager step that is then captured and two replays give the loss and the
    parameters of three eager steps, bit for bit."""
    from addk.train import TrainStep
    x, t = _batch(SHAPE[2:], 19)
    res = {}
    for mode in ('eager', 'graph'):
        ts = TrainStep(_model(dev, 19), SHAPE, use_graph=False, **kw)
        ts.load_batch(x.to(dev), t.to(dev))
        if mode == 'graph':
            ts.enable_capture()
        ls = [ts.step().item() for _ in range(3)]
        torch.cuda.synchronize()
        assert (ts.graph is not None) == (mode == 'graph')
        res[mode] = (ls, ts.flat_p.clone())
        ts.close()
    assert res['graph'][0] == res['eager'][0], (res['graph'][0], res['eager'][0])
    assert torch.equal(res['graph'][1], res['eager'][1])
    assert all(np.isfinite(v) for v in res['eager'][0]) and len(set(res['eager'][0])) == 3
