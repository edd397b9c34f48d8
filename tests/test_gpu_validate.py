"""GPU tests of the validation pass: the fused scoring kernel (addk_score_upsample) through the C ABI against fp64 / fp32 CPU
references, and addk.validate.ValidationStep against the hand-assembled path (model.eval()(x) + CrossEntropyLoss +
argmax_logits + Evaluator + normalized_shannon_entropy) on the same model and batches."""
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
from _util import (ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, GENOTYPE_BASELINE_2, NETWORK_PATH_BASELINE, fill_params,   # noqa: E402
                   make_args, rand_tensor)

LD = 24
NEAR_TIE_GAP = 1e-4          # relative to max |logit|: ~100x the fp32 rounding of a four-term interpolation
NEAR_TIE_SHARE = 0.005


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
CASES = {'x8': (2, (8, 16), (64, 128)), 'odd_ladder': (2, (9, 17), (65, 129)), 'partial_tiles': (2, (5, 7), (33, 49)),
         'band13': (2, (3, 5), (40, 70)), 'x32_n1': (1, (4, 4), (128, 128))}


def _targets(n, hw, seed):
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, 19, (n,) + hw)).long()
    t[torch.from_numpy(r.random((n,) + hw) < 0.05)] = 255
    flat = t.view(-1)
    pos = torch.from_numpy(r.choice(flat.numel(), 12, replace=False))
    flat[pos] = torch.tensor([19, 20, 254, 256, 1000, 2 ** 40, -1, -2, -255, -1000, -2 ** 40, 19])
    return t


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Inputs and CPU references of one case, computed once and shared (never modified) by the tests of that case."""
    N, lo, hi = CASES[case]
    x = rand_tensor(41, 'score_x:' + case, (N,) + lo + (19,)) * 3
    t = _targets(N, hi, 17)
    w = torch.rand(19, generator=torch.Generator().manual_seed(4)) + 0.5
    t_ce = t.clone()
    t_ce[(t < 0) | (t >= 19)] = 255               # the kernels skip every label outside [0, 19); torch's criterion raises on them
    up64 = Fn.interpolate(x.double().permute(0, 3, 1, 2), size=hi, mode='bilinear', align_corners=False)
    up32 = Fn.interpolate(x.permute(0, 3, 1, 2), size=hi, mode='bilinear', align_corners=False)
    ref = dict(x=x, t=t, w=w)
    for key, weight in (('plain', None), ('weighted', w)):
        ref['loss64', key] = float(nn.CrossEntropyLoss(weight=None if weight is None else weight.double(), ignore_index=255)(up64, t_ce))
        ref['loss32', key] = float(nn.CrossEntropyLoss(weight=weight, ignore_index=255)(up32, t_ce))
    lp = torch.log_softmax(up64, dim=1)
    ref['ent64'] = float(-(lp.exp() * lp).sum())            # operations.py:161-170 before its normalisation
    lp32 = torch.log_softmax(up32, dim=1)
    ref['ent32'] = float(-(lp32.exp() * lp32).sum())
    top = up32.topk(2, dim=1).values
    ref['near_tie'] = (top[:, 0] - top[:, 1]) < NEAR_TIE_GAP * float(up32.abs().max())
    ref['pred32'] = up32.argmax(1)
    ref['pred64'] = up64.argmax(1)
    return ref


def _padded(x, dev, seed, ld=LD):
    """the logits in a pixel stride `ld` with finite garbage in the padding channels"""
    xa = (rand_tensor(seed, 'score_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
    xa[..., :19] = x.to(dev)
    return xa.contiguous()


def _score(lib, L, xa, ld, shape, ta, wa, wsum, want_map=True, cm0=None, loss0=0.25, ent0=0.5, scale=0.5):
    N, (H, W), (OH, OW) = shape
    dev = ta.device
    loss = torch.full((1,), loss0, device=dev)
    ent = torch.full((1,), ent0, device=dev)
    cm = (cm0.clone() if cm0 is not None else torch.zeros((19, 19), dtype=torch.int64)).to(dev)
    pred = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=dev) if want_map else None
    ws = torch.zeros(int(lib.addk_score_upsample_ws_floats(N, OH, OW)), device=dev)
    a = L.ScoreUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, 19, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), wa.data_ptr() if wa is not None else None, 255
    a.wsum, a.scale, a.loss_out, a.ent_out = wsum.data_ptr(), scale, loss.data_ptr(), ent.data_ptr()
    a.cm, a.pred_out, a.ws = cm.data_ptr(), pred.data_ptr() if pred is not None else None, ws.data_ptr()
    L.check(lib.addk_score_upsample(C.byref(a), torch.cuda.current_stream().cuda_stream), 'score_upsample')
    torch.cuda.synchronize()
    return loss.cpu(), ent.cpu(), cm.cpu(), pred.cpu() if pred is not None else None


def _unfused_entropy(lib, L, xa, shape, dev):
    """the parent's path: addk_resize_fwd materialises the fp32 full-resolution logits, addk_entropy_sum reads them"""
    N, (H, W), (OH, OW) = shape
    y = torch.empty((N, 19, OH, OW), device=dev)
    ar = L.ResizeArgs()
    ar.src.x, ar.src.ld, ar.src.C = xa.data_ptr(), LD, 19
    ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.addk_resize_fwd(C.byref(ar), st), 'resize_fwd')
    out, ws = torch.zeros(1, device=dev), torch.zeros(1024, device=dev)
    L.check(lib.addk_entropy_sum(y.data_ptr(), N, 19, OH * OW, out.data_ptr(), ws.data_ptr(), st), 'entropy_sum')
    torch.cuda.synchronize()
    return float(out), y.cpu()


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('case', list(CASES))
def test_score_upsample_matches_cpu_references(dev, case, weighted):
    """addk_score_upsample against F.interpolate(bilinear, align_corners=False) + nn.CrossEntropyLoss + the reference's entropy
    in fp64 (fp32 for the arg-max): loss, entropy, prediction map, confusion matrix, determinism, padding channels.
    Measured on the MI355X over the five shapes (every run prints its figures; DESIGN.md section 12 has the table): loss within 1.3e-7
    of fp64 (bound 2e-6), entropy within 8.3e-8 (the materialised path: 5.5e-8), near-ties 0.09-0.18 % of the pixels, no arg-max
    mismatch anywhere."""
    import addk._lib as L
    lib = L.load()
    N, (H, W), (OH, OW) = shape = CASES[case]
    ref = _reference(case)
    key = 'weighted' if weighted else 'plain'
    assert lib.addk_score_upsample_supported(N, H, W, OH, OW, 19) == 1       # the gather form has no band limit (x32_n1 included)
    xa = _padded(ref['x'], dev, 1)
    ta = ref['t'].to(dev)
    wa = ref['w'].to(dev) if weighted else None
    wsum, ws1 = torch.zeros(1, device=dev), torch.zeros(int(lib.addk_ce_ws_floats(N, OH * OW)), device=dev)
    L.check(lib.addk_ce_count(ta.data_ptr(), N * OH * OW, wa.data_ptr() if wa is not None else None, 255, 19, wsum.data_ptr(),
                              ws1.data_ptr(), torch.cuda.current_stream().cuda_stream), 'ce_count')
    cm0 = torch.from_numpy(np.random.default_rng(3).integers(0, 1 << 40, (19, 19)))
    loss, ent, cm, pred = _score(lib, L, xa, LD, shape, ta, wa, wsum, cm0=cm0)

    # loss: accumulated onto 0.25 with scale 0.5
    l64 = 0.5 * ref['loss64', key]
    got = float(loss.double() - 0.25)
    print('%s/%s loss %.9g ref64 %.9g rel %.3g (fp32 CPU reference: rel %.3g)' % (
        case, key, got, l64, abs(got - l64) / abs(l64), abs(0.5 * ref['loss32', key] - l64) / abs(l64)))
    # entropy: accumulated onto 0.5; the parent's path on the same inputs gives the yardstick
    e64 = ref['ent64']
    e_fused = float(ent.double() - 0.5)
    e_unf, y_unf = _unfused_entropy(lib, L, xa, shape, dev)
    err_f, err_u = abs(e_fused - e64), abs(e_unf - e64)
    print('%s/%s entropy fused %.9g unfused %.9g ref64 %.9g: rel err fused %.3g unfused %.3g (fp32 CPU reference %.3g)' % (
        case, key, e_fused, e_unf, e64, err_f / e64, err_u / e64, abs(ref['ent32'] - e64) / e64))
    # predictions
    tie = ref['near_tie']
    share = float(tie.float().mean())
    wrong = (pred.long() != ref['pred32']) & ~tie
    print('%s/%s near-tie share %.4f%%, mismatches outside near-ties %d, fp32-vs-fp64 reference arg-max disagreements %d, '
          'fused vs materialised arg-max disagreements %d' % (case, key, 100 * share, int(wrong.sum()), int((ref['pred32'] != ref['pred64']).sum()),
                                                             int((pred.long() != y_unf.argmax(1)).sum())))
    assert abs(got - l64) <= 2e-6 * abs(l64)
    assert err_f <= max(4 * err_u, 2e-6 * abs(e64))
    assert share <= NEAR_TIE_SHARE
    assert int(wrong.sum()) == 0
    # confusion: exact against the kernel's own map, on top of the starting matrix
    t = ref['t']
    ok = (t >= 0) & (t < 19)
    want = torch.bincount(19 * t[ok] + pred.long()[ok], minlength=361).view(19, 19)
    assert int(want.sum()) == int(ok.sum()) < t.numel()
    assert torch.equal(cm, cm0 + want)
    # the same without the map output, and run to run
    loss2, ent2, cm2, none = _score(lib, L, xa, LD, shape, ta, wa, wsum, want_map=False, cm0=cm0)
    assert none is None and torch.equal(cm2, cm) and torch.equal(loss2, loss) and torch.equal(ent2, ent)
    loss3, ent3, cm3, pred3 = _score(lib, L, xa, LD, shape, ta, wa, wsum, cm0=cm0)
    assert torch.equal(loss3, loss) and torch.equal(ent3, ent) and torch.equal(cm3, cm) and torch.equal(pred3, pred)
    # other garbage in the padding channels: nothing moves
    loss4, ent4, cm4, pred4 = _score(lib, L, _padded(ref['x'], dev, 2), LD, shape, ta, wa, wsum, cm0=cm0)
    assert torch.equal(loss4, loss) and torch.equal(ent4, ent) and torch.equal(cm4, cm) and torch.equal(pred4, pred)
    # dense pixel stride (19: the scalar-load kernel) computes the same bits as the 16-byte-load kernel
    loss5, ent5, cm5, pred5 = _score(lib, L, ref['x'].to(dev).contiguous(), 19, shape, ta, wa, wsum, cm0=cm0)
    assert torch.equal(loss5, loss) and torch.equal(ent5, ent) and torch.equal(cm5, cm) and torch.equal(pred5, pred)


def test_score_upsample_refuses_what_it_does_not_take(dev):
    import addk
    import addk._lib as L
    lib = L.load()
    assert lib.addk_score_upsample_supported(2, 8, 16, 64, 128, 7) == 0
    a = L.ScoreUpsampleArgs()
    assert lib.addk_score_upsample(C.byref(a), None) != 0                      # null pointers: an error code, no launch
    with pytest.raises(addk.AddkError):
        L.check(lib.addk_score_upsample(C.byref(a), None), 'score_upsample')


# ------------------------------------------------------------------------------------------------------------------------
# step level
# ------------------------------------------------------------------------------------------------------------------------
def _models(dev, kind='c2', Fv=4, seed=600):
    from addk.modeling.ADD import ADD
    from addk.modeling.baseline_model import Baselin_Model
    if kind == 'baseline':
        args, ca, co = (NETWORK_PATH_BASELINE, [5], GENOTYPE_BASELINE_2, 19, make_args(Fv), 1), Baselin_Model, oracle.Baselin_Model
    else:
        arch = ARCH_C3 if kind == 'c3' else ARCH_C2
        args, ca, co = (arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(Fv), 0), ADD, oracle.ADD
    mo = co(*args)
    fill_params(mo, seed)
    # synthetic weights drive the logits of the last exit to |z| ~ 1e5 - 1e6 (every softmax one-hot, the entropy a sum of rounding
    # noise): the classifier is scaled down so that the exits span |z| ~ 0.01 - 30 and loss and entropy are well-conditioned sums.
    # A positive scale leaves the arg-max, and the relative near-tie gaps, as they were (checked on the CPU oracle: <= 0.19 %).
    with torch.no_grad():
        mo.decoder._conv[7].weight.mul_(4e-5)
        mo.decoder._conv[7].bias.mul_(4e-5)
    ma = ca(*args)
    ma.load_state_dict(mo.state_dict())
    return ma.to(dev), mo


def _batch(n, hw, seed):
    x = rand_tensor(seed, 'ts_x', (n, 3) + hw)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, 19, (n,) + hw)).long()
    t[torch.from_numpy(r.random((n,) + hw) < 0.05)] = 255
    return x, t


def _hand_assembled(ma, batches, weight, dev):
    """the path a user assembles today (train.py:250-322 on the drop-in pieces)"""
    from addk.loss import CrossEntropyLoss
    from addk.metrics import Evaluator, argmax_logits
    from addk.modeling.operations import normalized_shannon_entropy
    ma.eval()
    crit = CrossEntropyLoss(weight=weight, ignore_index=255).to(dev)
    evs, conf, test_loss, ties, pixels = None, None, 0.0, 0, 0
    for x, t in batches:
        with torch.no_grad():
            outs = ma(x.to(dev))
        if evs is None:
            evs, conf = [Evaluator(19, dev) for _ in outs], [[] for _ in outs]
        test_loss += (sum(crit(o, t.to(dev)) for o in outs) / len(outs)).item()
        for i, o in enumerate(outs):
            evs[i].add_batch(t.to(dev), argmax_logits(o))
            conf[i].append(normalized_shannon_entropy(o))
            top = o.topk(2, dim=1).values
            ties += int(((top[:, 0] - top[:, 1]) < NEAR_TIE_GAP * float(o.abs().max())).sum())
            pixels += top[:, 0].numel()
    return dict(test_loss=test_loss, confidence=[sum(c) / len(c) for c in conf], cm=[e._cm.clone() for e in evs],
                mIoU=[e.Mean_Intersection_over_Union() for e in evs], ties=ties, pixels=pixels)


def _compare(tag, r, hand):
    nex = len(hand['cm'])
    assert len(r['exits']) == nex
    d_loss = abs(r['test_loss'] - hand['test_loss']) / abs(hand['test_loss'])
    d_conf = [abs(e['confidence'] - c) / abs(c) for e, c in zip(r['exits'], hand['confidence'])]
    d_cm = [int((e['confusion'] - c).abs().sum()) for e, c in zip(r['exits'], hand['cm'])]
    share = hand['ties'] / hand['pixels']
    print('%s: test_loss %.8g vs %.8g (rel %.3g); confidence rel diff %s; sum|dcm| %s; near-ties %d of %d (%.4f%%); mIoU %s vs %s' % (
        tag, r['test_loss'], hand['test_loss'], d_loss, ['%.3g' % d for d in d_conf], d_cm, hand['ties'], hand['pixels'], 100 * share,
        [e['mIoU'] for e in r['exits']], hand['mIoU']))
    assert d_loss <= 1e-5 and max(d_conf) <= 1e-5
    assert share <= NEAR_TIE_SHARE
    assert sum(d_cm) <= 2 * hand['ties']
    for e, c, m in zip(r['exits'], hand['cm'], hand['mIoU']):
        assert int(e['confusion'].sum()) == int(c.sum())                       # every valid label counted once on both paths
        if int((e['confusion'] - c).abs().sum()) == 0:
            assert e['mIoU'] == m                                              # the evaluator's formula on the same matrix
    assert abs(r['new_pred'] - sum(e['mIoU'] for e in r['exits']) / nex) < 1e-12


@pytest.mark.parametrize('hw', [(65, 129), (64, 128)], ids=['65x129', '64x128'])
def test_validation_step_equals_hand_assembled_path(dev, hw):
    """Three batches (two eager passes, then the captured replay) against the hand-assembled path on the same model, with class
    weights; the model's state is bit-equal afterwards and the evaluator interface takes the matrices."""
    from addk.metrics import Evaluator
    from addk.validate import ValidationStep
    ma, _ = _models(dev)
    ma.train()
    w = torch.rand(19, generator=torch.Generator().manual_seed(4)) + 0.5
    batches = [_batch(2, hw, 5 + i) for i in range(3)]
    before = {k: v.clone() for k, v in ma.state_dict().items()}
    vs = ValidationStep(ma, (2, 3) + hw, class_weight=w, keep_predictions=True)
    names = [c.name for c in vs.g.fwd]
    assert names.count('score_upsample') == 2 and 'resize_nchw' not in names
    for x, t in batches:
        vs.step(x.to(dev), t.to(dev))
    assert vs.graph is not None and vs.batches == 3 and ma.training
    r = vs.result()
    preds = vs.predictions()
    after = ma.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    hand = _hand_assembled(ma, batches, w, dev)
    _compare('c2 %dx%d' % hw, r, hand)
    # the last batch's maps reproduce that batch's share of the matrix
    t = batches[-1][1]
    ok = (t >= 0) & (t < 19)
    vs.reset()
    vs.step(batches[-1][0].to(dev), t.to(dev))
    r1 = vs.result()
    for p, e in zip(preds, r1['exits']):
        assert p.dtype == torch.uint8 and tuple(p.shape) == (2,) + hw
        assert torch.equal(torch.bincount(19 * t[ok] + p.cpu().long()[ok], minlength=361).view(19, 19), e['confusion'].cpu())
    assert r1['batches'] == 1
    ev = Evaluator(19, dev)
    ev.add_confusion(r1['exits'][0]['confusion'])
    assert ev.Mean_Intersection_over_Union() == r1['exits'][0]['mIoU']
    vs.close()


@pytest.mark.parametrize('kind', ['c3', 'baseline'])
def test_validation_step_three_exits_and_baseline(dev, kind):
    from addk.validate import ValidationStep
    ma, _ = _models(dev, kind)
    batches = [_batch(2, (65, 129), 8)]
    vs = ValidationStep(ma, (2, 3, 65, 129))
    assert [c.name for c in vs.g.fwd].count('score_upsample') == (3 if kind == 'c3' else 2)
    vs.step(batches[0][0].to(dev), batches[0][1].to(dev))
    _compare(kind, vs.result(), _hand_assembled(ma, batches, None, dev))
    vs.close()


def test_validation_between_train_steps_changes_nothing(dev):
    """The epoch loop of the reference: train, validate, train on ONE model.  The validation plan is built before the TrainStep
    re-points the parameters (so it has to follow them) and runs between two optimisation steps; the second step's loss and the
    parameters equal those of a run without the validation in between, bit for bit."""
    from addk.train import TrainStep
    from addk.validate import ValidationStep
    x, t = _batch(2, (65, 129), 5)
    xv, tv = _batch(2, (65, 129), 6)
    res = {}
    for with_val in (False, True):
        ma, _ = _models(dev)
        vs = ValidationStep(ma, (2, 3, 65, 129)) if with_val else None
        ts = TrainStep(ma, (2, 3, 65, 129), use_graph=False)
        ts.load_batch(x.to(dev), t.to(dev))
        losses = [ts.step().item()]
        if vs is not None:
            g0 = vs.g
            vs.step(xv.to(dev), tv.to(dev))
            assert vs.g is not g0                                              # rebuilt on the flat parameter buffer
            r_mid = vs.result()
            assert ma.training
        losses.append(ts.step().item())
        if vs is not None:
            # and the plan follows the optimiser: the same batch scores differently after the second update
            vs.reset()
            vs.step(xv.to(dev), tv.to(dev))
            r_end = vs.result()
            assert math.isfinite(r_end['test_loss']) and r_end['test_loss'] != r_mid['test_loss']
            vs.close()
        torch.cuda.synchronize()
        res[with_val] = (losses, ts.flat_p.clone(), {k: v.clone() for k, v in ma.state_dict().items()})
        ts.close()
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert all(torch.equal(res[True][2][k], res[False][2][k]) for k in res[False][2])
