"""GPU tests of the exit profile: the per-image profile kernel (addk_profile_upsample) through the C ABI, bit for bit against the two
kernels it combines (addk_gate_upsample for entropy and shares, addk_score_upsample for matrix and map — both held to fp64 by
tests/test_gpu_gate.py and tests/test_gpu_validate.py), and addk.exit_profile.ExitProfile against model.dynamic_inference image by
image and against ValidationStep batch by batch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402

LD = 24
THRESHOLDS = (0.2, 0.35, 0.5, 0.8)
CASES = {'partial_tiles': (1, (5, 7), (33, 49)), 'x8': (1, (8, 16), (64, 128)), 'x32': (1, (4, 4), (128, 128)),
         'n3': (3, (6, 9), (41, 67))}
NEAR_TIE_GAP = 1e-4          # tests/test_gpu_validate.py: relative to max |logit|
NEAR_TIE_SHARE = 0.005


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
def _targets(n, hw, seed):
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, 19, (n,) + hw)).long()
    t[torch.from_numpy(r.random((n,) + hw) < 0.05)] = 255
    flat = t.view(-1)
    pos = torch.from_numpy(r.choice(flat.numel(), 12, replace=False))
    flat[pos] = torch.tensor([19, 20, 254, 256, 1000, 2 ** 40, -1, -2, -255, -1000, -2 ** 40, 19])
    return t


def _padded(x, dev, seed, ld=LD):
    """the logits in a pixel stride `ld` with finite garbage in the padding channels"""
    xa = (rand_tensor(seed, 'gate_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
    xa[..., :19] = x.to(dev)
    return xa.contiguous()


def _gate(lib, L, xa, ld, shape, thr):
    """addk_gate_upsample -> [N, 2] (entropy, share at thr)"""
    N, (H, W), (OH, OW) = shape
    dev = xa.device
    word, out = torch.full((1,), thr, device=dev), torch.full((N, 2), -7.0, device=dev)
    ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    a = L.GateUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, 19, OH, OW
    a.max_thr, a.out, a.out_host, a.ws = word.data_ptr(), out.data_ptr(), None, ws.data_ptr()
    L.check(lib.addk_gate_upsample(C.byref(a), _stream()), 'gate_upsample')
    torch.cuda.synchronize()
    return out.cpu()


def _score(lib, L, xa, ld, shape, ta):
    """addk_score_upsample on a zeroed matrix -> (cm [19,19], map [N,OH,OW])"""
    N, (H, W), (OH, OW) = shape
    dev = xa.device
    loss, ent, wsum = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.ones(1, device=dev)
    cm = torch.zeros((19, 19), dtype=torch.int64, device=dev)
    pred = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(lib.addk_score_upsample_ws_floats(N, OH, OW)), device=dev)
    a = L.ScoreUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, 19, OH, OW
    a.target, a.class_w, a.ignore_index = ta.data_ptr(), None, 255
    a.wsum, a.scale, a.loss_out, a.ent_out = wsum.data_ptr(), 1.0, loss.data_ptr(), ent.data_ptr()
    a.cm, a.pred_out, a.ws = cm.data_ptr(), pred.data_ptr(), ws.data_ptr()
    L.check(lib.addk_score_upsample(C.byref(a), _stream()), 'score_upsample')
    torch.cuda.synchronize()
    return cm.cpu(), pred.cpu()


@functools.lru_cache(maxsize=None)
def _parents(case):
    """Inputs of one case and what the two parent kernels make of them, computed once and never modified."""
    import addk._lib as L
    lib = L.load()
    dev = torch.device('cuda:0')
    N, lo, hi = shape = CASES[case]
    x = rand_tensor(43, 'gate_x:' + case, (N,) + lo + (19,)) * 3
    t = _targets(N, hi, 17)
    xa, ta = _padded(x, dev, 1), t.to(dev)
    gates = [_gate(lib, L, xa, LD, shape, thr) for thr in THRESHOLDS]
    assert all(torch.equal(g[:, 0], gates[0][:, 0]) for g in gates)
    per_image = [_score(lib, L, xa[n], LD, (1, lo, hi), ta[n]) for n in range(N)]
    cm_b, pred_b = _score(lib, L, xa, LD, shape, ta)
    return dict(x=x, t=t, ent=gates[0][:, 0].clone(), share=torch.stack([g[:, 1] for g in gates], dim=1),
                cm=torch.stack([c for c, _ in per_image]), cm_batched=cm_b, pred=pred_b)


class _Profile:
    """One set of buffers of the profile launch: sentinel-filled outputs, zero-initialised workspace."""

    def __init__(self, lib, L, shape, dev, thresholds=THRESHOLDS):
        self.lib, self.L, self.shape = lib, L, shape
        N, _, (OH, OW) = shape
        self.thr = torch.tensor(thresholds, dtype=torch.float32, device=dev)
        self.ent = torch.full((N,), -7.0, device=dev)
        self.share = torch.full((N, max(len(thresholds), 1)), -7.0, device=dev)[:, :len(thresholds)].contiguous()
        self.cm = torch.zeros((N, 19, 19), dtype=torch.int64, device=dev)
        self.pred = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=dev)
        self.ws = torch.zeros(int(lib.addk_profile_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)

    def args(self, xa, ld, ta, nthr=None, C_=19, want_map=True, share=True):
        N, (H, W), (OH, OW) = self.shape
        a = self.L.ProfileUpsampleArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, C_, OH, OW
        a.target, a.thr, a.nthr = ta.data_ptr(), self.thr.data_ptr(), self.thr.numel() if nthr is None else nthr
        a.ent_out, a.share_out, a.cm = self.ent.data_ptr(), self.share.data_ptr() if share else None, self.cm.data_ptr()
        a.pred_out, a.ws = self.pred.data_ptr() if want_map else None, self.ws.data_ptr()
        return a

    def __call__(self, xa, ld, ta, zero=True, **kw):
        if zero:
            self.cm.zero_()
        self.ent.fill_(-7.0)
        self.share.fill_(-7.0)
        rc = self.lib.addk_profile_upsample(C.byref(self.args(xa, ld, ta, **kw)), _stream())
        torch.cuda.synchronize()
        return rc, self.ent.cpu(), self.share.cpu(), self.cm.cpu(), self.pred.cpu()


@pytest.mark.parametrize('case', list(CASES))
def test_profile_upsample_carries_the_bits_of_gate_and_score(dev, case):
    """Per image: entropy and every share are the gate kernel's words, the matrix is the scoring kernel's on that image alone (their
    sum the batched launch's) and the map is its map; the ticket returns to zero, a second launch adds to the matrix and rewrites the
    rest, padding channels and the dense stride change nothing, and the entropy alone (no thresholds) runs."""
    import addk._lib as L
    lib = L.load()
    N, (H, W), (OH, OW) = shape = CASES[case]
    ref = _parents(case)
    assert lib.addk_profile_upsample_supported(N, H, W, OH, OW, 19, len(THRESHOLDS)) == 1
    xa, ta = _padded(ref['x'], dev, 1), ref['t'].to(dev)
    prof = _Profile(lib, L, shape, dev)
    rc, ent, share, cm, pred = prof(xa, LD, ta)
    assert rc == 0
    for n in range(N):
        print('%s[%d] entropy %.9g (gate %.9g) shares %s (gate %s) matrix sum %d' % (
            case, n, float(ent[n]), float(ref['ent'][n]), share[n].tolist(), ref['share'][n].tolist(), int(cm[n].sum())))
    assert torch.equal(ent.view(torch.int32), ref['ent'].view(torch.int32))
    assert torch.equal(share.view(torch.int32), ref['share'].view(torch.int32))
    assert torch.equal(cm, ref['cm'])
    assert torch.equal(cm.sum(0), ref['cm_batched'])
    assert torch.equal(pred, ref['pred'])
    ok = (ref['t'] >= 0) & (ref['t'] < 19)
    assert 0 < int(cm.sum()) == int(ok.sum()) < ref['t'].numel()                 # the out-of-range labels are skipped
    assert int(prof.ws[:4].view(torch.int32).item()) == 0                        # the ticket is back at zero
    if N > 1:                                                                    # the images do not share a result
        for i in range(N):
            for j in range(i + 1, N):
                assert float(ent[i]) != float(ent[j]) and not torch.equal(share[i], share[j]) and not torch.equal(cm[i], cm[j])
    # a second launch without zeroing: the matrix doubles, entropy and shares are written, not accumulated
    rc, ent2, share2, cm2, pred2 = prof(xa, LD, ta, zero=False)
    assert rc == 0 and torch.equal(cm2, 2 * cm) and torch.equal(ent2, ent) and torch.equal(share2, share) and torch.equal(pred2, pred)
    assert int(prof.ws[:4].view(torch.int32).item()) == 0
    # other garbage in the padding channels: nothing moves
    rc, ent3, share3, cm3, pred3 = prof(_padded(ref['x'], dev, 2), LD, ta)
    assert rc == 0 and torch.equal(ent3, ent) and torch.equal(share3, share) and torch.equal(cm3, cm) and torch.equal(pred3, pred)
    # dense pixel stride (19: the scalar-load kernel) computes the same bits as the 16-byte-load kernel
    rc, ent4, share4, cm4, pred4 = prof(ref['x'].to(dev).contiguous(), 19, ta)
    assert rc == 0 and torch.equal(ent4, ent) and torch.equal(share4, share) and torch.equal(cm4, cm) and torch.equal(pred4, pred)
    # no thresholds, no share array, no map: entropy and matrix alone
    prof.pred.fill_(77)
    rc, ent5, share5, cm5, pred5 = prof(xa, LD, ta, nthr=0, share=False, want_map=False)
    assert rc == 0 and torch.equal(ent5, ent) and torch.equal(cm5, cm)
    assert torch.equal(share5, torch.full_like(share5, -7.0)) and torch.equal(pred5, torch.full_like(pred5, 77))
    # sixteen thresholds: every slot has its own counter
    many = tuple(THRESHOLDS[j % 4] + 0.01 * (j // 4) for j in range(16))
    p16 = _Profile(lib, L, shape, dev, many)
    rc, ent6, share6, cm6, _ = p16(xa, LD, ta)
    assert rc == 0 and torch.equal(ent6, ent) and torch.equal(cm6, cm)
    assert torch.equal(share6[:, :4], share)
    assert bool((share6[:, 4:] <= share6[:, :12]).all()) and not torch.equal(share6[:, 12:], share6[:, :4])


def test_profile_upsample_refuses_what_it_does_not_take(dev):
    import addk
    import addk._lib as L
    lib = L.load()
    shape = (1, (8, 16), (64, 128))
    prof = _Profile(lib, L, shape, dev)
    prof.cm.fill_(5)
    xa, ta = torch.zeros((1, 8, 16, 24), device=dev), torch.zeros((1, 64, 128), dtype=torch.int64, device=dev)

    def untouched(rc, ent, share, cm, pred):
        assert rc != 0                                                           # an error code ...
        assert torch.equal(ent, torch.full_like(ent, -7.0)) and torch.equal(share, torch.full_like(share, -7.0))      # ... and no launch
        assert torch.equal(cm, torch.full_like(cm, 5)) and torch.equal(pred, torch.full_like(pred, 77))
        with pytest.raises(addk.AddkError):
            L.check(rc, 'profile_upsample')
    assert lib.addk_profile_upsample_supported(1, 8, 16, 64, 128, 19, 17) == 0
    untouched(*prof(xa, 24, ta, zero=False, nthr=17))
    untouched(*prof(xa, 24, ta, zero=False, nthr=-1))
    untouched(*prof(xa, 24, ta, zero=False, C_=21))
    untouched(*prof(xa, 16, ta, zero=False))                                     # a stride shorter than the channels
    untouched(*prof(xa, 24, ta, zero=False, share=False))                        # thresholds without a place for their shares
    for field in ('logits', 'target', 'ent_out', 'cm', 'ws', 'thr'):
        a = prof.args(xa, 24, ta)
        setattr(a, field, None)
        rc = lib.addk_profile_upsample(C.byref(a), _stream())
        torch.cuda.synchronize()
        untouched(rc, prof.ent.cpu(), prof.share.cpu(), prof.cm.cpu(), prof.pred.cpu())
    assert lib.addk_profile_upsample(C.byref(L.ProfileUpsampleArgs()), None) != 0
    assert lib.addk_profile_upsample(None, None) != 0


# ------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------
HW = (65, 129)
# rand_tensor / numpy seeds of the four images of test (a).  Picked from seeds 0..13 for exit-0 entropies that lie far apart (measured on the
# MI355X: 0.730, 0.639, 0.692, 0.601) and top-probability shares that cross share(t) = t between 0.3 and 0.45, so MAX_T splits them
SEEDS = (0, 2, 5, 12)
MAX_T = (0.1, 0.2, 0.3, 0.35, 0.4, 0.5, 0.7, 0.9)


def _model(dev, arch=ARCH_C2, seed=600, scale=4e-3):
    from addk.modeling.ADD import ADD
    m = ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), arch['low_level_layer'])
    fill_params(m, seed)
    # as tests/test_gpu_validate.py: synthetic weights drive the logits to |z| ~ 1e3 - 1e5 (every softmax one-hot, every gate value 0 or
    # 1); scaling the classifier leaves the arg-max alone and brings the gated exit to |z| ~ 6, its entropies and shares spread over (0, 1)
    with torch.no_grad():
        m.decoder._conv[7].weight.mul_(scale)
        m.decoder._conv[7].bias.mul_(scale)
    return m.to(dev)


def _batch(n, seed):
    x = rand_tensor(seed, 'ep_x', (n, 3) + HW)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, 19, (n,) + HW)).long()
    t[torch.from_numpy(r.random((n,) + HW) < 0.05)] = 255
    return x, t


def test_exit_profile_equals_dynamic_inference_image_by_image(dev):
    """F = 4, config 2, 65 x 129, four images (SEEDS).  For both gates and every threshold the curve's exit pattern is the `earlier_exit`
    pattern of model.dynamic_inference, each image's confidence is the value it returns (==), and the confusion matrix is that of
    Evaluator.add_batch(target, argmax_logits(y)) over the four returned logits, under the near-tie allowance of
    tests/test_gpu_validate.py::_compare.  Entropy thresholds: +-inf and the midpoints between the sorted exit-0 entropies that lie more than
    1e-6 apart (at least three must remain); 'max' thresholds: MAX_T.  For each gate a finite threshold splits the images."""
    from addk.exit_profile import ExitProfile
    from addk.metrics import Evaluator, argmax_logits, mean_iou
    m = _model(dev).eval()
    images = [_batch(1, s) for s in SEEDS]
    prof = ExitProfile(m, (1, 3) + HW, max_thresholds=MAX_T)
    for x, t in images:
        prof.step(x.to(dev), t.to(dev))
    assert prof.graph is not None
    rec = prof.records()
    M, nex = len(images), prof.nex
    assert nex == 2 and tuple(rec['entropy'].shape) == (nex, M) and tuple(rec['share'].shape) == (nex, M, len(MAX_T))
    e0 = sorted(float(v) for v in rec['entropy'][0])
    print('exit-0 entropies %s' % (['%.9g' % v for v in rec['entropy'][0].tolist()],))
    for i in range(M):
        print('image %d exit-0 shares %s' % (i, ['%.4f' % v for v in rec['share'][0, i].tolist()]))
    mids = [0.5 * (a + b) for a, b in zip(e0, e0[1:]) if b - a > 1e-6]
    assert len(mids) >= 3
    sweeps = {'entropy': [float('-inf')] + mids + [float('inf')], 'max': list(MAX_T)}
    for kind, thresholds in sweeps.items():
        pts = prof.curve(kind, thresholds)
        split = 0
        for pt, thr in zip(pts, thresholds):
            ev, ties, pixels = Evaluator(19, dev), 0, 0
            for i, (x, t) in enumerate(images):
                with torch.no_grad():
                    y, early, _, val = m.dynamic_inference(x.to(dev), thr, kind)
                assert int(pt['exit_of_image'][i]) == (0 if early else nex - 1), (kind, thr, i)
                assert float(pt['confidence_of_image'][i]) == val, (kind, thr, i, float(pt['confidence_of_image'][i]), val)
                ev.add_batch(t.to(dev), argmax_logits(y))
                top = y.topk(2, dim=1).values
                ties += int(((top[:, 0] - top[:, 1]) < NEAR_TIE_GAP * float(y.abs().max())).sum())
                pixels += top[:, 0].numel()
            want = ev._cm.cpu()
            d_cm = int((pt['confusion'] - want).abs().sum())
            print('%s thr %.9g: exits %s, avg_confidence %.9g, mIoU %.6f vs %.6f, sum|dcm| %d, near-ties %d of %d' % (
                kind, thr, pt['exit_counts'], pt['avg_confidence'], pt['mIoU'], ev.Mean_Intersection_over_Union(), d_cm, ties, pixels))
            assert ties <= NEAR_TIE_SHARE * pixels
            assert d_cm <= 2 * ties
            assert int(pt['confusion'].sum()) == int(want.sum())
            if d_cm == 0:
                # the evaluator's formula on the same matrix: exactly on the device the curve computes on (the CPU); against the
                # evaluator's own fp32 figure from the GPU within the roundings of a 19-term fp32 mean of ratios (21 x 2^-24 < 2e-6)
                assert pt['mIoU'] == float(mean_iou(want))
                assert abs(pt['mIoU'] - ev.Mean_Intersection_over_Union()) <= 2e-6 * pt['mIoU']
            assert pt['num_earlier_exit'] == 100.0 * pt['exit_counts'][0] / M
            if thr not in (float('-inf'), float('inf')) and 0 < pt['exit_counts'][0] < M:
                split += 1
        assert split >= 1, kind
        if kind == 'entropy':
            assert pts[0]['exit_counts'] == [0, M] and pts[-1]['exit_counts'] == [M, 0]
            assert [p['exit_counts'][0] for p in pts] == sorted(p['exit_counts'][0] for p in pts)
    prof.close()


def test_exit_profile_equals_validation_step_batch_by_batch(dev):
    """Two full batches and a short one (count = 1): the summed matrices are ValidationStep's, exactly, per exit; five images are
    logged; the third step runs from the captured graph and repeats the first batch, so its record equals the eager one; the model's
    mode and state are untouched.  Config 3 builds and yields three exits."""
    from addk.exit_profile import ExitProfile
    from addk.validate import ValidationStep
    m = _model(dev).train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    a, b = _batch(2, 11), _batch(2, 12)
    prof = ExitProfile(m, (2, 3) + HW, max_thresholds=(0.2, 0.5, 0.8), keep_predictions=True)
    prof.step(a[0].to(dev), a[1].to(dev))
    prof.step(b[0].to(dev), b[1].to(dev))
    assert prof.graph is None
    four = prof.records()
    prof.step(a[0].to(dev), a[1].to(dev), count=1)
    assert prof.graph is not None and prof.batches == 3 and m.training
    rec = prof.records()
    assert rec['entropy'].shape[1] == rec['share'].shape[1] == rec['confusion'].shape[1] == 5
    for key in ('entropy', 'share', 'confusion'):
        assert torch.equal(rec[key][:, :4], four[key])
        assert torch.equal(rec[key][:, 4], rec[key][:, 0]), key                   # the captured replay against the eager run
    assert len({float(v) for v in rec['entropy'][0, :4]}) == 4                     # ... of images that differ
    preds = prof.predictions()
    ok = (a[1] >= 0) & (a[1] < 19)
    for k, p in enumerate(preds):                                                  # the last batch's maps reproduce its matrices
        for n in range(2):
            want = torch.bincount(19 * a[1][n][ok[n]] + p[n].cpu().long()[ok[n]], minlength=361).view(19, 19)
            assert torch.equal(want, prof.cm[k, n].cpu())
    vs = ValidationStep(m, (2, 3) + HW)
    vs.step(a[0].to(dev), a[1].to(dev))
    vs.step(b[0].to(dev), b[1].to(dev))
    r = vs.result()
    assert len(r['exits']) == prof.nex == 2
    for k, e in enumerate(r['exits']):
        assert torch.equal(e['confusion'].cpu(), four['confusion'][k].sum(0))
        assert torch.equal(e['confusion'].cpu(), four['static'][k]['confusion']) and e['mIoU'] == four['static'][k]['mIoU']
        print('exit %d mIoU %.6f (ValidationStep %.6f)' % (k, four['static'][k]['mIoU'], e['mIoU']))
    after = m.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    vs.close()
    prof.close()
    m3 = _model(dev, ARCH_C3)
    p3 = ExitProfile(m3, (2, 3) + HW, max_thresholds=(0.5,))
    assert [c.name for c in p3.g.fwd].count('profile_upsample') == 3
    p3.step(a[0].to(dev), a[1].to(dev))
    r3 = p3.records()
    assert tuple(r3['entropy'].shape) == (3, 2) and tuple(r3['confusion'].shape) == (3, 2, 19, 19) and len(r3['static']) == 3
    assert all(int(r3['confusion'][k].sum()) == int(ok.sum()) for k in range(3))
    assert len(p3.curve('entropy', [0.5])[0]['exit_counts']) == 3
    p3.close()
