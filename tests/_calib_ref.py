"""fp64 reference of the calibration head and of the tempered gates (tests/test_gpu_calib.py, tests/test_gpu_calibrate.py), and the
bounds both files hold the fp32 kernels to.  CPU only; nothing here touches the library."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

BINS = 16
TEMPERATURES = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0)
NEAR = 1e-5                  # tests/test_gpu_gate.py: |confidence - edge| window inside which fp32 and fp64 may fall on different sides
NEAR_TIE_GAP = 1e-4          # tests/test_gpu_validate.py: top-two gap relative to max |logit| below which the arg-max may differ
CAP = 0.005                  # share of the valid pixels that may sit inside either window


def inverse_words(temperatures):
    """the fp32 words 1 / T a launch reads: the kernel's input, which the reference takes as it is (promoted to fp64)"""
    return torch.tensor([1.0 / t for t in temperatures], dtype=torch.float32)


def upsample64(x, hi):
    """low-resolution NHWC logits [N,H,W,C] -> fp64 [N,C,OH,OW] (decoder.py:28)"""
    return Fn.interpolate(x.double().permute(0, 3, 1, 2), size=tuple(hi), mode='bilinear', align_corners=False)


def correlated_input(x, hi, seed=17):
    """The `correlated` input of a case from its plain logits x [N,H,W,19]: 9 is added to one random channel per low-resolution pixel; the
    target is the arg-max of the fp64 up-sample, 20 % of the pixels redrawn uniformly, 5 % set to 255 -> (logits, target)."""
    r = np.random.default_rng(seed)
    N, H, W, Cc = x.shape
    ch = torch.from_numpy(r.integers(0, Cc, (N, H, W)))
    x = x.clone()
    x.scatter_add_(3, ch[..., None], torch.full((N, H, W, 1), 9.0))
    t = upsample64(x, hi).argmax(1)
    shape = (N,) + tuple(hi)
    redraw = torch.from_numpy(r.random(shape) < 0.2)
    t[redraw] = torch.from_numpy(r.integers(0, Cc, shape))[redraw]
    t[torch.from_numpy(r.random(shape) < 0.05)] = 255
    return x, t


def reference(z64, t, inv):
    """Calibration statistics of fp64 logits z64 [N,C,OH,OW] against targets t [N,OH,OW] at the inverse temperatures `inv` (any float
    tensor, promoted to fp64), by the definitions of include/addk.h -> dict: valid, ties, count [nt,B], hits [nt,B], conf [nt,B]
    (fp64 sums), nll [nt] (fp64 sums), edge [nt] (pixels whose confidence lies within NEAR of an interior bin edge), accuracy."""
    Cc = z64.shape[1]
    ok = (t >= 0) & (t < Cc)
    z = z64.permute(0, 2, 3, 1)[ok]                                  # [P, C]
    tt = t[ok]
    P = int(tt.numel())
    top = z.topk(2, dim=1).values
    ties = int(((top[:, 0] - top[:, 1]) < NEAR_TIE_GAP * float(z64.abs().max())).sum())
    mx, am = z.max(1)
    hit = am == tt
    d = z - mx[:, None]
    dt = d.gather(1, tt[:, None])[:, 0]
    nt = len(inv)
    count, hits = torch.zeros((nt, BINS), dtype=torch.int64), torch.zeros((nt, BINS), dtype=torch.int64)
    conf, nll, edge = torch.zeros((nt, BINS), dtype=torch.float64), torch.zeros(nt, dtype=torch.float64), []
    for j, it in enumerate(inv.double().tolist()):
        se = (d * it).exp().sum(1)
        nll[j] = (se.log() - dt * it).sum()
        c = 1.0 / se
        b = (c * BINS).long().clamp(max=BINS - 1)
        count[j] = torch.bincount(b, minlength=BINS)
        hits[j] = torch.bincount(b[hit], minlength=BINS)
        conf[j] = torch.zeros(BINS, dtype=torch.float64).index_add_(0, b, c)
        k = (c * BINS).round().clamp(1, BINS - 1)                    # the nearest interior edge k / BINS
        edge.append(int(((c - k / BINS).abs() < NEAR).sum()))
    return dict(valid=P, ties=ties, count=count, hits=hits, conf=conf, nll=nll, edge=edge, accuracy=float(hit.sum()) / max(P, 1))


def check_bins(tag, bins, ref):
    """The bounds of the bins of one launch (int64 [nt,B,3]: count, hits, confidence sum in units of 2^-24) against reference(): prints
    each figure, then asserts."""
    valid = ref['valid']
    print('%s: valid %d, near-ties %d (cap %.1f), accuracy %.4f' % (tag, valid, ref['ties'], CAP * valid, ref['accuracy']))
    assert ref['ties'] <= CAP * valid
    for j in range(bins.shape[0]):
        E = ref['edge'][j]
        cnt, hit, cs = bins[j, :, 0], bins[j, :, 1], bins[j, :, 2].double() * 2.0 ** -24
        d_cnt = int((cnt - ref['count'][j]).abs().sum())
        d_hit = int((hit - ref['hits'][j]).abs().sum())
        d_conf = (cs - ref['conf'][j]).abs()
        slack = NEAR * ref['count'][j].double() + E
        print('%s[T%d]: near-edge %d (cap %.1f), sum|dcount| %d, sum|dhits| %d, max |dconf| - bound %.3g, top bin %d of %d' % (
            tag, j, E, CAP * valid, d_cnt, d_hit, float((d_conf - slack).max()), int(cnt[-1]), valid))
        assert E <= CAP * valid
        assert int(cnt.sum()) == valid
        assert d_cnt <= 2 * E
        assert d_hit <= 2 * E + 2 * ref['ties']
        assert bool((d_conf <= slack).all())


def check_nll(tag, nll, ref, unfused):
    """The bound of the NLL sums [nt] against reference(): 4x the error of the materialised fp32 form `unfused` [nt] against the same
    reference, or 2e-6 relative."""
    for j in range(len(nll)):
        want = float(ref['nll'][j])
        err, err_u = abs(float(nll[j]) - want), abs(float(unfused[j]) - want)
        print('%s[T%d]: NLL sum %.12g ref64 %.12g unfused %.12g: rel err fused %.3g unfused %.3g' % (
            tag, j, float(nll[j]), want, float(unfused[j]), err / abs(want), err_u / abs(want)))
        assert err <= max(4 * err_u, 2e-6 * abs(want))


def tempered_gate_reference(z64, T):
    """per image: normalised entropy [N] of softmax(z64 / T) and its top probability [N,OH,OW], fp64"""
    lp = torch.log_softmax(z64 / T, dim=1)
    ent = -(lp.exp() * lp).sum((1, 2, 3)) / (math.log(z64.shape[1]) * z64.shape[2] * z64.shape[3])
    return ent, lp.exp().amax(1)
