"""Torch reference of the two per-pixel loss shapes of the fused loss head (include/addk.h, addk_ce_upsample_shaped_fwd_bwd): focal loss and
label-smoothed cross-entropy, for any dtype.  focal_loss / smooth_loss take the FULL-resolution logits `up` [N,C,OH,OW] and return the loss;
focal_grad / smooth_grad are the written gradients of include/addk.h with respect to `up`; reference() up-samples low-resolution logits
with F.interpolate(bilinear, align_corners=False) on the CPU and returns loss and gradient (by autograd, with respect to the low-resolution
logits), optionally with a kept mask and with the soft-Dice term of _dice_ref.

Notation of the header: t the pixel's target, p = softmax(up), w_c the class weights (1 without), W = sum_c w_c, keep = valid (target !=
ignore_index and 0 <= target < C) and, with a mask, inside it; n = sum over keep of w_t, the head's normaliser."""
import torch
import torch.nn.functional as Fn


def _common(up, target, class_w, ignore_index, mask):
    C = up.shape[1]
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    keep = valid if mask is None else valid & mask
    tc = torch.where(valid, target, torch.zeros_like(target))
    w = class_w.to(up.dtype) if class_w is not None else torch.ones(C, dtype=up.dtype)
    wt = w[tc] * keep.to(up.dtype)
    onehot = Fn.one_hot(tc, C).permute(0, 3, 1, 2).to(up.dtype)
    return valid, keep, tc, w, wt, onehot


def _pow(q, e):
    """q ** e with 0 ** 0 = 1 (gamma == 1: the exponent gamma - 1 is 0)"""
    return torch.ones_like(q) if e == 0 else q ** e


def _focal_parts(up, tc, onehot):
    logp = torch.log_softmax(up, dim=1)
    p = logp.exp()
    nll = -logp.gather(1, tc[:, None]).squeeze(1)
    q = (p * (1 - onehot)).sum(1)                # 1 - p_t as the sum of the other classes: no cancellation where p_t -> 1
    pt = (p * onehot).sum(1)
    return p, nll, q, pt


def focal_loss(up, target, gamma, class_w=None, ignore_index=255, mask=None):
    """(1/n) sum_keep w_t (1 - p_t)^gamma (-log p_t); exactly 0 when nothing is kept"""
    _, keep, tc, _, wt, onehot = _common(up, target, class_w, ignore_index, mask)
    _, nll, q, _ = _focal_parts(up, tc, onehot)
    n = wt.sum()
    if float(n) == 0:
        return up.sum() * 0
    return (wt * _pow(q, gamma - 1) * q * nll).sum() / n


def focal_grad(up, target, gamma, class_w=None, ignore_index=255, mask=None):
    """d focal_loss / d up as include/addk.h writes it: (1/n) w_t F (p_j - [j = t]), F = (1-p_t)^(gamma-1) ((1-p_t) + gamma p_t (-log p_t))"""
    _, keep, tc, _, wt, onehot = _common(up, target, class_w, ignore_index, mask)
    p, nll, q, pt = _focal_parts(up, tc, onehot)
    n = wt.sum()
    if float(n) == 0:
        return torch.zeros_like(up)
    F = _pow(q, gamma - 1) * (q + gamma * pt * nll)
    return (wt * F / n)[:, None] * (p - onehot)


def smooth_loss(up, target, eps, class_w=None, ignore_index=255, mask=None):
    """(1/n) sum_keep [(1-eps) w_t (-log p_t) + (eps/C) sum_c w_c (-log p_c)]; exactly 0 when nothing is kept"""
    C = up.shape[1]
    _, keep, tc, w, wt, _ = _common(up, target, class_w, ignore_index, mask)
    logp = torch.log_softmax(up, dim=1)
    nll = -logp.gather(1, tc[:, None]).squeeze(1)
    allc = -(logp * w[None, :, None, None]).sum(1)
    n = wt.sum()
    if float(n) == 0:
        return up.sum() * 0
    return ((1 - eps) * (wt * nll).sum() + (eps / C) * (allc * keep.to(up.dtype)).sum()) / n


def smooth_grad(up, target, eps, class_w=None, ignore_index=255, mask=None):
    """d smooth_loss / d up as include/addk.h writes it: (1/n) [(1-eps) w_t (p_j - [j = t]) + (eps/C) (p_j W - w_j)] on the kept pixels"""
    C = up.shape[1]
    _, keep, tc, w, wt, onehot = _common(up, target, class_w, ignore_index, mask)
    p = torch.softmax(up, dim=1)
    n = wt.sum()
    if float(n) == 0:
        return torch.zeros_like(up)
    k = keep.to(up.dtype)[:, None]
    return ((1 - eps) * wt[:, None] * (p - onehot) + (eps / C) * k * (p * w.sum() - w[None, :, None, None])) / n


def upsample(x, hi_hw, dtype):
    """(leaf [N,H,W,C] in `dtype`, its bilinear up-sampling [N,C,OH,OW])"""
    xr = x.detach().to(dtype).requires_grad_(True)
    return xr, Fn.interpolate(xr.permute(0, 3, 1, 2), size=tuple(hi_hw), mode='bilinear', align_corners=False)


def reference(x, target, hi_hw, focal=None, smooth=None, class_w=None, ignore_index=255, dtype=torch.float64, mask=None, scale=1.0, dice=None):
    """x: [N,H,W,C] low-resolution logits, target: [N,OH,OW] int64; exactly one of focal (gamma) and smooth (eps); mask: the kept set of a
    mining head (None: every valid pixel); dice = (weight, smooth): the soft-Dice term of _dice_ref over ALL valid pixels, unweighted.
    Returns a dict: loss = scale * (shaped CE + Dice), dice = scale * Dice (0.0 without), grad = d loss / d x [N,H,W,C]."""
    assert (focal is None) != (smooth is None)
    xr, up = upsample(x, hi_hw, dtype)
    kw = dict(class_w=class_w, ignore_index=ignore_index, mask=mask)
    loss = scale * (focal_loss(up, target, focal, **kw) if focal is not None else smooth_loss(up, target, smooth, **kw))
    term = 0.0
    if dice is not None:
        from _dice_ref import dice_term
        valid = (target != ignore_index) & (target >= 0) & (target < x.shape[-1])
        d, _ = dice_term(up, target, valid, *dice)
        loss = loss + scale * d
        term = float(scale * d.detach())
    loss.backward()
    return dict(loss=float(loss.detach()), dice=term, grad=xr.grad)
