"""Torch reference of the soft-Dice region term in the fused loss head (include/addk.h, addk_dice_stats / addk_ce_upsample_dice_fwd_bwd):
F.interpolate(bilinear, align_corners=False) of the low-resolution logits on the CPU, in fp64 or fp32; the cross-entropy term as in
_ohem_ref.reference / _distill_ref.reference (optional kept mask, class weights and the distillation term), the Dice term over ALL valid
pixels of the batch, unweighted, by autograd."""
import torch
import torch.nn.functional as Fn

from _distill_ref import kd_term


def dice_sums(up, target, valid):
    """I_c, P_c, Y_c over the valid pixels; up: [N,C,OH,OW] logits, target: [N,OH,OW] int64, valid: [N,OH,OW] bool"""
    C = up.shape[1]
    p = torch.softmax(up, dim=1)
    v = valid.to(up.dtype)[:, None]
    tc = torch.where(valid, target, torch.zeros_like(target))
    onehot = Fn.one_hot(tc, C).permute(0, 3, 1, 2).to(up.dtype) * v
    return (p * onehot).sum((0, 2, 3)), (p * v).sum((0, 2, 3)), onehot.sum((0, 2, 3))


def dice_term(up, target, valid, weight, smooth):
    """weight * (1 - mean over the present classes of D_c) and (I, P, Y, D); exactly 0, with no gradient, when no class is present"""
    I, P, Y = dice_sums(up, target, valid)
    present = Y > 0
    m = int(present.sum())
    D = (2 * I + smooth) / (P + Y + smooth).clamp(min=1e-300 if up.dtype == torch.float64 else 1e-30)
    if m == 0:
        return up.sum() * 0, (I, P, Y, D)
    return weight * (1 - torch.where(present, D, torch.zeros_like(D)).sum() / m), (I, P, Y, D)


def reference(x, target, hi_hw, weight, smooth, class_w=None, ignore_index=255, dtype=torch.float64, mask=None, scale=1.0,
              teacher=None, alpha=None, T=None, ce=True):
    """x: [N,H,W,C] low-resolution logits, target: [N,OH,OW] int64; mask: the kept set of a mining head (None: every valid pixel); teacher,
    alpha, T: the distillation term of _distill_ref; ce=False: the Dice term alone.  Returns a dict: loss = scale * (CE + KD + Dice),
    dice = scale * Dice, grad = d loss / d x [N,H,W,C], I, P, Y, D (per class; D where Y > 0 only), present, m, and the coefficient table
    A, B of the header."""
    C = x.shape[-1]
    xr = x.detach().to(dtype).requires_grad_(True)
    up = Fn.interpolate(xr.permute(0, 3, 1, 2), size=tuple(hi_hw), mode='bilinear', align_corners=False)
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    tc = torch.where(valid, target, torch.zeros_like(target))
    loss = up.sum() * 0
    if ce:
        nll = -torch.log_softmax(up, dim=1).gather(1, tc[:, None]).squeeze(1)
        keep = valid if mask is None else mask
        w = (class_w.to(dtype)[tc] if class_w is not None else torch.ones_like(nll)) * keep.to(dtype)
        loss = loss + scale * (w * nll).sum() / w.sum()
    if teacher is not None:
        upt = Fn.interpolate(teacher.detach().to(dtype).permute(0, 3, 1, 2), size=tuple(hi_hw), mode='bilinear', align_corners=False)
        loss = loss + scale * kd_term(up, upt, valid, alpha, T)
    dice, (I, P, Y, D) = dice_term(up, target, valid, weight, smooth)
    dice = scale * dice
    loss = loss + dice
    loss.backward()
    I, P, Y, D = (v.detach() for v in (I, P, Y, D))
    present = Y > 0
    m = int(present.sum())
    den = P + Y + smooth
    k = scale * weight / max(m, 1)
    zero = torch.zeros_like(den)
    A = torch.where(present, k * 2 / den, zero)
    B = torch.where(present, k * (2 * I + smooth) / den ** 2, zero)
    return dict(loss=float(loss.detach()), dice=float(dice.detach()), grad=xr.grad, I=I, P=P, Y=Y, D=D, present=present, m=m, A=A, B=B)
