"""Torch reference of self-distillation from the final exit in the fused loss head (include/addk.h, addk_ce_upsample_kd_fwd_bwd):
F.interpolate(bilinear, align_corners=False) of the student's and the teacher's low-resolution logits on the CPU, in fp64 or fp32; the
cross-entropy term as in _ohem_ref.reference (optional kept mask and class weights), the distillation term over ALL valid pixels with the
teacher detached."""
import torch
import torch.nn.functional as Fn


def kd_term(up_s, up_t, valid, alpha, T):
    """alpha * T^2 * (1/n) * sum over valid pixels of KL(softmax(up_t / T) || softmax(up_s / T)); up_*: [N,C,OH,OW], valid: [N,OH,OW] bool.
    Exactly 0 (and no gradient) when no pixel is valid."""
    n = int(valid.sum())
    if n == 0:
        return up_s.sum() * 0
    ls = torch.log_softmax(up_s / T, dim=1)
    lt = torch.log_softmax(up_t.detach() / T, dim=1)
    kl = (lt.exp() * (lt - ls)).sum(1)
    return alpha * T * T * torch.where(valid, kl, torch.zeros_like(kl)).sum() / n


def reference(x, teacher, target, hi_hw, alpha, T, class_w=None, ignore_index=255, dtype=torch.float64, mask=None, scale=1.0):
    """x, teacher: [N,H,W,C] low-resolution logits, target: [N,OH,OW] int64; mask: the kept set of a mining head (None: every valid pixel).
    Returns a dict: loss = scale * (CE + KD), kd = scale * KD, ce = scale * CE, grad = d loss / d x [N,H,W,C], valid (count)."""
    C = x.shape[-1]
    xr = x.detach().to(dtype).requires_grad_(True)
    tr = teacher.detach().to(dtype)
    up = Fn.interpolate(xr.permute(0, 3, 1, 2), size=tuple(hi_hw), mode='bilinear', align_corners=False)
    upt = Fn.interpolate(tr.permute(0, 3, 1, 2), size=tuple(hi_hw), mode='bilinear', align_corners=False)
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    tc = torch.where(valid, target, torch.zeros_like(target))
    nll = -torch.log_softmax(up, dim=1).gather(1, tc[:, None]).squeeze(1)
    keep = valid if mask is None else mask
    w = (class_w.to(dtype)[tc] if class_w is not None else torch.ones_like(nll)) * keep.to(dtype)
    ce = scale * (w * nll).sum() / w.sum()
    kd = scale * kd_term(up, upt, valid, alpha, T)
    loss = ce + kd
    loss.backward()
    return dict(loss=float(loss.detach()), kd=float(kd.detach()), ce=float(ce.detach()), grad=xr.grad, valid=int(valid.sum()))
