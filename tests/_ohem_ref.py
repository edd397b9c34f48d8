"""Torch reference of online hard example mining in the loss head (include/addk.h, addk_ohem_select / addk_ce_upsample_ohem_fwd_bwd):
F.interpolate(bilinear, align_corners=False) + log_softmax on the CPU, in fp64 or fp32; tau from a full torch.sort."""
import math

import torch
import torch.nn.functional as Fn


def tau_theta(thresh, dtype=torch.float32):
    """-log(theta) for the fp32 word `thresh` the library receives: evaluated in double, rounded to fp32 for the fp32 forms"""
    v = -math.log(float(torch.tensor(thresh, dtype=torch.float32))) if thresh < 1.0 else 0.0
    return float(torch.tensor(v, dtype=dtype))


def select_tau(vals, thresh, K, dtype=torch.float32):
    """tau = min(-log theta, K-th largest of vals (the largest min(K, n) when fewer)) and the count of vals >= tau; vals: 1-D, valid pixels only"""
    tt = tau_theta(thresh, dtype)
    n = vals.numel()
    if n == 0:
        return tt, 0
    kth = float(torch.sort(vals, descending=True).values[min(int(K), n) - 1])
    tau = min(tt, kth)
    return tau, int((vals >= tau).sum())


def reference(x, target, hi_hw, thresh, K, class_w=None, ignore_index=255, dtype=torch.float64, mask=None, scale=1.0):
    """x: [N,H,W,C] low-resolution logits, target: [N,OH,OW] int64.  Returns a dict:
    l     [N,OH,OW] per-pixel loss max(0, logsumexp(z) - z[t]), -1 where the pixel is not valid
    tau, valid (count), mask (valid & l >= tau, or the `mask` handed in), kept (count)
    loss  scale * sum_mask w*nll / sum_mask w, grad = d loss / d x  [N,H,W,C]"""
    C = x.shape[-1]
    xr = x.detach().to(dtype).requires_grad_(True)
    up = Fn.interpolate(xr.permute(0, 3, 1, 2), size=tuple(hi_hw), mode='bilinear', align_corners=False)
    lsm = torch.log_softmax(up, dim=1)
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    tc = torch.where(valid, target, torch.zeros_like(target))
    nll = -lsm.gather(1, tc[:, None]).squeeze(1)
    l = torch.where(valid, nll.detach().clamp(min=0), torch.full_like(nll.detach(), -1.0))
    tau, _ = select_tau(l[valid], thresh, K, dtype)
    if mask is None:
        mask = valid & (l >= tau)
    w = (class_w.to(dtype)[tc] if class_w is not None else torch.ones_like(nll)) * mask.to(dtype)
    loss = scale * (w * nll).sum() / w.sum()
    loss.backward()
    return dict(l=l, tau=tau, valid=int(valid.sum()), mask=mask, kept=int(mask.sum()), loss=float(loss.detach()), grad=xr.grad)
