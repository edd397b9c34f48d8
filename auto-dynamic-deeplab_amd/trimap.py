"""Boundary-band ("trimap") mIoU: the evaluator's confusion matrix restricted to the pixels within d pixels of a ground-truth class
boundary, for a ladder of widths d (the trimap plot of the DeepLab papers).  The definition is include/addk.h's ("Boundary-band
confusion"): Euclidean distance to the nearest edge pixel of the same image, rounded up to an integer; csrc/trimap.hip counts disjoint
rings and the cumulative matrix "within d" is their prefix sum, taken here.  What validate.ValidationStep and exit_profile.ExitProfile
share of it: the check of the width list, the one `boundary_dist` launch of a batch and the result entries."""
import ctypes as C

import torch

from . import _lib as L
from .metrics import mean_iou


def check_widths(trimap):
    """The width ladder as a tuple of ints: strictly ascending, each in [1, 64], at most 8 of them."""
    try:
        raw = list(trimap)
    except TypeError:
        raise ValueError('trimap must be an iterable of widths (got %r)' % (trimap,)) from None
    ws = []
    for w in raw:
        if isinstance(w, bool) or int(w) != w:
            raise ValueError('trimap widths must be integers (got %r)' % (w,))
        ws.append(int(w))
    if not 1 <= len(ws) <= L.TRIMAP_MAX_WIDTHS:
        raise ValueError('trimap takes 1 to %d widths (got %d)' % (L.TRIMAP_MAX_WIDTHS, len(ws)))
    if any(not 1 <= w <= L.TRIMAP_MAX_RADIUS for w in ws) or any(not b > a for a, b in zip(ws, ws[1:])):
        raise ValueError('trimap widths must be strictly ascending integers in [1, %d] (got %r)' % (L.TRIMAP_MAX_RADIUS, tuple(ws)))
    return tuple(ws)


def emit_boundary_dist(g, target, dist, ncls, widths):
    """ONE `boundary_dist` launch (`addk_boundary_dist`) into the forward list of plan `g`: the distance map of the resident targets,
    shared by every exit of the batch.  Radius = the largest width."""
    lib = g.lib
    N, OH, OW = (int(v) for v in target.shape)
    radius = widths[-1]
    if lib.addk_boundary_dist_supported(N, OH, OW, ncls, radius) != 1 or lib.addk_confusion_banded_supported(N, OH, OW, ncls, len(widths)) != 1:
        raise ValueError('the trimap metric takes 1 to 32 classes and fewer than 2^31 pixels (got %d classes, [%d,%d,%d])' % (ncls, N, OH, OW))
    ws = torch.zeros(int(lib.addk_boundary_dist_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=g.device)
    a = L.BoundaryDistArgs()
    a.target, a.N, a.OH, a.OW, a.C, a.radius = target.data_ptr(), N, OH, OW, ncls, radius
    a.dist, a.ws = dist.data_ptr(), ws.data_ptr()
    g.keep += [a, ws]
    g.nbytes += dist.numel() + ws.numel()
    g._add(g.fwd, 'boundary_dist', lib.addk_boundary_dist, C.byref(a), rd=[target], wr=[dist, ws])


def band_figures(cum):
    """[..., nw, C, C] cumulative matrices -> 1-D fp64 tensor on their device: mIoU (metrics.mean_iou) of every matrix, then its pixel
    count (exact below 2^53).  No host synchronisation."""
    flat = cum.reshape(-1, cum.shape[-2], cum.shape[-1])
    miou = [mean_iou(m).double() for m in flat]
    return torch.cat([torch.stack(miou) if miou else cum.new_zeros(0, dtype=torch.float64), flat.sum((1, 2)).double()])


def band_entries(widths, cum, figures):
    """One dict per width for ONE exit: `width`, `confusion` (cumulative int64 [C,C]: the pixels within `width` of a boundary), `mIoU`
    and `pixels`.  `cum` [nw, C, C]; `figures` = (mIoU per width, pixels per width) as host numbers."""
    miou, pixels = figures
    return [dict(width=w, confusion=cum[j].clone(), mIoU=float(miou[j]), pixels=int(pixels[j])) for j, w in enumerate(widths)]
