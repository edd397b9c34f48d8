"""What tests/test_tile_views_plan.py (CPU) and tests/test_gpu_tile_views.py share: the cases and inputs of the tiled multi-view label head's
kernel test and the formula it implements (include/addk.h, addk_label_tile_views_upsample), evaluated with torch in a given dtype.

For one image (OH, OW), window (th, tw), a window's low-resolution grid (h, w), views v = (scale, mirror, weight) in order, (Hv, Wv) =
view_size(OH, OW, scale) and the windows ys_v x xs_v = tile_starts(Hv, th, sy) x tile_starts(Wv, tw, sx):

    Xm = mirror ? OW-1-X : X;   u_y = (Y + 1/2) Hv/OH,  u_x = (Xm + 1/2) Wv/OW
    window (iy, ix) covers (Y, X) iff 2 OH y0 <= (2Y+1) Hv < 2 OH (y0 + th) and likewise x: integers, never floats
    k_v(Y, X) = (covering window rows) * (covering window columns)
    acc[c,Y,X] = sum_v sum over the covering windows, ascending iy then ix, of (w_v / k_v) * softmax_c(z),
    z = bilinear sample of the window's logits at a_y = (u_y - y0) h/th - 1/2, a_x = (u_x - x0) w/tw - 1/2 (a < 0 -> 0, i0 = floor(a)
    capped at h-1, i1 = min(i0+1, h-1), lambda = a - i0)

The coordinates are computed in the dtype of the evaluation, the membership in integers.  The store layout of a case is the head's: view v's
tiles start at t0_v, image n's window (iy, ix) of view v is tile t0_v + (n ny_v + iy) nx_v + ix; the views' blocks follow each other.

The rule that says which pixels a comparison of arg-max maps may excuse is tests/_views_ref.py's, imported and not copied: A64 and A32
are the formula in fp64 and fp32 on the CPU, e32 = max |A32 - A64|, tau = 64 * e32 per case; a pixel whose fp64 top-2 gap is below tau is
excused, at most CAP = 0.2 % of a case's pixels may be, every other pixel must carry the fp64 arg-max.

The inputs are consistent across views: independent logits per window average to flat sums over six views, and the fp32 reference alone
then excuses more than the cap.  Every image has one coarse scene [C,5,9] ~ N(0, 3^2); a window's low-resolution pixel (a, b) samples it
(grid_sample, bilinear, align_corners=True, border) at its centre in image-normalised coordinates, v = (y0 + (a + 1/2) th/h) / Hv and
u = (x0 + (b + 1/2) tw/w) / Wv (1 - u in a mirrored view), plus independent N(0, 0.5^2) noise.  tests/test_tile_views_plan.py prints e32 and
the excused share of every case."""
import functools
import re

import torch
import torch.nn.functional as F

from _util import rand_tensor
from _views_ref import CAP, FACTOR, check_map, judge      # noqa: F401  (the rule: shared, not copied)
from addk.segment import tile_starts, view_size

SEED = 83
CLASSES = (19, 21)
# name: (N, image, window, stride, low-resolution grid, views as (scale, mirror, weight))
CASES = {
    'three': (2, (40, 70), (33, 65), (17, 33), (9, 17),
              tuple((s, m, 1.0 / 6) for s in (0.75, 1.0, 1.25) for m in (False, True))),                    # 18 windows per image
    'odd': (1, (37, 61), (32, 64), (16, 32), (5, 8), ((0.5, False, 0.25), (1.5, True, 0.25), (1.75, False, 0.5))),      # non-integer ratios everywhere
    'weights': (1, (30, 50), (16, 24), (8, 12), (4, 6),
                ((0.75, False, 0.5), (1.0, True, 1.0), (1.25, False, 1.5), (2.0, True, 2.0))),             # 94 windows, clamped last windows
    'pad': (2, (21, 40), (33, 65), (17, 33), (9, 17), ((1.0, False, 0.5), (1.0, True, 0.5), (0.5, False, 1.0))),        # image smaller than the window in every view
}


def grids_of(N, size, tile, stride, views, t0=0):
    """[(Hv, Wv, y origins, x origins, first tile)] per view: the views' blocks of N * ny * nx tiles follow each other from tile t0"""
    out = []
    for s, _, _ in views:
        Hv, Wv = view_size(size[0], size[1], s)
        ys, xs = tile_starts(Hv, tile[0], stride[0]), tile_starts(Wv, tile[1], stride[1])
        out.append((Hv, Wv, ys, xs, t0))
        t0 += N * len(ys) * len(xs)
    return out


def grids(case, t0=0):
    N, size, tile, stride, _, views = CASES[case]
    return grids_of(N, size, tile, stride, views, t0)


def ntiles(case):
    N = CASES[case][0]
    return sum(N * len(ys) * len(xs) for _, _, ys, xs, _ in grids(case))


def member(O, Lv, origins, t, mirror=False):
    """bool [len(origins), O]: window i covers output index o of an axis of O pixels whose scaled length is Lv — in integers"""
    o = torch.arange(O, dtype=torch.int64)
    c = (2 * (O - 1 - o if mirror else o) + 1) * int(Lv)
    return torch.stack([(2 * O * int(o0) <= c) & (c < 2 * O * (int(o0) + int(t))) for o0 in origins])


def _axis(O, Lv, origins, t, lo, dtype, mirror=False):
    """per window of an axis: (membership [n,O] bool, i0 [n,O], i1 [n,O], lambda [n,O] in dtype)"""
    o = torch.arange(O, dtype=torch.int64)
    om = O - 1 - o if mirror else o
    u = (om.to(dtype) + 0.5) * (torch.tensor(Lv, dtype=dtype) / torch.tensor(O, dtype=dtype))
    sc = torch.tensor(lo, dtype=dtype) / torch.tensor(t, dtype=dtype)
    i0s, i1s, ls = [], [], []
    for o0 in origins:
        a = ((u - o0) * sc - 0.5).clamp(min=0)
        i0 = a.floor().long().clamp(max=lo - 1)
        i0s.append(i0)
        i1s.append((i0 + 1).clamp(max=lo - 1))
        ls.append(a - i0.to(dtype))
    return member(O, Lv, origins, t, mirror), torch.stack(i0s), torch.stack(i1s), torch.stack(ls)


def formula(x, N, size, tile, low, views, gr, dtype, wrong=None):
    """acc [N,C,OH,OW] in `dtype` of the store x ([.,h,w,C] NHWC) with torch ops on the CPU.  `gr`: grids_of().  `wrong` names a deliberately
    wrong formula (the sensitivity test): 'mirror' ignores the mirror, 'cover' does not divide by k, 'weights' takes all weights equal,
    'row' takes only the first covering window row."""
    (OH, OW), (th, tw), (h, w) = size, tile, low
    acc = torch.zeros((N, x.shape[3], OH, OW), dtype=dtype)
    for (_, mirror, weight), (Hv, Wv, ys, xs, t0) in zip(views, gr):
        if wrong == 'mirror':
            mirror = False
        if wrong == 'weights':
            weight = 1.0 / len(views)
        my, i0y, i1y, ly = _axis(OH, Hv, ys, th, h, dtype)
        mx, i0x, i1x, lx = _axis(OW, Wv, xs, tw, w, dtype, mirror)
        if wrong == 'row':
            my = my & (my.long().cumsum(0) == 1)
        k = my.sum(0)[:, None] * mx.sum(0)[None, :]
        assert int(k.min()) >= 1
        wk = torch.tensor(weight, dtype=dtype) / (torch.ones_like(k) if wrong == 'cover' else k).to(dtype)
        for n in range(N):
            for iy in range(len(ys)):
                Yi = my[iy].nonzero().flatten()
                for ix in range(len(xs)):
                    Xi = mx[ix].nonzero().flatten()
                    if not len(Yi) or not len(Xi):
                        continue
                    z = x[t0 + (n * len(ys) + iy) * len(xs) + ix].to(dtype)
                    l1 = lx[ix][Xi][None, :, None]
                    zw = (1 - l1) * z[:, i0x[ix][Xi]] + l1 * z[:, i1x[ix][Xi]]                    # [h, nX, C]
                    l1 = ly[iy][Yi][:, None, None]
                    zz = (1 - l1) * zw[i0y[iy][Yi]] + l1 * zw[i1y[iy][Yi]]                        # [nY, nX, C]
                    p = torch.softmax(zz, 2) * wk[Yi][:, Xi][:, :, None]
                    acc[n][:, Yi[:, None], Xi[None, :]] += p.permute(2, 0, 1)
    return acc


@functools.lru_cache(maxsize=None)
def logits(case, C):
    """[T,h,w,C] fp32 on the CPU in the head's store layout (grids(case)); never modified"""
    N, size, (th, tw), _, (h, w), views = CASES[case]
    x = rand_tensor(SEED, 'tile_views_noise:%s:%d' % (case, C), (ntiles(case), h, w, C)) * 0.5
    a, b = torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5
    for n in range(N):
        scene = rand_tensor(SEED, 'tile_views_scene:%s:%d:%d' % (case, C, n), (1, C, 5, 9)) * 3
        for (_, mirror, _), (Hv, Wv, ys, xs, t0) in zip(views, grids(case)):
            for iy, y0 in enumerate(ys):
                for ix, x0 in enumerate(xs):
                    v = (y0 + a * th / h) / Hv
                    u = (x0 + b * tw / w) / Wv
                    if mirror:
                        u = 1 - u
                    grid = torch.stack([(2 * u - 1)[None, :].expand(h, w), (2 * v - 1)[:, None].expand(h, w)], 2)
                    s = F.grid_sample(scene, grid[None], mode='bilinear', padding_mode='border', align_corners=True)
                    x[t0 + (n * len(ys) + iy) * len(xs) + ix] += s[0].permute(1, 2, 0)
    return x


def judge_views(x, N, size, tile, low, views, gr):
    """the rule on a store: (A64, fp64 arg-max uint8, excused pixels, e32, tau)"""
    a64 = formula(x, N, size, tile, low, views, gr, torch.float64)
    e32 = float((formula(x, N, size, tile, low, views, gr, torch.float32).double() - a64).abs().max())
    return judge(a64, FACTOR * e32) + (e32, FACTOR * e32)


@functools.lru_cache(maxsize=None)
def reference(case, C):
    """(A64, its arg-max as uint8 [N,OH,OW], the excused pixels as bool [N,OH,OW], e32, tau) of a case; computed once, never modified"""
    N, size, tile, _, low, views = CASES[case]
    return judge_views(logits(case, C), N, size, tile, low, views, grids(case))


def fill_args(a, case, C, t0=0):
    """the geometry of a case in a LabelTileViewsArgs (no pointers, no stride); the case's tiles are tiles t0.. of the store"""
    N, size, tile, _, (h, w), views = CASES[case]
    a.nview, a.h, a.w, a.th, a.tw = len(views), h, w, tile[0], tile[1]
    a.N, a.C, a.OH, a.OW = N, C, size[0], size[1]
    for v, (_, mirror, weight), (Hv, Wv, ys, xs, tv) in zip(a.view, views, grids(case, t0)):
        v.Hv, v.Wv, v.t0, v.ny, v.nx, v.mirror, v.weight = Hv, Wv, tv, len(ys), len(xs), int(mirror), weight
        v.y0[:len(ys)], v.x0[:len(xs)] = ys, xs
    return a


def _set(*pairs):
    """an edit of a LabelTileViewsArgs: _set('view[4].y0[1]', 34, 'C', 7) sets the named fields"""
    pairs = list(zip(pairs[::2], pairs[1::2]))

    def edit(a):
        for path, value in pairs:
            steps = re.findall(r'(\w+)(?:\[(\d+)\])?', path)
            obj = a
            for i, (name, idx) in enumerate(steps):
                last = i == len(steps) - 1
                if idx == '':
                    if last:
                        setattr(obj, name, value)
                    else:
                        obj = getattr(obj, name)
                elif last:
                    getattr(obj, name)[int(idx)] = value
                else:
                    obj = getattr(obj, name)[int(idx)]
    edit.what = pairs
    return edit


# Every refusal of addk_label_tile_views_upsample, as edits of the arguments of case `three` at C = 19: image (40, 70), window (33, 65); the views
# are (30, 53) with one window (views 0, 1), (40, 70) with y0 = 0, 7 and x0 = 0, 5 (views 2, 3) and (50, 88) with y0 = 0, 17 and x0 = 0, 23 (views 4, 5).
# tests/test_tile_views_plan.py makes the calls over dummy addresses (nothing is launched), tests/test_gpu_tile_views.py over real buffers between guards.
REFUSALS = [_set('nview', 0), _set('nview', 9), _set('nview', -1),                                                     # outside 1..8
            _set('C', 7), _set('C', 20), _set('C', 0),                                                                # not in addk_head_classes()
            _set('N', 0), _set('OH', 0), _set('OW', -3), _set('h', 0), _set('w', -1), _set('th', 0), _set('tw', 0),   # non-positive sizes
            _set('ld', 18), _set('logits', None), _set('labels', None),
            _set('view[2].t0', -1), _set('view[0].Hv', 0), _set('view[1].Wv', -1),
            _set('view[2].ny', 0), _set('view[2].ny', 17), _set('view[5].nx', 0), _set('view[5].nx', 17), _set('view[3].nx', -1),       # outside 1..16
            _set('view[0].weight', 0.0), _set('view[3].weight', -1.0), _set('view[5].weight', float('inf')), _set('view[1].weight', float('nan')),
            _set('view[2].y0[0]', 1), _set('view[5].x0[0]', 2),                                                       # the first origin is not 0
            _set('view[4].y0[1]', 0), _set('view[4].x0[1]', 0),                                                       # not strictly increasing
            _set('view[4].y0[1]', 34), _set('view[4].x0[1]', 66),                                                     # a gap behind the first window
            _set('view[4].y0[1]', 50), _set('view[4].x0[1]', 88),                                                     # an origin at the scaled image's end
            _set('view[4].Hv', 51), _set('view[3].Wv', 71), _set('view[2].ny', 1), _set('view[0].Hv', 34),            # the last window ends before the scaled image
            _set('N', 65536), _set('OH', 65536 * 16 + 1)]                                                             # the grid limits of the label heads
