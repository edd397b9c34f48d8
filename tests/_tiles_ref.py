"""What tests/test_tiles_plan.py (CPU) and tests/test_gpu_tiles.py share: the inputs of the tiled label head's kernel test and the formula
it implements, evaluated with torch.

    acc[n,c,Y,X] = sum over the windows (iy, ix) of image n that cover (Y, X), ascending iy, then ix, of
                   softmax_c( interpolate(logits[tile], (th,tw), bilinear, align_corners=False) )[Y - y0[iy], X - x0[ix]]

A case is (N images, image size, window size, stride, a window's low-resolution grid); the window origins are segment.tile_starts' and
image n's window (iy, ix) is tile (n*ny + iy)*nx + ix of a [T,h,w,C] NHWC tensor.  Every case exists at C = 19 and C = 21.

The rule that says which pixels a comparison of arg-max maps may excuse is tests/_views_ref.py's, imported and not copied: the formula
is evaluated on the CPU in fp64 (A64) and in fp32 (A32), e32 = max |A32 - A64|, tau = 64 * e32; a pixel whose fp64 top-2 gap is below tau is
excused, at most CAP = 0.2 % of a case's pixels may be, and every other pixel must carry the fp64 arg-max.  tests/test_tiles_plan.py
prints e32 and the excused share of every case (measured there with these inputs: e32 between 4.7e-7 and 4.8e-6; excused 0 / 0.12 % of `pad` at C = 19 / 21, 0 / 0.09 % of `exact`,
0.14 / 0.11 % of `grid`, 0.01 / 0.07 % of `odd`)."""
import functools

import torch
import torch.nn.functional as F

from _util import rand_tensor
from _views_ref import CAP, FACTOR, check_map, judge      # noqa: F401  (the rule: shared, not copied)
from addk.segment import tile_starts

SEED = 71
CLASSES = (19, 21)
# name: (N, image, tile, stride, low-resolution grid)
CASES = {'pad': (2, (21, 40), (33, 65), (17, 33), (9, 17)),          # one window larger than the image
         'exact': (1, (33, 65), (33, 65), (17, 33), (9, 17)),        # one window, exact fit
         'grid': (2, (70, 150), (33, 65), (17, 33), (9, 17)),        # 4x4 windows, clamped last ones, up to 3 deep per axis, 9 covers
         'odd': (1, (67, 131), (32, 64), (16, 32), (5, 8))}          # 4x4 windows, non-integer scales


def origins(case):
    """(y origins, x origins) of a case's images"""
    _, (OH, OW), (th, tw), (sy, sx), _ = CASES[case]
    return tile_starts(OH, th, sy), tile_starts(OW, tw, sx)


@functools.lru_cache(maxsize=None)
def logits(case, C):
    """[T,h,w,C] fp32 on the CPU, T = N*ny*nx; never modified"""
    N, _, _, _, (h, w) = CASES[case]
    ys, xs = origins(case)
    return rand_tensor(SEED, 'tiles_x:%s:%d' % (case, C), (N * len(ys) * len(xs), h, w, C)) * 3


def formula(x, N, size, tile, ys, xs, dtype, t0=0):
    """acc [N,C,OH,OW] in `dtype` of the tiles x[t0:] ([.,h,w,C] NHWC) over images of `size`, with torch ops on the CPU"""
    (OH, OW), (th, tw) = size, tile
    acc = torch.zeros((N, x.shape[3], OH, OW), dtype=dtype)
    for n in range(N):
        for iy, y0 in enumerate(ys):
            for ix, x0 in enumerate(xs):
                t = t0 + (n * len(ys) + iy) * len(xs) + ix
                z = F.interpolate(x[t:t + 1].permute(0, 3, 1, 2).to(dtype), (th, tw), mode='bilinear', align_corners=False)
                p = torch.softmax(z, 1)[0]
                y1, x1 = min(y0 + th, OH), min(x0 + tw, OW)                  # the part of a window beyond the image is never sampled
                acc[n, :, y0:y1, x0:x1] += p[:, :y1 - y0, :x1 - x0]
    return acc


def covers(size, tile, ys, xs):
    """how many windows cover each pixel: int64 [OH,OW]"""
    cnt = torch.zeros(size, dtype=torch.int64)
    for y0 in ys:
        for x0 in xs:
            cnt[y0:y0 + tile[0], x0:x0 + tile[1]] += 1
    return cnt


def judge_tiles(x, N, size, tile, ys, xs, t0=0):
    """the rule on tiles given as an NHWC tensor: (A64, fp64 arg-max uint8, excused pixels, e32, tau)"""
    a64 = formula(x, N, size, tile, ys, xs, torch.float64, t0)
    e32 = float((formula(x, N, size, tile, ys, xs, torch.float32, t0).double() - a64).abs().max())
    return judge(a64, FACTOR * e32) + (e32, FACTOR * e32)


@functools.lru_cache(maxsize=None)
def reference(case, C):
    """(A64, its arg-max as uint8 [N,OH,OW], the excused pixels as bool [N,OH,OW], e32, tau) of a case; computed once, never modified"""
    N, size, tile, _, _ = CASES[case]
    ys, xs = origins(case)
    return judge_tiles(logits(case, C), N, size, tile, ys, xs)


def _set(**kw):
    """an edit of a LabelTilesArgs: fields by name, `y0_2=17` sets y0[2]"""
    def edit(a):
        for k, v in kw.items():
            if k[:3] in ('y0_', 'x0_'):
                getattr(a, k[:2])[int(k[3:])] = v
            else:
                setattr(a, k, v)
    edit.what = kw
    return edit


# Every refusal of addk_label_tiles_upsample, as edits of the arguments of case `grid` at C = 19 (y0 = 0, 17, 34, 37 with th = 33 over 70 rows;
# x0 = 0, 33, 66, 85 with tw = 65 over 150 columns).  tests/test_tiles_plan.py makes the calls over dummy addresses (nothing is launched),
# tests/test_gpu_tiles.py over real buffers between guards.
REFUSALS = [_set(C=7), _set(C=20), _set(C=0),                                                                       # not in addk_head_classes()
            _set(ny=0), _set(ny=17), _set(nx=0), _set(nx=17), _set(nx=-1),                                          # outside 1..16
            _set(N=0), _set(OH=0), _set(OW=-3), _set(h=0), _set(w=-1), _set(th=0), _set(tw=0),                      # non-positive sizes
            _set(ld=18), _set(logits=None), _set(labels=None), _set(t0=-1),
            _set(y0_0=1), _set(x0_0=2),                                                                             # the first origin is not 0
            _set(y0_2=17), _set(x0_2=33), _set(y0_2=16), _set(x0_1=70),                                             # not strictly increasing
            _set(y0_1=34), _set(x0_1=66),                                                                           # a gap behind the first window
            _set(y0_3=70), _set(x0_3=150),                                                                          # an origin at the image's end
            _set(ny=3, y0_2=36), _set(nx=3), _set(OH=71), _set(OW=151),                                             # the last window ends before the image
            _set(N=65536), _set(OH=65536 * 16 + 1, ny=1, th=65536 * 16 + 1)]                                        # the grid limits of the label heads
