"""What tests/test_views_plan.py (CPU) and tests/test_gpu_views.py share: the inputs of the multi-view label head's kernel test, the
formula it implements evaluated with torch, and the rule that says which pixels a comparison of arg-max maps may excuse.

    acc[n,c,Y,X] = sum_v weight_v * softmax_c( flip_v( interpolate(logits_v[n0_v + n], (OH,OW), bilinear, align_corners=False) ) )

A view is (logits [B,h,w,19] NHWC, n0, mirror, weight).  The formula is evaluated on the CPU in fp64 (A64) and in fp32 (A32);
e32 = max |A32 - A64| is the reference's own error and tau = 64 * e32 — room for another summation order, fused multiply-adds and the
hardware exponential.  A pixel whose top-2 gap of A64 is below tau is excused, at most CAP of a case's pixels may be, and on every other
pixel the arg-max must be A64's.

Measured with N(0, 3^2) logits: e32 = 9.4e-8 (three_scales), 6.3e-7 (odd), 5.3e-7 (down_one), 1.8e-5 (eight).  The weights of `eight` sum
to 18 and its largest view carries weight 4, so its error is thirty times the others'.  One tau from the largest e32 (1.1e-3) would
excuse 2.4 % of three_scales, 2.6 % of odd and one of down_one's 25 pixels, past the cap, so every case is judged with the tau of ITS OWN
e32, computed where the test runs: 6.0e-6, 4.0e-5, 3.4e-5 and 1.1e-3.  None is larger than the single tau, so no pixel is excused that
the single tau would not excuse; the excused shares are 0.006 %, 0.08 %, 0 and 0.04 %."""
import functools

import torch
import torch.nn.functional as F

from _util import rand_tensor

FACTOR = 64           # tau = FACTOR * e32
CAP = 0.002

# name: (N, view sizes, output size)
CASES = {'three_scales': (2, ((6, 12), (8, 16), (10, 20)), (64, 128)),
         'odd': (2, ((7, 13), (9, 17), (11, 21)), (65, 129)),
         'down_one': (1, ((9, 9),), (5, 5)),
         'eight': (1, ((3, 5), (5, 9), (6, 11), (12, 20)), (40, 70))}


@functools.lru_cache(maxsize=None)
def views(case):
    """[(logits [B,h,w,19] fp32 on the CPU, n0, mirror, weight)] in kernel order; never modified.  `three_scales`, `odd` and `eight` take the
    plain and the mirrored view of a size from one batch-2N tensor (n0 = 0 and n0 = N); `down_one` is a single mirrored view."""
    N, sizes, _ = CASES[case]
    if case == 'down_one':
        return ((rand_tensor(53, 'views_x:down_one', (N,) + sizes[0] + (19,)) * 3, 0, 1, 1.0),)
    nview = 2 * len(sizes)
    weights = [0.5 * (i + 1) for i in range(nview)] if case == 'eight' else [1.0 / nview] * nview
    out = []
    for i, hw in enumerate(sizes):
        x = rand_tensor(53, 'views_x:%s:%d' % (case, i), (2 * N,) + hw + (19,)) * 3
        out += [(x, 0, 0, weights[2 * i]), (x, N, 1, weights[2 * i + 1])]
    return tuple(out)


def formula(vs, N, size, dtype):
    """acc [N,19,OH,OW] of the views `vs` in `dtype`, with torch ops on the CPU"""
    acc = 0
    for x, n0, mirror, weight in vs:
        z = F.interpolate(x[n0:n0 + N].permute(0, 3, 1, 2).to(dtype), size, mode='bilinear', align_corners=False)
        if mirror:
            z = z.flip(3)
        acc = acc + weight * torch.softmax(z, 1)
    return acc


@functools.lru_cache(maxsize=None)
def reference(case):
    """(A64, its arg-max as uint8 [N,OH,OW], the excused pixels as bool [N,OH,OW], e32, tau) of a case; computed once, never modified"""
    N, _, size = CASES[case]
    a64 = formula(views(case), N, size, torch.float64)
    e32 = float((formula(views(case), N, size, torch.float32).double() - a64).abs().max())
    return judge(a64, FACTOR * e32) + (e32, FACTOR * e32)


def judge(a64, tau):
    """(a64, its arg-max, the pixels whose top-2 gap is below tau)"""
    top = a64.topk(2, 1).values
    return a64, a64.argmax(1).to(torch.uint8), (top[:, 0] - top[:, 1]) < tau


def check_map(got, want, excused, what=''):
    """`got` equals the fp64 arg-max outside the excused pixels, and those are within the cap"""
    share = float(excused.float().mean())
    wrong = int(((got != want) & ~excused).sum())
    print('%s: excused %d of %d pixels (%.4f %%), differing outside them: %d, inside: %d'
          % (what, int(excused.sum()), excused.numel(), 100 * share, wrong, int(((got != want) & excused).sum())))
    assert share <= CAP, (what, share)
    assert wrong == 0, (what, wrong)
