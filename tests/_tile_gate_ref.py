"""What tests/test_tile_gate_plan.py (CPU) and tests/test_gpu_tile_gate.py share: the inputs of the kernel test of addk_gate_tiles_upsample
and the formula it implements, evaluated with torch on the CPU.

    z          = interpolate(logits[b], (th, tw), bilinear, align_corners=False) * s          s = 1 / temperature, or 1
    p          = softmax_c(z)
    entropy[b] = sum over Y < vh, X < vw of -sum_c p log p / (log C * vh * vw)
    share[b]   = #{Y < vh, X < vw: max_c p > thr} / (vh * vw)

with (vh, vw) the slot's extent clamped to 1..th, 1..tw.  A case is (h, w, th, tw); every case exists at C = 19 and 21, with and without
the inverse temperature 1 / 1.7, and its B = 3 slots take the extents EXTENTS[(b + r) % 4] for the rotation r in 0, 1, so that two
launches cover every extent; for the 17 x 40 window (33, 33), (33, 7) and (20, 33) exceed the window and are clamped.

The rule of a comparison with fp64 is tests/_views_ref.py's (FACTOR, CAP): e32 is the error of the fp32 formula against the fp64 one for these
very inputs — for the entropy max_b |entropy32 - entropy64|, and the kernel may differ from fp64 by FACTOR * e32; for the share
e32p = max over the valid pixels of |pmax32 - pmax64|, a pixel whose fp64 pmax lies within FACTOR * e32p of the threshold is excused, at most
CAP of a window's valid pixels may be, and the count over the other pixels must be exact.  THR = 0.6 with N(0, 3^2) logits excuses no
pixel of any case (tests/test_tile_gate_plan.py asserts it and prints every case's figures)."""
import functools
import math

import torch
import torch.nn.functional as F

from _util import rand_tensor
from _views_ref import CAP, FACTOR      # noqa: F401  (the rule: shared, not copied)

SEED = 83
B = 3
CLASSES = (19, 21)
CASES = {'x4': (9, 9, 33, 33), 'odd': (5, 9, 17, 40)}
EXTENTS = ((33, 33), (33, 7), (1, 1), (20, 33))
INV_TEMP = (None, 1 / 1.7)
THR = 0.6


def extents(r):
    """the extents of the B slots at rotation r, as given to the kernel (unclamped)"""
    return [EXTENTS[(b + r) % len(EXTENTS)] for b in range(B)]


def clamp(ext, th, tw):
    return [(min(max(vh, 1), th), min(max(vw, 1), tw)) for vh, vw in ext]


@functools.lru_cache(maxsize=None)
def logits(case, C):
    """[B,h,w,C] fp32 on the CPU; never modified"""
    h, w, _, _ = CASES[case]
    return rand_tensor(SEED, 'tile_gate_x:%s:%d' % (case, C), (B, h, w, C)) * 3


def formula(x, size, ext, s, thr, dtype):
    """-> (entropy [B], pmax maps [(vh, vw)] per slot) of the NHWC logits x in `dtype`"""
    Cc = x.shape[3]
    z = F.interpolate(x.permute(0, 3, 1, 2).to(dtype), size, mode='bilinear', align_corners=False)
    if s is not None:
        z = z * torch.tensor(s, dtype=torch.float32).to(dtype)               # the kernel reads the fp32 word
    logp = torch.log_softmax(z, 1)
    ent = -(logp.exp() * logp).sum(1)
    pmax = logp.exp().amax(1)
    out, maps = [], []
    for b, (vh, vw) in enumerate(clamp(ext, *size)):
        out.append(ent[b, :vh, :vw].sum() / (math.log(Cc) * vh * vw))
        maps.append(pmax[b, :vh, :vw])
    return torch.stack(out), maps


@functools.lru_cache(maxsize=None)
def reference(case, C, temp, r):
    """-> dict: entropy64 [B], e32 (entropy), per slot (valid pixels, fp64 hits outside the excused pixels, excused pixels), e32p; computed
    once, never modified"""
    _, _, th, tw = CASES[case]
    ext = extents(r)
    e64, p64 = formula(logits(case, C), (th, tw), ext, INV_TEMP[temp], THR, torch.float64)
    e32, p32 = formula(logits(case, C), (th, tw), ext, INV_TEMP[temp], THR, torch.float32)
    e32p = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    slots = []
    for p in p64:
        excused = (p - THR).abs() <= FACTOR * e32p
        slots.append((p.numel(), int(((p > THR) & ~excused).sum()), int(excused.sum())))
    return dict(entropy=e64, e32=float((e32.double() - e64).abs().max()), slots=slots, e32p=e32p, ext=clamp(ext, th, tw))


def check_share(word, npix, hits, excused, what=''):
    """the share word against the fp64 count: the excused pixels within the cap, the count over the others exact"""
    assert excused <= CAP * npix, (what, excused, npix)
    ok = [torch.tensor(c / npix, dtype=torch.float64).float().item() for c in range(hits, hits + excused + 1)]
    assert word in ok, (what, word, ok)
