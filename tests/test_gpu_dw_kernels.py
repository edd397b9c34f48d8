"""Kernel-level tests of the depthwise convolution kernels (csrc/dw.hip: generic and LDS-tiled forward and backward, their table-driven
batch forms, the two weight-gradient reductions) and of the 3x3 pooling kernels (csrc/misc.hip), called through the C ABI and compared,
element by element, with fp64 evaluations of the same fp32 inputs.

Shapes: first every distinct depthwise launch of config 2's train plan at 2x1024x2048 (NET_DW; tests/test_dw_shapes.py dry-builds that plan
and fails when it runs a launch the table does not list), then the rest of the C ABI contract at the smallest shapes that reach each edge
(CONTRACT; the kernel each shape takes is asserted from addk_dw_fwd_config / addk_dw_bwd_config, on the CPU too).  Every output, workspace
and slab holds NaN before a launch, padding channels included, so an element a kernel does not write — or one it should not — fails.
Where a launch accumulates, the whole buffer holds finite random data and the padding channels must come back bit-unchanged.

The reference is a plain tap loop in fp64: a sum over taps of shifted slices of z = relu(a x + b), which also yields, per element, the sum S
of the magnitudes of the terms.  Bounds follow the arithmetic (U = 2^-24 the fp32 unit roundoff, ULP = 2^-23; one fp32 operation on a
partial sum moves it by at most U times the magnitudes summed so far, and the bounds allow an ulp, 2 U, per operation):
 * y: one fma for z, `taps` fmas: (taps + 2) ULP sum_t |w_t| |z_t| per element;
 * g: `taps` fmas, the mask, one multiply by a, one add when accumulating: (taps + 3) ULP (|a| sum_t |w_t| |dy_t| + |old|) per element;
 * dab: fp64 sums over the pixels of gm (fp32, `taps` fmas) times x: (taps + 2) ULP sum_p S_p |x_p| per channel, plus the fp64 summation
   term (rows + 64) 2^-53 sum |terms| of the BatchNorm tests;
 * dw: fp32 sums over the pixels: (L + 2) ULP sum_p |dy z| per weight element, L the longest chain of additions a partial sum goes
   through (_chain): the fmas of one thread (its pixels), the block's fixed-order sum over its npl pixel lanes, then the reduction over
   the workspace rows — dw_wreduce_kernel: ceil(rows / 64) per lane and a 6-step butterfly; dw_wreduce_batch_kernel: at most
   ceil(rows / 4) per thread and 4 combining adds.
For dw and dab the bound must lie below the median non-zero single term (a zero term — a masked pixel, a tap in the padding — changes
nothing when dropped), so one pixel dropped or counted twice cannot pass; tests/test_dw_shapes.py asserts the same on the CPU.
The kernels decide the ReLU mask on fmaf(a, x, b) > 0 in fp32; inputs with |a x + b| < 4 U (|a x| + |b|) are replaced (_clear_of_zero).
The batched launches are held bit-identical to the single ones.  Nothing in dw.hip claims bit identity between the tiled and the generic
kernels, so the generic kernel (addk_set_fast_paths(0)) is held to the same fp64 bounds instead.
3x3 pooling: max is exact up to the one rounding of the affine (U |v| of the window's largest magnitude), average within 11 ulps of
sum |v| / cnt; gradients within (9 + 3) ulps of the magnitudes routed to the element.
Every measured error / bound goes to dw_kernel_errors.txt in the directory ADDK_REPORT_DIR names (the system's temporary directory
when it is unset), the worst ratio per output kind at its end."""
import collections
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import addk  # noqa: F401  (registers the package)
from addk import _lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ULP = 2.0 ** -23
E64 = 2.0 ** -53
f64 = torch.float64
DEV = 'cuda'

# ---- config 2's train plan at 2x1024x2048 (F = 20, ARCH_C2): every distinct depthwise launch (all on the 32x64, 160-channel level) ----
# (N, H, W, C, k, stride, dil, src.ld, ldy / lddy, ldg, relu, lazy a/b, has g, accumulate, has dab); the forward launch of a tuple is its
# (N, H, W, C, k, stride, dil, src.ld, ldy, relu, lazy).  src.ld = 800: the input is a slot of a cell's concat buffer, the gradient is
# accumulated into the same slot.  Every backward launch defers its weight reduction (addk_dw_wreduce_batch), dw_accumulate = 0.
NET_DW = [
    (2, 32, 64, 160, 3, 1, 1, 160, 160, 160, 1, True, True, 0, True),
    (2, 32, 64, 160, 3, 1, 1, 160, 160, 160, 1, True, True, 1, True),
    (2, 32, 64, 160, 3, 1, 1, 800, 160, 800, 1, False, True, 1, False),
    (2, 32, 64, 160, 5, 1, 1, 160, 160, 160, 1, True, True, 0, True),
    (2, 32, 64, 160, 5, 1, 1, 800, 160, 800, 1, False, True, 1, False),
]
# the plan runs no addk_pool3_* launch (the genotype has no pooling primitive): (N, H, W, C, stride, mode, ld, ldy)
NET_POOL = []

Spec = collections.namedtuple('Spec', 'name N H W C k stride dil ld ldy lddy ldg relu lazy g acc dab dw_acc xoff expect')


def S(name, N, H, W, Cc, k, stride=1, dil=1, ld=None, ldy=None, lddy=None, ldg=None, relu=1, lazy=True, g=True, acc=0, dab=True, dw_acc=0,
      xoff=0, expect=None):
    return Spec(name, N, H, W, Cc, k, stride, dil, ld or Cc, ldy or Cc, lddy or ldy or Cc, ldg or ld or Cc, relu, lazy, g, acc, dab, dw_acc,
                xoff, expect)


def net_spec(i):
    N, H, W, Cc, k, stride, dil, ld, ldy, ldg, relu, lazy, g, acc, dab = NET_DW[i]
    return S('net%d' % i, N, H, W, Cc, k, stride, dil, ld, ldy, ldy, ldg, relu, lazy, g, acc, dab, 0, 320 if ld > Cc else 0,
             expect=dict(fwd=(1, 15 if k == 3 else 11), bwd=(1, 12 if k == 3 else 8, 24 if k == 3 else 32, 341), ngrp=4))


# expect: fwd = (tiled, rows per tile), bwd = (tiled, rows per tile, grid x, workspace rows), ngrp = channel groups of the tiled kernels
#         (addk_dw_*_config; a generic kernel has 0 rows per tile and one group).  rows = P / (2 npl), npl = 256 / ceil(C / 4).
CONTRACT = [
    # the 2048-pixel floor of the tiled kernels, k = 3 and 5, dilation 1 and 2; bwd grid x < rows: the zero-fill makes dw / dab correct
    S('floor_k3', 1, 32, 64, 40, 3, expect=dict(fwd=(1, 15), bwd=(1, 12, 12, 40), ngrp=1)),
    S('floor_k5', 1, 32, 64, 40, 5, expect=dict(fwd=(1, 11), bwd=(1, 8, 16, 40), ngrp=1)),
    S('floor_k3_d2', 1, 32, 64, 40, 3, dil=2, expect=dict(fwd=(1, 11), bwd=(1, 8, 16, 40), ngrp=1)),
    S('floor_k5_d2', 1, 32, 64, 40, 5, dil=2, expect=dict(fwd=(1, 4), bwd=(1, 2, 40, 40), ngrp=1)),
    S('below_k3', 1, 31, 66, 40, 3, expect=dict(fwd=(0, 0), bwd=(0, 0, 40, 40), ngrp=1)),
    S('below_k5_d2', 1, 31, 66, 40, 5, dil=2, expect=dict(fwd=(0, 0), bwd=(0, 0, 40, 40), ngrp=1)),
    # stride 2: the forward is tiled from 2048 OUTPUT pixels on, the backward falls to the generic kernel
    S('s2_k3', 1, 65, 127, 40, 3, stride=2, expect=dict(fwd=(1, 4), bwd=(0, 0, 165, 165), ngrp=1)),
    S('s2_k5', 1, 65, 127, 40, 5, stride=2, expect=dict(fwd=(1, 2), bwd=(0, 0, 165, 165), ngrp=1)),
    S('s2_k3_d2', 1, 65, 127, 40, 3, stride=2, dil=2, expect=dict(fwd=(1, 2), bwd=(0, 0, 165, 165), ngrp=1)),
    # W % 16 != 0, H % TH != 0, a partly full last channel group (C = 44: 8 + 3 quads, C = 48: 8 + 4), H < TH
    S('rem_c44_k3', 1, 37, 70, 44, 3, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 56), ngrp=2)),
    S('rem_c44_k5', 1, 37, 70, 44, 5, expect=dict(fwd=(1, 15), bwd=(1, 12, 20, 56), ngrp=2)),
    S('rem_c48_k5_d2', 1, 37, 70, 48, 5, dil=2, expect=dict(fwd=(1, 8), bwd=(1, 5, 40, 61), ngrp=2)),
    S('short_c48_k3', 1, 9, 250, 48, 3, expect=dict(fwd=(1, 9), bwd=(1, 9, 16, 53), ngrp=2)),
    S('c160_k5', 1, 32, 64, 160, 5, expect=dict(fwd=(1, 11), bwd=(1, 8, 16, 170), ngrp=4)),
    # more tiles than workspace rows: a block of the backward walks several tiles (C = 4: 256 pixel lanes, rows = P / 512)
    S('walk_c4_k3', 1, 32, 64, 4, 3, expect=dict(fwd=(1, 16), bwd=(1, 16, 4, 4), ngrp=1)),
    S('walk_c8_k5', 2, 40, 50, 8, 5, expect=dict(fwd=(1, 16), bwd=(1, 16, 15, 15), ngrp=1)),
    # generic only: C % 4 != 0 (scalar path), ld % 4 != 0 at a size the tiled kernels would take
    S('c6_k3', 1, 13, 19, 6, 3, expect=dict(fwd=(0, 0), bwd=(0, 0, 1, 1), ngrp=1)),
    S('c6_k5_d2', 2, 13, 19, 6, 5, dil=2, ld=7, ldy=9, ldg=8, expect=dict(fwd=(0, 0), bwd=(0, 0, 1, 1), ngrp=1)),
    S('c37_k5', 1, 13, 19, 37, 5, expect=dict(fwd=(0, 0), bwd=(0, 0, 4, 4), ngrp=1)),
    S('c37_k3_s2', 2, 13, 19, 37, 3, stride=2, ld=40, ldy=40, ldg=40, expect=dict(fwd=(0, 0), bwd=(0, 0, 9, 9), ngrp=1)),
    S('ld42_k3', 1, 32, 64, 40, 3, ld=42, expect=dict(fwd=(0, 0), bwd=(0, 0, 40, 40), ngrp=1)),
    S('ldy42_k5', 1, 32, 64, 40, 5, ldy=42, ldg=40, expect=dict(fwd=(0, 0), bwd=(0, 0, 40, 40), ngrp=1)),
    # the contract's switches on a tiled shape (each runs on the generic kernel too), then on a generic-only one
    S('sw_pad', 1, 33, 70, 44, 3, ld=48, ldy=52, lddy=56, ldg=60, xoff=4, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 50), ngrp=2)),
    S('sw_no_g', 1, 33, 70, 44, 3, g=False, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 50), ngrp=2)),
    S('sw_no_dab', 1, 33, 70, 44, 5, dab=False, expect=dict(fwd=(1, 15), bwd=(1, 12, 15, 50), ngrp=2)),
    S('sw_no_g_no_dab', 1, 33, 70, 44, 3, g=False, dab=False, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 50), ngrp=2)),
    S('sw_plain', 1, 33, 70, 44, 5, lazy=False, expect=dict(fwd=(1, 15), bwd=(1, 12, 15, 50), ngrp=2)),
    S('sw_no_relu', 1, 33, 70, 44, 3, relu=0, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 50), ngrp=2)),
    S('sw_plain_no_relu', 1, 33, 70, 44, 3, relu=0, lazy=False, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 50), ngrp=2)),
    S('sw_acc', 1, 33, 70, 44, 5, acc=1, ldg=48, expect=dict(fwd=(1, 15), bwd=(1, 12, 15, 50), ngrp=2)),
    S('sw_dw_acc', 1, 33, 70, 44, 3, dw_acc=1, expect=dict(fwd=(1, 16), bwd=(1, 15, 15, 50), ngrp=2)),
    S('sw_all_k5_d2', 2, 33, 70, 44, 5, dil=2, ld=48, ldy=48, lddy=52, ldg=56, acc=1, dw_acc=1, xoff=4,
      expect=dict(fwd=(1, 8), bwd=(1, 5, 70, 100), ngrp=2)),
    S('gen_sw_pad_acc', 1, 13, 19, 6, 3, ld=9, ldy=8, lddy=7, ldg=10, acc=1, dw_acc=1, xoff=2, expect=dict(fwd=(0, 0), bwd=(0, 0, 1, 1), ngrp=1)),
    S('gen_sw_plain_no_g', 1, 13, 19, 37, 5, lazy=False, relu=0, g=False, dab=False, expect=dict(fwd=(0, 0), bwd=(0, 0, 4, 4), ngrp=1)),
]

REPORT = []
WORST = {}


def _log(fmt, *a):
    REPORT.append(fmt % a)


def teardown_module(module):
    d = os.environ.get('ADDK_REPORT_DIR') or tempfile.gettempdir()
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'dw_kernel_errors.txt'), 'w') as f:
        f.write('\n'.join(REPORT) + '\n')
        f.write('worst error / bound per output kind: %s\n' % ', '.join('%s %.3f' % kv for kv in sorted(WORST.items())))


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return L.load()


@pytest.fixture
def generic(lib):
    """Switches the fast paths off (the generic kernels run) and restores the mask, whatever the test does."""
    mask = int(lib.addk_get_fast_paths())

    def switch(on):
        lib.addk_set_fast_paths(0 if on else mask)
    yield switch
    lib.addk_set_fast_paths(mask)


def _st(dev):
    return torch.cuda.current_stream().cuda_stream if dev != 'cpu' else 0


def _rng(seed):
    return torch.Generator().manual_seed(seed)      # a CPU generator: the same data here and on the CPU check of the bounds


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen)


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _table(structs, dev):
    """A device table of argument structs, uploaded as Graph._table does: the bytes of a ctypes array in a uint8 tensor."""
    arr = (type(structs[0]) * len(structs))(*structs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == f64 else torch.int32)


def _same_bits(what, a, b):
    d = int((_bits(a) != _bits(b)).sum())
    assert d == 0, '%s: not bit-identical (%d elements differ)' % (what, d)


def _all_nan(what, t):
    n = int((~torch.isnan(t)).sum())
    assert n == 0, '%s: %d elements written' % (what, n)


def _close(kind, what, got, ref, bound):
    """Every element of `got` written (no NaN left) and within its own `bound` of the fp64 `ref`; logs the largest error / bound."""
    nn = int(torch.isnan(got).sum())
    assert nn == 0, '%s: %d elements not written' % (what, nn)
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(r.max())
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    _log('%-4s %-92s err/bound %.3f  max err %.2e', kind, what, worst, float(err.max()))
    assert worst <= 1.0, '%s: error %.3e is %.2f x its bound (flat index %d)' % (what, float(err.reshape(-1)[int(r.argmax())]), worst,
                                                                               int(r.argmax()))


def _clear_of_zero(x, a, b):
    """The kernels decide the ReLU mask on fmaf(a, x, b) > 0 in fp32, the reference on a x + b in fp64.  Replaces every x whose
    |a x + b| < 4 U (|a x| + |b|) by (1 - b) / a, where a x + b is 1, and asserts that none remains.  Returns (x, replaced)."""
    if a is None:
        return x, 0                                  # z = x itself: fp32 and fp64 see the same sign
    ad, bd = a.double(), b.double()

    def near(v):
        ax = ad * v.double()
        return (ax + bd).abs() < 4 * U * (ax.abs() + bd.abs())
    bad = near(x)
    x = torch.where(bad, ((1.0 - bd) / ad).float().expand_as(x), x)
    left = int(near(x).sum())
    assert left == 0, '%d inputs still within 4 U of the ReLU threshold' % left
    return x, int(bad.sum())


def _nonzero_median(t):
    """Per column of t [n, ...]: the median of its non-zero magnitudes."""
    t = t.abs()
    return torch.where(t > 0, t, torch.full_like(t, float('nan'))).nanmedian(0).values


def _cdiv(a, b):
    return -(-a // b)


class Out:
    pass


class Dw:
    """One depthwise convolution: fp32 inputs in buffers of the spec's row strides (NaN in the padding channels), the fp64 reference,
    fresh outputs for every launch."""

    def __init__(self, s, seed, dev=DEV):
        self.s, self.dev = s, dev
        N, H, W, Cc, k = s.N, s.H, s.W, s.C, s.k
        self.pad = s.dil * (k // 2)
        self.OH = (H + 2 * self.pad - s.dil * (k - 1) - 1) // s.stride + 1
        self.OW = (W + 2 * self.pad - s.dil * (k - 1) - 1) // s.stride + 1
        self.P, self.Po, self.taps = N * H * W, N * self.OH * self.OW, k * k
        gen = _rng(seed)
        x = _randn(gen, self.P, Cc)
        a = (0.5 + _rand(gen, Cc)) * torch.where(_rand(gen, Cc) < 0.5, -1.0, 1.0) if s.lazy else None
        b = 0.3 * _randn(gen, Cc) if s.lazy else None
        w = 0.3 * _randn(gen, Cc, self.taps)
        dy = _randn(gen, self.Po, Cc)
        gold = _randn(gen, self.P, s.ldg)
        dwold = _randn(gen, Cc, self.taps)
        self.replaced = 0
        if s.relu:
            x, self.replaced = _clear_of_zero(x, a, b)
        self.xb = _nan(dev, self.P, s.ld)
        self.x = self.xb[:, s.xoff:s.xoff + Cc]
        self.x.copy_(x)
        self.a, self.b = (a.to(dev), b.to(dev)) if s.lazy else (None, None)
        self.w = w.to(dev)
        self.dyb = _nan(dev, self.Po, s.lddy)
        self.dy = self.dyb[:, :Cc]
        self.dy.copy_(dy)
        self.gold, self.dwold = gold.to(dev), dwold.to(dev)
        self.ref = self._reference()

    def _reference(self):
        """fp64 tap loop: y, dz (the gradient of z), dw as sums over taps of shifted slices, each with the sum of its terms' magnitudes."""
        s, pad = self.s, self.pad
        N, H, W, Cc, OH, OW = s.N, s.H, s.W, s.C, self.OH, self.OW
        x = self.x.double().view(N, H, W, Cc)
        zp = x if self.a is None else self.a.double() * x + self.b.double()
        m = zp > 0 if s.relu else torch.ones_like(zp, dtype=torch.bool)
        z = torch.where(m, zp, torch.zeros_like(zp))
        zpad = F.pad(z, (0, 0, pad, pad, pad, pad))
        dy, w = self.dy.double().view(N, OH, OW, Cc), self.w.double()
        y, Sy = torch.zeros_like(dy), torch.zeros_like(dy)
        dz, Sdz = torch.zeros_like(zpad), torch.zeros_like(zpad)
        dw, Sdw, Mdw = (torch.zeros(Cc, self.taps, dtype=f64, device=self.dev) for _ in range(3))
        for kh in range(s.k):
            for kw in range(s.k):
                t = kh * s.k + kw
                sl = (slice(None), slice(kh * s.dil, kh * s.dil + (OH - 1) * s.stride + 1, s.stride),
                      slice(kw * s.dil, kw * s.dil + (OW - 1) * s.stride + 1, s.stride))
                zt, wt = zpad[sl], w[:, t]
                y += wt * zt
                Sy += wt.abs() * zt.abs()
                dz[sl] += wt * dy
                Sdz[sl] += wt.abs() * dy.abs()
                terms = (dy * zt).reshape(-1, Cc)
                dw[:, t], Sdw[:, t], Mdw[:, t] = terms.sum(0), terms.abs().sum(0), _nonzero_median(terms)
        inner = (slice(None), slice(pad, pad + H), slice(pad, pad + W))
        gm, Sgm = dz[inner] * m, Sdz[inner] * m
        av = self.a.double().abs() if self.a is not None else 1.0
        g = gm * (self.a.double() if self.a is not None else 1.0)
        tA, tB = (gm * x).reshape(-1, Cc), gm.reshape(-1, Cc)
        R = Out()
        R.y, R.Sy = y.reshape(-1, Cc), Sy.reshape(-1, Cc)
        R.g, R.Sg = g.reshape(-1, Cc), (Sgm * av).reshape(-1, Cc)
        R.dab = torch.stack((tA.sum(0), tB.sum(0)), -1)
        R.Sdab = torch.stack(((Sgm * x.abs()).reshape(-1, Cc).sum(0), Sgm.reshape(-1, Cc).sum(0)), -1)      # sum_p S_p |x_p|, sum_p S_p
        R.Tdab = torch.stack((tA.abs().sum(0), tB.abs().sum(0)), -1)                                         # sum |terms| (fp64 summation)
        R.Mdab = torch.stack((_nonzero_median(tA), _nonzero_median(tB)), -1)
        R.dw, R.Sdw, R.Mdw = dw, Sdw, Mdw
        return R

    # ---- arguments ----
    def src(self):
        sr = L.Src()
        sr.x, sr.a, sr.b, sr.ld, sr.C, sr.relu, sr.rs_hw = self.x.data_ptr(), _p(self.a), _p(self.b), self.s.ld, self.s.C, int(self.s.relu), 0
        return sr

    def _geom(self, ar):
        s = self.s
        ar.N, ar.H, ar.W, ar.OH, ar.OW, ar.KH, ar.KW, ar.stride, ar.pad, ar.dil = s.N, s.H, s.W, self.OH, self.OW, s.k, s.k, s.stride, self.pad, s.dil

    def out(self, rows):
        """NaN in every output, workspace and slab; where the launch accumulates, the old finite content (the same for every launch)."""
        s, o = self.s, Out()
        o.yb = _nan(self.dev, self.Po, s.ldy)
        o.gb = (self.gold.clone() if s.acc else _nan(self.dev, self.P, s.ldg)) if s.g else None
        o.dab = _nan(self.dev, rows, s.C, 2, dtype=f64) if s.dab else None
        o.ws = _nan(self.dev, rows, s.C * self.taps)
        o.dw = self.dwold.clone() if s.dw_acc else _nan(self.dev, s.C, self.taps)
        return o

    def goff(self):
        return self.s.xoff if self.s.ldg == self.s.ld else 0       # a gradient accumulated into the input's slot of a concat buffer

    def fwd_args(self, o):
        ar = L.DwArgs()
        ar.src = self.src()
        self._geom(ar)
        ar.w, ar.y, ar.ldy = self.w.data_ptr(), o.yb.data_ptr(), self.s.ldy
        return ar

    def bwd_args(self, o, defer):
        s, ba = self.s, L.DwBwdArgs()
        ba.dy, ba.lddy = self.dy.data_ptr(), s.lddy
        self._geom(ba)
        ba.src, ba.w = self.src(), self.w.data_ptr()
        if s.g:
            ba.g, ba.ldg, ba.accumulate = o.gb[:, self.goff():].data_ptr(), s.ldg, int(s.acc)
        ba.dab = _p(o.dab)
        ba.dw, ba.dw_accumulate, ba.ws, ba.defer_wreduce = o.dw.data_ptr(), int(s.dw_acc), o.ws.data_ptr(), int(defer)
        return ba

    def configs(self, lib):
        """cfg[8] of the forward and of the backward launch (addk.h): kind, k, rows per tile, grid x, grid y, LDS bytes, rows, batch key."""
        rows = int(lib.addk_dw_rows(self.P, self.s.C))
        o = self.out(rows)
        cf, cb = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        L.check(lib.addk_dw_fwd_config(C.byref(self.fwd_args(o)), cf), 'dw_fwd_config')
        L.check(lib.addk_dw_bwd_config(C.byref(self.bwd_args(o, 1)), cb), 'dw_bwd_config')
        return list(cf), list(cb), rows

    def chain(self, cb, batched):
        """L of the dw bound: the longest chain of fp32 additions a weight-gradient partial sum goes through.
        Generic kernel: a thread walks ceil(P / (grid x * npl)) pixels (one fma each per tap); tiled kernel: a block walks
        ceil(ntiles / grid x) tiles, a thread ceil(TH * 16 / npl) pixels of each.  Then the block adds its npl pixel lanes one after the
        other, and the workspace rows are reduced: by dw_wreduce_kernel (a lane adds ceil(rows / 64) rows, then 6 butterfly steps) or by
        dw_wreduce_batch_kernel (a thread adds at most ceil(rows / 4) rows, then 4 combining adds)."""
        s = self.s
        tiled, _, TH, gx, ngrp, _, rows, _ = cb
        nq = min(256, _cdiv(s.C, 4))
        if tiled:
            nqb = nq if nq <= 10 else (10 if nq % 10 == 0 else 8)
            assert ngrp == _cdiv(nq, nqb)
            npl = 256 // nqb
            per = _cdiv(s.N * _cdiv(s.H, TH) * _cdiv(s.W, 16), gx) * _cdiv(TH * 16, npl)
        else:
            npl = max(1, 256 // nq)
            per = _cdiv(self.P, gx * npl)
        return per + npl + (_cdiv(rows, 4) + 4 if batched else _cdiv(rows, 64) + 6)

    # ---- bounds and checks ----
    def dw_bound(self, chain):
        return (chain + 2) * ULP * self.ref.Sdw

    def dab_bound(self, rows):
        return (self.taps + 2) * ULP * self.ref.Sdab + (rows + 64) * E64 * self.ref.Tdab

    def assert_sums_see_one_term(self, chains, rows):
        """One dropped or doubled pixel must not pass: the bounds of the sums lie below the median non-zero single term."""
        for ch in chains:
            assert bool((self.dw_bound(ch) < self.ref.Mdw).all()), '%s: the dw bound (chain %d) does not resolve one term' % (self.s.name, ch)
        if self.s.dab:
            assert bool((self.dab_bound(rows) < self.ref.Mdab).all()), '%s: the dab bound does not resolve one term' % self.s.name

    def check_fwd(self, tag, o):
        s = self.s
        _close('y', '%s %s y' % (s.name, tag), o.yb[:, :s.C], self.ref.y, (self.taps + 2) * ULP * self.ref.Sy)
        _all_nan('%s %s: y padding channels' % (s.name, tag), o.yb[:, s.C:])

    def check_bwd(self, tag, o, chain, rows):
        s, R = self.s, self.ref
        if s.g:
            g0, g1 = self.goff(), self.goff() + s.C
            ref, Sg = R.g, R.Sg
            if s.acc:
                old = self.gold[:, g0:g1].double()
                ref, Sg = ref + old, Sg + old.abs()
                _same_bits('%s %s: g outside its channels' % (s.name, tag), torch.cat((o.gb[:, :g0], o.gb[:, g1:]), 1),
                           torch.cat((self.gold[:, :g0], self.gold[:, g1:]), 1))
            else:
                _all_nan('%s %s: g padding channels' % (s.name, tag), torch.cat((o.gb[:, :g0], o.gb[:, g1:]), 1))
            _close('g', '%s %s g' % (s.name, tag), o.gb[:, g0:g1], ref, (self.taps + 3) * ULP * Sg)
        if o.dab is not None:
            nn = int(torch.isnan(o.dab).sum())
            assert nn == 0, '%s %s: %d of the %d x %d dab slab entries not written' % (s.name, tag, nn, rows, 2 * s.C)
            _close('dab', '%s %s dab (%d rows)' % (s.name, tag, rows), o.dab.sum(0), R.dab, self.dab_bound(rows))
        nn = int(torch.isnan(o.ws).sum())
        assert nn == 0, '%s %s: %d of the %d x %d workspace entries not written' % (s.name, tag, nn, rows, s.C * self.taps)
        ref, Sdw = R.dw, R.Sdw
        if s.dw_acc:
            ref, Sdw = ref + self.dwold.double(), Sdw + self.dwold.double().abs()
        _close('dw', '%s %s dw (chain %d)' % (s.name, tag, chain), o.dw, ref, (chain + 2) * ULP * Sdw)


def _wreduce_item(ws, dw, rows, n, acc):
    it = L.DwWreduceItem()
    it.ws, it.dw, it.rows, it.n, it.accumulate = ws.data_ptr(), dw.data_ptr(), rows, n, int(acc)
    return it


def _launch(lib, d, tag, rows, cb):
    """Forward, backward with its own weight reduction, backward with the reduction deferred to addk_dw_wreduce_batch: each against
    fp64.  Returns the outputs of the single launches (the deferred backward's)."""
    st = _st(d.dev)
    o = d.out(rows)
    L.check(lib.addk_dw_fwd(C.byref(d.fwd_args(o)), st), 'dw_fwd')
    d.check_fwd(tag, o)
    L.check(lib.addk_dw_bwd(C.byref(d.bwd_args(o, 0)), st), 'dw_bwd')
    d.check_bwd(tag + ' wave-reduced', o, d.chain(cb, False), rows)
    q = d.out(rows)
    q.yb = o.yb
    L.check(lib.addk_dw_bwd(C.byref(d.bwd_args(q, 1)), st), 'dw_bwd (deferred)')
    if d.s.dw_acc:
        _same_bits('%s %s: a deferred launch leaves dw alone' % (d.s.name, tag), q.dw, d.dwold)
    else:
        _all_nan('%s %s: a deferred launch leaves dw alone' % (d.s.name, tag), q.dw)
    tab = _table([_wreduce_item(q.ws, q.dw, rows, d.s.C * d.taps, d.s.dw_acc)], d.dev)
    L.check(lib.addk_dw_wreduce_batch(tab.data_ptr(), 1, st), 'dw_wreduce_batch')
    d.check_bwd(tag + ' batch-reduced', q, d.chain(cb, True), rows)
    _same_bits('%s %s: workspace of the deferred launch' % (d.s.name, tag), q.ws, o.ws)
    if q.gb is not None:
        _same_bits('%s %s: g of the deferred launch' % (d.s.name, tag), q.gb, o.gb)
    if q.dab is not None:
        _same_bits('%s %s: dab of the deferred launch' % (d.s.name, tag), q.dab, o.dab)
    return q


def _expect(d, cf, cb, rows):
    e = d.s.expect
    got = dict(fwd=(cf[0], cf[2]), bwd=(cb[0], cb[2], cb[3], cb[6]), ngrp=max(cf[4], cb[4]))
    assert got == e, '%s: kernel choice %s, the table expects %s' % (d.s.name, got, e)
    assert cb[6] == rows and cb[3] <= rows
    assert cf[7] == (d.s.k if cf[0] else -1) and cb[7] == ((d.s.k | 16) if cb[0] else -1)      # batch keys (deferred reduction)


def _case(lib, generic, s, seed):
    """One spec: the kernels the library chooses for it (asserted), then the generic kernels, under the same bounds."""
    d = Dw(s, seed)
    cf, cb, rows = d.configs(lib)
    _expect(d, cf, cb, rows)
    chains = [d.chain(cb, False), d.chain(cb, True)]
    q = _launch(lib, d, 'tiled' if cb[0] else ('tiled fwd' if cf[0] else 'generic'), rows, cb)
    if cf[0] or cb[0]:
        generic(True)
        gf, gb, _ = d.configs(lib)
        assert gf[0] == 0 and gb[0] == 0 and gb[6] == rows
        chains += [d.chain(gb, False), d.chain(gb, True)]
        _launch(lib, d, 'generic (fast paths off)', rows, gb)
        generic(False)
    d.assert_sums_see_one_term(chains, rows)
    return d, q, rows


def _batched(lib, runs, bwd):
    """The launches of `runs` [(Dw, single outputs, rows)] that share a batch key, each key's through *_batch_prepare + addk_dw_batch_run
    into fresh NaN outputs: bit-identical to the single launches.  Returns the number of batches run."""
    groups = collections.defaultdict(list)
    for d, q, rows in runs:
        o = d.out(rows)
        ar = d.bwd_args(o, 1) if bwd else d.fwd_args(o)
        key = int((lib.addk_dw_bwd_batch_key if bwd else lib.addk_dw_fwd_batch_key)(C.byref(ar)))
        if key >= 0:
            groups[key].append((d, q, o, ar))
    prep = lib.addk_dw_bwd_batch_prepare if bwd else lib.addk_dw_fwd_batch_prepare
    for key, items in sorted(groups.items()):
        n = len(items)
        arr = (type(items[0][3]) * n)(*[it[3] for it in items])
        meta = (C.c_int64 * 8)()
        size = int(prep(arr, n, None, 0, meta))
        assert size > 0, 'batch_prepare: %s' % lib.addk_last_error().decode()
        blob = (C.c_uint8 * size)()
        assert int(prep(arr, n, blob, size, meta)) == size
        assert meta[0] == key and meta[1] == n
        tab = torch.frombuffer(bytearray(bytes(blob)), dtype=torch.uint8).to(items[0][0].dev)
        L.check(lib.addk_dw_batch_run(tab.data_ptr(), meta, _st(items[0][0].dev)), 'dw_batch_run')
        for d, q, o, _ in items:
            tag = '%s batched %s (key %d, %d launches)' % (d.s.name, 'bwd' if bwd else 'fwd', key, n)
            if not bwd:
                _same_bits(tag + ' y', o.yb, q.yb)
                continue
            _same_bits(tag + ' ws', o.ws, q.ws)
            if o.gb is not None:
                _same_bits(tag + ' g', o.gb, q.gb)
            if o.dab is not None:
                _same_bits(tag + ' dab', o.dab, q.dab)
        _log('batch %s key %d: %d launches bit-identical to the single ones', 'bwd' if bwd else 'fwd', key, n)
    return len(groups)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the network's launches
# ------------------------------------------------------------------------------------------------------------------------------------
def test_dw_at_network_shapes_single_deferred_and_batched(lib, generic):
    """Every distinct depthwise launch of config 2's train plan, single and deferred; then the launches addk_dw_*_batch_key groups (the
    3x3 ones, the 5x5 ones; forward and backward) through prepare + addk_dw_batch_run, bit-identical; then all five deferred weight
    reductions in one addk_dw_wreduce_batch table, bit-identical to the one-item tables."""
    runs = [_case(lib, generic, net_spec(i), 100 + i) for i in range(len(NET_DW))]
    assert _batched(lib, runs, False) == 2 and _batched(lib, runs, True) == 2
    dws = [_nan(DEV, d.s.C, d.taps) for d, _, _ in runs]
    tab = _table([_wreduce_item(q.ws, dw, rows, d.s.C * d.taps, 0) for (d, q, rows), dw in zip(runs, dws)], DEV)
    L.check(lib.addk_dw_wreduce_batch(tab.data_ptr(), len(runs), _st(DEV)), 'dw_wreduce_batch')
    for (d, q, _), dw in zip(runs, dws):
        _same_bits('%s dw_wreduce_batch of %d items' % (d.s.name, len(runs)), dw, q.dw)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the contract at the smallest shapes that reach each edge
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(CONTRACT)), ids=[s.name for s in CONTRACT])
def test_dw_contract(lib, generic, i):
    _case(lib, generic, CONTRACT[i], 200 + i)


def test_dw_contract_batches_of_mixed_shapes(lib):
    """All tiled contract launches of one key in ONE table: items of different grids (grid x 4 .. 70, one to four channel groups), so the
    blocks beyond an item's own grid must leave at once; with and without g / dab, accumulating or not."""
    runs = []
    for i, s in enumerate(CONTRACT):
        if not (s.expect['fwd'][0] or s.expect['bwd'][0]):
            continue
        d = Dw(s, 200 + i)
        _, cb, rows = d.configs(lib)
        q = d.out(rows)
        L.check(lib.addk_dw_fwd(C.byref(d.fwd_args(q)), _st(DEV)), 'dw_fwd')
        L.check(lib.addk_dw_bwd(C.byref(d.bwd_args(q, 1)), _st(DEV)), 'dw_bwd')
        runs.append((d, q, rows))
    assert _batched(lib, runs, False) == 2 and _batched(lib, runs, True) == 2


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. addk_dw_wreduce_batch on its own
# ------------------------------------------------------------------------------------------------------------------------------------
WREDUCE_ROWS = [1, 2, 3, 4, 5, 13, 16, 17, 341, 1024]
WREDUCE_N = [36, 64, 360, 4000, 4100]


def wreduce_data(rows, dev=DEV):
    """The items of one table: ws [rows][n] for every n of WREDUCE_N, accumulate alternating (dw: old finite values or NaN)."""
    gen = _rng(300 + rows)
    items = []
    for j, n in enumerate(WREDUCE_N):
        acc = (j + rows) % 2
        ws = (0.5 + _rand(gen, rows, n)) * torch.where(_rand(gen, rows, n) < 0.5, -1.0, 1.0)      # magnitudes in [0.5, 1.5): no term near 0
        items.append((n, acc, ws.to(dev), _randn(gen, n).to(dev)))
    return items


def wreduce_bound(rows, ws, old):
    """A thread adds at most ceil(rows / 4) rows (four accumulators of every fourth of them: the chain is shorter still), two adds join
    the accumulators, two the row groups, one the old value: (ceil(rows / 4) + 4 + 2) ULP (sum |ws| + |old|)."""
    S = ws.double().abs().sum(0)
    if old is not None:
        S = S + old.double().abs()
    return (_cdiv(rows, 4) + 4 + 2) * ULP * S


@pytest.mark.parametrize('rows', WREDUCE_ROWS)
def test_dw_wreduce_batch_against_fp64_column_sums(lib, rows):
    """rows around the 16-row unroll and its 4-row tail, n up to 4100 (a second pass of the 64-block grid, its last block partly
    full), five items of mixed accumulate in one table.  The wave-per-element dw_wreduce_kernel has no entry point of its own: every
    `wave-reduced` line of the depthwise cases above holds it to the same fp64 sums."""
    items = wreduce_data(rows)
    outs = [old.clone() if acc else _nan(DEV, n) for n, acc, _, old in items]
    tab = _table([_wreduce_item(ws, o, rows, n, acc) for (n, acc, ws, _), o in zip(items, outs)], DEV)
    L.check(lib.addk_dw_wreduce_batch(tab.data_ptr(), len(items), _st(DEV)), 'dw_wreduce_batch')
    for (n, acc, ws, old), o in zip(items, outs):
        ref = ws.double().sum(0) + (old.double() if acc else 0.0)
        bound = wreduce_bound(rows, ws, old if acc else None)
        assert bool((bound < ws.abs().double().median(0).values).all())
        _close('wred', 'dw_wreduce_batch rows=%d n=%d accumulate=%d' % (rows, n, acc), o, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. 3x3 pooling
# ------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 7, 9, 5), (1, 16, 17, 40), (1, 1, 3, 8)]


class Pool:
    def __init__(self, N, H, W, Cc, stride, mode, lazy, relu, ties=False, seed=0, dev=DEV):
        self.N, self.H, self.W, self.C, self.stride, self.mode, self.relu, self.dev = N, H, W, Cc, stride, mode, relu, dev
        self.OH, self.OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        P, Po = N * H * W, N * self.OH * self.OW
        gen = _rng(seed)
        x = torch.randint(-1, 2, (P, Cc), generator=gen).float() if ties else _randn(gen, P, Cc)
        a = (0.5 + _rand(gen, Cc)) * torch.where(_rand(gen, Cc) < 0.5, -1.0, 1.0) if lazy else None
        b = 0.3 * _randn(gen, Cc) if lazy else None
        dy, gold = _randn(gen, Po, Cc), _randn(gen, P, Cc + 1)
        if relu:
            x, _ = _clear_of_zero(x, a, b)
        self.xb, self.dyb, self.gold = _nan(dev, P, Cc + 3), _nan(dev, Po, Cc + 2), gold.to(dev)
        self.x, self.dy = self.xb[:, :Cc], self.dyb[:, :Cc]
        self.x.copy_(x)
        self.dy.copy_(dy)
        self.a, self.b = (a.to(dev), b.to(dev)) if lazy else (None, None)
        self.P, self.Po = P, Po

    def src(self):
        sr = L.Src()
        sr.x, sr.a, sr.b, sr.ld, sr.C, sr.relu, sr.rs_hw = self.x.data_ptr(), _p(self.a), _p(self.b), self.C + 3, self.C, int(self.relu), 0
        return sr

    def nchw(self, t, H, W):
        return t.double().reshape(self.N, H, W, self.C).permute(0, 3, 1, 2).contiguous()

    def nhwc(self, t):
        return t.permute(0, 2, 3, 1).reshape(-1, self.C)

    def pool(self, v):
        if self.mode == 0:
            return F.max_pool2d(v, 3, self.stride, 1)
        return F.avg_pool2d(v, 3, self.stride, 1, count_include_pad=False)

    def reference(self):
        """F.max_pool2d / F.avg_pool2d in fp64 on the lazily transformed input, and their autograd (with dy, and with |dy| for the
        magnitudes routed to an element)."""
        x = self.nchw(self.x, self.H, self.W)
        if self.a is not None:
            av, bv = self.a.double().view(1, -1, 1, 1), self.b.double().view(1, -1, 1, 1)
            pre = av * x + bv
        else:
            av, pre = 1.0, x
        m = pre > 0 if self.relu else torch.ones_like(pre, dtype=torch.bool)
        v = torch.where(m, pre, torch.zeros_like(pre)).requires_grad_(True)
        out = self.pool(v)
        assert out.shape[2:] == (self.OH, self.OW)
        dy = self.nchw(self.dy, self.OH, self.OW)
        gv, = torch.autograd.grad(out, v, dy, retain_graph=True)
        gs, = torch.autograd.grad(out, v, dy.abs())
        R = Out()
        R.y = self.nhwc(out.detach())
        va = v.detach().abs()
        # max: the one rounding of the affine, of the window's largest magnitude; average: 11 ulps of sum |v| / cnt
        R.ybound = self.nhwc(U * F.max_pool2d(va, 3, self.stride, 1) if self.mode == 0 else 11 * ULP * self.pool(va))
        R.g, R.Sg = self.nhwc(gv * m * av), self.nhwc(gs * m * (av.abs() if self.a is not None else 1.0))
        return R


def _pool_run(lib, p, acc, tag):
    R = p.reference()
    st, Cc = _st(p.dev), p.C
    yb = _nan(p.dev, p.Po, Cc + 5)
    L.check(lib.addk_pool3_fwd(C.byref(p.src()), p.N, p.H, p.W, p.OH, p.OW, p.stride, p.mode, yb.data_ptr(), Cc + 5, st), 'pool3_fwd')
    _close('pool', tag + ' y', yb[:, :Cc], R.y, R.ybound)
    _all_nan(tag + ': y padding channels', yb[:, Cc:])
    gb = p.gold.clone() if acc else _nan(p.dev, p.P, Cc + 1)
    L.check(lib.addk_pool3_bwd(C.byref(p.src()), p.N, p.H, p.W, p.OH, p.OW, p.stride, p.mode, p.dy.data_ptr(), Cc + 2, gb.data_ptr(), Cc + 1,
                               int(acc), st), 'pool3_bwd')
    ref, Sg = R.g, R.Sg
    if acc:
        old = p.gold[:, :Cc].double()
        ref, Sg = ref + old, Sg + old.abs()
        _same_bits(tag + ': g padding channel', gb[:, Cc:], p.gold[:, Cc:])
    else:
        _all_nan(tag + ': g padding channel', gb[:, Cc:])
    # up to 9 windows added one after the other (the average divides each first), one multiply by a, one add of the old value
    _close('pool', tag + ' g', gb[:, :Cc], ref, (9 + 3) * ULP * Sg)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=['x'.join(map(str, s)) for s in POOL_SHAPES])
def test_pool3_against_fp64_pooling_and_autograd(lib, shape, stride):
    """Max and average, with and without the lazy a / b / ReLU, accumulate 0 and 1; every buffer with a padded row (ld = C + 3,
    ldy = C + 5, lddy = C + 2, ldg = C + 1).  With the ReLU half of the values tie at 0: the first of a window wins in both."""
    for mode in (0, 1):
        for lazy, relu in ((False, 0), (True, 0), (True, 1), (False, 1)):
            for acc in (0, 1):
                p = Pool(*shape, stride, mode, lazy, relu, seed=400 + 2 * mode + acc)
                _pool_run(lib, p, acc, 'pool3 %s %s stride=%d lazy=%d relu=%d acc=%d' % ('avg' if mode else 'max', 'x'.join(map(str, shape)),
                                                                                         stride, lazy, relu, acc))


@pytest.mark.parametrize('stride', [1, 2])
def test_pool3_max_ties_route_to_the_first_maximum(lib, stride):
    """Inputs from {-1, 0, 1}: ties in every window; the gradient lands on the first maximum in window scan order, as in ATen."""
    for shape in POOL_SHAPES:
        p = Pool(*shape, stride, 0, False, 0, ties=True, seed=450)
        _pool_run(lib, p, 0, 'pool3 max ties %s stride=%d' % ('x'.join(map(str, shape)), stride))


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, what):
    msg = lib.addk_last_error().decode()
    assert rc != 0 and msg, '%s: accepted (code %d, message %r)' % (what, rc, msg)
    _log('refusal %-40s code %d: %s', what, rc, msg)


def test_dw_and_pool3_refusals(lib):
    """Arguments outside the contract return a non-zero code with a message and launch nothing: every output still holds NaN.  The
    buffers are large enough for the launch that must not happen."""
    st = _st(DEV)

    def attempt(what, s, fwd=True, bwd=True, k2=None, edit=None):
        d = Dw(s, 500)
        rows = int(lib.addk_dw_rows(d.P, min(s.C, 1024)))
        o = d.out(rows)
        for run, fn, ar in ((fwd, lib.addk_dw_fwd, d.fwd_args(o)), (bwd, lib.addk_dw_bwd, d.bwd_args(o, 0))):
            if not run:
                continue
            if k2:
                ar.KH = ar.KW = k2
            if edit:
                edit(ar)
            _refused(lib, fn(C.byref(ar), st), what)
        torch.cuda.synchronize()
        for name, t in (('y', o.yb), ('g', o.gb), ('dab', o.dab), ('ws', o.ws), ('dw', o.dw)):
            _all_nan('%s: %s' % (what, name), t)

    # the data are those of a 5x5 (the largest window built), so a launch that must not happen would stay inside its buffers
    attempt('KH * KW = 36 > 25', S('r', 1, 8, 8, 8, 5), k2=6)
    attempt('C = 1028 > 1024', S('r', 1, 4, 4, 1028, 3))

    def short_ldy(ar):
        if isinstance(ar, L.DwArgs):
            ar.ldy = 36
        else:
            ar.lddy = 36
    attempt('ldy / lddy < C', S('r', 1, 8, 8, 40, 3), edit=short_ldy)

    def short_ldg(ar):
        ar.ldg = 36
    attempt('ldg < C', S('r', 1, 8, 8, 40, 3), fwd=False, edit=short_ldg)

    def a_without_b(ar):
        ar.src.b = None
    attempt('a without b', S('r', 1, 8, 8, 40, 3), edit=a_without_b)
    attempt('backward with 16 taps', S('r', 1, 8, 8, 8, 5), fwd=False, k2=4)
    attempt('backward with 4 taps', S('r', 1, 8, 8, 8, 5), fwd=False, k2=2)
    p = Pool(2, 7, 9, 5, 1, 0, True, 1, seed=501)
    yb, gb = _nan(DEV, p.Po, p.C), _nan(DEV, p.P, p.C)
    _refused(lib, lib.addk_pool3_fwd(C.byref(p.src()), p.N, p.H, p.W, p.OH, p.OW, 1, 2, yb.data_ptr(), p.C, st), 'pool3_fwd mode 2')
    _refused(lib, lib.addk_pool3_bwd(C.byref(p.src()), p.N, p.H, p.W, p.OH, p.OW, 1, 2, p.dy.data_ptr(), p.C + 2, gb.data_ptr(), p.C, 0, st),
             'pool3_bwd mode 2')
    _refused(lib, lib.addk_pool3_fwd(C.byref(p.src()), p.N, p.H, p.W, p.OH, p.OW, 1, 0, yb.data_ptr(), p.C - 1, st), 'pool3_fwd ldy < C')
    torch.cuda.synchronize()
    _all_nan('pool3 refusals: y', yb)
    _all_nan('pool3 refusals: g', gb)
