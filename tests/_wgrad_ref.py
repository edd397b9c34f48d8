"""fp64 reference of the dense weight gradient as include/addk.h defines it (addk_conv_wgrad_args), and what the tests around it share:

    dw[co][tap*cin_total + w_choff + ci] = sum_{n,oy,ox} dy[n,oy,ox,co] * z[n, oy*s - pad + ky*d, ox*s - pad + kx*d, ci]

with z = relu?(a*x + b) inside the map and exactly 0 in the padding (the padding comes AFTER the affine).  The sum is evaluated with torch
in float64 on the CPU as unfold + matmul, so it depends neither on the GPU's fp64 convolution nor on autograd.

Also here: the cases (tests/tools/make_wgrad_bits.CASES: the lone launches) and the mixed batches of tests/test_gpu_wgrad_fp64.py with
their pinned launch keys (tests/test_wgrad_dispatch.py pins them without a GPU), the seeded inputs, the ConvWgradArgs builder and the
guard-band allocator."""
import importlib.util
import math
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location('make_wgrad_bits', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'make_wgrad_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)
CASES, MODES, geometry = bits.CASES, bits.MODES, bits.geometry

TOL = 2e-5          # tests/test_gpu_fast_kernels.py: all three arithmetics, weight gradients summed over up to 65536 pixels
ALL_MODES = dict(MODES, tail_x3=3)
FAST_ALL = bits.FAST_ALL
# the source forms: (a, b present, relu)
FORMS = ((True, 1), (True, 0), (False, 1), (False, 0))
FORM_NAMES = ('ab_relu', 'ab', 'relu', 'plain')
GUARD = 4096        # floats on either side of an output buffer
GUARD_BITS = 0x7fc5a5a5        # a quiet NaN with a payload nothing computes
FIRST_TOUCH_BITS = 0x7fc1e1e1  # what a first-touch dw and every workspace hold before the launch

# One weight gradient of a test: the conv, its strides, the slice of the wider weight it writes, its source form, and the seed of its inputs.
Op = namedtuple('Op', 'N H W C Cout k stride dil pad OH OW ld lddy w_choff cin_total ldw form accumulate seed')


def make_op(shape, seed, ld=None, lddy=None, form=0, accumulate=0, w_choff=8):
    """shape = (N, H, W, Cin, Cout, k, stride, dil), pad = dil * (k // 2).  The gradient is a slice of a wider weight: columns
    w_choff .. w_choff + C of cin_total = C + 12 per tap, and four more floats of row padding."""
    N, H, W, Ci, Cout, k, s, d = shape
    pad = d * (k // 2)
    OH, OW = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
    cin_total = Ci + 12
    return Op(N, H, W, Ci, Cout, k, s, d, pad, OH, OW, ld or Ci, lddy or Cout, w_choff, cin_total, k * k * cin_total + 4, form, accumulate, seed)


def case_op(case, form=0, accumulate=0):
    """The lone launch of a case of make_wgrad_bits.CASES, with the case's padded or unpadded strides and its seed."""
    g = geometry(case)
    return make_op(case[1], case[4], g[11], g[12], form, accumulate)


# The mixed batches: name, fast-path mask, {mode: (kind, cty, ctz)}, member shapes (N, H, W, Cin, Cout, k, stride, dil).
# Under one key the members differ in pixel count, channel counts, dilation, stride and (kinds 0-3, 6) tap count; rs33, os2 and pix33 have
# n >= 4 (min_steps = 8, the smaller budget); the last member of rs33 has 9 pixel slices at px_chunk = 2048 (a partial last XCD group);
# h3_41, h3_8x, hk33, hk35 and os2 mix the wave and the block reduction; pix33's last two members take the scalar-load path (vecY = vecZ = 0).
_K3 = lambda key, split=None: {'fp32': key, 'f16x3': split or key, 'bf16x6': split or key}
BATCHES = [
    ('rs33',  FAST_ALL, _K3((6, 3, 3)), [(1, 33, 125, 40, 40, 1, 1, 1), (2, 97, 129, 48, 96, 3, 2, 1), (2, 91, 93, 80, 40, 1, 2, 1), (1, 130, 140, 40, 40, 1, 1, 1)]),
    ('rs44',  FAST_ALL, _K3((6, 4, 4)), [(1, 33, 125, 64, 64, 1, 1, 1), (1, 64, 66, 56, 64, 1, 1, 1)]),
    ('rs34',  FAST_ALL, _K3((6, 3, 4)), [(1, 33, 125, 64, 40, 1, 1, 1), (1, 64, 66, 56, 80, 1, 1, 1)]),
    ('rs43',  FAST_ALL, _K3((6, 4, 3)), [(1, 33, 125, 40, 64, 1, 1, 1), (1, 64, 66, 80, 56, 1, 1, 1)]),
    ('h3_41', FAST_ALL, _K3((5, 4, 1)), [(2, 33, 129, 24, 64, 3, 1, 2), (1, 65, 130, 48, 64, 3, 1, 1), (1, 64, 128, 16, 64, 3, 1, 18)]),
    ('h3_81', FAST_ALL, _K3((5, 8, 1)), [(1, 40, 256, 16, 128, 3, 1, 1), (1, 70, 128, 48, 256, 3, 1, 6)]),
    ('h3_8x', FAST_ALL, _K3((5, 8, 1), (5, 8, 2)), [(1, 40, 256, 32, 128, 3, 1, 1), (1, 70, 128, 64, 256, 3, 1, 6)]),
    ('h3_42', FAST_ALL, _K3((5, 4, 1), (5, 4, 2)), [(1, 65, 130, 32, 64, 3, 1, 1), (2, 33, 129, 64, 64, 3, 1, 2)]),
    ('hk33',  FAST_ALL, _K3((7, 3, 3)), [(1, 70, 125, 40, 40, 3, 1, 2), (1, 64, 66, 32, 48, 3, 1, 1)]),
    ('hk35',  FAST_ALL, _K3((7, 3, 5)), [(1, 70, 125, 40, 40, 5, 1, 2), (2, 32, 64, 48, 160, 5, 1, 2)]),
    ('hk53',  FAST_ALL, _K3((7, 5, 3)), [(2, 40, 104, 32, 160, 3, 1, 2), (1, 70, 125, 80, 80, 3, 1, 2)]),
    ('os1',   FAST_ALL, _K3((1, 8, 4)), [(1, 16, 32, 64, 128, 1, 1, 1), (1, 20, 24, 48, 256, 3, 1, 1)]),
    ('os2',   FAST_ALL, _K3((2, 6, 6)), [(2, 16, 32, 80, 80, 1, 1, 1), (1, 30, 40, 96, 96, 1, 1, 1), (1, 31, 33, 72, 88, 3, 2, 1), (2, 16, 32, 80, 80, 1, 1, 1)]),
    ('os3',   FAST_ALL, _K3((3, 4, 4)), [(2, 16, 32, 64, 64, 1, 1, 1), (1, 21, 23, 52, 60, 3, 1, 1)]),
    ('pix33', 0,        _K3((0, 3, 3)), [(1, 70, 125, 40, 40, 3, 1, 2), (1, 33, 65, 40, 36, 1, 1, 1), (1, 20, 30, 37, 39, 3, 2, 1), (1, 17, 19, 35, 41, 5, 1, 1)]),
    ('pix21', FAST_ALL, _K3((0, 2, 1)), [(1, 9, 11, 20, 24, 3, 1, 1), (1, 7, 9, 10, 30, 1, 1, 1)]),
    ('h1',    FAST_ALL, {'f16x3': (9, 8, 4), 'bf16x6': (9, 8, 4)}, [(1, 70, 130, 200, 128, 1, 1, 1), (2, 64, 64, 64, 256, 1, 1, 1)]),
    ('st',    FAST_ALL, _K3((8, 4, 2)), [(2, 256, 511, 3, 64, 3, 2, 1), (1, 513, 515, 3, 32, 3, 2, 1)]),
]


def batch_ops(batch):
    """The members of a batch as the GPU test launches them: member i has source form i mod 4, accumulate = i mod 2, padded strides
    (ld = C + 8, lddy = Cout + 4) when i is odd; a member whose channel count is no multiple of 4 gets an odd ld and an odd w_choff instead."""
    bi = [b[0] for b in BATCHES].index(batch[0])
    ops = []
    for i, shape in enumerate(batch[3]):
        Ci, Cout = shape[3], shape[4]
        seed = 1000 + 16 * bi + i
        if Ci % 4:
            ops.append(make_op(shape, seed, (Ci + 2) | 1, Cout, i % 4, i % 2, w_choff=9))
        else:
            ops.append(make_op(shape, seed, Ci + 8 if i % 2 else Ci, Cout + 4 if i % 2 else Cout, i % 4, i % 2))
    return ops


_INPUTS = OrderedDict()


def make_inputs(op):
    """(x, a, b, dy, dw0) as float32 numpy arrays, the distributions of make_wgrad_bits.make_inputs: x and dy carry their row strides (the
    padded columns hold random values of the data's magnitude), dw0 is the whole [Cout][ldw] weight an accumulating launch starts from,
    scaled by sqrt(P): the gradient's own magnitude.  Shared between the forms and modes of an op and never modified."""
    key = (op.N, op.H, op.W, op.C, op.Cout, op.k, op.stride, op.dil, op.ld, op.lddy, op.ldw, op.seed)
    if key not in _INPUTS:
        while len(_INPUTS) >= 6:
            _INPUTS.popitem(last=False)
        rs = np.random.RandomState(op.seed)
        f = lambda scale, *sh: (scale * rs.standard_normal(sh)).astype(np.float32)
        P = op.N * op.OH * op.OW
        _INPUTS[key] = (f(1.0, op.N * op.H * op.W, op.ld), (1.0 + 0.25 * rs.standard_normal(op.C)).astype(np.float32), f(0.3, op.C),
                        f(1.0, P, op.lddy), f(math.sqrt(P), op.Cout, op.ldw))
        for v in _INPUTS[key]:
            v.setflags(write=False)
    return _INPUTS[key]


_t64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64))      # a contiguous float64 copy


def activation(op, x, a, b, aff, relu):
    """z = relu?(a*x + b) of the map as [N, C, H, W] float64 (no padding yet)"""
    z = _t64(x[:, :op.C]).view(op.N, op.H, op.W, op.C)
    if aff:
        z = _t64(a) * z + _t64(b)
    if relu:
        z = F.relu(z)
    return z.permute(0, 3, 1, 2)


def grad_fp64(op, x, a, b, dy, aff, relu, drop_last=False, affine_on_padding=False):
    """The gradient [Cout][taps][C] in float64.  The two flags are the deliberate mistakes of tests/test_wgrad_ref.py: the last output pixel
    of the last image left out; the affine (and ReLU) applied to the zero padding too, instead of padding after them."""
    if affine_on_padding:
        xp = F.pad(_t64(x[:, :op.C]).view(op.N, op.H, op.W, op.C), (0, 0, op.pad, op.pad, op.pad, op.pad))
        big = op._replace(H=op.H + 2 * op.pad, W=op.W + 2 * op.pad)
        z, pad = activation(big, xp.reshape(-1, op.C).numpy(), a, b, aff, relu), 0
    else:
        z, pad = activation(op, x, a, b, aff, relu), op.pad
    cols = F.unfold(z, op.k, dilation=op.dil, padding=pad, stride=op.stride)               # [N][C * taps][OH * OW], rows ordered (c, ky, kx)
    g = _t64(dy[:, :op.Cout]).view(op.N, op.OH * op.OW, op.Cout)
    if drop_last:
        g = g.clone()
        g[-1, -1] = 0
    dw = g.reshape(-1, op.Cout).t() @ cols.permute(0, 2, 1).reshape(-1, cols.shape[1])      # [Cout][C * taps]
    return dw.view(op.Cout, op.C, op.k * op.k).permute(0, 2, 1).contiguous()


_REF = {}


def reference(op):
    """grad_fp64 of an op's seeded inputs in its source form, cached per (shape, strides, seed, form); read-only"""
    key = (op.N, op.H, op.W, op.C, op.Cout, op.k, op.stride, op.dil, op.ld, op.lddy, op.seed, op.form)
    if key not in _REF:
        x, a, b, dy, _ = make_inputs(op)
        _REF[key] = grad_fp64(op, x, a, b, dy, *FORMS[op.form]).numpy()
        _REF[key].setflags(write=False)
    return _REF[key]


def slice_mask(op):
    """bool [Cout][ldw]: the elements of the wider weight this op writes"""
    m = np.zeros((op.Cout, op.ldw), dtype=bool)
    for t in range(op.k * op.k):
        m[:, t * op.cin_total + op.w_choff: t * op.cin_total + op.w_choff + op.C] = True
    return m


def expected(op, grad, dw_init, accumulate=None, w_choff=None):
    """The whole [Cout][ldw] weight after the launch, float64: dw_init outside the slice, grad (accumulate: dw_init + grad) inside"""
    accumulate = op.accumulate if accumulate is None else accumulate
    w_choff = op.w_choff if w_choff is None else w_choff
    out = np.array(dw_init, dtype=np.float64)
    for t in range(op.k * op.k):
        c0 = t * op.cin_total + w_choff
        out[:, c0:c0 + op.C] = grad[:, t] + (out[:, c0:c0 + op.C] if accumulate else 0.0)
    return out


def rel_err(got, ref):
    """the project's error measure: max|got - ref| / max|ref|"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def wgrad_args(L, op, ptr, ws_floats=0):
    """ConvWgradArgs of an op; `ptr` maps dy, x, a, b, dw, ws to addresses.  a and b are passed only in the forms that have them."""
    aff, relu = FORMS[op.form]
    wa = L.ConvWgradArgs()
    wa.dy, wa.lddy, wa.Cout = ptr['dy'], op.lddy, op.Cout
    wa.N, wa.H, wa.W, wa.OH, wa.OW, wa.KH, wa.KW, wa.stride, wa.pad, wa.dil = op.N, op.H, op.W, op.OH, op.OW, op.k, op.k, op.stride, op.pad, op.dil
    wa.src.x, wa.src.a, wa.src.b = ptr['x'], ptr['a'] if aff else None, ptr['b'] if aff else None
    wa.src.ld, wa.src.C, wa.src.relu = op.ld, op.C, relu
    wa.dw, wa.ldw, wa.cin_total, wa.w_choff, wa.accumulate = ptr['dw'], op.ldw, op.cin_total, op.w_choff, op.accumulate
    wa.ws, wa.ws_floats = ptr.get('ws'), ws_floats
    return wa


class Guarded:
    """`n` floats carved out of a larger buffer with GUARD floats on both sides that hold a NaN of known payload.  `data` is the float32
    view a launch gets; intact() tells whether every guard word still has its bits."""

    def __init__(self, n, device='cpu', guard=GUARD):
        self.n, self.guard = int(n), guard
        self.raw = torch.full((self.n + 2 * guard,), GUARD_BITS, dtype=torch.int32, device=device)
        self.data = self.raw[guard:guard + self.n].view(torch.float32)

    def fill_bits(self, word):
        self.raw[self.guard:self.guard + self.n] = word
        return self

    def intact(self):
        g = self.guard
        return bool((self.raw[:g] == GUARD_BITS).all()) and bool((self.raw[g + self.n:] == GUARD_BITS).all())
