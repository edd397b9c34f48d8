"""fp64 reference of the fused SepConv half as include/addk.h defines it (addk_sep_args, addk_sep_bwd_args), the case list that reaches the
twelve instantiated variants of csrc/sep.h in both directions, and what the tests around them share.

Forward, with z = relu?(a*x + b) inside the map and exactly 0 in the padding (the padding comes AFTER the affine):

    t[n,h,w,c] = sum_{ky,kx} dw_w[c][ky*K + kx] * z[n, h + ky - K/2, w + kx - K/2, c]
    y[p,co]    = sum_c pw_w[co*ldw + c] * t[p,c]                stats[co] = (sum_p y, sum_p y^2)
    finalize   : mean = sum/P, var = sumsq/P - mean^2, invstd = 1/sqrt(var + eps), a = gamma*invstd, b = beta - mean*a,
                 running_mean = (1 - m) rm + m mean, running_var = (1 - m) rv + m var P/(P - 1)
    inference  : y' = ea*y + eb + sum_i relu_i?(a_i*term_i + b_i)        (ea == NULL: y' = y + sum)

Backward, of y with respect to x, (a, b) and dw_w for a given dy:

    dt = dy pw_w,   dz = the transposed depthwise convolution of dt,   m = relu ? (a*x + b > 0) : 1     (a = 1, b = 0 without an affine)
    g (+)= a*m*dz,   dA[c] = sum_p m*dz*x,   dB[c] = sum_p m*dz,   dW_dw[c][tap] = sum_p dt[p] z[p + tap]

The forward is torch's conv2d in float64 on the CPU, the backward float64 autograd of it; backward_taps evaluates the same formulae tap by tap
without autograd and carries the deliberate mistakes of tests/test_sep_ref.py, which also compares everything with explicit Python loops.
Guarded, GUARD_BITS, FIRST_TOUCH_BITS, SLAB_BITS, rel_err and TOL are those of tests/_wgrad_ref.py and tests/_conv_ref.py."""
import ctypes as C
import os
import re
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from _wgrad_ref import FIRST_TOUCH_BITS, FORM_NAMES, FORMS, GUARD_BITS, Guarded, TOL, rel_err  # noqa: F401  (re-exported)
from _conv_ref import SLAB_BITS  # noqa: F401

FAST_ALL = 31
MOMENTUM, EPS = 0.1, 1e-5
XOFF = WOFF = 8                  # x starts at channel 8 of its rows, pw_w at column 8 of its rows
KP = {36: 40, 40: 40, 44: 56, 48: 56, 68: 72, 72: 72, 76: 88, 80: 88}      # the padded pixel stride in LDS: each met at C = KP - 4 or - 12 and at its upper end
SHAPE_R1, SHAPE_R2 = (2, 13, 37), (4, 19, 507)
SHAPE_R2_OTHER = (4, 9, 771)     # 392 two-row blocks: the second tile row holds 1 of 8 rows, the last tile column 3 of 16 pixels
TINY, SMALL = (1, 1, 1), (3, 5, 16)
# the inference epilogues: (nterm, ea present); term i of epilogue j is in source form (i + j) % 4, so term 0 (staged through LDS) meets the forms
# relu, plain, ab_relu, ab and the later terms (read from global memory) ab_relu; ab, relu; relu, plain, ab_relu
EPILOGUES = ((0, False), (0, True), (1, True), (2, False), (3, True), (4, True))

# One launch: the map, the channels, the kernel size, the seed of its inputs and `wide`, which is added to every row stride
Op = namedtuple('Op', 'N H W C K seed wide')
# A case: the variant (ks, kg, kp, r) it names and its launch
Case = namedtuple('Case', 'variant op')


def make_op(shape, C, K, member=0, wide=0):
    N, H, W = shape
    return Op(N, H, W, C, K, 100000 * member + 1000 * K + 10 * C + (N * H * W) % 7, wide)


def _cases():
    out = []
    for K in (3, 5):
        for r, shape, chans in ((1, SHAPE_R1, (36, 40, 44, 48, 68, 72, 76, 80)), (2, SHAPE_R2, (36, 40, 44, 48))):
            out += [Case((K, (Cc + 15) // 16, KP[Cc], r), make_op(shape, Cc, K)) for Cc in chans]
    return out


CASES = _cases()


def case_id(c):
    return 'k%d_g%d_p%d_r%d-c%d-%dx%dx%d' % (c.variant + (c.op.C, c.op.N, c.op.H, c.op.W))


def batch_members(c):
    """the three members of a case's batch: R = 1: the case, 3 x 5 x 16 and 1 x 1 x 1; R = 2: the case, the case's shape again with another seed and wider
    strides, and a second shape of at least 384 two-row blocks"""
    Cc, K = c.op.C, c.op.K
    if c.variant[3] == 1:
        return [c.op, make_op(SMALL, Cc, K, 1), make_op(TINY, Cc, K, 2)]
    return [c.op, make_op(SHAPE_R2, Cc, K, 1, wide=8), make_op(SHAPE_R2_OTHER, Cc, K, 2)]


def built_variants():
    """the (KS, KG, KP, R) of ADDK_SEP_VARIANTS, parsed from csrc/sep.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'auto-dynamic-deeplab_amd', 'csrc', 'sep.h')
    with open(path) as f:
        text = f.read()
    body = re.search(r'#define ADDK_SEP_VARIANTS\(X\)((?:.*\\\n)*.*)\n', text).group(1)
    return [tuple(map(int, m)) for m in re.findall(r'X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)', body)]


def pixels(op):
    return op.N * op.H * op.W


def ld(op, what):
    """row strides in floats: x, pw_w, y, dy and g are slices of rows of C + 12, t of C + 8, the statistics slab of C + 4 channels"""
    return op.C + {'x': 12, 'w': 12, 'y': 12, 't': 8, 'dy': 12, 'g': 12, 'stats': 4}[what] + op.wide


def term_ld(op, i):
    return op.C + 4 * i + 4 + op.wide


def term_forms(j):
    return [(i + j) % 4 for i in range(EPILOGUES[j][0])]


# ---------------------------------------------------------------------------------------------------------------- arguments

PTR = {'x': 0x10000000, 'a': 0x11000000, 'b': 0x11001000, 'dw_w': 0x20000000, 'pw_w': 0x20100000, 'y': 0x30000000, 't': 0x38000000, 'stats': 0x40000000,
       'dy': 0x50000000, 'g': 0x60000000, 'dab': 0x70000000, 'ws': 0x78000000, 'ea': 0x12000000, 'eb': 0x12001000, 'counter': 0x13000000,
       'fin': [0x14000000 + 0x1000 * i for i in range(8)], 'term': [0x80000000 + 0x8000000 * i for i in range(4)],
       'ta': [0x15000000 + 0x1000 * i for i in range(4)], 'tb': [0x16000000 + 0x1000 * i for i in range(4)]}    # 16-byte aligned placeholders for the host-side queries


def _src(s, op, x, a, b, form, row):
    aff, relu = FORMS[form]
    s.x, s.ld, s.C, s.relu = x, row, op.C, relu
    if aff:
        s.a, s.b = a, b


def fwd_args(L, op, ptr, form=0, t=False, stats_rows=0, epilogue=None, fin=False):
    """SepArgs of an op.  `ptr` maps x, a, b, dw_w, pw_w (both at their slice's first element), y, t, stats, ea, eb, term / ta / tb (lists), counter and
    fin (gamma, beta, running_mean, running_var, a, b, mean, invstd) to addresses.  stats_rows > 0: the training form; epilogue = j: EPILOGUES[j]."""
    ar = L.SepArgs()
    _src(ar.src, op, ptr['x'], ptr['a'], ptr['b'], form, ld(op, 'x'))
    ar.N, ar.H, ar.W, ar.K, ar.Cout, ar.ldw = op.N, op.H, op.W, op.K, op.C, ld(op, 'w')
    ar.dw_w, ar.pw_w, ar.y, ar.ldy = ptr['dw_w'], ptr['pw_w'], ptr['y'], ld(op, 'y')
    if t:
        ar.t, ar.ldt = ptr['t'], ld(op, 't')
    if stats_rows:
        ar.stats, ar.stats_ld, ar.stats_rows = ptr['stats'], ld(op, 'stats'), stats_rows
    if epilogue is not None:
        ar.nterm, ea = EPILOGUES[epilogue]
        if ea:
            ar.ea, ar.eb = ptr['ea'], ptr['eb']
        for i, f in enumerate(term_forms(epilogue)):
            _src(ar.term[i], op, ptr['term'][i], ptr['ta'][i], ptr['tb'][i], f, term_ld(op, i))
    if fin:
        fa = ar.fin
        fa.gamma, fa.beta, fa.running_mean, fa.running_var, fa.a, fa.b, fa.mean, fa.invstd = ptr['fin']
        fa.count, fa.momentum, fa.eps = float(pixels(op)), MOMENTUM, EPS
        ar.fin_counter = ptr['counter']
    return ar


def bwd_args(L, op, ptr, form=0, accumulate=0, g=True, dab=True):
    """SepBwdArgs of an op; `ptr` maps dy, x, a, b, dw_w, pw_w, g, dab, ws to addresses"""
    ba = L.SepBwdArgs()
    ba.dy, ba.lddy, ba.N, ba.H, ba.W, ba.K = ptr['dy'], ld(op, 'dy'), op.N, op.H, op.W, op.K
    _src(ba.src, op, ptr['x'], ptr['a'], ptr['b'], form, ld(op, 'x'))
    ba.Cout, ba.ldw, ba.dw_w, ba.pw_w = op.C, ld(op, 'w'), ptr['dw_w'], ptr['pw_w']
    if g:
        ba.g, ba.ldg, ba.accumulate = ptr['g'], ld(op, 'g'), accumulate
    ba.dab, ba.ws = ptr['dab'] if dab else None, ptr['ws']
    return ba


def config(L, lib, args):
    cfg = (C.c_int32 * 8)()
    fn = lib.addk_sep_bwd_config if isinstance(args, L.SepBwdArgs) else lib.addk_sep_fwd_config
    L.check(fn(C.byref(args), cfg), 'sep_config')
    return list(cfg)


# ---------------------------------------------------------------------------------------------------------------- inputs

_INPUTS = OrderedDict()
_t64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64))      # a contiguous float64 copy


def make_inputs(op):
    """float32 numpy arrays, seeded per op, shared by its launches and never modified.  The scales are those of tests/test_gpu_fast_kernels.py
    (a ~ N(0, 1), b ~ 0.3 N, dw_w ~ 0.3 N, pw_w ~ 0.2 N): about half the ReLU masks are off and some a are negative.  x, pw_w, dy, g0 and the terms are
    whole wider buffers (random values of the data's magnitude outside the slice too)."""
    if op not in _INPUTS:
        while len(_INPUTS) >= 3:
            _INPUTS.popitem(last=False)
        rs = np.random.RandomState(op.seed)
        f = lambda scale, *sh: (scale * rs.standard_normal(sh)).astype(np.float32)
        P, Cc = pixels(op), op.C
        d = {'x': f(1.0, P, ld(op, 'x')), 'a': f(1.0, Cc), 'b': f(0.3, Cc), 'dw_w': f(0.3, Cc, op.K * op.K), 'pw_w': f(0.2, Cc, ld(op, 'w')),
             'dy': f(1.0, P, ld(op, 'dy')), 'g0': f(1.0, P, ld(op, 'g')),
             'gamma': (1.0 + 0.2 * rs.standard_normal(Cc)).astype(np.float32), 'beta': f(0.2, Cc), 'rm0': f(0.3, Cc),
             'rv0': (0.5 + rs.random_sample(Cc)).astype(np.float32), 'ea': (1.0 + 0.2 * rs.standard_normal(Cc)).astype(np.float32), 'eb': f(0.2, Cc),
             'term': [f(1.0, P, term_ld(op, i)) for i in range(4)], 'ta': [f(1.0, Cc) for _ in range(4)], 'tb': [f(0.3, Cc) for _ in range(4)]}
        for v in d.values():
            for u in (v if isinstance(v, list) else [v]):
                u.setflags(write=False)
        _INPUTS[op] = d
    return _INPUTS[op]


def x_of(op, inp):
    return inp['x'][:, XOFF:XOFF + op.C]


def pw_of(op, inp):
    return inp['pw_w'][:, WOFF:WOFF + op.C]


# ---------------------------------------------------------------------------------------------------------------- the reference

def _nchw(op, v):
    return v.view(op.N, op.H, op.W, -1).permute(0, 3, 1, 2)


def _flat(v):
    return v.permute(0, 2, 3, 1).reshape(-1, v.shape[1])


def apply_form(x, a, b, form, drop_relu=False):
    """relu?(a*x + b), float64 torch, channels last"""
    aff, relu = FORMS[form]
    z = _t64(x)
    if aff:
        z = _t64(a) * z + _t64(b)
    return F.relu(z) if relu and not drop_relu else z


def forward_fp64(op, inp, form, pad_from_neighbour=False, zero_last_quad=False):
    """(t, y), [P][C] float64 each.  The keyword arguments are deliberate mistakes of tests/test_sep_ref.py: the padding row just above images 1.. holds
    the last row of the image before instead of zeros; the last four channels of t are zero (y is then computed from that t)."""
    p = op.K // 2
    z = F.pad(_nchw(op, apply_form(x_of(op, inp), inp['a'], inp['b'], form)), (p, p, p, p)).contiguous()
    if pad_from_neighbour:
        z[1:, :, p - 1, p:p + op.W] = z[:-1, :, p + op.H - 1, p:p + op.W].clone()
    t = _flat(F.conv2d(z, _t64(inp['dw_w']).view(op.C, 1, op.K, op.K), groups=op.C))
    if zero_last_quad:
        t[:, op.C - 4:] = 0
    y = t @ _t64(pw_of(op, inp)).t()
    return t.numpy(), y.numpy()


def stats_fp64(op, y, skip_last_tile_row_in_sumsq=0):
    """[C][2]: (sum, sum of squares) per channel.  skip_last_tile_row_in_sumsq = r (a mistake): the rows of the last tile row (tiles of 4 r rows) are
    missing from the sum of squares"""
    y4 = y.reshape(op.N, op.H, op.W, -1)
    rows = op.H
    if skip_last_tile_row_in_sumsq:
        rows = (op.H - 1) // (4 * skip_last_tile_row_in_sumsq) * (4 * skip_last_tile_row_in_sumsq)
    return np.stack([y4.sum((0, 1, 2)), (y4[:, :rows] ** 2).sum((0, 1, 2))], 1)


FIN_NAMES = ('a', 'b', 'mean', 'invstd', 'running_mean', 'running_var')


def finalize_fp64(op, inp, y):
    """the six outputs of the fused finalize from y, in FIN_NAMES' order; the unbiased factor P / (P - 1) (1 for a single value) on the running variance"""
    P = y.shape[0]
    s = stats_fp64(op, y)
    mean = s[:, 0] / P
    var = np.maximum(s[:, 1] / P - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + EPS)
    g, be = inp['gamma'].astype(np.float64), inp['beta'].astype(np.float64)
    unb = var * P / (P - 1) if P > 1 else var
    return (g * invstd, be - mean * g * invstd, mean, invstd, (1 - MOMENTUM) * inp['rm0'].astype(np.float64) + MOMENTUM * mean,
            (1 - MOMENTUM) * inp['rv0'].astype(np.float64) + MOMENTUM * unb)


def epilogue_fp64(op, inp, y, j, drop_relu_of=None, ea_on_terms=False):
    """EPILOGUES[j] applied to y.  Mistakes: the ReLU of term `drop_relu_of` left out; ea applied to the terms as well"""
    nterm, ea = EPILOGUES[j]
    s = np.zeros_like(y)
    for i, f in enumerate(term_forms(j)):
        s = s + apply_form(inp['term'][i][:, :op.C], inp['ta'][i], inp['tb'][i], f, drop_relu=(i == drop_relu_of)).numpy()
    if not ea:
        return y + s
    a, b = inp['ea'].astype(np.float64), inp['eb'].astype(np.float64)
    return a * (y + s) + b if ea_on_terms else a * y + b + s


def backward_fp64(op, inp, form):
    """(dx [P][C], dab [C][2], dW_dw [C][K*K]) by float64 autograd of the forward.  Without an affine a = 1 and b = 0 are leaves all the same, so that
    (dA, dB) are the sums of m*dz*x and m*dz; dx is the gradient before any accumulation."""
    aff, relu = FORMS[form]
    Cc, K = op.C, op.K
    x = _nchw(op, _t64(x_of(op, inp))).contiguous().requires_grad_(True)
    a = (_t64(inp['a']) if aff else torch.ones(Cc, dtype=torch.float64)).requires_grad_(True)
    b = (_t64(inp['b']) if aff else torch.zeros(Cc, dtype=torch.float64)).requires_grad_(True)
    w = _t64(inp['dw_w']).view(Cc, 1, K, K).requires_grad_(True)
    z = a.view(1, -1, 1, 1) * x + b.view(1, -1, 1, 1)
    if relu:
        z = F.relu(z)
    y = F.conv2d(F.conv2d(z, w, padding=K // 2, groups=Cc), _t64(pw_of(op, inp)).view(Cc, Cc, 1, 1))
    y.backward(_nchw(op, _t64(inp['dy'][:, :Cc])))
    return _flat(x.grad).numpy(), torch.stack([a.grad, b.grad], 1).numpy(), w.grad.view(Cc, K * K).numpy()


MISTAKES = ('taps_not_flipped', 'mask_from_x', 'pw_not_transposed', 'dA_without_x', 'dw_skips_lane_15')


def backward_taps(op, inp, form, mistake=None):
    """The same three results from the formulae in this module's docstring, tap by tap and without autograd.  `mistake` is one of MISTAKES: the depthwise
    taps not flipped in dz; the ReLU mask taken from x instead of a*x + b; dt = dy pw_w^T; dA without its x factor; the pixels whose column is 15 mod 16
    missing from dW_dw."""
    assert mistake is None or mistake in MISTAKES
    aff, relu = FORMS[form]
    Cc, K, p = op.C, op.K, op.K // 2
    x = _t64(x_of(op, inp))
    a = _t64(inp['a']) if aff else torch.ones(Cc, dtype=torch.float64)
    b = _t64(inp['b']) if aff else torch.zeros(Cc, dtype=torch.float64)
    pre = a * x + b
    m = ((x if mistake == 'mask_from_x' else pre) > 0).double() if relu else torch.ones_like(pre)
    z = _nchw(op, F.relu(pre) if relu else pre)
    pw = _t64(pw_of(op, inp))
    dt = _nchw(op, _t64(inp['dy'][:, :Cc]) @ (pw.t() if mistake == 'pw_not_transposed' else pw))
    w = _t64(inp['dw_w']).view(Cc, K, K)
    dtp = F.pad(dt, (p, p, p, p))
    zp = F.pad(z, (p, p, p, p))
    if mistake == 'dw_skips_lane_15':
        zp = zp.clone()
        zp[:, :, :, p + 15::16] = 0
    dz = torch.zeros_like(dt)
    dW = torch.zeros(Cc, K * K, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            # t[h, w] reads z[h + ky - p, w + kx - p]: z[h, w] feeds t[h - ky + p, w - kx + p]
            fy, fx = (ky, kx) if mistake == 'taps_not_flipped' else (K - 1 - ky, K - 1 - kx)
            dz += w[:, ky, kx].view(1, -1, 1, 1) * dtp[:, :, fy:fy + op.H, fx:fx + op.W]
            dW[:, ky * K + kx] = (dt * zp[:, :, ky:ky + op.H, kx:kx + op.W]).sum((0, 2, 3))
    mdz = m * _flat(dz)
    dab = torch.stack([mdz.sum(0) if mistake == 'dA_without_x' else (mdz * x).sum(0), mdz.sum(0)], 1)
    return (a * mdz).numpy(), dab.numpy(), dW.numpy()


def widen(slice_, init, row, accumulate=0):
    """the whole [P][row] buffer after a launch, float64: init outside the first columns, slice_ (accumulate: init + slice_) inside"""
    out = np.array(init, dtype=np.float64).reshape(-1, row)
    n = slice_.shape[1]
    out[:, :n] = slice_ + (out[:, :n] if accumulate else 0.0)
    return out


_REF = OrderedDict()


def _cached(key, make, keep=16):
    if key not in _REF:
        while len(_REF) >= keep:
            _REF.popitem(last=False)
        v = make()
        for u in v:
            u.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def ref_forward(op, form):
    """(t, y) of an op's seeded inputs in a source form: computed once, shared by the launches of the op, read-only"""
    return _cached(('fwd', op, form), lambda: forward_fp64(op, make_inputs(op), form))


def ref_backward(op, form):
    """(dx, dab, dW_dw) of an op's seeded inputs in a source form: computed once, read-only"""
    return _cached(('bwd', op, form), lambda: backward_fp64(op, make_inputs(op), form))
