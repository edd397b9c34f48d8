"""fp64 reference of the dense convolution's forward and data gradient as include/addk.h defines them (addk_conv_args, addk_conv_dgrad_args),
the case list that reaches every instantiated halo-patch kernel (tests/_conv_cases.py), and what the tests around them share.

Forward, over virtually concatenated sources i with z_i = relu_i?(a_i * x_i + b_i) inside the map and exactly 0 in the padding (the padding
comes AFTER the affine):

    y[n,oy,ox,co] = bias[co] + bias_n[n,co] + sum_{tap,ci} w[co*ldw + tap*cin_total + w_choff + ci] * z[n, oy*s - pad + ky*d, ox*s - pad + kx*d, ci]
    stats[co]     = (sum_p y, sum_p y^2)

Data gradient with respect to ONE source (the destination, whose channels start at its own w_choff inside a tap):

    dz[n,iy,ix,c] = sum_{tap,co} dy[n,oy,ox,co] * w[co*ldw + tap*cin_total + w_choff + c]     over the (oy, ox, tap) that read (iy, ix)
    mask          = relu ? (a*x + b > 0) : 1                   (a = 1, b = 0 without an affine)
    g (+)= a * mask * dz,      dA[c] = sum_p mask * dz * x,      dB[c] = sum_p mask * dz

Both run in float64 on the CPU from the host copies of the inputs: torch's conv2d for the forward, conv_transpose2d (no autograd) for dz;
tests/test_conv_ref.py compares both with explicit tap-by-tap sums.  Guarded, GUARD_BITS, FIRST_TOUCH_BITS, rel_err and TOL are those of
tests/_wgrad_ref.py."""
import ctypes as C
import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from _wgrad_ref import FIRST_TOUCH_BITS, FORM_NAMES, FORMS, GUARD_BITS, Guarded, TOL, rel_err  # noqa: F401  (re-exported)
from _conv_cases import CASES  # noqa: F401

MODES = {'fp32': 0, 'f16x3': 1, 'bf16x6': 2, 'tail_x3': 3}
FAST_ALL = 31
FWD, DGRAD = 0, 1
HALO, SPLIT, SPLIT_S2D, C3N = 6, 7, 8, 9                 # the kinds of addk_conv_*_config that read wpack
BIAS_FORMS = ('nobias', 'bias', 'bias_n')
PTR = {'x': 0x10000000, 'a': 0x11000000, 'b': 0x11001000, 'w': 0x20000000, 'y': 0x30000000, 'stats': 0x40000000, 'dy': 0x50000000, 'g': 0x60000000,
       'dab': 0x70000000, 'wpack': 0x80000000, 'bias': 0x12000000, 'bias_n': 0x12001000}      # 16-byte aligned placeholders: a config call dereferences nothing
WPACK_ANY = 1 << 40
SLAB_BITS = 0x7ff8e1e1       # both words of every double of a statistics / (dA, dB) slab before the launch: a NaN as fp64 and as fp32

# One convolution of a test.  Cs: channels of the sources; the weight is a slice (w_choff .. w_choff + sum(Cs) of cin_total channels per tap, ldw floats
# per row); y, g and the statistics slab are slices of wider rows (ldy, ldg[i] = Cs[i] + 12, stats_ld).
Op = namedtuple('Op', 'N H W Cs Cout k stride dil pad OH OW w_choff cin_total ldw ldy stats_ld seed')
# A case of CASES: the variant (lookup, arguments) and the launch that reaches it.  `direction` is 'fwd' or 'dgrad' (of the only source); `ruled_out`
# names the shape constraints (W, H, K, C: see constraints()) the variant's own gates leave no launch for.
Case = namedtuple('Case', 'lookup args N H W Cs Cout k stride dil direction mode ruled_out')


def case_of(entry):
    lookup, args, (N, H, W), Cs, Cout, k, s, d, direction, mode, ruled = entry
    return Case(lookup, tuple(args), N, H, W, (Cs,) if isinstance(Cs, int) else tuple(Cs), Cout, k, s, d, direction, mode, ruled)


def case_id(c):
    return '%s%s-%s-%dx%dx%d_%s_%d_k%ds%dd%d-%s' % (c.lookup.replace('_variant', ''), ''.join('_%d' % v for v in c.args), c.direction, c.N, c.H, c.W,
                                                     '+'.join(map(str, c.Cs)), c.Cout, c.k, c.stride, c.dil, c.mode)


def make_op(N, H, W, Cs, Cout, k, stride, dil, seed=0, w_choff=8, extra=12):
    """pad = dil * (k // 2) ('same' for stride 1; the stride-2 3x3 pads 1).  The weight is a slice of a wider one: cin_total = sum(Cs) + extra channels
    per tap, four more floats of row padding."""
    pad = dil * (k // 2)
    OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    cin_total = sum(Cs) + extra
    return Op(N, H, W, tuple(Cs), Cout, k, stride, dil, pad, OH, OW, w_choff, cin_total, k * k * cin_total + 4, Cout + 12, Cout + 4, seed)


def case_op(c):
    """the op of a case; the seed leaves the plane count out, so the 2- and 3-plane variants of one shape share inputs and references"""
    key = c.args if c.lookup == 'c3_variant_fp32' else c.args[:-1]
    return make_op(c.N, c.H, c.W, c.Cs, c.Cout, c.k, c.stride, c.dil, seed=sum(map(ord, '%s%s' % (c.lookup, key))) + 7 * c.dil)


def ldg(op, i):
    return op.Cs[i] + 12


def choff(op, i):
    """channel offset of source i inside a tap of the wider weight"""
    return op.w_choff + sum(op.Cs[:i])


# ---------------------------------------------------------------------------------------------------------------- arguments and the choice

def fwd_args(L, op, forms, bias_form, ptr, wpack_floats=WPACK_ANY):
    """ConvArgs of an op; `forms` holds an index into FORMS per source; ptr maps x (a list), a, b (lists), w, y, stats, bias, bias_n, wpack to
    addresses.  a and b are passed only in the forms that have them, bias / bias_n only in their bias form."""
    ar = L.ConvArgs()
    for i, Ci in enumerate(op.Cs):
        aff, relu = FORMS[forms[i]]
        ar.src[i].x, ar.src[i].ld, ar.src[i].C, ar.src[i].relu = ptr['x'][i], Ci, Ci, relu
        if aff:
            ar.src[i].a, ar.src[i].b = ptr['a'][i], ptr['b'][i]
    ar.nsrc = len(op.Cs)
    ar.N, ar.H, ar.W, ar.OH, ar.OW, ar.KH, ar.KW, ar.stride, ar.pad, ar.dil, ar.Cout = op.N, op.H, op.W, op.OH, op.OW, op.k, op.k, op.stride, op.pad, op.dil, op.Cout
    ar.ldw, ar.cin_total, ar.w_choff, ar.ldy = op.ldw, op.cin_total, op.w_choff, op.ldy
    ar.w, ar.y, ar.stats, ar.stats_ld = ptr['w'], ptr['y'], ptr.get('stats'), op.stats_ld
    if bias_form == 1:
        ar.bias = ptr['bias']
    elif bias_form == 2:
        ar.bias_n = ptr['bias_n']
    ar.wpack, ar.wpack_floats = ptr['wpack'], wpack_floats
    return ar


def dgrad_args(L, op, i, form, accumulate, ptr, wpack_floats=WPACK_ANY, dab=True):
    """ConvDgradArgs of the gradient with respect to source i in destination form `form`; ptr maps dy, w, x, a, b (of the destination), g, dab, wpack"""
    aff, relu = FORMS[form]
    da = L.ConvDgradArgs()
    da.dy, da.lddy, da.Cout = ptr['dy'], op.Cout, op.Cout
    da.N, da.H, da.W, da.OH, da.OW, da.KH, da.KW, da.stride, da.pad, da.dil = op.N, op.H, op.W, op.OH, op.OW, op.k, op.k, op.stride, op.pad, op.dil
    da.w, da.ldw, da.cin_total, da.w_choff = ptr['w'], op.ldw, op.cin_total, choff(op, i)
    da.dst.x, da.dst.ld, da.dst.C, da.dst.relu = ptr['x'], op.Cs[i], op.Cs[i], relu
    if aff:
        da.dst.a, da.dst.b = ptr['a'], ptr['b']
    da.g, da.ldg, da.accumulate, da.dab = ptr['g'], ldg(op, i), accumulate, ptr['dab'] if dab else None
    da.wpack, da.wpack_floats = ptr['wpack'], wpack_floats
    return da


def host_ptr(op):
    """placeholder addresses for the host-side config calls"""
    p = dict(PTR)
    p['x'] = [PTR['x'] + 0x100000 * i for i in range(len(op.Cs))]
    p['a'] = [PTR['a'] + 0x400 * i for i in range(len(op.Cs))]
    p['b'] = [PTR['b'] + 0x400 * i for i in range(len(op.Cs))]
    return p


def host_args(L, op, direction, form=0, bias_form=0, i=0):
    """the launch of a case with placeholder pointers and a large enough wpack: for addk_conv_*_config only"""
    p = host_ptr(op)
    if direction == 'fwd':
        return fwd_args(L, op, [form] * len(op.Cs), bias_form, p)
    return dgrad_args(L, op, i, form, 0, dict(p, x=p['x'][i], a=p['a'][i], b=p['b'][i]))


def config(L, lib, args):
    cfg = (C.c_int32 * 8)()
    fn = lib.addk_conv_dgrad_config if isinstance(args, L.ConvDgradArgs) else lib.addk_conv_fwd_config
    L.check(fn(C.byref(args), cfg), 'conv_config')
    return list(cfg)


def planes_of(mode, Cn):
    """conv3.hip c3_planes: fp16 planes (2) in f16x3 and in tail_x3's >= 192-channel launches, bf16 planes (3) otherwise; 0: the exact fp32 kernel"""
    return {'fp32': 0, 'f16x3': 2, 'bf16x6': 3, 'tail_x3': 2 if Cn >= 192 else 3}[mode]


def variant_of(cfg, op, direction, mode, i=0):
    """(lookup, arguments) of the kernel a config answer names for this launch, or ('kind', kind) for a kind without a lookup"""
    kind, v, di = cfg[0], cfg[1:5], FWD if direction == 'fwd' else DGRAD
    np_ = planes_of(mode, op.Cout if direction == 'fwd' else op.Cs[i])
    if kind == HALO:
        return 'c3_variant_fp32', (v[0], v[1], di)
    if kind == SPLIT_S2D:
        return 'c3b_variant_s2d', (v[0],)
    if kind == C3N:
        return 'c3n_variant', (v[0], di, v[1])
    if kind != SPLIT:
        return 'kind', (kind,)
    if v[3] == 2:
        return 'c3b_variant_tr%d' % v[1], (v[0], v[2], di, np_)
    if op.stride == 2:
        return 'c3b_variant_s2f', (v[0], v[2], np_)
    return 'c3b_variant_row', (v[0], v[1], int(op.k == 3 and op.dil > 2), v[2], di, np_)


def variant_planes(lookup, args):
    """bf16 / fp16 planes of a variant (0: fp32)"""
    return 0 if lookup == 'c3_variant_fp32' else args[-1]


def constraints(lookup, args, op, direction):
    """The four properties a case's shape should have, as {letter: holds}:
    W  the tiled width is no multiple of the tile-row width;
    H  (two-row tiles) the second row of the last row pair lies beyond the map: H mod 2 dil in 1 .. dil;
    K  the K side (source channels of the forward, dy channels of the gradient) ends in a chunk of fewer than 16 channels;
    C  the output-side channel count is no multiple of the block's columns."""
    Cn, K = (op.Cout, sum(op.Cs)) if direction == 'fwd' else (op.Cs[0], op.Cout)
    width = op.OW if op.stride == 2 else op.W            # the stride-2 gradient tiles 64 positions of dy per row
    if lookup == 'c3_variant_fp32':
        row, cols, two = 128, 16 * args[0], False
    elif lookup in ('c3b_variant_tr3', 'c3b_variant_tr5'):
        row, cols, two = args[1], 32 * args[0], True
    elif lookup == 'c3b_variant_row':
        row, cols, two = args[3], 32 * args[0], False
    elif lookup == 'c3b_variant_s2f':
        row, cols, two = args[1], 32 * args[0], False
    elif lookup == 'c3b_variant_s2d':
        row, cols, two = 64, 64, False
    else:
        row, cols, two = 128, 48, True
    out = {'W': width % row != 0, 'K': K % 16 != 0, 'C': Cn % cols != 0}
    if two:
        out['H'] = 1 <= op.H % (2 * op.dil) <= op.dil
    return out


def out_channels(c):
    """the output-side channel count of a case: Cout of a forward, the destination's channels of a data gradient"""
    return c.Cout if c.direction == 'fwd' else c.Cs[0]


def first_case(lookup, direction, planes, pred=lambda c: True):
    """the first case of CASES with this lookup, direction and plane count (the odd dilation of a pair), or None"""
    return next((c for c in map(case_of, CASES) if c.lookup == lookup and c.direction == direction and variant_planes(c.lookup, c.args) == planes and pred(c)), None)


# one (forward case, data-gradient case) per pack layout and plane count; the stride-2 forward's counterpart is the stride-2 data gradient
LAYOUTS = [(first_case(f, 'fwd', np_), first_case(d, 'dgrad', np_)) for f, d in (('c3b_variant_row', 'c3b_variant_row'), ('c3b_variant_tr3', 'c3b_variant_tr3'),
           ('c3b_variant_tr5', 'c3b_variant_tr5'), ('c3b_variant_s2f', 'c3b_variant_s2d'), ('c3n_variant', 'c3n_variant')) for np_ in (2, 3)]
LAYOUTS.append((first_case('c3_variant_fp32', 'fwd', 0), first_case('c3_variant_fp32', 'dgrad', 0)))
# tail_x3: one case per kernel family and direction on either side of the 192-channel line where the family has launches there (conv3n and the
# stride-2 data gradient take <= 48 / <= 64 channels only): 2 planes at >= 192 output-side channels, 3 below
TAIL = [c for c in (first_case(lk, di, np_, lambda c: (out_channels(c) >= 192) == (np_ == 2))
                    for lk in ('c3b_variant_row', 'c3b_variant_tr3', 'c3b_variant_tr5', 'c3b_variant_s2f', 'c3b_variant_s2d', 'c3n_variant')
                    for di in ('fwd', 'dgrad') for np_ in (2, 3)) if c is not None]
# the stride-2 forward above the line: no case of the list has >= 192 channels there, so the list's case with 200 output channels (4-wave blocks still)
TAIL.append(first_case('c3b_variant_s2f', 'fwd', 2)._replace(Cout=200))


def three_sources(c):
    """a forward case with three sources of 24 + 16 + 8 channels instead of one: a tail chunk of 8 channels after the first source, a lone chunk of 8"""
    return c._replace(Cs=(24, 16, 8))


def three_destinations(c):
    """a data-gradient case with three sources of the case's channel count instead of one: every source's gradient takes the case's variant (the choice
    follows the destination's channels, the dy channels and the map) and reads its own weight columns, from w_choff = 8, 8 + C and 8 + 2 C"""
    return c._replace(Cs=(c.Cs[0],) * 3)


# ---------------------------------------------------------------------------------------------------------------- inputs

_INPUTS = OrderedDict()
_t64 = lambda v: torch.from_numpy(np.array(v, dtype=np.float64))      # a contiguous float64 copy


def make_inputs(op):
    """float32 numpy arrays, shared between the forms and modes of an op and never modified: x, a, b (lists per source), w (the whole [Cout][ldw] wider
    weight), bias [Cout], bias_n [N][Cout], dy [N*OH*OW][Cout], g0 (per source, [N*H*W][ldg]: what an accumulating gradient starts from, of the
    gradient's own magnitude)."""
    if op not in _INPUTS:
        while len(_INPUTS) >= 4:
            _INPUTS.popitem(last=False)
        rs = np.random.RandomState(op.seed)
        f = lambda scale, *sh: (scale * rs.standard_normal(sh)).astype(np.float32)
        Pin, Pout = op.N * op.H * op.W, op.N * op.OH * op.OW
        gs = 0.1 * math.sqrt(op.k * op.k * op.Cout)
        d = {'x': [f(1.0, Pin, Ci) for Ci in op.Cs], 'a': [(1.0 + 0.25 * rs.standard_normal(Ci)).astype(np.float32) for Ci in op.Cs],
             'b': [f(0.3, Ci) for Ci in op.Cs], 'w': f(0.1, op.Cout, op.ldw), 'bias': f(1.0, op.Cout), 'bias_n': f(1.0, op.N, op.Cout),
             'dy': f(1.0, Pout, op.Cout), 'g0': [f(gs, Pin, ldg(op, i)) for i in range(len(op.Cs))]}
        for v in d.values():
            for u in (v if isinstance(v, list) else [v]):
                u.setflags(write=False)
        _INPUTS[op] = d
    return _INPUTS[op]


# ---------------------------------------------------------------------------------------------------------------- the reference

def weight_fp64(op, w, c0, Cn):
    """[Cout][Cn][k][k] float64: channels c0 .. c0 + Cn of every tap of the wider weight"""
    taps = op.k * op.k
    wt = _t64(w[:, :taps * op.cin_total]).view(op.Cout, taps, op.cin_total)[:, :, c0:c0 + Cn]
    return wt.permute(0, 2, 1).reshape(op.Cout, Cn, op.k, op.k).contiguous()


def activation(op, x, a, b, form, affine_on_padding=False):
    """z = relu?(a*x + b) as [N][C][H + 2 pad][W + 2 pad] float64 with the zero padding around it.  affine_on_padding (a mistake): the affine and ReLU
    applied to the padded map instead"""
    aff, relu = FORMS[form]
    z = _t64(x).view(op.N, op.H, op.W, -1)
    p = op.pad
    if affine_on_padding:
        z = F.pad(z, (0, 0, p, p, p, p))
    if aff:
        z = _t64(a) * z + _t64(b)
    if relu:
        z = F.relu(z)
    if not affine_on_padding:
        z = F.pad(z, (0, 0, p, p, p, p))
    return z.permute(0, 3, 1, 2).contiguous()


def forward_fp64(op, inp, forms, bias_form=0, affine_on_padding=False, drop_tap=False, w_choff=None, flip_tap=False, bias_n_shift=0):
    """y [N*OH*OW][Cout] float64.  The keyword arguments are the deliberate mistakes of tests/test_conv_ref.py: the affine applied to the padding; tap
    (k // 2, 0) left out at the last output column; the slice read from another channel offset; the sign of tap (0, k - 1) (1x1: the only tap) flipped;
    bias_n taken from the image `bias_n_shift` further on."""
    z = torch.cat([activation(op, inp['x'][i], inp['a'][i], inp['b'][i], forms[i], affine_on_padding) for i in range(len(op.Cs))], 1)
    w = weight_fp64(op, inp['w'], op.w_choff if w_choff is None else w_choff, sum(op.Cs))
    if flip_tap:
        w[:, :, 0, op.k - 1] *= -1
    y = F.conv2d(z, w, stride=op.stride, dilation=op.dil)[:, :, :op.OH, :op.OW]
    if drop_tap:
        w1 = torch.zeros_like(w)
        w1[:, :, op.k // 2, 0] = w[:, :, op.k // 2, 0]
        y[:, :, :, -1] -= F.conv2d(z, w1, stride=op.stride, dilation=op.dil)[:, :, :op.OH, op.OW - 1]
    y = y.permute(0, 2, 3, 1)
    if bias_form == 1:
        y = y + _t64(inp['bias'])
    elif bias_form == 2:
        y = y + torch.roll(_t64(inp['bias_n']), -bias_n_shift, 0).view(op.N, 1, 1, op.Cout)
    return y.reshape(-1, op.Cout).numpy()


def stats_fp64(y):
    """[Cout][2]: (sum, sum of squares) per channel"""
    return np.stack([y.sum(0), (y * y).sum(0)], 1)


def dz_fp64(op, inp, i, no_mirror=False, w_choff=None, flip_tap=False):
    """gradient wrt z_i, [N*H*W][Cs[i]] float64: the transposed convolution of dy.  no_mirror (a mistake): the taps not mirrored"""
    w = weight_fp64(op, inp['w'], choff(op, i) if w_choff is None else w_choff, op.Cs[i])
    if flip_tap:
        w[:, :, 0, op.k - 1] *= -1
    if no_mirror:
        w = w.flip(2, 3)
    dy = _t64(inp['dy']).view(op.N, op.OH, op.OW, op.Cout).permute(0, 3, 1, 2)
    full = lambda on: (on - 1) * op.stride - 2 * op.pad + op.dil * (op.k - 1) + 1
    dz = F.conv_transpose2d(dy, w, stride=op.stride, padding=op.pad, dilation=op.dil, output_padding=(op.H - full(op.OH), op.W - full(op.OW)))
    return dz.permute(0, 2, 3, 1).reshape(-1, op.Cs[i]).numpy()


def dgrad_fp64(op, inp, i, form, dz, ignore_relu_mask=False):
    """(g [N*H*W][C], dab [C][2]) float64 from dz, without the accumulation.  ignore_relu_mask (a mistake): the mask taken as 1"""
    aff, relu = FORMS[form]
    x = np.asarray(inp['x'][i], dtype=np.float64)
    a = np.asarray(inp['a'][i], dtype=np.float64) if aff else np.ones(op.Cs[i])
    b = np.asarray(inp['b'][i], dtype=np.float64) if aff else np.zeros(op.Cs[i])
    m = dz * ((a * x + b > 0) if relu and not ignore_relu_mask else 1.0)
    return a * m, np.stack([(m * x).sum(0), m.sum(0)], 1)


def widen(slice_, init, ld, accumulate=0):
    """the whole [P][ld] buffer after a launch, float64: init outside the first columns, slice_ (accumulate: init + slice_) inside"""
    out = np.array(init, dtype=np.float64).reshape(-1, ld)
    n = slice_.shape[1]
    out[:, :n] = slice_ + (out[:, :n] if accumulate else 0.0)
    return out


_REF = OrderedDict()


def _cached(key, make, keep=24):
    if key not in _REF:
        while len(_REF) >= keep:
            _REF.popitem(last=False)
        v = make()
        for u in (v if isinstance(v, tuple) else (v,)):
            u.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def ref_forward(op, forms, bias_form=0):
    """forward_fp64 of an op's seeded inputs without a bias (cached per (op, forms), read-only) plus the bias form"""
    y = _cached(('y', op, tuple(forms)), lambda: forward_fp64(op, make_inputs(op), forms))
    inp = make_inputs(op)
    if bias_form == 1:
        return y + inp['bias'].astype(np.float64)
    if bias_form == 2:
        return (y.reshape(op.N, -1, op.Cout) + inp['bias_n'].astype(np.float64)[:, None, :]).reshape(-1, op.Cout)
    return y


def ref_dz(op, i):
    return _cached(('dz', op, i), lambda: dz_fp64(op, make_inputs(op), i))


def ref_dgrad(op, i, form, dy_scale=1.0):
    """(g, dab) of source i in a destination form, dy scaled by an exact power of two"""
    g, dab = dgrad_fp64(op, make_inputs(op), i, form, ref_dz(op, i))
    return g * dy_scale, dab * dy_scale
