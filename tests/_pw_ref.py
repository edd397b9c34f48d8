"""fp64 reference of what the kernels of csrc/pw.hip compute, as include/addk.h defines it (addk_conv_args, addk_conv_dgrad_args), the case table that
reaches each of their 46 lone instantiations and the mixed batches for the 30 batched ones, and what tests/test_pw_ref.py (no GPU) and
tests/test_gpu_pw_fp64.py share.  numpy only.

Forward of a 1x1 convolution over virtually concatenated sources i:

    r_i = x_i                                                   a plain source
        = bilinear(x_i, align_corners = False) onto [N, H, W]   a resampled one (addk_src.rs_hw: x_i is an [N, RH, RW] map)
    z_i = relu_i?(a_i * r_i + b_i)                              (a = 1, b = 0 without an affine: the four source FORMS)
    y[p, n]  = bias[n] + sum_i sum_k w[n*ldw + w_choff + C_0 + .. + C_{i-1} + k] * z_i[p, k]
    stats[n] = (sum_p y, sum_p y^2)                             the bias enters both
    rs_y     = r_0                                              the interpolated raw source 0, before the affine

Data gradient with respect to the only source of a 1x1 convolution (K = channels of dy):

    dz[p, n] = sum_k dy[p, k] * w[k*ldw + w_choff + n]
    m        = !relu || a*x + b > 0                             from a*x + b in fp64 on the fp32 inputs: the product is exact, the one rounding of
                                                                the sum keeps the sign, so this IS the sign of the kernel's fmaf(a, x, b)
    g (+)= m ? dz * a : 0,      dA[n] = sum_p m * dz * x,      dB[n] = sum_p m * dz

stem0: y[n, oy, ox, co] = sum_{ky, kx, c < 3} w[co*ldw + (3 ky + kx) * 3 + c] * x[n, 2 oy - 1 + ky, 2 ox - 1 + kx, c], zero outside the map, rows of x of
pixel stride 4.

Every launch is shaped as a plan shapes it: the weight is a slice (w_choff = 8 of cin_total = K + 12 channels, ldw = cin_total + 4), x, dy, y, g and rs_y
are slices of rows 8 floats wider than their channels (rounded up to a multiple of 4), stats_ld = Cout + 4; the padding floats of every input row and the
four padding floats of a weight row hold NaN, so a kernel that lets a masked k slot through shows up as a NaN.  The keyword switches of the reference
functions are the deliberate mistakes of tests/test_pw_ref.py."""
import ctypes as C
import importlib.util
import os
from collections import OrderedDict, namedtuple

import numpy as np

from _wgrad_ref import FIRST_TOUCH_BITS, FORM_NAMES, FORMS, GUARD_BITS, Guarded, TOL, rel_err  # noqa: F401  (re-exported)
from _conv_ref import SLAB_BITS  # noqa: F401

_spec = importlib.util.spec_from_file_location('make_pw_bits', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'make_pw_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)
STEM0, PW, PWK, K1S = bits.STEM0, bits.PW, bits.PWK, bits.K1S

FAST_ALL = 31
W_CHOFF = 8
SMALL = (2, 33, 31)        # P = 2046 < 4096: fp64 lane sums; two images, a partial last 16-pixel tile
LARGE = (2, 40, 52)        # P = 4160 >= 4096: fp32 lane sums
TINY = (1, 1, 5)           # P = 5: one workgroup, three of its four waves without a tile
MAP_UP = (17, 33)          # a resampled source's map smaller than the grid's rows ...
MAP_DOWN = {SMALL: (45, 38), LARGE: (47, 61)}      # ... and one larger than the grid in both directions

# One launch's shapes.  kind: 'fwd' (1x1 forward; Cs: channels of the sources, maps: per source None or the (RH, RW) it is sampled from), 'dgrad' (1x1
# data gradient: Cs = (channels of the destination,), Cout = channels of dy) or 'stem0' (N, H, W: the input map).
Op = namedtuple('Op', 'kind N H W Cs Cout maps seed')
# A case: the launch and the [kind, v0..v3] of addk_conv_*_config and the batch key (-1: not batchable) it must get.
Case = namedtuple('Case', 'name op cfg key')


def pw_key(mode, ct, kg, rs, red32):
    """the batch key of a register-stationary launch (csrc/pw.hip pw_key; tests/test_pw_dispatch.py pins the same fields)"""
    return (mode << 12) | (ct << 8) | (kg << 4) | (rs << 1) | red32


def _cases():
    out = []

    def add(name, kind, grid, Cs, Cout, cfg, key=-1, maps=None):
        Cs = (Cs,) if isinstance(Cs, int) else tuple(Cs)
        out.append(Case(name, Op(kind, grid[0], grid[1], grid[2], Cs, Cout, tuple(maps or (None,) * len(Cs)), 700 + len(out)), list(cfg), key))

    # pw_kernel <CT, KG>: every reduction length (36: one live quad in group 2; 40, 48; 68, 80) and every output width (12; 20, 24: a partial second tile;
    # 40: a half third tile; 160: gy = 4; 80 at KG 5: 32 + 32 + 16, the last block's second tile wholly beyond the output) on either side
    fwd = {('s', 0): [(36, 12, 1, 3), (48, 20, 2, 3), (40, 160, 3, 3), (68, 16, 1, 5), (80, 80, 2, 5)],
           ('s', 1): [(40, 12, 1, 3), (36, 24, 2, 3), (48, 40, 3, 3), (80, 12, 1, 5), (68, 40, 2, 5)],
           ('l', 0): [(40, 12, 1, 3), (36, 24, 2, 3), (48, 40, 3, 3), (80, 16, 1, 5), (68, 40, 2, 5)],
           ('l', 1): [(36, 12, 1, 3), (48, 20, 2, 3), (40, 160, 3, 3), (68, 16, 1, 5), (80, 80, 2, 5)]}
    for (side, rs), rows in fwd.items():
        grid, r32 = (SMALL, 0) if side == 's' else (LARGE, 1)
        for K, co, ct, kg in rows:
            add('pw_fwd%s_%dto%d_%s' % ('_rs' if rs else '', K, co, side), 'fwd', grid, K, co, (PW, ct, kg, rs, r32), pw_key(0, ct, kg, rs, r32), [MAP_UP] if rs else None)
    # the data gradient: (channels of dy = the reduction, channels of the destination = the output side)
    dg = {'s': [(36, 12, 1, 3), (40, 20, 2, 3), (48, 160, 3, 3), (68, 16, 1, 5), (80, 80, 2, 5)],
          'l': [(48, 12, 1, 3), (36, 24, 2, 3), (40, 40, 3, 3), (80, 16, 1, 5), (68, 40, 2, 5)]}
    for side, rows in dg.items():
        grid, r32 = (SMALL, 0) if side == 's' else (LARGE, 1)
        for K, cn, ct, kg in rows:
            add('pw_dgrad_%dinto%d_%s' % (K, cn, side), 'dgrad', grid, cn, K, (PW, ct, kg, 0, r32), pw_key(1, ct, kg, 0, r32))
    # pwk_kernel <CT>: 200 = 12 groups and a half; 64 + 8 + 24: a source of a single half group in the middle of the walk; rs1: source 1, not source 0, is
    # the resampled one
    add('pwk_128to16_s', 'fwd', SMALL, 128, 16, (PWK, 1, 0, 0, 0))
    add('pwk_rs_128to16_s', 'fwd', SMALL, 128, 16, (PWK, 1, 1, 0, 0), maps=[MAP_UP])
    add('pwk_64+32to24_s', 'fwd', SMALL, (64, 32), 24, (PWK, 2, 0, 0, 0))
    add('pwk_rs1_64+32to24_s', 'fwd', SMALL, (64, 32), 24, (PWK, 2, 1, 0, 0), maps=[None, MAP_UP])
    add('pwk_200to160_s', 'fwd', SMALL, 200, 160, (PWK, 3, 0, 0, 0))
    add('pwk_rs_200to40_s', 'fwd', SMALL, 200, 40, (PWK, 3, 1, 0, 0), maps=[MAP_UP])
    add('pwk_64+8+24to16_l', 'fwd', LARGE, (64, 8, 24), 16, (PWK, 1, 0, 1, 0))
    add('pwk_rs_64+8+24to12_l', 'fwd', LARGE, (64, 8, 24), 12, (PWK, 1, 1, 1, 0), maps=[MAP_UP, None, None])
    add('pwk_64+32to20_l', 'fwd', LARGE, (64, 32), 20, (PWK, 2, 0, 1, 0))
    add('pwk_rs_64+32to24_l', 'fwd', LARGE, (64, 32), 24, (PWK, 2, 1, 1, 0), maps=[MAP_UP, None])
    add('pwk_200to40_l', 'fwd', LARGE, 200, 40, (PWK, 3, 0, 1, 0))
    add('pwk_rs_200to160_l', 'fwd', LARGE, 200, 160, (PWK, 3, 1, 1, 0), maps=[MAP_UP])
    add('stem0_s', 'stem0', (1, 33, 65), 3, 64, (STEM0, 4, 0, 0, 0))         # 17 x 33 = 561 output pixels
    add('stem0_l', 'stem0', (2, 91, 95), 3, 64, (STEM0, 4, 1, 0, 0))         # 2 x 46 x 48 = 4416
    add('k1s_19into256', 'dgrad', SMALL, 256, 19, (K1S, 20, 0, 0, 0))
    add('k1s_24into128', 'dgrad', SMALL, 128, 24, (K1S, 32, 0, 0, 0))
    n = len(out)
    # further shapes of variants the list above has reached: 132 channels (31 idle lanes), the widest launch, one dy channel; and the tiny map
    add('k1s_21into132', 'dgrad', SMALL, 132, 21, (K1S, 32, 0, 0, 0))
    add('k1s_32into256', 'dgrad', SMALL, 256, 32, (K1S, 32, 0, 0, 0))
    add('k1s_1into128', 'dgrad', SMALL, 128, 1, (K1S, 20, 0, 0, 0))
    add('pw_fwd_36to24_tiny', 'fwd', TINY, 36, 24, (PW, 2, 3, 0, 0), pw_key(0, 2, 3, 0, 0))
    add('pw_dgrad_68into40_tiny', 'dgrad', TINY, 40, 68, (PW, 2, 5, 0, 0), pw_key(1, 2, 5, 0, 0))
    add('k1s_19into256_tiny', 'dgrad', TINY, 256, 19, (K1S, 20, 0, 0, 0))      # a trip whose second pixel is missing for three of the four waves
    return out, n


CASES, N_VARIANTS = _cases()          # the first N_VARIANTS cases: one per lone instantiation
BY_NAME = {c.name: c for c in CASES}


def other_map(op):
    """an RS case on the map larger than its grid"""
    return op._replace(maps=tuple(m and MAP_DOWN[(op.N, op.H, op.W)] for m in op.maps))


# ---------------------------------------------------------------------------------------------------------------- mixed batches

# One launch of a test: forward (forms per source, bias, stats, rs_y) or data gradient (forms = (form,), accumulate, stats = dab present, dy_scale).
Launch = namedtuple('Launch', 'op forms bias stats rs_y accumulate dy_scale')


def fwd_launch(op, forms, bias=False, stats=True, rs_y=False):
    return Launch(op, tuple(forms), bias, stats, rs_y, 0, 1.0)


def dgrad_launch(op, form, accumulate=0, dab=True, dy_scale=1.0):
    return Launch(op, (form,), False, dab, False, accumulate, dy_scale)


BATCH_GRIDS = {0: [(2, 33, 31), (1, 33, 65), (3, 20, 25)], 1: [(2, 40, 52), (1, 65, 67), (2, 47, 61)]}      # gx 16, 17, 12 | 33, 35, 45
BATCH_K = {3: (36, 40, 48), 5: (68, 80, 68)}
BATCH_CN = {(1, 3): (12, 16, 8), (2, 3): (20, 24, 20), (3, 3): (40, 80, 160), (1, 5): (12, 16, 8), (2, 5): (20, 40, 80)}      # gy 1, 2, 4 at CT 3; 1, 2, 3 at <2, 5>
BATCH_MAPS = [(17, 33), (70, 75), (9, 11)]
# (mode, CT, KG, RS, red32) of the 30 batched instantiations
BATCH_VARIANTS = [(0, ct, kg, rs, r32) for ct, kg in BATCH_CN for rs in (0, 1) for r32 in (0, 1)] + [(1, ct, kg, 0, r32) for ct, kg in BATCH_CN for r32 in (0, 1)]


def batch_id(v):
    return '%s%s_ct%d_kg%d_%s' % ('dgrad' if v[0] else 'fwd', '_rs' if v[3] else '', v[1], v[2], 'red32' if v[4] else 'red64')


def batch_members(v):
    """Three launches of one key that differ in pixel count (gx), output width (gy, where CT leaves a choice), reduction length, source form, bias and
    accumulate, with the statistics / (dA, dB) slab of the last one NULL; the RS members also in the map they sample and in rs_y present or NULL."""
    mode, ct, kg, rs, r32 = v
    out = []
    for i in range(3):
        grid, K, cn = BATCH_GRIDS[r32][i], BATCH_K[kg][i], BATCH_CN[(ct, kg)][i]
        seed = 900 + 8 * BATCH_VARIANTS.index(v) + i
        if mode == 0:
            op = Op('fwd', grid[0], grid[1], grid[2], (K,), cn, (BATCH_MAPS[i] if rs else None,), seed)
            out.append(fwd_launch(op, [(0, 3, 1)[i]], bias=i == 1, stats=i != 2, rs_y=bool(rs) and i != 1))
        else:
            op = Op('dgrad', grid[0], grid[1], grid[2], (cn,), K, (None,), seed)
            out.append(dgrad_launch(op, (0, 3, 2)[i], accumulate=(0, 1, 1)[i], dab=i != 2))
    return out


# ---------------------------------------------------------------------------------------------------------------- strides, inputs, arguments

def wide(c):
    """row stride of a slice of c channels: 8 more floats, rounded up to a multiple of 4 (the three image channels of stem0: 4)"""
    return 4 if c == 3 else (c + 8 + 3) // 4 * 4


def out_hw(op):
    return ((op.H - 1) // 2 + 1, (op.W - 1) // 2 + 1) if op.kind == 'stem0' else (op.H, op.W)


def pixels(op):
    """pixels of the launch's output side"""
    oh, ow = out_hw(op)
    return op.N * oh * ow


def layout(op, ldy=None):
    """the strides of an op's launch"""
    if op.kind == 'stem0':
        return dict(cin_total=3, w_choff=0, ldw=32, ldy=ldy or 72, stats_ld=op.Cout + 4, wrows=op.Cout)
    ctot = sum(op.Cs)
    d = dict(cin_total=ctot + 12, w_choff=W_CHOFF, ldw=ctot + 16, stats_ld=op.Cout + 4)
    if op.kind == 'fwd':
        d.update(ldy=wide(op.Cout), rs_ldy=wide(op.Cs[0]), wrows=op.Cout)
    else:
        d.update(lddy=wide(op.Cout), ldg=wide(ctot), wrows=op.Cout)
    return d


_INPUTS = OrderedDict()


def _nan_pad(v, c):
    v[:, c:] = np.nan
    return v


def make_inputs(op):
    """float32 numpy arrays, read-only and shared by every launch of an op: x, a, b (lists per source), the whole wider weight w, bias; a data gradient
    also has dy and g0 (what an accumulating launch starts from, finite in its padding too).  NaN in the padding of every x and dy row and in the last
    four floats of every weight row."""
    if op not in _INPUTS:
        while len(_INPUTS) >= 8:
            _INPUTS.popitem(last=False)
        rs = np.random.RandomState(op.seed)
        f = lambda scale, *sh: (scale * rs.standard_normal(sh)).astype(np.float32)
        lay, P = layout(op), pixels(op)
        d = {'x': [], 'a': [], 'b': []}
        for i, c in enumerate(op.Cs):
            rows = op.N * op.maps[i][0] * op.maps[i][1] if op.maps[i] else op.N * op.H * op.W
            d['x'].append(_nan_pad(f(1.0, rows, wide(c)), c))
            d['a'].append((1.0 + 0.25 * rs.standard_normal(c)).astype(np.float32))
            d['b'].append(f(0.3, c))
        ktot = 27 if op.kind == 'stem0' else sum(op.Cs) if op.kind == 'fwd' else op.Cout
        d['w'] = _nan_pad(f(1.0 / np.sqrt(ktot), lay['wrows'], lay['ldw']), 27 if op.kind == 'stem0' else lay['cin_total'])
        d['bias'] = f(0.5, op.Cout)
        if op.kind == 'dgrad':
            d['dy'] = _nan_pad(f(1.0, P, lay['lddy']), op.Cout)
            d['g0'] = f(1.0, P, lay['ldg'])
        for v in d.values():
            for u in (v if isinstance(v, list) else [v]):
                u.setflags(write=False)
        _INPUTS[op] = d
    return _INPUTS[op]


PTR = {'x': 0x10000000, 'a': 0x11000000, 'b': 0x11001000, 'w': 0x20000000, 'y': 0x30000000, 'slab': 0x40000000, 'dy': 0x50000000, 'rs_y': 0x60000000,
       'bias': 0x12000000}      # 16-byte aligned placeholders: a config call dereferences nothing


def host_ptr(op):
    p = dict(PTR)
    for k, step in (('x', 0x100000), ('a', 0x400), ('b', 0x400)):
        p[k] = [PTR[k] + step * i for i in range(len(op.Cs))]
    return p


def launch_args(L, la, ptr, ldy=None):
    """ConvArgs / ConvDgradArgs of a launch; `ptr` maps x, a, b (lists per source), w, bias, dy, y (the output: y or g), slab, rs_y to addresses.  a and b
    are passed only in the forms that have them, bias / slab / rs_y only where the launch has them."""
    op, lay = la.op, layout(la.op, ldy)
    oh, ow = out_hw(op)
    if op.kind == 'dgrad':
        aff, relu = FORMS[la.forms[0]]
        da = L.ConvDgradArgs()
        da.dy, da.lddy, da.Cout = ptr['dy'], lay['lddy'], op.Cout
        da.N, da.H, da.W, da.OH, da.OW, da.KH, da.KW, da.stride, da.pad, da.dil = op.N, op.H, op.W, op.H, op.W, 1, 1, 1, 0, 1
        da.w, da.ldw, da.cin_total, da.w_choff = ptr['w'], lay['ldw'], lay['cin_total'], lay['w_choff']
        da.dst.x, da.dst.ld, da.dst.C, da.dst.relu = ptr['x'][0], wide(op.Cs[0]), op.Cs[0], relu
        if aff:
            da.dst.a, da.dst.b = ptr['a'][0], ptr['b'][0]
        da.g, da.ldg, da.accumulate, da.dab = ptr['y'], lay['ldg'], la.accumulate, ptr['slab'] if la.stats else None
        return da
    ar = L.ConvArgs()
    for i, c in enumerate(op.Cs):
        aff, relu = FORMS[la.forms[i]]
        s = ar.src[i]
        s.x, s.ld, s.C, s.relu = ptr['x'][i], wide(c), c, relu
        if aff:
            s.a, s.b = ptr['a'][i], ptr['b'][i]
        if op.maps[i]:
            s.rs_hw = (op.maps[i][0] << 16) | op.maps[i][1]
    k, stride, pad = (3, 2, 1) if op.kind == 'stem0' else (1, 1, 0)
    ar.nsrc = len(op.Cs)
    ar.N, ar.H, ar.W, ar.OH, ar.OW, ar.KH, ar.KW, ar.stride, ar.pad, ar.dil, ar.Cout = op.N, op.H, op.W, oh, ow, k, k, stride, pad, 1, op.Cout
    ar.ldw, ar.cin_total, ar.w_choff, ar.ldy = lay['ldw'], lay['cin_total'], lay['w_choff'], lay['ldy']
    ar.w, ar.y, ar.stats, ar.stats_ld = ptr['w'], ptr['y'], ptr['slab'] if la.stats else None, lay['stats_ld']
    if la.bias:
        ar.bias = ptr['bias']
    if la.rs_y:
        ar.rs_y, ar.rs_ldy = ptr['rs_y'], lay['rs_ldy']
    return ar


def default_launch(op):
    """the first launch of a case: every source with (a, b) + ReLU (stem0: plain), no bias, with statistics, rs_y where source 0 is resampled"""
    if op.kind == 'dgrad':
        return dgrad_launch(op, 0)
    return fwd_launch(op, [3 if op.kind == 'stem0' else 0] * len(op.Cs), rs_y=op.maps[0] is not None)


def config(lb, L, la, ptr=None):
    """([kind, v0..v3], gx, gy, batch key) of a launch (make_pw_bits.config), by default from placeholder pointers"""
    return bits.config(lb, L, (None, 'dgrad' if la.op.kind == 'dgrad' else 'fwd'), launch_args(L, la, ptr or host_ptr(la.op)))


def batch_prepare(lb, L, args, blob=False):
    """(meta[0..3], the host blob or None) of addk_conv_*_batch_prepare over a list of ConvArgs / ConvDgradArgs"""
    arr = (type(args[0]) * len(args))(*args)
    prep = getattr(lb, 'addk_conv_%s_batch_prepare' % ('dgrad' if isinstance(args[0], L.ConvDgradArgs) else 'fwd'))
    meta = (C.c_int64 * 8)()
    size = int(prep(arr, len(args), None, 0, meta))
    if size < 0:
        L.check(size, 'conv_batch_prepare')
    host = None
    if blob:
        host = (C.c_uint8 * size)()
        rc = int(prep(arr, len(args), host, size, meta))
        if rc < 0:
            L.check(rc, 'conv_batch_prepare')
    return meta, host


def batch_meta(lb, L, launches):
    """meta of a batch of launches with placeholder pointers"""
    return batch_prepare(lb, L, [launch_args(L, la, host_ptr(la.op)) for la in launches])


# ---------------------------------------------------------------------------------------------------------------- the reference

def _axis(out, inn, align_corners):
    """source indices and weights of one axis, F.interpolate(mode='bilinear') in float64"""
    d = np.arange(out, dtype=np.float64)
    if align_corners:
        s = d * ((inn - 1) / (out - 1) if out > 1 else 0.0)
    else:
        s = np.maximum(inn / out * (d + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), inn - 1)
    i1 = np.minimum(i0 + 1, inn - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1


def interp(x, N, RH, RW, H, W, align_corners=False, image0=False):
    """[N*RH*RW][C] -> [N*H*W][C] in x's dtype.  image0 (a mistake): every image samples image 0"""
    v = x.reshape(N, RH, RW, -1)
    if image0:
        v = np.repeat(v[:1], N, 0)
    h0, h1, lh0, lh1 = _axis(H, RH, align_corners)
    w0, w1, lw0, lw1 = _axis(W, RW, align_corners)
    t = x.dtype.type
    lh0, lh1, lw0, lw1 = (u.astype(t) for u in (lh0, lh1, lw0, lw1))
    rows0, rows1 = v[:, h0], v[:, h1]
    top = lw0[None, None, :, None] * rows0[:, :, w0] + lw1[None, None, :, None] * rows0[:, :, w1]
    bot = lw0[None, None, :, None] * rows1[:, :, w0] + lw1[None, None, :, None] * rows1[:, :, w1]
    return (lh0[None, :, None, None] * top + lh1[None, :, None, None] * bot).reshape(N * H * W, -1)


def source(op, inp, i, form, dt=np.float64, align_corners=False, affine_first=False, image0=False):
    """(z_i [P][C_i], r_i or None for a plain source).  affine_first (a mistake): the affine and ReLU applied to the map, then the interpolation"""
    c = op.Cs[i]
    aff, relu = FORMS[form]
    x = inp['x'][i][:, :c].astype(dt)

    def pro(v):
        if aff:
            v = inp['a'][i].astype(dt) * v + inp['b'][i].astype(dt)
        return np.maximum(v, 0) if relu else v
    if not op.maps[i]:
        return pro(x), None
    rs = lambda v: interp(v, op.N, op.maps[i][0], op.maps[i][1], op.H, op.W, align_corners, image0)
    raw = rs(x)
    return (rs(pro(x)) if affine_first else pro(raw)), raw


def forward(op, inp, forms, bias=False, dt=np.float64, drop_last_quad=False, w_choff_shift=0, second_source_offset0=False, **rs_mistakes):
    """(y [P][Cout], r_0 or None) in dt.  Mistakes: the last four channels of the reduction left out; the slice read 4 channels further on; source 1 read
    with source 0's weight columns; and those of source()."""
    w = inp['w'].astype(dt)
    lay = layout(op)
    y, raw0, c0 = 0, None, lay['w_choff'] + w_choff_shift
    for i, c in enumerate(op.Cs):
        z, raw = source(op, inp, i, forms[i], dt, **rs_mistakes)
        raw0 = raw if i == 0 else raw0
        if drop_last_quad and i == len(op.Cs) - 1:
            z = z.copy()
            z[:, -4:] = 0
        cw = lay['w_choff'] + w_choff_shift if (second_source_offset0 and i == 1) else c0
        y = y + z @ w[:, cw:cw + c].T
        c0 += c
    if bias:
        y = y + inp['bias'].astype(dt)
    return y, raw0


def stem0(op, inp, dt=np.float64, pad=1):
    """y [N*OH*OW][64] in dt; pad = 0 is a mistake (the output grid stays that of pad 1)"""
    oh, ow = out_hw(op)
    x = inp['x'][0][:, :3].astype(dt).reshape(op.N, op.H, op.W, 3)
    xp = np.zeros((op.N, op.H + 3, op.W + 3, 3), dtype=dt)
    xp[:, pad:pad + op.H, pad:pad + op.W] = x
    w = inp['w'].astype(dt)
    y = np.zeros((op.N, oh, ow, op.Cout), dtype=dt)
    for ky in range(3):
        for kx in range(3):
            t = 3 * ky + kx
            y += xp[:, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2] @ w[:, 3 * t:3 * t + 3].T
    return y.reshape(-1, op.Cout)


def stats(y, without=None, drop_partial_tile=False):
    """[Cout][2]: (sum, sum of squares) per channel.  Mistakes: `without` (the bias) taken out of y first; the pixels of the partial last 16-pixel
    tile left out"""
    if without is not None:
        y = y - without.astype(y.dtype)
    if drop_partial_tile:
        y = y[:len(y) - len(y) % 16]
    return np.stack([y.sum(0), (y * y).sum(0)], 1)


def dgrad(op, inp, form, accumulate=0, dy_scale=1.0, dt=np.float64, no_transpose=False, mask_from_x=False, da_without_x=False, overwrite=False,
          second_pixel_stride=0, w_choff_shift=0):
    """(the [P][C] slice of g after the launch, dab [C][2]) in dt; the mask always from a*x + b in float64.  Mistakes: the weight read as the forward reads
    it (w[n*ldw + w_choff + k], zero where that leaves the array's finite part); the mask from x; dA without its x factor; an accumulating launch that
    overwrites; the pixels with (p // second_pixel_stride) odd, k1s's second pixel of a trip, missing from (dA, dB); the slice 4 channels further on."""
    c, K = op.Cs[0], op.Cout
    lay = layout(op)
    aff, relu = FORMS[form]
    off = lay['w_choff'] + w_choff_shift
    w = inp['w'].astype(dt)
    wm = w[:K, off:off + c]
    if no_transpose:
        wm = np.zeros((K, c), dtype=dt)
        n, k = min(c, K), min(K, lay['cin_total'] - off)
        wm[:k, :n] = w[:n, off:off + k].T
    dz = (inp['dy'][:, :K].astype(dt) * dt(dy_scale)) @ wm
    x = inp['x'][0][:, :c]
    a = inp['a'][0] if aff else np.ones(c, dtype=np.float32)
    b = inp['b'][0] if aff else np.zeros(c, dtype=np.float32)
    m = np.ones(x.shape, dtype=bool)
    if relu:
        m = (x > 0) if mask_from_x else (a.astype(np.float64) * x.astype(np.float64) + b.astype(np.float64) > 0)
    md = np.where(m, dz, dt(0))
    g = md * a.astype(dt)
    ms = md
    if second_pixel_stride:
        ms = md * ((np.arange(len(md)) // second_pixel_stride) % 2 == 0)[:, None].astype(dt)
    dab = np.stack([(ms * (1 if da_without_x else x.astype(dt))).sum(0), ms.sum(0)], 1)
    if accumulate and not overwrite:
        g = g + inp['g0'][:, :c].astype(dt)
    return g, dab


_REF = OrderedDict()


def _cached(key, make, keep=32):
    if key not in _REF:
        while len(_REF) >= keep:
            _REF.popitem(last=False)
        v = make()
        for u in (v if isinstance(v, tuple) else (v,)):
            if u is not None:
                u.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def reference(la):
    """What a launch leaves behind, float64: {'y' or 'g': the slice of the output, 'stats' or 'dab': [C][2] (None without a slab), 'rs_y': r_0 (None
    without rs_y)}.  The bias-free forward and the unscaled gradient are cached per (op, forms) and never modified."""
    op, inp = la.op, make_inputs(la.op)
    if op.kind == 'dgrad':
        g, dab = _cached(('g', op, la.forms[0], la.accumulate), lambda: dgrad(op, inp, la.forms[0], la.accumulate))
        if la.dy_scale != 1.0:       # a power of two scales dz, g and (dA, dB) exactly; the seeded g0 is not scaled
            g0 = inp['g0'][:, :op.Cs[0]].astype(np.float64) if la.accumulate else 0.0
            g, dab = (g - g0) * la.dy_scale + g0, dab * la.dy_scale
        return {'g': g, 'dab': dab if la.stats else None}
    if op.kind == 'stem0':
        y = _cached(('y', op), lambda: stem0(op, inp))
        return {'y': y, 'stats': stats(y) if la.stats else None, 'rs_y': None}
    y, raw = _cached(('y', op, la.forms), lambda: forward(op, inp, la.forms))
    if la.bias:
        y = y + inp['bias'].astype(np.float64)
    return {'y': y, 'stats': stats(y) if la.stats else None, 'rs_y': raw if la.rs_y else None}


# ---------------------------------------------------------------------------------------------------------------- the launches of the GPU test

TINY_DY = 2.0 ** -30


def case_launches(case):
    """[(label, launch, ldy or None)]: every launch tests/test_gpu_pw_fp64.py makes for a lone case.  Forward: the four source forms (source i of several
    in form (f + i) mod 4) x {no bias, bias}, rs_y wherever source 0 is resampled; once without statistics; an RS case twice more on the map larger than
    its grid, once without rs_y.  Data gradient: the four destination forms x {first touch, accumulate}; once without dab; once with dy * 2^-30.
    stem0: ldy = 64 and 72."""
    op = case.op
    if op.kind == 'stem0':
        return [('ldy%d' % ldy, default_launch(op), ldy) for ldy in (64, 72)]
    out = []
    if op.kind == 'dgrad':
        for f in range(4):
            for acc in (0, 1):
                out.append(('%s/%s' % (FORM_NAMES[f], 'acc' if acc else 'first'), dgrad_launch(op, f, acc), None))
        out.append(('ab/acc/no_dab', dgrad_launch(op, 1, 1, dab=False), None))
        out.append(('ab_relu/first/dy*2^-30', dgrad_launch(op, 0, 0, dy_scale=TINY_DY), None))
        return out
    rs0, n = op.maps[0] is not None, len(op.Cs)
    forms = lambda f: [(f + i) % 4 for i in range(n)]
    for f in range(4):
        for bias in (False, True):
            out.append(('%s/%s' % ('+'.join(FORM_NAMES[v] for v in forms(f)), 'bias' if bias else 'nobias'), fwd_launch(op, forms(f), bias, True, rs0), None))
    if any(op.maps):
        big = other_map(op)
        out.append(('map_down/ab_relu/bias/no_stats', fwd_launch(big, forms(0), True, False, rs0), None))
        out.append(('map_down/ab/nobias/no_rs_y', fwd_launch(big, forms(1), False, True, False), None))
    else:
        out.append(('ab_relu/bias/no_stats', fwd_launch(op, forms(0), True, False, False), None))
    return out
