"""Host-side choice of the fused SepConv kernels (csrc/sep.h sep_choose) and of the depthwise kernels (dw.hip dw_choose_*), no GPU: the
library is called with aligned placeholder pointers (nothing is dereferenced before a launch).  For every shape x fast-path mask:
addk_sep_fwd_supported, addk_sep_rows, addk_sep_bwd_rows, the batch keys and the meta of a one-item batch prepare agree with what
addk_sep_*_config / addk_dw_*_config report; forward and backward of one shape get the same variant and tiles; the rules of the choice
(channel ranges, the 512-workgroup rule, the two-row rule, the depthwise pixel floor) are pinned on both sides; the batch key is
ks << 16 | kg << 12 | kp << 4 | r with the parent's values, and decode(encode) is the identity for the twelve built variants; config 2's
dry-built plans keep their launch counts."""
import collections
import ctypes as C
import os
import subprocess

import pytest
import torch

import addk
import addk.plan as P
from addk import _lib as L
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args
import test_gpu_fast_kernels as FK
import _sep_ref as SR
from test_conv_dispatch import MASKS, PTR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_PW, FAST_DWTILE = 1, 8

# (name, N, H, W, C, K) -> expected (kg, kp, r, workgroups), 'fused' / 'unfused', or None: the shape of a GPU kernel test, which must be covered
SEP = [(s, None) for s in FK.SEP_SHAPES]
SEP += [(('c2_%d_c%d_%dx%d_k%d' % (N, Cc, H, W, k), N, H, W, Cc, k), 'fused')
        for N in (2, 1) for Cc, H, W in ((40, 125, 253), (40, 128, 256), (80, 63, 127), (80, 64, 128)) for k in (3, 5)]
SEP += [(('c2_%d_c160_k%d' % (N, k), N, 32, 64, 160, k), 'unfused') for N in (2, 1) for k in (3, 5)]
# channel ranges: (32, 48] and (64, 80], multiples of 4
SEP += [(('edge_c%d' % Cc, 1, 40, 70, Cc, 3), 'fused' if Cc in (48, 80) else 'unfused') for Cc in (32, 33, 48, 49, 52, 64, 65, 80, 81)]
SEP += [(('c80_256wg', 2, 64, 128, 80, 5), (5, 88, 1, 256)), (('c80_512wg', 1, 128, 256, 80, 3), (5, 88, 1, 512)),       # 80 channels: at most 512 workgroups
        (('c80_1024wg', 2, 128, 256, 80, 3), 'unfused'),
        (('c40_368blocks', 1, 184, 256, 40, 3), (3, 40, 1, 46 * 16)), (('c40_384blocks', 1, 192, 256, 40, 3), (3, 40, 2, 24 * 16))]   # two rows per wave from 384 two-row blocks
SEP_IDS = [s[0][0] for s in SEP]

# name, N, H, W, C, k, stride, dil -> expected tiled (forward, backward) with every fast path on; None: the library refuses the launch
DW = [(s, 'any') for s in FK.DW_SHAPES]
DW += [(('c2_%d_c160_k%d' % (N, k), N, 32, 64, 160, k, 1, 1), (True, True)) for N in (2, 1) for k in (3, 5)]
DW += [(('px2047', 1, 23, 89, 40, 3, 1, 1), (False, False)), (('px2048', 1, 32, 64, 40, 3, 1, 1), (True, True)),          # the 2048-pixel floor
       (('stride2', 2, 64, 128, 80, 3, 2, 1), (True, False)),                                                          # tiled backward: stride 1 only
       (('k7', 1, 64, 64, 40, 7, 1, 1), None)]                                                                          # 49 taps: not built
DW_IDS = [s[0][0] for s in DW]


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    fast = lb.addk_get_fast_paths()
    yield lb
    lb.addk_set_fast_paths(fast)


def _src(s, Cc):
    s.x, s.a, s.b, s.ld, s.C, s.relu = PTR['x'], PTR['a'], PTR['b'], Cc, Cc, 1


def _sep_fwd(shape):
    _, N, H, W, Cc, k = shape
    ar = L.SepArgs()
    _src(ar.src, Cc)
    ar.N, ar.H, ar.W, ar.K, ar.Cout, ar.ldw = N, H, W, k, Cc, Cc
    ar.dw_w, ar.pw_w, ar.y, ar.ldy = PTR['w'], PTR['w'] + 0x10000, PTR['y'], Cc
    return ar


def _sep_bwd(shape):
    _, N, H, W, Cc, k = shape
    ba = L.SepBwdArgs()
    ba.dy, ba.lddy, ba.N, ba.H, ba.W, ba.K = PTR['dy'], Cc, N, H, W, k
    _src(ba.src, Cc)
    ba.Cout, ba.ldw, ba.dw_w, ba.pw_w = Cc, Cc, PTR['w'], PTR['w'] + 0x10000
    ba.g, ba.ldg, ba.dab, ba.ws = PTR['g'], Cc, PTR['dab'], PTR['wpack']
    return ba


def _dw(shape):
    _, N, H, W, Cc, k, s, d = shape
    pad = d * (k // 2)
    OH, OW = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
    ar, ba = L.DwArgs(), L.DwBwdArgs()
    for a in (ar, ba):
        _src(a.src, Cc)
        a.N, a.H, a.W, a.OH, a.OW, a.KH, a.KW, a.stride, a.pad, a.dil, a.w = N, H, W, OH, OW, k, k, s, pad, d, PTR['w']
    ar.y, ar.ldy = PTR['y'], Cc
    ba.dy, ba.lddy, ba.g, ba.ldg, ba.dab, ba.dw, ba.ws, ba.defer_wreduce = PTR['dy'], Cc, PTR['g'], Cc, PTR['dab'], PTR['stats'], PTR['wpack'], 1
    return ar, ba, (N * OH * OW, N * H * W)


def _cfg(fn, a):
    cfg = (C.c_int32 * 8)()
    return list(cfg) if fn(C.byref(a), cfg) == 0 else None


def _prepare(lib, what, items):
    arr = (type(items[0]) * len(items))(*items)
    meta = (C.c_int64 * 8)()
    size = getattr(lib, what)(arr, len(items), None, 0, meta)
    return (int(size), list(meta[:5]))


def _key(cfg):
    return cfg[1] << 16 | cfg[2] << 12 | cfg[3] << 4 | cfg[4]


@pytest.mark.parametrize('shape,expect', SEP, ids=SEP_IDS)
def test_sepconv_queries_follow_the_one_choice(lib, shape, expect):
    name, N, H, W, Cc, k = shape
    ar, ba = _sep_fwd(shape), _sep_bwd(shape)
    for mask in MASKS:
        lib.addk_set_fast_paths(mask)
        on = bool(mask & FAST_PW)
        f, b = _cfg(lib.addk_sep_fwd_config, ar), _cfg(lib.addk_sep_bwd_config, ba)
        assert f is not None and b is not None, (name, mask, lib.addk_last_error())
        assert f[1:7] == b[1:7], (name, mask, f, b)                        # one choice: same variant, same tiles, same rows
        covered = f[5] > 0
        if expect is None:
            assert covered, name                                             # every SepConv shape of the GPU kernel tests runs fused
        elif isinstance(expect, str):
            assert covered == (expect == 'fused'), (name, f)
        else:
            assert covered and (f[1], f[2], f[3], f[4], f[5]) == (k,) + expect, (name, f)
        # the mask gates what the library recommends, not the geometry
        assert f[0] == b[0] == int(covered and on), (name, mask, f, b)
        assert int(lib.addk_sep_fwd_supported(C.byref(ar))) == f[0]
        assert int(lib.addk_sep_rows(C.byref(ar))) == f[6] == f[5]
        assert int(lib.addk_sep_bwd_rows(C.byref(ba))) == (b[6] if b[0] else 0)
        for cfg, a, d in ((f, ar, 'fwd'), (b, ba, 'bwd')):
            key = int(getattr(lib, 'addk_sep_%s_batch_key' % d)(C.byref(a)))
            assert key == cfg[7] == (_key(cfg) if cfg[0] else -1), (name, mask, d, key, cfg)
            size, meta = _prepare(lib, 'addk_sep_%s_batch_prepare' % d, [a])         # a direct call runs the fused kernel whatever the mask
            assert (size > 0) == covered, (name, mask, d, size, lib.addk_last_error())
            if covered:
                assert meta[:4] == [_key(cfg), 1, cfg[5], 1], (name, mask, d, meta, cfg)
        if covered:
            assert f[5] == N * -(-H // (4 * f[4])) * -(-W // 16) and f[2] == -(-Cc // 16) and f[3] % 16 == 8 and Cc <= f[3] < Cc + 16
    # the backward's shape query needs neither dy nor the workspace
    lib.addk_set_fast_paths(31)
    ba.dy, ba.ws, ba.g = None, None, None
    assert int(lib.addk_sep_bwd_rows(C.byref(ba))) == _cfg(lib.addk_sep_bwd_config, ba)[6] == f[5]
    assert int(lib.addk_sep_bwd_batch_key(C.byref(ba))) == -1


def test_sepconv_batches_hold_one_variant_and_the_largest_grid(lib):
    lib.addk_set_fast_paths(31)
    big, small, other = ('a', 2, 128, 256, 40, 3), ('b', 1, 192, 256, 40, 3), ('c', 1, 184, 256, 40, 3)       # r = 2 (512), r = 2 (384), r = 1
    for mk, what in ((_sep_fwd, 'addk_sep_fwd_batch_prepare'), (_sep_bwd, 'addk_sep_bwd_batch_prepare')):
        size, meta = _prepare(lib, what, [mk(small), mk(big)])
        assert size > 0 and meta[:4] == [0x33282, 2, 512, 1], (what, size, meta)
        assert _prepare(lib, what, [mk(big), mk(other)])[0] < 0, what
        assert b'mixed kernel variants' in lib.addk_last_error()
        assert _prepare(lib, what, [mk(big), mk(('d', 2, 32, 64, 160, 3))])[0] < 0, what


def test_batch_keys_are_the_parents_and_decode_inverts_encode(lib, tmp_path):
    lib.addk_set_fast_paths(31)
    keys = {}
    for Cc, kp in ((40, 40), (48, 56), (72, 72), (80, 88)):
        for k in (3, 5):
            for N, H, W in ((1, 40, 70), (2, 128, 256)) if Cc < 64 else ((1, 64, 128),):
                f = _cfg(lib.addk_sep_fwd_config, _sep_fwd(('v', N, H, W, Cc, k)))
                assert f[0] == 1 and f[3] == kp and f[7] == _key(f), f
                keys[f[7]] = tuple(f[1:5])
    assert len(keys) == 12
    assert keys[0x33281] == (3, 3, 40, 1) and keys[0x55581] == (5, 5, 88, 1) and keys[0x53282] == (5, 3, 40, 2) and keys[0x35481] == (3, 5, 72, 1)
    # csrc/sep.h itself, on the host: the twelve built variants are these twelve keys, and sep_from_key inverts sep_key
    src = tmp_path / 'sep_keys.cpp'
    src.write_text('#include <stdio.h>\n#include "sep.h"\nint main() {\n'
                   '#define V(KS, KG, KP, R) { SepChoice c{KS, KG, KP, R, 0, 0, 0}; const SepChoice d = sep_from_key(sep_key(c));\\\n'
                   '  if (!sep_is(d, KS, KG, KP, R) || sep_key(d) != sep_key(c)) return 1; printf("%d %d %d %d %d\\n", sep_key(c), KS, KG, KP, R); }\n'
                   '  ADDK_SEP_VARIANTS(V)\n  return 0;\n}\n')
    exe = tmp_path / 'sep_keys'
    subprocess.run(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'auto-dynamic-deeplab_amd', 'csrc'),
                    str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    built = {int(l.split()[0]): tuple(map(int, l.split()[1:])) for l in out.strip().splitlines()}
    assert built == keys


def _set(path, value):
    """a change of an argument block: the field at the dotted `path` becomes `value`, or what `value` makes of (block, old value, channels)"""
    def change(a, Cc):
        *head, leaf = path.split('.')
        for h in head:
            a = a[int(h)] if h.isdigit() else getattr(a, h)
        setattr(a, leaf, value(getattr(a, leaf), Cc) if callable(value) else value)
    return change


def _all(*changes):
    return lambda a, Cc: [ch(a, Cc) for ch in changes]


_off = lambda v, Cc: v + 4                 # four bytes on: no longer 16-byte aligned
_odd = lambda v, Cc: v + 2                 # a row stride that is no multiple of 4 floats
_short = lambda v, Cc: Cc - 4              # a row that does not hold its channels
# what addk_sep_fwd refuses: (name, block, change).  Blocks: 'train' (t, statistics, fused finalize), 'infer' (EPILOGUES[5]: ea and four terms)
FWD_REFUSED = [
    ('a_without_b', 'train', _set('src.b', None)), ('b_without_a', 'train', _set('src.a', None)), ('src_rs_hw', 'train', _set('src.rs_hw', (7 << 16) | 19)),
    ('term0_a_without_b', 'infer', _set('term.0.b', None)), ('term3_b_without_a', 'infer', _set('term.3.a', None)),
    ('term0_rs_hw', 'infer', _set('term.0.rs_hw', (7 << 16) | 19)), ('term2_rs_hw', 'infer', _set('term.2.rs_hw', (7 << 16) | 19)),
    ('y_misaligned', 'train', _set('y', _off)), ('t_misaligned', 'train', _set('t', _off)), ('pw_w_misaligned', 'train', _set('pw_w', _off)),
    ('x_misaligned', 'train', _set('src.x', _off)), ('ea_misaligned', 'infer', _set('ea', _off)), ('eb_misaligned', 'infer', _set('eb', _off)),
    ('term1_x_misaligned', 'infer', _set('term.1.x', _off)),
    ('ldy_mod4', 'train', _set('ldy', _odd)), ('ldt_mod4', 'train', _set('ldt', _odd)), ('ldw_mod4', 'train', _set('ldw', _odd)),
    ('src_ld_mod4', 'train', _set('src.ld', _odd)), ('term1_ld_mod4', 'infer', _set('term.1.ld', _odd)),
    ('ldy_short', 'train', _set('ldy', _short)), ('ldt_short', 'train', _set('ldt', _short)), ('ldw_short', 'train', _set('ldw', _short)),
    ('src_ld_short', 'train', _set('src.ld', _short)), ('term1_ld_short', 'infer', _set('term.1.ld', _short)),
    ('nterm_5', 'infer', _set('nterm', L.MAX_TERMS + 1)), ('nterm_negative', 'infer', _set('nterm', -1)),
    ('term1_other_C', 'infer', _set('term.1.C', _short)), ('ea_without_eb', 'infer', _set('eb', None)),
    ('stats_with_sum_epilogue', 'infer', _all(_set('stats', SR.PTR['stats']), _set('stats_rows', 4096))),
    ('stats_with_ea', 'train', _all(_set('ea', SR.PTR['ea']), _set('eb', SR.PTR['eb']))),
    ('fin_without_counter', 'train', _set('fin_counter', None)), ('fin_without_stats', 'train', _set('stats', None)),
    ('stats_rows_short', 'train', _set('stats_rows', lambda v, Cc: v - 1)),
]
BWD_REFUSED = [
    ('a_without_b', _set('src.b', None)), ('b_without_a', _set('src.a', None)), ('src_rs_hw', _set('src.rs_hw', (7 << 16) | 19)),
    ('g_misaligned', _set('g', _off)), ('dy_misaligned', _set('dy', _off)), ('x_misaligned', _set('src.x', _off)),
    ('lddy_mod4', _set('lddy', _odd)), ('ldg_mod4', _set('ldg', _odd)), ('src_ld_mod4', _set('src.ld', _odd)),
    ('lddy_short', _set('lddy', _short)), ('ldg_short', _set('ldg', _short)), ('ldw_short', _set('ldw', _short)), ('src_ld_short', _set('src.ld', _short)),
    ('no_ws', _set('ws', None)), ('no_dy', _set('dy', None)),
]


def _fwd_block(lib, kind):
    op = SR.CASES[0].op
    if kind == 'infer':
        return op, SR.fwd_args(L, op, SR.PTR, epilogue=5)
    ar = SR.fwd_args(L, op, SR.PTR, t=True, stats_rows=1, fin=True)
    ar.stats_rows = int(lib.addk_sep_rows(C.byref(ar)))           # exactly the launch's rows: one fewer is too few
    return op, ar


def _queries(lib, d, a):
    q = {'batch_key': int(getattr(lib, 'addk_sep_%s_batch_key' % d)(C.byref(a))), 'batch_prepare': _prepare(lib, 'addk_sep_%s_batch_prepare' % d, [a])[0]}
    if d == 'fwd':
        q['supported'] = int(lib.addk_sep_fwd_supported(C.byref(a)))
    return q


@pytest.mark.parametrize('name,kind,change', FWD_REFUSED, ids=[r[0] for r in FWD_REFUSED])
def test_sepconv_forward_refuses_what_its_kernel_cannot_read(lib, name, kind, change):
    """Host only (a refused block never reaches a launch): the unchanged block is supported, has its batch key and prepares; with one field changed
    addk_sep_fwd_supported is 0, the batch key -1 and addk_sep_fwd_batch_prepare fails, alone and as the second member of a batch."""
    lib.addk_set_fast_paths(31)
    op, ar = _fwd_block(lib, kind)
    good = _queries(lib, 'fwd', ar)
    assert good['supported'] == 1 and good['batch_key'] == _key(SR.config(L, lib, ar)) and good['batch_prepare'] > 0, (name, good, lib.addk_last_error())
    _, bad = _fwd_block(lib, kind)
    change(bad, op.C)
    q = _queries(lib, 'fwd', bad)
    assert q['supported'] == 0 and q['batch_key'] == -1 and q['batch_prepare'] < 0, (name, q)
    assert _prepare(lib, 'addk_sep_fwd_batch_prepare', [ar, bad])[0] < 0 and b'launch 1' in lib.addk_last_error(), name
    f = SR.config(L, lib, bad)
    assert f[0] == 0 and f[7] == -1 and tuple(f[1:5]) == SR.CASES[0].variant, (name, f)        # the geometry is still the shape's


@pytest.mark.parametrize('name,change', BWD_REFUSED, ids=[r[0] for r in BWD_REFUSED])
def test_sepconv_backward_refuses_what_its_kernel_cannot_read(lib, name, change):
    """The same for addk_sep_bwd: batch key -1 and a failing addk_sep_bwd_batch_prepare (addk_sep_bwd_rows reads the shape alone and stays)."""
    lib.addk_set_fast_paths(31)
    op = SR.CASES[0].op
    ba = SR.bwd_args(L, op, SR.PTR, accumulate=1)
    good = _queries(lib, 'bwd', ba)
    assert good['batch_key'] == _key(SR.config(L, lib, ba)) and good['batch_prepare'] > 0, (name, good, lib.addk_last_error())
    bad = SR.bwd_args(L, op, SR.PTR, accumulate=1)
    change(bad, op.C)
    q = _queries(lib, 'bwd', bad)
    assert q['batch_key'] == -1 and q['batch_prepare'] < 0, (name, q)
    assert _prepare(lib, 'addk_sep_bwd_batch_prepare', [ba, bad])[0] < 0 and b'launch 1' in lib.addk_last_error(), name
    assert int(lib.addk_sep_bwd_rows(C.byref(bad))) == int(lib.addk_sep_bwd_rows(C.byref(ba))) == 24


def test_sepconv_takes_every_source_form_it_documents(lib):
    """the four forms of addk_src (a, b present or not, relu 0 or 1) on the source and on the terms, g = NULL and dab = NULL: all supported"""
    lib.addk_set_fast_paths(31)
    op = SR.CASES[0].op
    for form in range(4):
        assert _queries(lib, 'fwd', SR.fwd_args(L, op, SR.PTR, form, t=True, stats_rows=64))['supported'] == 1, form
        for g, dab in ((True, True), (True, False), (False, False)):
            assert _queries(lib, 'bwd', SR.bwd_args(L, op, SR.PTR, form, g=g, dab=dab))['batch_prepare'] > 0, (form, g, dab)
    for j in range(len(SR.EPILOGUES)):
        assert _queries(lib, 'fwd', SR.fwd_args(L, op, SR.PTR, epilogue=j))['supported'] == 1, j


def test_no_plan_hands_a_sepconv_a_resampled_or_half_affine_source():
    """Graph.src sets rs_hw only with fold=True, and a and b together or not at all; sep_half, _sep_bwd_args and the sum terms never ask for a fold"""
    import inspect
    src = inspect.getsource(P.Graph.src)
    assert 's.a, s.b = act.bn.a.ptr, act.bn.b.ptr' in src and 'if r is not act.raw' in src
    for fn in (P.Graph.sep_half, P.Graph._sep_bwd_args):
        text = inspect.getsource(fn)
        assert 'self.src(' in text and 'fold' not in text, fn.__name__


@pytest.mark.parametrize('shape,expect', DW, ids=DW_IDS)
def test_depthwise_queries_follow_the_one_choice(lib, shape, expect):
    name, N, H, W, Cc, k, s, d = shape
    ar, ba, pixels = _dw(shape)
    for mask in MASKS:
        lib.addk_set_fast_paths(mask)
        for i, (a, t) in enumerate(((ar, 'fwd'), (ba, 'bwd'))):
            cfg = _cfg(getattr(lib, 'addk_dw_%s_config' % t), a)
            key = int(getattr(lib, 'addk_dw_%s_batch_key' % t)(C.byref(a)))
            size, meta = _prepare(lib, 'addk_dw_%s_batch_prepare' % t, [a])
            if expect is None:
                assert cfg is None and key == -1 and size < 0, (name, mask, t, cfg, key)
                continue
            assert cfg is not None, (name, mask, t, lib.addk_last_error())
            tiled = bool(cfg[0])
            if not mask & FAST_DWTILE:
                assert not tiled, (name, mask, t, cfg)                        # here the mask gates the launch itself
            elif expect != 'any':
                assert tiled == expect[i], (name, mask, t, cfg)
            if tiled:
                assert k in (3, 5) and pixels[i] >= 2048 and (t == 'fwd' or s == 1) and 2 <= cfg[2] <= 16, (name, t, cfg)
            assert cfg[1] == k and cfg[6] == (int(lib.addk_dw_rows(pixels[1], Cc)) if t == 'bwd' else 0), (name, t, cfg)
            assert key == cfg[7] == ((k | 16 * i) if tiled else -1), (name, mask, t, key, cfg)
            assert (size > 0) == tiled, (name, mask, t, size)
            if tiled:
                assert meta == [key, 1, cfg[3], cfg[4], cfg[5]], (name, mask, t, meta, cfg)
    if expect is not None:
        lib.addk_set_fast_paths(31)
        ba.defer_wreduce = 0                       # the batched backward has no per-conv weight reduction
        cfg = _cfg(lib.addk_dw_bwd_config, ba)
        assert cfg[7] == -1 == int(lib.addk_dw_bwd_batch_key(C.byref(ba))) and _prepare(lib, 'addk_dw_bwd_batch_prepare', [ba])[0] < 0


def test_depthwise_batches_hold_one_kernel_size_and_the_largest_grid(lib):
    lib.addk_set_fast_paths(31)
    for i, t in enumerate(('fwd', 'bwd')):
        a3, a5, small = _dw(('x', 2, 32, 64, 160, 3, 1, 1))[i], _dw(('x', 2, 32, 64, 160, 5, 1, 1))[i], _dw(('y', 1, 32, 64, 40, 3, 1, 1))[i]
        c3, cs = (_cfg(getattr(lib, 'addk_dw_%s_config' % t), a) for a in (a3, small))
        size, meta = _prepare(lib, 'addk_dw_%s_batch_prepare' % t, [small, a3])
        assert size > 0 and meta == [3 | 16 * i, 2, max(c3[3], cs[3]), max(c3[4], cs[4]), max(c3[5], cs[5])], (t, meta, c3, cs)
        assert c3[4] > cs[4]                       # 160 channels: several channel groups, 40: one
        assert _prepare(lib, 'addk_dw_%s_batch_prepare' % t, [a3, a5])[0] < 0, t


def test_config2_plans_keep_their_sepconv_and_depthwise_launches(lib, monkeypatch):
    """Launch counts of config 2's dry-built plans (F = 20, f16x3, every fast path on), as measured on the parent commit."""
    L.check(lib.addk_set_conv_precision(1), 'set_conv_precision')
    lib.addk_set_fast_paths(31)
    monkeypatch.setattr(P.Graph, 'run', lambda self, cmds, stream: None)
    monkeypatch.setattr(P, 'require_device', lambda x: None)
    monkeypatch.setattr(P, 'current_stream', lambda: 0)
    from addk.modeling.ADD import ADD

    def counts(train, N):
        m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), ARCH_C2['low_level_layer'])
        m.train(train)
        with torch.set_grad_enabled(train):
            m(torch.empty(N, 3, 1024, 2048))
        g = next(iter(m._plans().values())).g
        return collections.Counter(c.name for c in g.fwd), collections.Counter(c.name for c in g.bwd)
    fwd, bwd = counts(True, 2)
    assert (fwd['sep_fwd'], fwd['sep_fwd_batch'], fwd['dw_fwd'], fwd['dw_fwd_batch']) == (154, 0, 6, 4), fwd
    assert (bwd['sep_bwd'], bwd['sep_bwd_batch'], bwd['dw_bwd'], bwd['dw_bwd_batch']) == (154, 0, 3, 5), bwd
    fwd, bwd = counts(False, 1)
    assert (fwd['sep_fwd'], fwd['sep_fwd_batch'], fwd['dw_fwd'], fwd['dw_fwd_batch']) == (91, 27, 6, 4) and not bwd, fwd
