"""Host-side choice of the forward / data-gradient convolution kernel (conv.hip conv_choose_*), no GPU: the library is called with aligned
placeholder pointers (nothing is dereferenced before a launch).  For every shape x direction x precision mode x fast-path mask, with and without a
weight-pack workspace: the pack size, the pack descriptor, the batch key and prepare, and addk_conv_fwd_resample_ok agree with the kernel kind
addk_conv_*_config reports.  The shapes of the GPU kernel tests get the kinds those tests rely on, and config 2's train plan only merges pointwise
launches and only packs weights for halo-patch launches."""
import ctypes as C

import pytest
import torch

import addk
import addk.plan as P
from addk import _lib as L
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args
import test_gpu_fast_kernels as FK

MODES = {'fp32': 0, 'f16x3': 1, 'bf16x6': 2, 'tail_x3': 3}
MASKS = [31, 0] + [31 & ~(1 << b) for b in range(5)]
GENERIC, PARITY, STEM0, PW, PWK, K1S, HALO, SPLIT, SPLIT_S2D, C3N = range(10)
HALO_KINDS = (HALO, SPLIT, SPLIT_S2D, C3N)
PTR = {'x': 0x10000000, 'a': 0x11000000, 'b': 0x11001000, 'w': 0x20000000, 'y': 0x30000000, 'stats': 0x40000000,
       'dy': 0x50000000, 'g': 0x60000000, 'dab': 0x70000000, 'wpack': 0x80000000}     # 16-byte aligned, never dereferenced

# name, N, H, W, source channels, Cout, k, stride, pad, dil, rs_hw of the sources (0: plain), lazy affine on the sources
FAST = [(s[0], s[1], s[2], s[3], s[4], s[5], s[7], 1, s[6] * (s[7] // 2), s[6], 0, True) for s in FK.SHAPES]
STEM2 = [(s[0], s[1], s[2], s[3], s[4], s[5], 3, 2, 1, 1, 0, True) for s in FK.S2_SHAPES]
OTHER = [
    ('stem0_even', 2, 70, 126, (3,), 64, 3, 2, 1, 1, 0, False), ('stem0_odd', 1, 65, 129, (3,), 64, 3, 2, 1, 1, 0, False),
    ('classifier', 2, 33, 65, (256,), 19, 1, 1, 0, 1, 0, True), ('classifier_k32', 2, 17, 31, (256,), 32, 1, 1, 0, 1, 0, True),
    ('fr_s2', 2, 64, 64, (24,), 8, 1, 2, 0, 1, 0, True), ('fr_s2_small', 1, 12, 10, (24,), 8, 1, 2, 0, 1, 0, True),
    ('pw40', 2, 63, 127, (40,), 40, 1, 1, 0, 1, 0, True), ('pw80', 1, 64, 128, (80,), 80, 1, 1, 0, 1, 0, True),
    ('glue200', 1, 50, 90, (200,), 40, 1, 1, 0, 1, 0, True), ('glue_cat', 2, 32, 64, (40, 40, 40, 40, 40), 40, 1, 1, 0, 1, 0, True),
    ('pw80_to_256', 2, 32, 64, (80,), 256, 1, 1, 0, 1, 0, True), ('pw40_to_256_small', 2, 16, 32, (40,), 256, 1, 1, 0, 1, 0, True),
    ('rs_pw80', 2, 32, 64, (80,), 40, 1, 1, 0, 1, (16 << 16) | 32, True), ('rs_pwk200', 2, 32, 64, (200,), 40, 1, 1, 0, 1, (64 << 16) | 128, True),
    ('rs_pw80_to_256', 2, 32, 64, (80,), 256, 1, 1, 0, 1, (31 << 16) | 63, True),
    ('dense3_s2', 2, 97, 129, (48,), 96, 3, 2, 1, 1, 0, True), ('tiny', 1, 9, 11, (20,), 24, 3, 1, 1, 1, 0, True)]
ALL = FAST + STEM2 + OTHER


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    yield lb
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


def _geom(shape):
    _, N, H, W, Cs, Cout, k, s, pad, d, rs, lazy = shape
    return N, H, W, (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1


def _fwd(shape):
    _, N, H, W, Cs, Cout, k, s, pad, d, rs, lazy = shape
    N, H, W, OH, OW = _geom(shape)
    ar = L.ConvArgs()
    off = 0
    for i, Ci in enumerate(Cs):
        ld = 4 if Ci == 3 else Ci
        ar.src[i].x, ar.src[i].ld, ar.src[i].C, ar.src[i].relu, ar.src[i].rs_hw = PTR['x'] + 0x100000 * i, ld, Ci, int(lazy), rs
        if lazy:
            ar.src[i].a, ar.src[i].b = PTR['a'] + 16 * off, PTR['b'] + 16 * off
        off += Ci
    ar.nsrc = len(Cs)
    ar.N, ar.H, ar.W, ar.OH, ar.OW, ar.KH, ar.KW, ar.stride, ar.pad, ar.dil, ar.Cout = N, H, W, OH, OW, k, k, s, pad, d, Cout
    ar.ldw, ar.cin_total, ar.w_choff, ar.ldy = k * k * off, off, 0, Cout
    ar.w, ar.y, ar.stats, ar.stats_ld = PTR['w'], PTR['y'], PTR['stats'], Cout
    return ar


def _dgrads(shape):
    _, N, H, W, Cs, Cout, k, s, pad, d, rs, lazy = shape
    N, H, W, OH, OW = _geom(shape)
    ar, out, choff = _fwd(shape), [], 0
    for i, Ci in enumerate(Cs):
        da = L.ConvDgradArgs()
        da.dy, da.lddy, da.Cout = PTR['dy'], Cout, Cout
        da.N, da.H, da.W, da.OH, da.OW, da.KH, da.KW, da.stride, da.pad, da.dil = N, H, W, OH, OW, k, k, s, pad, d
        da.w, da.ldw, da.cin_total, da.w_choff = PTR['w'], ar.ldw, ar.cin_total, choff
        da.dst = ar.src[i]
        da.dst.rs_hw = 0
        da.g, da.ldg, da.accumulate, da.dab = PTR['g'], Ci, 0, PTR['dab']
        out.append(da)
        choff += Ci
    return out


def _config(lib, a):
    cfg = (C.c_int32 * 8)()
    fn = lib.addk_conv_dgrad_config if isinstance(a, L.ConvDgradArgs) else lib.addk_conv_fwd_config
    rc = fn(C.byref(a), cfg)
    return list(cfg) if rc == 0 else None


def _t(a):
    return 'dgrad' if isinstance(a, L.ConvDgradArgs) else 'fwd'


def _check_launch(lib, a, name):
    t = _t(a)
    pf = int(getattr(lib, 'addk_conv_%s_pack_floats' % t)(C.byref(a)))
    for present in (False, True):
        a.wpack, a.wpack_floats = (PTR['wpack'], pf if pf > 0 else 1 << 40) if present else (None, 0)
        cfg = _config(lib, a)
        if cfg is None:                    # a launch the library refuses (a resampled source no pointwise kernel takes), in every form
            assert t == 'fwd' and a.src[0].rs_hw and pf == 0 and not int(lib.addk_conv_fwd_resample_ok(C.byref(a))), name
            continue
        kind = cfg[0]
        assert (kind in HALO_KINDS) == (present and pf > 0), (name, t, present, pf, cfg)
        desc = (C.c_uint8 * int(lib.addk_conv_pack_desc_bytes()))()
        assert (getattr(lib, 'addk_conv_%s_pack_desc' % t)(C.byref(a), desc) == 0) == (kind in HALO_KINDS), (name, t, present, cfg)
        key = int(getattr(lib, 'addk_conv_%s_batch_key' % t)(C.byref(a)))
        assert (key >= 0) == (kind == PW), (name, t, present, key, cfg)
        if key >= 0:
            arr = (type(a) * 1)(a)
            meta = (C.c_int64 * 8)()
            assert getattr(lib, 'addk_conv_%s_batch_prepare' % t)(arr, 1, None, 0, meta) > 0, (name, lib.addk_last_error())
            assert list(meta[:4]) == [key, 1, cfg[5], cfg[6]], (name, t, list(meta[:4]), cfg)
        if t == 'fwd':
            rs = any(a.src[i].rs_hw for i in range(a.nsrc))
            assert int(lib.addk_conv_fwd_resample_ok(C.byref(a))) == int(rs and kind in (PW, PWK)), (name, present, cfg)
    a.wpack, a.wpack_floats = None, 0


@pytest.mark.parametrize('mode', list(MODES))
def test_pack_desc_batch_key_and_resample_follow_the_kind(lib, mode):
    L.check(lib.addk_set_conv_precision(MODES[mode]), 'set_conv_precision')
    for mask in MASKS:
        lib.addk_set_fast_paths(mask)
        for shape in ALL:
            for a in [_fwd(shape)] + _dgrads(shape):
                _check_launch(lib, a, (shape[0], mask))


def _kinds(lib, shape, mode, mask=31):
    """config of the forward and of each data gradient, every launch given the workspace its pack size asks for"""
    L.check(lib.addk_set_conv_precision(MODES[mode]), 'set_conv_precision')
    lib.addk_set_fast_paths(mask)
    out = []
    for a in [_fwd(shape)] + _dgrads(shape):
        pf = int(getattr(lib, 'addk_conv_%s_pack_floats' % _t(a))(C.byref(a)))
        if pf:
            a.wpack, a.wpack_floats = PTR['wpack'], pf
        out.append(_config(lib, a))
    return out


@pytest.mark.parametrize('mode', ['f16x3', 'bf16x6'])
def test_gpu_test_shapes_get_their_kinds(lib, mode):
    for shape in FAST:
        fwd, dgrads = _kinds(lib, shape, mode)[0], _kinds(lib, shape, mode)[1:]
        name = shape[0]
        if name.startswith('n16_'):
            assert fwd[0] == C3N, (name, fwd)
        elif name.startswith('l3_'):
            assert fwd[0] == SPLIT and fwd[3] == 32, (name, fwd)          # quarter-width tiles
        elif name.startswith('pw_'):
            assert fwd[0] == SPLIT and fwd[2] == 1, (name, fwd)           # the split kernel as a 1x1 GEMM
        else:
            assert fwd[0] in (SPLIT, C3N), (name, fwd)
        for Ci, cfg in zip(shape[4], dgrads):                           # a gradient of fewer than 32 channels stays on the generic kernel
            assert (cfg[0] in (SPLIT, C3N)) == (Ci >= 32), (name, Ci, cfg)
    for shape in STEM2:
        fwd, dgrads = _kinds(lib, shape, mode)[0], _kinds(lib, shape, mode)[1:]
        assert fwd[0] == SPLIT and fwd[1] == 4 and fwd[3] == 64, (shape[0], fwd)     # stride-2 forward: 4-wave blocks, 64-pixel tiles
        if shape[0].startswith('stem2'):
            assert [c[0] for c in dgrads] == [SPLIT_S2D], (shape[0], dgrads)
    for shape in ALL:
        if shape[0].startswith('stem0'):
            assert _kinds(lib, shape, mode)[0][0] == STEM0, shape[0]
        if shape[0].startswith('classifier'):
            assert _kinds(lib, shape, mode)[1][0] == K1S, shape[0]
        if shape[0].startswith('fr_s2'):
            assert _kinds(lib, shape, mode)[1][0] == PARITY, shape[0]
    assert _kinds(lib, OTHER[4], mode)[1][7] == 1 and _kinds(lib, OTHER[5], mode)[1][7] == 4      # one launch for all classes / one per class


def test_fp32_mode_takes_the_fp32_halo_kernel(lib):
    for shape in FAST:
        if shape[0].startswith(('pw_', 'l3_')):
            continue                        # split-kernel shapes only (a 1x1, a map below the fp32 halo kernel's floor)
        for Ci, cfg in zip((shape[5],) + shape[4], _kinds(lib, shape, 'fp32')):
            assert (cfg[0] == HALO) == (Ci >= 32), (shape[0], Ci, cfg)
        for cfg in _kinds(lib, shape, 'fp32', mask=31 & ~2):
            assert cfg[0] not in HALO_KINDS, (shape[0], cfg)


def test_train_plan_merges_pointwise_launches_and_packs_halo_launches(lib, monkeypatch):
    """config 2's train plan at 2x1024x2048 (F = 20) in f16x3: every member of a merged conv batch would take the pointwise kernel with the
    batch's key on its own, and every hoisted weight pack belongs to a launch that takes a halo-patch kernel."""
    L.check(lib.addk_set_conv_precision(1), 'set_conv_precision')
    lib.addk_set_fast_paths(31)
    monkeypatch.setattr(P.Graph, 'run', lambda self, cmds, stream: None)
    monkeypatch.setattr(P, 'require_device', lambda x: None)
    monkeypatch.setattr(P, 'current_stream', lambda: 0)
    batches, packs = [], []
    prepare, hoist = P.Graph._prepare, P.Graph._hoist_pack

    def spy_prepare(self, prep, arr, n, what):
        blob, meta = prepare(self, prep, arr, n, what)
        batches.append((what, [arr[i] for i in range(n)], list(meta)))
        return blob, meta

    def spy_hoist(self, desc_fn, args, weight, wpk, create):
        n0 = len(self._packs)
        hoist(self, desc_fn, args, weight, wpk, create)
        if len(self._packs) > n0:
            packs.append(type(args).from_buffer_copy(args))
    monkeypatch.setattr(P.Graph, '_prepare', spy_prepare)
    monkeypatch.setattr(P.Graph, '_hoist_pack', spy_hoist)
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), ARCH_C2['low_level_layer'])
    m.train()
    m(torch.empty(2, 3, 1024, 2048))
    plan = next(iter(m._plans().values()))
    conv = [(what, members, meta) for what, members, meta in batches if what.startswith('addk_conv_')]
    assert conv, 'the plan merged no conv launches'
    for what, members, meta in conv:
        cfgs = [_config(lib, a) for a in members]
        assert all(c[0] == PW for c in cfgs), (what, cfgs)
        keys = {int(getattr(lib, 'addk_conv_%s_batch_key' % _t(a))(C.byref(a))) for a in members}
        assert keys == {meta[0]}, (what, keys, meta[:4])
        assert meta[2:4] == [max(c[5] for c in cfgs), max(c[6] for c in cfgs)], (what, meta[:4])
    for a in packs:
        assert _config(lib, a)[0] in HALO_KINDS, _t(a)
    assert len(plan.g._packs) == len(packs) == 113
