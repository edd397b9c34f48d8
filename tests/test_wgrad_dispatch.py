"""Host-side choice of the weight-gradient kernel (csrc/wgrad.hip: wg_choose, wg_fill and the dispatch over the kernel families in
wgrad_pix.hip, wgrad_h3.hip, wgrad_hk.hip and wgrad_rs.hip), no GPU: the library is called with aligned placeholder pointers (nothing is
dereferenced before a launch).  For every shape x precision mode x fast-path mask: the launch key addk_conv_wgrad_config reports is the one a
batch of that conv carries, and a workspace of exactly addk_conv_wgrad_ws floats passes the checked batch prepare.  The shapes of the GPU
kernel tests get the kinds those tests assert, and every (case, mode) of the bit-for-bit fixture (tests/tools/make_wgrad_bits.py) its launch key.
The mixed batches of the fp64 test (tests/_wgrad_ref.BATCHES, tests/test_gpu_wgrad_fp64.py) get their keys member by member and as a whole, and a
batch prepared for a split-precision kernel is refused, not launched, once the precision mode has changed."""
import ctypes as C
import importlib.util
import os

import pytest

import _wgrad_ref as R
import addk
from addk import _lib as L

_spec = importlib.util.spec_from_file_location('make_wgrad_bits', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'make_wgrad_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

MODES = {'fp32': 0, 'f16x3': 1, 'bf16x6': 2, 'tail_x3': 3}
PTR = {'dy': 0x10000000, 'x': 0x20000000, 'a': 0x30000000, 'b': 0x30001000, 'dw': 0x40000000, 'ws': 0x50000000}      # 16-byte aligned

# name, N, H, W, Ci, Cout, k, stride, dil: the register-streaming / few-channel cases of
# test_gpu_fast_kernels.test_register_streaming_wgrad_matches_fp64_reference
RS_SHAPES = [
    ('pw40', 2, 63, 127, 40, 40, 1, 1, 1), ('pw80', 1, 64, 128, 80, 80, 1, 1, 1), ('glue200', 1, 50, 90, 200, 40, 1, 1, 1),
    ('reduce_s2', 2, 128, 96, 80, 40, 1, 2, 1), ('dense3_s2', 2, 97, 129, 48, 96, 3, 2, 1), ('pw160', 2, 32, 64, 160, 160, 1, 1, 1),
    ('stem0_like', 2, 256, 511, 3, 64, 3, 2, 1)]
# test_gpu_round5.test_wide_pointwise_weight_gradient_with_128_outputs: 1x1, C -> 128
WIDE_PW_SHAPES = [('c320_o128', 2, 64, 128, 320, 128, 1, 1, 1), ('c200_o128_odd', 1, 70, 130, 200, 128, 1, 1, 1),
                  ('c400_o256', 2, 64, 128, 400, 256, 1, 1, 1)]
# the 3x3 / 5x5 halo cases of test_gpu_fast_kernels.SHAPES, one entry per source
HALO_SHAPES = [
    ('two_src_d1_s0', 1, 40, 256, 32, 128, 3, 1, 1), ('two_src_d1_s1', 1, 40, 256, 16, 128, 3, 1, 1),
    ('odd_tail_d2', 2, 33, 129, 24, 64, 3, 1, 2), ('aspp_like_d6', 1, 70, 128, 48, 256, 3, 1, 6),
    ('wide_blocks_d1', 2, 64, 256, 32, 256, 3, 1, 1), ('max_dil_d18', 1, 64, 128, 16, 64, 3, 1, 18),
    ('tworow_odd', 2, 65, 300, 24, 128, 3, 1, 1), ('tworow_c64', 1, 129, 200, 32, 64, 3, 1, 1),
    ('cell_dil5_40', 1, 70, 125, 40, 40, 5, 1, 2), ('cell_dil5_80', 2, 63, 127, 80, 80, 5, 1, 2),
    ('cell_dil3_40', 1, 70, 125, 40, 40, 3, 1, 2), ('cell_dil3_160', 2, 40, 104, 32, 160, 3, 1, 2),
    ('n16_two_src_s0', 2, 33, 200, 24, 48, 5, 1, 2), ('n16_two_src_s1', 2, 33, 200, 16, 48, 5, 1, 2),
    ('n16_k8_d1', 2, 40, 130, 8, 40, 5, 1, 1), ('n16_c36', 1, 90, 100, 36, 36, 5, 1, 2),
    ('l3_dil5_160', 2, 32, 64, 48, 160, 5, 1, 2), ('l3_dil3_160', 2, 32, 64, 32, 160, 3, 1, 2)]
# the other kinds: the network's wide heads (output-split), 80- and 64-channel 1x1s, stem1, a strided dense conv, a small map
OTHER_SHAPES = [
    ('head_1x1_256', 2, 64, 128, 256, 256, 1, 1, 1), ('pw80_small', 2, 16, 32, 80, 80, 1, 1, 1), ('pw64_small', 2, 16, 32, 64, 64, 1, 1, 1),
    ('stem1', 2, 256, 512, 64, 64, 3, 1, 1), ('stem2_s2', 2, 256, 512, 64, 128, 3, 2, 1), ('tiny', 1, 9, 11, 20, 24, 3, 1, 1)]
ALL_SHAPES = RS_SHAPES + WIDE_PW_SHAPES + HALO_SHAPES + OTHER_SHAPES


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    yield lb
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


def _args(lb, shape):
    _, N, H, W, Ci, Cout, k, s, d = shape
    pad = d * (k // 2)
    OH, OW = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
    wa = L.ConvWgradArgs()
    wa.dy, wa.lddy, wa.Cout = PTR['dy'], Cout, Cout
    wa.N, wa.H, wa.W, wa.OH, wa.OW, wa.KH, wa.KW, wa.stride, wa.pad, wa.dil = N, H, W, OH, OW, k, k, s, pad, d
    wa.src.x, wa.src.a, wa.src.b, wa.src.ld, wa.src.C, wa.src.relu = PTR['x'], PTR['a'], PTR['b'], Ci, Ci, 1
    wa.dw, wa.ldw, wa.cin_total, wa.w_choff, wa.accumulate = PTR['dw'], k * k * Ci, Ci, 0, 0
    wa.ws, wa.ws_floats = PTR['ws'], lb.addk_conv_wgrad_ws(N * OH * OW, Cout, Ci, k * k)
    return wa


def _config(lb, wa):
    cfg = (C.c_int32 * 4)()
    L.check(lb.addk_conv_wgrad_config(C.byref(wa), cfg), 'conv_wgrad_config')
    return list(cfg)


@pytest.mark.parametrize('fast', [31, 0])
@pytest.mark.parametrize('mode', list(MODES))
def test_config_key_matches_batch_and_workspace_bound_suffices(lib, mode, fast):
    L.check(lib.addk_set_conv_precision(MODES[mode]), 'set_conv_precision')
    lib.addk_set_fast_paths(fast)
    for shape in ALL_SHAPES:
        wa = _args(lib, shape)
        cfg = _config(lib, wa)
        arr = (L.ConvWgradArgs * 1)(wa)
        meta = (C.c_int64 * 8)()
        size = lib.addk_conv_wgrad_batch_prepare(arr, 1, None, 0, meta)
        assert size > 0, (shape[0], lib.addk_last_error())
        assert list(meta[:3]) == cfg[:3], (shape[0], list(meta[:3]), cfg)
        blob = (C.c_uint8 * size)()
        filled = (C.c_int64 * 8)()
        rc = lib.addk_conv_wgrad_batch_prepare(arr, 1, blob, size, filled)      # checked: the workspace holds every slice
        assert rc == size and list(filled) == list(meta), (shape[0], cfg, rc, size)
        assert meta[5] == cfg[3], (shape[0], 'blocks of a one-conv batch with a lone launch\'s budget', meta[5], cfg)


@pytest.mark.parametrize('mode', ['bf16x6', 'f16x3'])
def test_gpu_test_shapes_get_their_kinds(lib, mode):
    L.check(lib.addk_set_conv_precision(MODES[mode]), 'set_conv_precision')
    for fast in (31, 0):
        lib.addk_set_fast_paths(fast)
        for shape in RS_SHAPES:
            kind = _config(lib, _args(lib, shape))[0]
            assert (kind == (8 if shape[4] <= 4 else 6)) == (fast == 31), (shape[0], fast, kind)
    lib.addk_set_fast_paths(31)
    for shape in WIDE_PW_SHAPES:
        assert _config(lib, _args(lib, shape))[:3] == [9, 8, 4], shape[0]


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6', 'f16x3'])
def test_halo_shapes_get_halo_kinds(lib, mode):
    for fast, m in ((31, mode), (0, 'fp32')):          # the fast launch in each mode, the generic one in fp32
        L.check(lib.addk_set_conv_precision(MODES[m]), 'set_conv_precision')
        lib.addk_set_fast_paths(fast)
        for shape in HALO_SHAPES:
            _, N, H, W, Ci, Cout, k, s, d = shape
            if shape[0].startswith('l3_') and m == 'fp32':
                continue                                # below the fp32 halo kernel's floor: a split-kernel launch shape only
            kind = _config(lib, _args(lib, shape))[0]
            if Ci >= 16 and k == 3 and Cout % 64 == 0:
                assert (kind == 5) == bool(fast & 4), (shape[0], fast, kind)
            elif Ci >= 16 and Cout <= 160 and d <= 2:
                assert (kind == 7) == bool(fast & 16), (shape[0], fast, kind)


def test_bit_fixture_cases_get_their_launch_keys(lib):
    """Every (case, mode) of tests/tools/make_wgrad_bits.CASES gets the (kind, cty, ctz) it lists, and between them the cases reach every
    kernel family, NT and NG in {1, 2} of the halo kernels in both split modes (NP = 2 and 3), the three tap / tile forms of the cells'
    halo kernels, the four lane layouts of the register-streaming kernel, and kind 9 in the split modes only."""
    seen = set()
    for case in bits.CASES:
        lib.addk_set_fast_paths(case[2])
        for mode, key in case[5].items():
            L.check(lib.addk_set_conv_precision(bits.MODES[mode]), 'set_conv_precision')
            wa = bits.wgrad_args(L, case, PTR)
            assert tuple(_config(lib, wa)[:3]) == key, (case[0], mode)
            seen.add((mode,) + key)
        assert set(case[5]) == set(bits.MODES) or case[5][next(iter(case[5]))][0] == 9, case[0]
    want = {(m, 0, 2, 1) for m in bits.MODES} | {(m, 0, 3, 3) for m in bits.MODES} | {(m, k, t, u) for m in bits.MODES for k, t, u in ((1, 8, 4), (2, 6, 6), (3, 4, 4), (8, 4, 2))}
    want |= {('fp32', 5, 4, 1), ('fp32', 5, 8, 1)} | {(m, 5, t, g) for m in ('f16x3', 'bf16x6') for t in (4, 8) for g in (1, 2)}
    want |= {(m, 9, 8, 4) for m in ('f16x3', 'bf16x6')}
    want |= {(m, 7, t, k) for m in bits.MODES for t, k in ((3, 3), (3, 5), (5, 3))} | {(m, 6, la, lb) for m in bits.MODES for la in (3, 4) for lb in (3, 4)}
    assert want <= seen, sorted(want - seen)


def _prepare(lib, ops):
    """(meta, host blob) of a checked batch prepare of `ops` (tests/_wgrad_ref.Op) on placeholder pointers, exact workspaces"""
    arr = (L.ConvWgradArgs * len(ops))(*[R.wgrad_args(L, op, PTR, lib.addk_conv_wgrad_ws(op.N * op.OH * op.OW, op.Cout, op.C, op.k * op.k)) for op in ops])
    meta = (C.c_int64 * 8)()
    size = lib.addk_conv_wgrad_batch_prepare(arr, len(ops), None, 0, meta)
    assert size > 0, lib.addk_last_error()
    blob = (C.c_uint8 * size)()
    assert lib.addk_conv_wgrad_batch_prepare(arr, len(ops), blob, size, meta) == size, lib.addk_last_error()
    return meta, blob


@pytest.mark.parametrize('mode', list(MODES))
def test_mixed_batches_of_the_fp64_test_get_their_keys(lib, mode):
    """Every member of tests/_wgrad_ref.BATCHES, with the strides, source form and weight slice the GPU test gives it, gets its batch's key in
    every mode (tail_x3: the split modes' key), and so does meta[:3] of a checked prepare of the whole batch with workspaces of exactly
    addk_conv_wgrad_ws floats.  The h1 batch exists in the split modes only; in fp32 its members fall to other kernels."""
    L.check(lib.addk_set_conv_precision(MODES[mode]), 'set_conv_precision')
    assert len(R.BATCHES) == 18
    for batch in R.BATCHES:
        name, fast, keys, shapes = batch
        key = keys.get('f16x3' if mode == 'tail_x3' else mode)
        lib.addk_set_fast_paths(fast)
        ops = R.batch_ops(batch)
        assert [(op.form, op.accumulate) for op in ops] == [(i % 4, i % 2) for i in range(len(ops))]
        got = [tuple(_config(lib, R.wgrad_args(L, op, PTR))[:3]) for op in ops]
        if key is None:
            assert name == 'h1' and mode == 'fp32' and all(g[0] != 9 for g in got), (name, mode, got)
            continue
        assert got == [key] * len(ops), (name, mode, got)
        meta, _ = _prepare(lib, ops)
        assert tuple(meta[:3]) == key and meta[3] == len(ops), (name, mode, list(meta))


def test_batch_members_cover_what_the_table_promises(lib):
    """The properties the batches are there for: mixed tap counts under the keys without taps, n >= 4, a kind-6 member with 9 pixel slices,
    members without 16-byte loads, odd strides and slice offsets, and every source form and both accumulate flags among the members."""
    by = {b[0]: R.batch_ops(b) for b in R.BATCHES}
    for name in ('rs33', 'os1', 'os2', 'os3', 'pix33', 'pix21'):
        assert len({op.k for op in by[name]}) > 1, name
    assert all(len(by[name]) >= 4 for name in ('rs33', 'os2', 'pix33'))
    op = by['rs33'][3]
    P = op.N * op.OH * op.OW
    assert -(-P // 2048) == 9
    odd = [op for op in by['pix33'] if op.C % 4]
    assert len(odd) == 2 and all(op.ld % 2 and op.w_choff % 2 and op.Cout % 4 for op in odd)
    assert {(op.form, op.accumulate) for ops in by.values() for op in ops} == {(0, 0), (1, 1), (2, 0), (3, 1)}
    assert any(op.ld > op.C and op.lddy > op.Cout for ops in by.values() for op in ops)
    # the wave reduction (one block per 64 weights) and the block reduction (one per 256) in one batch: the reduce work list is longer than
    # with the block form alone and shorter than with the wave form alone
    lib.addk_set_fast_paths(31)
    L.check(lib.addk_set_conv_precision(MODES['f16x3']), 'set_conv_precision')
    for name in ('h3_41', 'h3_81', 'h3_8x', 'hk33', 'hk35', 'h1'):
        ne = [op.Cout * op.k * op.k * op.C for op in by[name]]
        meta, _ = _prepare(lib, by[name])
        assert sum(-(-v // 256) for v in ne) < meta[7] < sum(-(-v // 64) for v in ne), (name, list(meta))


@pytest.mark.parametrize('shape,key', [((1, 70, 130, 200, 128, 1, 1, 1), (9, 8, 4)), ((1, 40, 256, 32, 128, 3, 1, 1), (5, 8, 2))], ids=['h1', 'h3_ng2'])
def test_batch_of_a_split_only_kernel_is_refused_after_a_mode_change(lib, shape, key):
    """A batch prepared in f16x3 for a geometry only the split-precision kernels have is refused in fp32 before anything is launched or
    dereferenced (wg_variant): the blob stays on the host and its pointers are placeholders."""
    lib.addk_set_fast_paths(31)
    L.check(lib.addk_set_conv_precision(MODES['f16x3']), 'set_conv_precision')
    meta, blob = _prepare(lib, [R.make_op(shape, 1)])
    assert tuple(meta[:3]) == key
    L.check(lib.addk_set_conv_precision(MODES['fp32']), 'set_conv_precision')
    rc = lib.addk_conv_wgrad_batch_run(C.cast(blob, C.c_void_p), meta, None)
    assert rc == -1 and b'precision mode changed' in lib.addk_last_error(), (rc, lib.addk_last_error())
