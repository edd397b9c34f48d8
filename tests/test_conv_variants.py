"""The forward / data-gradient convolution choice against a recorded sweep, and against the kernels that exist, no GPU.  For every launch of
tests/tools/make_conv_dispatch.py's sweep (maps x channel pairs x geometries x both directions x the four arithmetic modes, every fast path on, a
large enough wpack) addk_conv_*_config, addk_conv_*_pack_floats and addk_conv_*_batch_key answer what tests/golden/conv_dispatch.json holds: the
library of the parent of the commit that made the choice resolve its kernel, with only that commit's fp32 column-block fix applied.  The halo-patch
kernels the records name are exactly the ones the units' lookup functions (csrc/conv3b.h c3_variant_fp32, c3b_variant_*, c3n_variant) offer: nothing
instantiated is out of the choice's reach, and the choice reaches nothing that is missing."""
import ctypes as C
import importlib.util
import itertools
import json
import os

import pytest

import addk
from test_conv_dispatch import HALO, SPLIT, SPLIT_S2D, C3N, HALO_KINDS, PTR

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_conv_dispatch', os.path.join(HERE, 'tools', 'make_conv_dispatch.py'))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

with open(os.path.join(HERE, 'golden', 'conv_dispatch.json')) as _f:
    GOLD = json.load(_f)
FWD, DGRAD = 0, 1


class Variant(C.Structure):
    _fields_ = [('fn', C.c_void_p), ('threads', C.c_uint), ('raise_lds', C.c_void_p)]


# lookup -> the values worth asking it for, argument by argument (every instantiated one and its neighbours)
WAVES, KS, WIDTHS, DIRS, PLANES = range(1, 7), (1, 3, 5, 7), (16, 32, 64, 128, 256), (FWD, DGRAD, 2), (1, 2, 3, 4)
LOOKUPS = {
    'c3_variant_fp32': (range(1, 10), KS, DIRS),
    'c3b_variant_tr3': (WAVES, WIDTHS, DIRS, PLANES),
    'c3b_variant_tr5': (WAVES, WIDTHS, DIRS, PLANES),
    'c3b_variant_row': (WAVES, KS, (0, 1), WIDTHS, DIRS, PLANES),
    'c3b_variant_s2f': (WAVES, WIDTHS, PLANES),
    'c3b_variant_s2d': (PLANES,),
    'c3n_variant': (KS, DIRS, PLANES),
}


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    lb.addk_set_split_min_channels(0)
    for name, domain in LOOKUPS.items():
        getattr(lb, name).restype, getattr(lb, name).argtypes = Variant, [C.c_int] * len(domain)
    yield lb
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


@pytest.fixture(scope='module')
def records(lib):
    return tool.sweep(lib, PTR)


def _planes(mode, Cn):
    """conv3.hip c3_planes: fp16 planes (2) in f16x3 and in tail_x3's >= 192-channel launches, bf16 planes (3) otherwise"""
    return {'f16x3': 2, 'bf16x6': 3, 'tail_x3': 2 if Cn >= 192 else 3}[mode]


def _variant(shape, t, mode, rec):
    """(lookup, arguments) of the kernel a record names; None for a kind without a lookup"""
    _, N, H, W, Cs, Cout, k, s, pad, d, rs, lazy = shape
    kind, v, di = rec[0], rec[1:5], FWD if t == 'fwd' else DGRAD
    if kind == HALO:
        return 'c3_variant_fp32', (v[0], v[1], di)
    if kind not in HALO_KINDS:
        return None
    np_ = _planes(mode, Cout if t == 'fwd' else Cs[0])
    if kind == SPLIT_S2D:
        assert v[0] == np_, (shape[0], t, mode, rec)
        return 'c3b_variant_s2d', (np_,)
    if kind == C3N:
        assert v[1] == np_, (shape[0], t, mode, rec)
        return 'c3n_variant', (v[0], di, np_)
    assert kind == SPLIT
    if v[3] == 2:                           # two-row tiles
        return 'c3b_variant_tr%d' % v[1], (v[0], v[2], di, np_)
    if s == 2:
        return 'c3b_variant_s2f', (v[0], v[2], np_)
    return 'c3b_variant_row', (v[0], v[1], int(k == 3 and d > 2), v[2], di, np_)


def test_fixture_is_the_tools_sweep():
    assert GOLD['modes'] == tool.MODES and [tuple(m) for m in GOLD['maps']] == tool.MAPS
    assert [tuple(c) for c in GOLD['channels']] == tool.CHANNELS and [tuple(g) for g in GOLD['geometries']] == tool.GEOMETRIES
    assert len(GOLD['launches']) == len(list(tool.launches())) and all(len(e) == len(tool.MODES) for e in GOLD['launches'])
    assert 'fp32 column-block fix' in GOLD['about']
    # what the sweep has to span
    assert {(1, 16, 48), (2, 512, 1024), (2, 63, 127), (2, 125, 253), (1, 33, 65)} <= set(tool.MAPS)
    counts = {c for pair in tool.CHANNELS for c in pair}
    assert {16, 40, 80, 160, 192, 208, 256, 304, 400, 640} <= counts and min(counts) == 16 and max(counts) == 640
    assert {(1, 1, 1), (3, 2, 1), (5, 1, 1), (5, 1, 2)} | {(3, 1, d) for d in (1, 2, 3, 6, 18)} == set(tool.GEOMETRIES)
    seen = {(tuple(s[1:4]), (s[4][0], s[5])) for s, _ in tool.launches()}
    assert {m for m, _ in seen} == set(tool.MAPS) and {c for _, c in seen} == set(tool.CHANNELS)


def test_every_recorded_launch_is_reproduced(records):
    gold = tool.decode(GOLD)
    bad = [(shape[0], t, tool.MODES[m], got[m], want[m]) for (shape, t), got, want in zip(tool.launches(), records, gold)
           for m in range(len(tool.MODES)) if got[m] != want[m]]
    assert not bad, '%d of %d records differ (name, direction, mode, got, recorded), the first: %s' % (len(bad), 4 * len(gold), bad[:5])


def test_the_choice_reaches_exactly_the_instantiated_kernels(lib, records):
    offered = set()
    for name, domain in LOOKUPS.items():
        for args in itertools.product(*domain):
            v = getattr(lib, name)(*args)
            if v.fn:
                assert v.threads in (192, 256, 320) and bool(v.raise_lds) == (name != 'c3_variant_fp32'), (name, args, v.threads)
                offered.add((name, args))
    reached = set()
    for (shape, t), recs in zip(tool.launches(), records):
        for mode, rec in zip(tool.MODES, recs):
            key = _variant(shape, t, mode, rec)
            if key is not None:
                assert getattr(lib, key[0])(*key[1]).fn, ('the choice names a kernel that is not instantiated', shape[0], t, mode, rec)
                reached.add(key)
    assert offered - reached == set(), 'instantiated, never chosen in the sweep: %s' % sorted(offered - reached)
    assert reached == offered
    by = {name: sum(1 for n, _ in offered if n == name) for name in LOOKUPS}
    assert by == {'c3_variant_fp32': 14, 'c3b_variant_tr3': 20, 'c3b_variant_tr5': 20, 'c3b_variant_row': 48, 'c3b_variant_s2f': 2, 'c3b_variant_s2d': 2,
                  'c3n_variant': 4}, by


def test_fp32_5x5_on_wide_heads_takes_a_64_channel_block(lib):
    """1x128x256, 16 -> 256 channels, 5x5: 512 column-block tiles of 128 channels, which only the 3x3 kernel has; it launched nothing before"""
    shape = ('halo5_c256', 1, 128, 256, (16,), 256, 5, 1, 2, 1, 0, True)
    mirror = ('halo5_c256_back', 1, 128, 256, (256,), 16, 5, 1, 2, 1, 0, True)      # its gradient side has 256 channels
    lib.addk_set_fast_paths(31)
    assert lib.addk_set_conv_precision(0) == 0
    for sh, t in ((shape, 'fwd'), (mirror, 'dgrad')):
        rec = tool.record(lib, tool.args_of(sh, t, PTR), t)
        assert rec[:3] == [HALO, 4, 5] and rec[6] == 4 and rec[8] > 0, (sh[0], t, rec)      # 4 tiles per block, 4 column blocks
    rec = tool.record(lib, tool.args_of(shape, 'dgrad', PTR), 'dgrad')
    assert rec[0] not in HALO_KINDS, rec                                                     # a 16-channel gradient stays generic
