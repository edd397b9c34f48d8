"""Host-side choice of the resize backward kernels (csrc/resize.hip rs_choose_bwd), no GPU: the library is called with aligned placeholder
pointers (nothing is dereferenced before a launch).  For every shape x fast-path mask: addk_resize_bwd_batch_key and the meta of a
one-item batch prepare are what the parent commit's library answered (tests/golden/resize_dispatch.json, written by
tests/tools/make_resize_dispatch.py) and agree with what addk_resize_bwd_config reports; the rules of the choice (the x2 / x4 / x8 edges,
the pixel lanes, alignment, the 1024-channel slices, the NCHW tile fit) are pinned by the kind each shape takes; rejected argument
structs have key -1; config 2's dry-built plans keep their launch counts."""
import collections
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch

import addk
import addk.plan as P
from addk import _lib as L
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args
from test_conv_dispatch import MASKS, PTR

HERE = os.path.dirname(os.path.abspath(__file__))
FAST_DWTILE = 8

_spec = importlib.util.spec_from_file_location('make_resize_dispatch', os.path.join(HERE, 'tools', 'make_resize_dispatch.py'))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)
NHWC, TAB, NCHW, TILE = tool.NHWC, tool.TAB, tool.NCHW, tool.TILE

with open(os.path.join(HERE, 'golden', 'resize_dispatch.json')) as _f:
    GOLD = json.load(_f)


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    fast = lb.addk_get_fast_paths()
    yield lb
    lb.addk_set_fast_paths(fast)


def _cfg(lib, ba):
    cfg = (C.c_int32 * 8)()
    return list(cfg) if lib.addk_resize_bwd_config(C.byref(ba), cfg) == 0 else None


def test_fixture_lists_the_tools_shapes_and_masks():
    assert GOLD['masks'] == MASKS
    assert [(k, v['shape']) for k, v in GOLD['shapes'].items()] == [(s[0], list(s[1:8])) for s in tool.SHAPES]
    assert all(sorted(v['masks']) == sorted(str(m) for m in MASKS) for v in GOLD['shapes'].values())


@pytest.mark.parametrize('shape', tool.SHAPES, ids=tool.IDS)
def test_resize_backward_queries_follow_the_one_choice(lib, shape):
    name, N, Cc, H, W, OH, OW, ld, kind31, taps31 = shape
    ba = tool.bwd_args(L, shape, PTR)
    for mask in MASKS:
        lib.addk_set_fast_paths(mask)
        gold = GOLD['shapes'][name]['masks'][str(mask)]
        got = tool.record(lib, ba)
        assert got == gold, (name, mask, got, gold)                       # key and one-item prepare: the parent's
        key, meta = got['key'], got['meta']
        cfg = _cfg(lib, ba)
        assert cfg is not None, (name, mask, lib.addk_last_error())
        assert cfg[7] == key and (cfg[0] == TAB) == (key >= 0) == (got['size'] > 0), (name, mask, cfg, got)
        if key >= 0:
            assert (cfg[1], cfg[2], cfg[4]) == (meta[0], meta[2], meta[3]) and key == cfg[1] and meta[1] == 1, (name, mask, cfg, meta)
            assert 1 <= cfg[5] <= min(W, 128) and cfg[3] == 1, (name, cfg)
        else:
            assert cfg[1] == 0 and cfg[5] == 0, (name, mask, cfg)
        if not mask & FAST_DWTILE:
            assert cfg[0] in (NHWC, NCHW), (name, mask, cfg)               # the mask gates the launch itself, table-driven and tiled alike
        else:
            assert (cfg[0], cfg[1]) == (kind31, taps31), (name, mask, cfg)
        assert (cfg[0] in (NCHW, TILE)) == (ld < 0), (name, cfg)
        assert cfg[6] == (-(-Cc // 1024) if ld >= 0 else 1), (name, cfg)   # a sliced launch reports its first slice
        if cfg[0] == TILE:
            assert (cfg[2], cfg[3], cfg[4]) == (N * -(-H // 8) * -(-W // 8), Cc, 0), (name, cfg)
        elif cfg[0] == NHWC:
            assert cfg[2] == int(lib.addk_ew_rows(N * H * W, min(Cc, 1024))), (name, cfg)


def test_rejected_argument_structs_have_no_key_and_no_config(lib):
    """What addk_resize_bwd refuses with an error has key -1 (no error from the key: the plan asks it of every launch) and fails the query."""
    lib.addk_set_fast_paths(31)
    shape = tool.SHAPES[0]
    good = tool.bwd_args(L, shape, PTR)
    assert _cfg(lib, good) is not None and int(lib.addk_resize_bwd_batch_key(C.byref(good))) == 5

    def broken(edit):
        ba = tool.bwd_args(L, shape, PTR)
        edit(ba)
        return ba
    for what, ba in (('null dy', broken(lambda a: setattr(a, 'dy', None))), ('ldg < C', broken(lambda a: setattr(a, 'ldg', shape[2] - 4))),
                     ('a without b', broken(lambda a: setattr(a.src, 'b', None)))):
        assert int(lib.addk_resize_bwd_batch_key(C.byref(ba))) == -1, what
        cfg = (C.c_int32 * 8)()
        assert lib.addk_resize_bwd_config(C.byref(ba), cfg) != 0 and lib.addk_last_error().startswith(b'resize_bwd: '), what
        assert tool.prepare(lib, [good, ba])[0] < 0, what                  # a rejected item fails the batch like any item off the table-driven kernel
    assert lib.addk_resize_bwd_config(C.byref(good), None) != 0


def test_resize_batches_hold_one_variant_and_the_largest_grid(lib):
    lib.addk_set_fast_paths(31)
    by = {s[0]: tool.bwd_args(L, s, PTR) for s in tool.SHAPES}
    a, b, other = by['up_32_63'], by['fit_128_125'], by['up4_c160']
    ca, cb = _cfg(lib, a), _cfg(lib, b)
    size, meta = tool.prepare(lib, [a, b])
    assert size == 2 * tool.prepare(lib, [a])[0] and meta == [5, 2, max(ca[2], cb[2]), max(ca[4], cb[4])], (size, meta, ca, cb)
    assert tool.prepare(lib, [a, other])[0] < 0 and b'mixed kernel variants' in lib.addk_last_error()
    assert tool.prepare(lib, [a, by['oh_8h2']])[0] < 0 and b'does not run on the batched kernel' in lib.addk_last_error()


def test_config2_plans_keep_their_resize_launches(lib, monkeypatch):
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
    assert (fwd['resize_fwd'], fwd['resize_nchw']) == (5, 2), fwd
    assert (bwd['resize_bwd'], bwd['resize_bwd_batch'], bwd['resize_nchw_bwd']) == (14, 8, 2), bwd
    fwd, bwd = counts(False, 1)
    assert (fwd['resize_fwd'], fwd['resize_nchw']) == (5, 2) and not bwd, fwd
