"""Host-logic tests (CPU, no GPU) of multi-scale + flip sliding windows: the C ABI of addk_gather_tile_views and of the tiled multi-view
label head, the integer membership test, the fp32-against-fp64 check of the torch formula that tests/test_gpu_tile_views.py holds the
kernel to, the formula's sensitivity to four deliberate mistakes, the per-call launches of segment.TiledSegmenter with views, and its
error paths.  Launches are stubbed as in tests/test_tiles_plan.py.

The reference check (tests/_tile_views_ref.py): tau = 64 * e32 per case; the test prints e32 and the excused share of every case and
asserts the cap of 0.2 % for the fp32 formula alone."""
import collections
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import addk
from addk import _lib as L
from addk.segment import tile_starts, view_size
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)
import _tile_views_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (3, 3, 65, 129)
STRIDE = (32, 71)


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer']).eval()


# ---------------- ABI ----------------
def _args(C_=19):
    """case `three` over a dummy non-null address (used only where the call is refused before any launch)"""
    a = R.fill_args(L.LabelTileViewsArgs(), 'three', C_)
    a.logits, a.ld, a.lut256, a.labels = 64, 24, None, 64
    return a


def test_tile_views_abi_declared_exported_and_bound():
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in ('addk_gather_tile_views', 'addk_label_tile_views_upsample_supported', 'addk_label_tile_views_upsample'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert int(re.search(r'#define ADDK_MAX_TILES_AXIS (\d+)', src).group(1)) == L.MAX_TILES_AXIS == 16
    assert int(re.search(r'#define ADDK_MAX_VIEWS (\d+)', src).group(1)) == L.MAX_VIEWS == 8
    sup = lib.addk_label_tile_views_upsample_supported                      # (nview, N, OH, OW, C)
    assert sup(6, 2, 40, 70, 19) == 1 and sup(6, 2, 40, 70, 21) == 1 and sup(1, 1, 1, 1, 19) == 1 and sup(8, 1, 500, 500, 21) == 1
    assert set(L.head_classes()) == {19, 21}
    for bad in ((0, 2, 40, 70, 19), (9, 2, 40, 70, 19), (6, 2, 40, 70, 7), (6, 2, 40, 70, 20), (6, 0, 40, 70, 19), (6, 2, 0, 70, 19),
                (6, 2, 40, -1, 19), (6, 65536, 40, 70, 19), (1, 1, 65536 * 16 + 1, 1, 19)):
        assert sup(*bad) == 0, bad
    # refused before anything is launched: needs no device
    assert lib.addk_label_tile_views_upsample(None, None) == -1
    assert lib.addk_label_tile_views_upsample(ctypes.byref(L.LabelTileViewsArgs()), None) == -1
    for edit in R.REFUSALS:
        a = _args()
        edit(a)
        assert lib.addk_label_tile_views_upsample(ctypes.byref(a), None) == -1, edit.what
    assert 'label_tile_views_upsample' in lib.addk_last_error().decode()
    # addk_gather_tile_views(table, ntiles, Cin, th, tw, x, B): addk_gather_tiles' refusals
    for bad in ((None, 1, 3, 8, 8, 64, 2), (64, 1, 3, 8, 8, None, 2), (None, 0, 3, 8, 8, None, 2), (64, 3, 3, 8, 8, 64, 2), (64, -1, 3, 8, 8, 64, 2),
                (64, 1, 0, 8, 8, 64, 2), (64, 1, 3, 0, 8, 64, 2), (64, 1, 3, 8, -2, 64, 2), (64, 0, 3, 8, 8, 64, 0)):
        assert lib.addk_gather_tile_views(*bad, None) == -1, bad
    assert 'gather_tile_views' in lib.addk_last_error().decode()


def test_tile_views_struct_layouts_match_header(tmp_path):
    structs = {'addk_tile_view_desc': 'TileViewDesc', 'addk_tile_view': 'TileView', 'addk_label_tile_views_args': 'LabelTileViewsArgs'}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    for cname, pyname in structs.items():
        assert L.STRUCTS[cname] is getattr(L, pyname)
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in getattr(L, pyname)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['return 0;}']
    c, exe = tmp_path / 'abi.c', tmp_path / 'abi'
    c.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, pyname in structs.items():
        cls = getattr(L, pyname)
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    assert [f for f, _ in L.TileViewDesc._fields_] == ['image', 'H', 'W', 'Hv', 'Wv', 'y0', 'x0', 'mirror'] and ctypes.sizeof(L.TileViewDesc) == 40
    assert [f for f, _ in L.TileView._fields_] == ['Hv', 'Wv', 't0', 'ny', 'nx', 'mirror', 'weight', 'y0', 'x0']
    assert [f for f, _ in L.LabelTileViewsArgs._fields_] == ['view', 'nview', 'logits', 'ld', 'h', 'w', 'th', 'tw', 'N', 'C', 'OH', 'OW', 'lut256', 'labels']
    assert dict(L.TileView._fields_)['y0']._length_ == dict(L.TileView._fields_)['x0']._length_ == 16
    assert dict(L.LabelTileViewsArgs._fields_)['view']._length_ == 8
    # the single-view structures are as they were
    assert ctypes.sizeof(L.TileDesc) == 24 and [f for f, _ in L.TileDesc._fields_] == ['image', 'H', 'W', 'y0', 'x0']


# ---------------- the membership test ----------------
def test_every_pixel_is_covered_in_every_view():
    """2 O o0 <= (2o+1) Lv < 2 O (o0 + t), in integers: over a sweep of sizes and scales every output index has a covering window, the
    covering windows are consecutive, and at scale 1 they are the windows [o0, o0 + t) of the single-view head"""
    deepest = 0
    for t, s in ((33, 17), (16, 8), (5, 5), (7, 1), (64, 32)):
        for O in (1, 2, 3, 7, 30, 37, 61, 70, 129):
            for scale in (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 3.1):
                Lv = view_size(O, O, scale)[0]
                if Lv < 1 or (Lv > t and math.ceil((Lv - t) / s) + 1 > 16):
                    continue
                o = tile_starts(Lv, t, s)
                for mirror in (False, True):
                    m = R.member(O, Lv, o, t, mirror)
                    k = m.sum(0)
                    assert int(k.min()) >= 1, (t, s, O, scale, mirror)
                    first, last = m.long().argmax(0), len(o) - 1 - m.flip(0).long().argmax(0)
                    assert torch.equal(k, last - first + 1), (t, s, O, scale, mirror)            # no hole between the covering windows
                    deepest = max(deepest, int(k.max()))
                    if Lv == O and not mirror:
                        want = torch.stack([(torch.arange(O) >= a) & (torch.arange(O) < a + t) for a in o])
                        assert torch.equal(m, want)
                assert torch.equal(R.member(O, Lv, o, t, True), R.member(O, Lv, o, t, False).flip(1))
    assert deepest >= 3


# ---------------- the reference the kernel test uses ----------------
def test_reference_fp32_agrees_with_fp64():
    for case, (N, size, tile, stride, low, views) in R.CASES.items():
        gr = R.grids(case)
        for C_ in R.CLASSES:
            x = R.logits(case, C_)
            a64, want, excused, e32, tau = R.reference(case, C_)
            a32 = R.formula(x, N, size, tile, low, views, gr, torch.float32)
            assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and tuple(a64.shape) == (N, C_) + size
            assert tuple(x.shape) == (R.ntiles(case),) + low + (C_,) and x.dtype == torch.float32
            assert e32 == float((a32.double() - a64).abs().max()) and tau == 64 * e32 and 0 < e32 < 1e-4
            # the sum is divided by the cover count: each pixel's probabilities add up to the weights' sum
            assert torch.allclose(a64.sum(1), torch.full((N,) + size, sum(v[2] for v in views), dtype=torch.float64), atol=1e-12, rtol=0)
            print('%s/C%d: e32 = %.2e, tau = %.2e, classes present %d' % (case, C_, e32, tau, len(want.unique())))
            assert len(want.unique()) > 4
            R.check_map(a32.argmax(1).to(torch.uint8), want, excused, '%s/C%d' % (case, C_))      # the cap, and no other pixel differs
    assert [N * sum(len(g[2]) * len(g[3]) for g in R.grids(c)) // N for c, (N, *_) in R.CASES.items()] == [18, 19, 94, 3]
    assert [(g[0], g[1], g[2], g[3]) for g in R.grids('three')[::2]] == [(30, 53, [0], [0]), (40, 70, [0, 7], [0, 5]), (50, 88, [0, 17], [0, 23])]
    assert all(len(g[2]) == len(g[3]) == 1 and g[0] < 33 and g[1] < 65 for g in R.grids('pad'))
    assert R.grids('weights')[3][2:4] == ([0, 8, 16, 24, 32, 40, 44], [0, 12, 24, 36, 48, 60, 72, 76])


def test_the_formula_is_sensitive_to_what_it_says():
    """four deliberately wrong fp64 formulas each move more than CAP of the pixels of at least one case they apply to"""
    seen = collections.defaultdict(list)
    for case, (N, size, tile, stride, low, views) in R.CASES.items():
        applies = {'mirror': any(v[1] for v in views), 'cover': True, 'weights': len({v[2] for v in views}) > 1, 'row': True}
        for C_ in R.CLASSES:
            x, want = R.logits(case, C_), R.reference(case, C_)[1]
            for wrong, on in applies.items():
                if on:
                    got = R.formula(x, N, size, tile, low, views, R.grids(case), torch.float64, wrong).argmax(1).to(torch.uint8)
                    share = float((got != want).float().mean())
                    print('%s/C%d without %s: %.2f %% of the pixels change' % (case, C_, wrong, 100 * share))
                    seen[wrong].append(share)
    assert set(seen) == {'mirror', 'cover', 'weights', 'row'}
    for wrong, shares in seen.items():
        assert max(shares) > R.CAP, (wrong, shares)


# ---------------- the launches of a call ----------------
def test_default_arguments_are_the_single_view_call(dry):
    from addk.segment import TiledSegmenter
    m = _add(4)
    a, b = TiledSegmenter(m, TILE, STRIDE), TiledSegmenter(m, TILE, STRIDE, scales=None, flip=False, weights=None)
    assert a.views is None and b.views is None
    assert [c.name for c in a.g.fwd] == [c.name for c in b.g.fwd]
    imgs = [torch.randn(3, 65, 129), torch.randn(3, 40, 100), torch.randn(3, 97, 200)]
    b.segment(imgs)
    assert b.tiles == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 0, 71), (2, 32, 0), (2, 32, 71)]
    assert dry['gather_tiles'] == dry['nchw_to_nhwc'] == 2 and dry['label_tiles_upsample'] == 3
    assert dry['gather_tile_views'] == dry['label_tile_views_upsample'] == 0


def test_a_call_with_views_launches_per_chunk_and_image(dry):
    from addk.segment import TiledSegmenter
    m = _add(4)
    plain = TiledSegmenter(m, TILE, STRIDE)
    seg = TiledSegmenter(m, TILE, STRIDE, scales=(0.5, 1.0, 1.5), flip=True)
    assert [c.name for c in seg.g.fwd] == [c.name for c in plain.g.fwd]                                     # the same tile plan
    assert seg.views == [(0.5, False, 1 / 6), (0.5, True, 1 / 6), (1.0, False, 1 / 6), (1.0, True, 1 / 6), (1.5, False, 1 / 6), (1.5, True, 1 / 6)]
    imgs = [torch.randn(3, 65, 129), torch.randn(3, 97, 200)]
    maps = seg.segment(imgs)
    want = []
    for k, (H, W) in enumerate(((65, 129), (97, 200))):
        for v, (s, _, _) in enumerate(seg.views):
            Hv, Wv = view_size(H, W, s)
            want += [(k, v, y, x) for y in tile_starts(Hv, 65, 32) for x in tile_starts(Wv, 129, 71)]
    assert seg.tiles == want                                                                               # image-major, then view, window row, window column
    assert [t for t in seg.tiles if t[0] == 1 and t[1] == 4] == [(1, 4, y, x) for y in (0, 32, 64, 81) for x in (0, 71, 142, 171)]   # 146 x 300
    T = len(seg.tiles)
    assert T == 2 * (1 + 1 + 3 * 2) + 2 * (1 + 2 * 2 + 4 * 4) == 58
    assert dry['gather_tile_views'] == dry['nchw_to_nhwc'] == math.ceil(T / 3) == 20                       # ceil(T / B) gathers and replays
    assert dry['label_tile_views_upsample'] == len(imgs) == 2                                              # one head launch per image
    assert not dry['gather_tiles'] and not dry['label_tiles_upsample'] and not dry['label_views_upsample'] and not dry['resize_nchw']
    assert [tuple(y.shape) for y in maps] == [(65, 129), (97, 200)] and all(y.dtype == torch.uint8 for y in maps)
    h, w = seg.low
    assert tuple(seg.tile_logits().shape) == (T, h, w, 19)
    # no full-resolution float tensor: the object owns the store, the descriptor words and the label bytes
    assert seg._label_buf.dtype == torch.uint8 and seg._label_buf.numel() == 65 * 129 + 97 * 200
    # weights, one scale, no flip; a batch tensor
    dry.clear()
    one = TiledSegmenter(m, TILE, STRIDE, scales=(1.0,), flip=False, weights=(1.0,))
    assert one.views == [(1.0, False, 1.0)]
    one.segment(torch.randn(2, 3, 97, 200))
    assert one.tiles == [(n, 0, y, x) for n in (0, 1) for y in (0, 32) for x in (0, 71)]
    assert dry['gather_tile_views'] == 3 and dry['label_tile_views_upsample'] == 2 and not dry['gather_tiles']
    flipped = TiledSegmenter(m, TILE, STRIDE, flip=True, weights=(1, 3))
    assert flipped.views == [(1.0, False, 1.0), (1.0, True, 3.0)]
    assert TiledSegmenter(m, TILE, STRIDE, weights=(2,)).views == [(1.0, False, 2.0)]


def test_errors_of_the_view_arguments(dry, monkeypatch):
    from addk.segment import TiledSegmenter
    m = _add(4)
    built = []
    real_build = TiledSegmenter._build
    monkeypatch.setattr(TiledSegmenter, '_build', lambda self: built.append(self))
    for kw in (dict(scales=()), dict(scales=(1.0, 0.0)), dict(scales=(-1.0,)), dict(scales=(float('inf'),)), dict(scales=(float('nan'),)),
               dict(scales=(0.5, 0.75, 1.0, 1.25, 1.5), flip=True), dict(scales=tuple(range(1, 10))),
               dict(scales=(1.0, 1.5), weights=(1.0,)), dict(flip=True, weights=(1.0,)), dict(weights=(1.0, 1.0)),
               dict(scales=(1.0,), weights=(0.0,)), dict(scales=(1.0,), weights=(-1.0,)), dict(scales=(1.0,), weights=(float('inf'),)),
               dict(scales=(1.0,), weights=(float('nan'),))):
        with pytest.raises(ValueError):
            TiledSegmenter(m, TILE, STRIDE, **kw)
    assert not built                                                           # every error came before any plan was built
    assert len(TiledSegmenter(m, TILE, STRIDE, scales=(0.5, 0.75, 1.0, 1.25), flip=True).views) == 8      # eight views are taken
    monkeypatch.setattr(TiledSegmenter, '_build', real_build)
    seg = TiledSegmenter(m, TILE, STRIDE, scales=(1.0, 2.0))
    # 65 + 15 * 32 rows are sixteen windows at scale 1 and more at scale 2; an image that a scale takes below one pixel
    for images in ([torch.zeros(3, 65 + 15 * 32, 129)], [torch.zeros(3, 65, 129 * 5)], [], [torch.zeros(3, 65, 129, dtype=torch.float64)]):
        with pytest.raises(ValueError):
            seg.segment(images)
    with pytest.raises(ValueError):
        TiledSegmenter(m, TILE, STRIDE, scales=(0.25,)).segment([torch.zeros(3, 1, 40)])
    assert not dry['gather_tile_views'] and not dry['label_tile_views_upsample']      # ... and before any launch
    seg.segment([torch.zeros(3, (65 + 15 * 32) // 2, 129)])
    assert max(t[2] for t in seg.tiles) == 544 - 65 and len(seg.tiles) == 8 * 1 + 16 * 3
