"""Host-logic tests (CPU, no GPU) of sliding-window label maps: the window grid (segment.tile_starts), the C ABI of addk_gather_tiles and
of the tiled label head, the launch plan and the per-call launches of segment.TiledSegmenter, its error paths, and the fp32-against-fp64
check of the torch formula that tests/test_gpu_tiles.py holds the kernel to.  Launches are stubbed as in tests/test_views_plan.py.

The reference check (tests/_tiles_ref.py): with N(0, 3^2) logits the fp32 formula differs from the fp64 one by e32 of 4.7e-7 ... 4.8e-6 (up to
nine probabilities are summed); tau = 64 * e32 per case excuses at most 0.14 % of a case's pixels (`grid` at C = 19), within the cap of 0.2 %,
and fp32's arg-max equals fp64's on every other pixel.  The test prints every case's figures."""
import collections
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import addk
from addk import _lib as L
from addk.segment import tile_starts
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)
import _tiles_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (3, 3, 65, 129)
STRIDE = (32, 71)


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer']).eval()


def _names(g):
    return [c.name for c in g.fwd]


# ---------------- the window grid ----------------
def test_tile_starts_properties():
    seen_three_deep = False
    for t in (1, 2, 5, 32, 33):
        for s in sorted({1, 2, (t + 1) // 2, t - 1, t} - {0}):
            if s > t:
                continue
            for L_ in list(range(1, 3 * t + 3)) + [t + 15 * s, t + 15 * s - 1]:
                if L_ > t and math.ceil((L_ - t) / s) + 1 > 16:
                    with pytest.raises(ValueError):
                        tile_starts(L_, t, s)
                    continue
                o = tile_starts(L_, t, s)
                assert o[0] == 0 and o[-1] + t == max(L_, t), (L_, t, s, o)               # from 0 to the end of the image (or of the padded window)
                assert all(a < b for a, b in zip(o, o[1:])), (L_, t, s, o)                # strictly increasing
                assert all(b <= a + t for a, b in zip(o, o[1:])), (L_, t, s, o)           # consecutive windows touch or overlap: no gap
                assert len(o) == (1 if L_ <= t else math.ceil((L_ - t) / s) + 1)
                assert o == [min(i * s, max(L_ - t, 0)) for i in range(len(o))]
                depth = max(sum(1 for a in o if a <= p < a + t) for p in range(L_))
                seen_three_deep |= depth >= 3 and s * 2 >= t                              # three deep although the stride alone gives two
    assert seen_three_deep
    assert tile_starts(70, 33, 17) == [0, 17, 34, 37]                                     # the clamped last window: 34, 37 and 17 overlap at 37..49
    assert tile_starts(21, 33, 17) == [0] and tile_starts(33, 33, 17) == [0] and tile_starts(34, 33, 17) == [0, 1]
    assert tile_starts(150, 65, 33) == [0, 33, 66, 85] and tile_starts(1024, 769, 513) == [0, 255] and tile_starts(2048, 769, 513) == [0, 513, 1026, 1279]
    assert len(tile_starts(33 + 15 * 17, 33, 17)) == 16 == L.MAX_TILES_AXIS                # the limit is taken ...
    with pytest.raises(ValueError, match='at most 16'):
        tile_starts(33 + 15 * 17 + 1, 33, 17)                                             # ... and one more window is not
    for bad in ((70, 33, 0), (70, 33, 34), (70, 33, -1), (0, 33, 17), (70, 0, 1)):
        with pytest.raises(ValueError):
            tile_starts(*bad)


# ---------------- ABI ----------------
def _tiles_args(ny=4, nx=4, OH=70, OW=150, C_=19):
    """arguments the launcher would take, over a dummy non-null address (used only where the call is refused before any launch)"""
    a = L.LabelTilesArgs()
    a.logits, a.ld, a.h, a.w, a.th, a.tw = 64, 24, 9, 17, 33, 65
    a.N, a.C, a.OH, a.OW, a.t0, a.ny, a.nx = 2, C_, OH, OW, 0, ny, nx
    a.y0[:4], a.x0[:4] = [0, 17, 34, 37], [0, 33, 66, 85]
    a.lut256, a.labels = None, 64
    return a


def test_tiles_abi_declared_exported_and_bound():
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in ('addk_gather_tiles', 'addk_label_tiles_upsample_supported', 'addk_label_tiles_upsample'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert int(re.search(r'#define ADDK_MAX_TILES_AXIS (\d+)', src).group(1)) == L.MAX_TILES_AXIS == 16
    sup = lib.addk_label_tiles_upsample_supported                      # (N, OH, OW, ny, nx, C)
    assert sup(2, 70, 150, 4, 4, 19) == 1 and sup(2, 70, 150, 4, 4, 21) == 1 and sup(1, 1, 1, 1, 1, 19) == 1 and sup(1, 500, 500, 16, 16, 21) == 1
    assert set(L.head_classes()) == {19, 21} and L.gate_head_classes() == (19,)       # the label heads' list, and the other one untouched
    for bad in ((2, 70, 150, 4, 4, 7), (2, 70, 150, 4, 4, 20), (2, 70, 150, 0, 4, 19), (2, 70, 150, 4, 17, 19), (0, 70, 150, 4, 4, 19),
                (2, 0, 150, 4, 4, 19), (2, 70, -1, 4, 4, 19), (65536, 70, 150, 4, 4, 19), (1, 65536 * 16 + 1, 1, 1, 1, 19)):
        assert sup(*bad) == 0, bad
    # refused before anything is launched: needs no device
    assert lib.addk_label_tiles_upsample(None, None) == -1 and lib.addk_label_tiles_upsample(ctypes.byref(L.LabelTilesArgs()), None) == -1
    for edit in R.REFUSALS:
        a = _tiles_args()
        edit(a)
        assert lib.addk_label_tiles_upsample(ctypes.byref(a), None) == -1, edit.what
    assert 'label_tiles_upsample' in lib.addk_last_error().decode()
    # addk_gather_tiles(table, ntiles, Cin, th, tw, x, B): null pointers, ntiles outside 0..B, non-positive sizes
    for bad in ((None, 1, 3, 8, 8, 64, 2), (64, 1, 3, 8, 8, None, 2), (None, 0, 3, 8, 8, None, 2), (64, 3, 3, 8, 8, 64, 2), (64, -1, 3, 8, 8, 64, 2),
                (64, 1, 0, 8, 8, 64, 2), (64, 1, 3, 0, 8, 64, 2), (64, 1, 3, 8, -2, 64, 2), (64, 0, 3, 8, 8, 64, 0)):
        assert lib.addk_gather_tiles(*bad, None) == -1, bad
    assert 'gather_tiles' in lib.addk_last_error().decode()
    assert lib.addk_version() >= 2


def test_tiles_struct_layouts_match_header(tmp_path):
    structs = {'addk_tile_desc': 'TileDesc', 'addk_label_tiles_args': 'LabelTilesArgs'}
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
    assert [f for f, _ in L.TileDesc._fields_] == ['image', 'H', 'W', 'y0', 'x0'] and ctypes.sizeof(L.TileDesc) == 24
    assert [f for f, _ in L.LabelTilesArgs._fields_] == ['logits', 'ld', 'h', 'w', 'th', 'tw', 'N', 'C', 'OH', 'OW', 't0', 'ny', 'nx', 'y0', 'x0',
                                                          'lut256', 'labels']
    assert dict(L.LabelTilesArgs._fields_)['y0']._length_ == dict(L.LabelTilesArgs._fields_)['x0']._length_ == 16


# ---------------- plan structure and the launches of a call ----------------
def test_tile_plan_materialises_nothing_and_a_call_launches_per_chunk_and_image(dry):
    from addk.segment import TiledSegmenter
    m = _add(4).train()
    seg = TiledSegmenter(m, TILE, STRIDE)
    g, names = seg.g, collections.Counter(_names(seg.g))
    assert names['resize_nchw'] == names['label_upsample'] == names['label_views_upsample'] == names['argmax_nchw'] == 0
    assert names['nchw_to_nhwc'] == 1 and names['bn_finalize'] == 0 and not g.bwd and m.training          # one staged input; inference form
    out = seg.out
    assert out.head == 'tiles' and out.y is None and tuple(out.shape) == (3, 19, 65, 129) and out.src is not None
    h, w = seg.low
    assert (h, w) == (out.src.raw.H, out.src.raw.W) and h < 65 and w < 129 and seg.ld == 20 and seg.ncls == 19
    # no [B,19,th,tw] tensor in either layout
    sizes = {3 * 65 * 129 * c for c in (19, 20)}
    assert not any(b.n in sizes for b in g._bufs) and not any(t.numel() in sizes for t in g.keep if isinstance(t, torch.Tensor))
    assert tuple(seg.x.shape) == TILE
    # a list of differently sized images: 1 + 1 + 2x2 windows ... then a batch of two 97 x 200 images
    imgs = [torch.randn(3, 65, 129), torch.randn(3, 40, 100), torch.randn(3, 97, 200)]
    maps = seg.segment(imgs)
    assert seg.tiles == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 0, 71), (2, 32, 0), (2, 32, 71)]
    T = len(seg.tiles)
    assert dry['gather_tiles'] == dry['nchw_to_nhwc'] == math.ceil(T / 3) == 2                             # ceil(T / B) gathers and replays
    assert dry['label_tiles_upsample'] == len(imgs) == 3                                                   # one head launch per image
    assert [tuple(y.shape) for y in maps] == [(65, 129), (40, 100), (97, 200)] and all(y.dtype == torch.uint8 for y in maps)
    assert tuple(seg.tile_logits().shape) == (T, h, w, 19) and tuple(seg._store.shape[1:]) == (h, w, 20)
    dry.clear()
    store = seg._store
    maps = seg.segment(torch.randn(2, 3, 97, 200))                                                         # 8 windows: the store grows
    assert seg.tiles == [(n, y, x) for n in (0, 1) for y in (0, 32) for x in (0, 71)]
    assert dry['gather_tiles'] == dry['nchw_to_nhwc'] == 3 and dry['label_tiles_upsample'] == 2
    assert seg._store is not store and seg._store.shape[0] >= 8 and len(maps) == 2
    dry.clear()
    store = seg._store
    seg.segment([torch.randn(3, 10, 300)])                                                                 # 1 x 4 windows: the store is kept
    assert seg._store is store and dry['gather_tiles'] == 2 and dry['label_tiles_upsample'] == 1
    assert seg.tiles == [(0, 0, x) for x in (0, 71, 142, 171)]


def test_exit_lut_and_21_classes(dry):
    from addk.data import decode_segmap_lut
    from addk.segment import TiledSegmenter
    m = _add(4)
    first, last = TiledSegmenter(m, TILE, STRIDE, exit=0), TiledSegmenter(m, TILE, STRIDE, exit=-1, label_lut=decode_segmap_lut())
    assert first.exit == 0 and last.exit == 1 and len(first.g.fwd) < len(last.g.fwd)
    assert first.lut is None and last.lut.tolist() == decode_segmap_lut().tolist()
    voc = TiledSegmenter(_add(4, classes=21), (2, 3, 33, 33), (17, 17))
    assert voc.ncls == 21 and voc.ld == 24 and voc.out.shape[1] == 21
    # the parameters move: the next call builds the plan again
    g0 = last.g
    p = next(m.parameters())
    p.data = p.data.clone()
    last.segment([torch.randn(3, 30, 30)])
    assert last.g is not g0 and last.calls == 1


# ---------------- error paths ----------------
def test_errors(dry, monkeypatch):
    from addk.modeling.baseline_model import Baselin_Model
    from addk.segment import TiledSegmenter
    from _util import GENOTYPE_BASELINE_2, NETWORK_PATH_BASELINE
    m = _add(4)
    built = []
    real_build = TiledSegmenter._build
    monkeypatch.setattr(TiledSegmenter, '_build', lambda self: built.append(self))
    with pytest.raises(TypeError):
        TiledSegmenter(Baselin_Model(NETWORK_PATH_BASELINE, [5], GENOTYPE_BASELINE_2, 19, make_args(4), 1), TILE, STRIDE)
    with pytest.raises(TypeError):
        TiledSegmenter(torch.nn.Conv2d(3, 19, 1), TILE, STRIDE)
    for stride in ((0, 71), (32, 0), (66, 71), (32, 130), (-1, 1)):
        with pytest.raises(ValueError, match='stride'):
            TiledSegmenter(m, TILE, stride)
    with pytest.raises(ValueError):
        TiledSegmenter(m, TILE, STRIDE, label_lut=np.zeros(19, np.uint8))
    for bad in (2, -3):
        with pytest.raises(IndexError):
            TiledSegmenter(m, TILE, STRIDE, exit=bad)
    assert not built                                                           # every error came before any plan was built
    monkeypatch.setattr(TiledSegmenter, '_build', real_build)
    seg = TiledSegmenter(m, TILE, STRIDE)
    for images in ([], torch.zeros(0, 3, 65, 129), [torch.zeros(4, 65, 129)], torch.zeros(1, 1, 65, 129), [torch.zeros(3, 65)],
                   torch.zeros(3, 65, 129), [torch.zeros(3, 65 + 15 * 32 + 1, 129)], [torch.zeros(3, 65, 129 + 15 * 71 + 1)],
                   [torch.zeros(3, 65, 129, dtype=torch.float64)]):
        with pytest.raises(ValueError):
            seg.segment(images)
    assert not dry['gather_tiles'] and not dry['label_tiles_upsample']         # ... and before any launch
    seg.segment([torch.zeros(3, 65 + 15 * 32, 129)])                           # sixteen windows on an axis are taken
    assert len(seg.tiles) == 16


def test_seven_classes_and_a_gate_raise_addk_error(dry):
    from addk.segment import TiledSegmenter
    with pytest.raises(addk.AddkError, match=re.escape(L.head_classes_text())):
        TiledSegmenter(_add(4, classes=7), TILE, STRIDE)
    assert L.head_classes_text() == '19 classes (or 21)'
    # a gate together with 'tiles': the plan refuses it
    m = _add(4)
    seg = TiledSegmenter(m, TILE, STRIDE)

    def gated(g, a):
        g.gate = {'host': None, 'thr': torch.zeros(1), 'kind': 'entropy'}
        return m._emit_exit(g, a, seg.exit)
    seg._emit = gated
    with pytest.raises(addk.AddkError, match='gate'):
        seg._build()


# ---------------- the reference the kernel test uses ----------------
def test_reference_fp32_agrees_with_fp64():
    for case, (n, size, tile, stride, low) in R.CASES.items():
        ys, xs = R.origins(case)
        cov = R.covers(size, tile, ys, xs)
        assert int(cov.min()) >= 1                                           # every pixel of the image is covered
        for C_ in R.CLASSES:
            x = R.logits(case, C_)
            a64, want, excused, e32, tau = R.reference(case, C_)
            a32 = R.formula(x, n, size, tile, ys, xs, torch.float32)
            assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and tuple(a64.shape) == (n, C_) + size
            assert tuple(x.shape) == (n * len(ys) * len(xs),) + low + (C_,)
            assert e32 == float((a32.double() - a64).abs().max()) and tau == 64 * e32 and 0 < e32 < 1e-4
            assert len(want.unique()) > 4
            # the sum is not divided by the cover count: each pixel's probabilities add up to it
            assert torch.allclose(a64.sum(1), cov.double().expand(n, -1, -1), atol=1e-12, rtol=0)
            print('%s/C%d: e32 = %.2e, tau = %.2e, covers up to %d' % (case, C_, e32, tau, int(cov.max())))
            R.check_map(a32.argmax(1).to(torch.uint8), want, excused, '%s/C%d' % (case, C_))      # the cap, and no other pixel differs
    assert [len(o) for o in R.origins('pad')] == [1, 1] and [len(o) for o in R.origins('exact')] == [1, 1]
    assert R.origins('grid') == ([0, 17, 34, 37], [0, 33, 66, 85]) and R.origins('odd') == ([0, 16, 32, 35], [0, 32, 64, 67])
    cov = R.covers(*R.CASES['grid'][1:3], *R.origins('grid'))
    assert int(cov.max()) == 9                                               # three deep on both axes
