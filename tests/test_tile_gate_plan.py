"""Host-logic tests (CPU, no GPU) of per-window early exits in segment.TiledSegmenter: the schedule (segment.TileGateSchedule) driven with
scripted decisions, the gated tile plan and the launches of a gated call (launches stubbed: the `dry` fixture), the untouched default path,
the error paths, the C ABI of addk_gate_tiles_upsample and addk_scatter_tile_logits, and the fp64 reference that tests/test_gpu_tile_gate.py
holds the gate kernel to (tests/_tile_gate_ref.py): no pixel of any case lies within tau of the threshold, so the share must be exact."""
import collections
import ctypes
import math
import os
import re
import subprocess
import types

import pytest
import torch

import addk
from addk import _lib as L
from addk.segment import TileGateSchedule
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)
import _tile_gate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (3, 3, 65, 129)
STRIDE = (32, 71)


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer']).eval()


# ---------------- the schedule ----------------
# a pattern says whether window t leaves at gate k
PATTERNS = {'all_leave': lambda k, t, B: True,
            'none_leave': lambda k, t, B: False,
            'alternating': lambda k, t, B: (t + k) % 2 == 0,
            'chunk1_stays_chunk2_leaves': lambda k, t, B: (t // B + k) % 2 == 1}


def _drive(B, G, T, leaves):
    """run the schedule with scripted decisions, replaying its operations on a model of the plan rows and the pool rings -> (schedule,
    runs per stage, windows per stage, exit of every window); asserts what must hold at every operation"""
    s = TileGateSchedule(B, G)
    rows, unresolved = [None] * B, set()            # the window in every plan row; the rows whose state nobody has taken yet
    rings = [dict() for _ in range(G)]              # per pool: ring slot -> window
    runs, reach, exit_of = collections.Counter(), collections.Counter(), {}
    last = [None]

    def execute(op):
        what = op[0]
        if what == 'gather':
            _, t0, n = op
            assert not unresolved and 1 <= n <= B and (t0 + n == T or n == B)
            rows[:n] = range(t0, t0 + n)
            last[0] = ('gather', list(range(t0, t0 + n)))
        elif what == 'run':
            _, k, ids = op
            assert 1 <= len(ids) <= B and rows[:len(ids)] == ids, 'the stage runs on the rows that were put there'
            if last[0][0] == 'run':                 # straight on from the stage before: the same rows, none of which left
                assert last[0][1] == k - 1 and last[0][2] == ids and unresolved == set(range(len(ids)))
                unresolved.clear()
            assert not unresolved
            assert (k == 0 and last[0][0] == 'gather') or (k > 0 and last[0][0] in ('unpark', 'run'))
            runs[k] += 1
            reach[k] += len(ids)
            unresolved.update(range(len(ids)))
            last[0] = ('run', k, ids)
            if k < G:
                return [leaves(k, t, B) for t in ids]
        elif what == 'scatter':
            _, k, rws, ids = op
            assert last[0][0] == 'run' and last[0][1] == k and len(rws) == len(ids) >= 1
            for r, t in zip(rws, ids):
                assert rows[r] == t and r in unresolved and t not in exit_of and (k == G or leaves(k, t, B))
                unresolved.discard(r)
                exit_of[t] = k
        elif what == 'park':
            _, k, rws, slots = op
            assert len(rws) == len(slots) >= 1 and len(set(slots)) == len(slots)
            for r, sl in zip(rws, slots):
                assert r in unresolved and not leaves(k, rows[r], B) and 0 <= sl < 2 * B and sl not in rings[k]
                rings[k][sl] = rows[r]
                unresolved.discard(r)
            assert len(rings[k]) <= 2 * B - 1, 'a pool never holds more than 2B - 1 rows'
        else:
            _, k, slots = op
            assert what == 'unpark' and not unresolved, 'nothing is unparked into rows that still wait to be parked'
            assert 1 <= len(slots) <= B
            rows[:len(slots)] = [rings[k].pop(sl) for sl in slots]
            last[0] = ('unpark', k)
    s.run(T, execute)
    assert not unresolved and not any(rings)
    return s, runs, reach, exit_of


@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('T', [1, 3, 7, 10])
@pytest.mark.parametrize('G', [1, 2])
def test_schedule_invariants(G, T, pattern):
    B, leaves = 3, PATTERNS[pattern]
    s, runs, reach, exit_of = _drive(B, G, T, leaves)
    want_exit = {t: next((k for k in range(G) if leaves(k, t, B)), G) for t in range(T)}
    assert exit_of == want_exit                                              # every window scattered exactly once, at its exit
    for k in range(G + 1):
        n_k = sum(1 for t in range(T) if want_exit[t] >= k)
        assert reach[k] == n_k and runs[k] == math.ceil(n_k / B), (k, n_k, runs[k])
    assert all(p <= 2 * B - 1 for p in s.peak)
    kinds = collections.Counter(op[0] for op in s.ops)
    assert kinds['gather'] == math.ceil(T / B)
    if pattern == 'none_leave':
        assert kinds['park'] == kinds['unpark'] == 0 and kinds['scatter'] == math.ceil(T / B)      # nobody leaves: no state is moved
    if pattern == 'all_leave':
        assert kinds['park'] == kinds['unpark'] == 0 and runs[1] == 0
    if pattern == 'alternating' and T >= 7:
        assert kinds['park'] >= 2 and kinds['unpark'] >= 1 and max(s.peak) >= B      # survivors of several chunks fill a batch again


def test_schedule_pools_survivors_of_several_chunks():
    # B = 3, one gate, windows 0 and 3 stay: chunk 0 parks one row, chunk 1 parks one, chunk 2 (window 6 leaves) none; the flush runs both at once
    s, runs, reach, exit_of = _drive(3, 1, 7, lambda k, t, B: t % 3 != 0 or t == 6)
    assert runs[0] == 3 and runs[1] == 1 and reach[1] == 2 and exit_of == {0: 1, 1: 0, 2: 0, 3: 1, 4: 0, 5: 0, 6: 0}
    assert [op for op in s.ops if op[0] in ('park', 'unpark')] == [('park', 0, [0], [0]), ('park', 0, [0], [1]), ('unpark', 0, [0, 1])]
    with pytest.raises(ValueError):
        TileGateSchedule(3, 0)
    with pytest.raises(ValueError):
        TileGateSchedule(0, 1)


# ---------------- the gated plan and a gated call ----------------
@pytest.mark.parametrize('arch,gates', [(ARCH_C2, 1), (ARCH_C3, 2)], ids=['c2', 'c3'])
def test_gated_plan_builds_and_a_call_launches(dry, arch, gates):
    from addk.segment import TiledSegmenter
    m = _add(4, arch)
    seg = TiledSegmenter(m, TILE, STRIDE, threshold=0.35)
    p, names = seg.plan, collections.Counter(c.name for c in seg.g.fwd)
    assert seg.gates == gates == len(p.heads) == len(p.cuts) and seg.g.head == 'tile_gate'
    assert names['gate_tiles_upsample'] == gates and names['nchw_to_nhwc'] == 1
    assert not {'resize_nchw', 'gate_upsample', 'gate_label_upsample', 'label_upsample'} & set(names)
    assert all(o.head == 'tile_gate' and o.y is None and o.src is not None for o in p.outs) and p.final.gate_out is None
    assert [seg.g.fwd[c - 1].name for c in p.cuts] == ['gate_tiles_upsample'] * gates       # every early stage ends in its gate
    assert [p.stage(k) for k in range(gates + 1)] == list(zip([0] + p.cuts, p.cuts + [-1]))
    # a pool per gate: 2B rows of every per-window live buffer behind the cut, and of the extents
    B = TILE[0]
    for k, (bufs, pool, pext) in enumerate(p.pools):
        assert bufs == p.live(p.cuts[k])[0] and len(bufs) == len(pool) >= 1 and tuple(pext.shape) == (2 * B, 2)
        assert all(t.numel() == 2 * b.n and b.geom[0] == B for b, t in zip(bufs, pool))
        assert p.park[k][1] == p.unpark[k][1] == len(bufs) + 1
    assert seg.nbytes == seg.g.nbytes + p.pool_bytes and p.pool_bytes > 0
    h, w = seg.low
    assert seg.ld == 20 and seg.ncls == 19 and tuple(p.ext.shape) == (B, 2) and p.ext.dtype == torch.int32
    # 1 + 1 + 2x2 windows; the stubbed gate words are zero: every window leaves at gate 0 ('entropy': 0 < 0.35)
    imgs = [torch.randn(3, 65, 129), torch.randn(3, 40, 100), torch.randn(3, 97, 200)]
    maps = seg.segment(imgs)
    T = len(seg.tiles)
    assert T == 6 and dry['gather_tiles'] == dry['gate_tiles_upsample'] == dry['scatter_tile_logits'] == 2 and dry['gather_rows'] == 0
    assert dry['label_tiles_upsample'] == 3 and [tuple(y.shape) for y in maps] == [(65, 129), (40, 100), (97, 200)]
    assert seg.exits.tolist() == [0] * T and seg.values[:, 0].tolist() == [0.0] * T and bool(seg.values[:, 1:].isnan().all())
    assert seg.counts == {('seg', 0): 2, 'scatter': 2} and seg.trace == [(0, 3), (0, 3)]
    # the extents travel behind the descriptor table: the window on the 40 x 100 image hangs over it
    ext = torch.frombuffer(bytearray(seg._desc.host.view(-1)[seg._ext_off:seg._ext_off + 8 * T].numpy().tobytes()), dtype=torch.int32).view(T, 2)
    assert ext.tolist() == [[65, 129], [40, 100]] + [[65, 129]] * 4 and seg._ext_off % 16 == 0
    # a threshold nobody passes: every stage runs for every chunk, nothing is parked, the last exit's logits take the same scatter launch
    dry.clear()
    seg.segment(imgs, threshold=-1.0)
    assert seg.exits.tolist() == [gates] * T and dry['gate_tiles_upsample'] == 2 * gates and dry['scatter_tile_logits'] == 2
    assert dry['gather_rows'] == 0 and seg.trace == [(k, 3) for _ in range(2) for k in range(gates + 1)]
    assert seg.counts[('seg', gates)] == 2 and seg.counts['park'] == seg.counts['unpark'] == 0
    # views compose: every window of every view is gated, extents on the view's scaled image
    dry.clear()
    sv = TiledSegmenter(m, TILE, STRIDE, threshold=[0.35] * gates, confidence='max', scales=(0.5, 1.0), flip=True, temperature=1.5)
    assert sv.plan._temp is not None and sv.temperature == (1.5,) * (gates + 1)
    sv.segment([torch.randn(3, 97, 200)])
    assert dry['gather_tile_views'] == math.ceil(len(sv.tiles) / 3) and dry['label_tile_views_upsample'] == 1 and len(sv.tiles) == 2 * (1 + 4)
    ext = torch.frombuffer(bytearray(sv._desc.host.view(-1)[sv._ext_off:sv._ext_off + 8 * 10].numpy().tobytes()), dtype=torch.int32).view(10, 2)
    assert ext.tolist() == [[49, 100]] * 2 + [[65, 129]] * 8
    sv.set_temperature(2.0)
    assert sv.temperature == (2.0,) * (gates + 1)
    # the parameters move: the next call builds the plan (and its pools) again
    g0 = seg.g
    q = next(m.parameters())
    q.data = q.data.clone()
    seg.segment(imgs)
    assert seg.g is not g0 and seg.plan is not p


def test_default_path_is_untouched(dry):
    from addk.segment import Segmenter, TiledSegmenter
    m = _add(4)
    for exit in (0, -1):
        seg = TiledSegmenter(m, TILE, STRIDE, exit=exit)
        one = Segmenter(m, TILE, exit=exit)
        # the launch list it emits today: the trunk and head of that exit, and nothing of the label head
        assert [c.name for c in seg.g.fwd] == [c.name for c in one.g.fwd if c.name != 'label_upsample']
        assert seg.g.head == 'tiles' and seg.threshold is None
        assert not any(hasattr(seg, a) for a in ('plan', 'exits', 'values', 'counts', 'trace', 'schedule', 'kind', 'gates'))
        dry.clear()
        seg.segment([torch.randn(3, 97, 200)])
        assert dry['gather_tiles'] == dry['nchw_to_nhwc'] == 2 and dry['label_tiles_upsample'] == 1
        assert not dry['gate_tiles_upsample'] and not dry['scatter_tile_logits'] and not dry['gather_rows']
        with pytest.raises(ValueError, match='without a threshold'):
            seg.segment([torch.randn(3, 97, 200)], threshold=0.3)
        with pytest.raises(ValueError, match='without a threshold'):
            seg.set_temperature(1.0)


def test_gated_errors(dry, monkeypatch):
    from addk import heads as H
    from addk.segment import TiledSegmenter
    m = _add(4, ARCH_C3)
    built = []
    real_build = TiledSegmenter._build
    monkeypatch.setattr(TiledSegmenter, '_build', lambda self: built.append(self))
    for exit in (0, 1, -2):
        with pytest.raises(ValueError, match='last exit'):
            TiledSegmenter(m, TILE, STRIDE, exit=exit, threshold=0.3)
    with pytest.raises(ValueError, match='edm'):
        TiledSegmenter(m, TILE, STRIDE, threshold=0.3, confidence='edm')
    with pytest.raises(ValueError, match='confidence'):
        TiledSegmenter(m, TILE, STRIDE, threshold=0.3, confidence='softmax')
    for thr in ([0.3], [0.3, 0.3, 0.3]):
        with pytest.raises(ValueError, match='one threshold per gate'):
            TiledSegmenter(m, TILE, STRIDE, threshold=thr)
    for temp in (0.0, -1.0, float('inf'), [1.0, 2.0]):
        with pytest.raises(ValueError, match='temperature'):
            TiledSegmenter(m, TILE, STRIDE, threshold=0.3, temperature=temp)
    single = _add(4)
    single.num_exits = lambda: 1                                             # a model with one exit has no gate
    with pytest.raises(ValueError, match='early exit'):
        TiledSegmenter(single, TILE, STRIDE, threshold=0.3)
    assert not built                                                           # every error came before any plan was built
    monkeypatch.setattr(TiledSegmenter, '_build', real_build)
    # exits whose low-resolution logits differ: one store row would not fit every exit
    real_head = H.HEADS['tile_gate']

    def odd_head(g, src, OH, OW):
        out = real_head(g, src, OH, OW)
        if g.gate is not None:
            r = out.src.raw
            out.src = types.SimpleNamespace(raw=types.SimpleNamespace(H=r.H + 1, W=r.W, C=r.C))
        return out
    monkeypatch.setitem(H.HEADS, 'tile_gate', odd_head)
    with pytest.raises(ValueError, match=r'share one \(h, w, C\)'):
        TiledSegmenter(m, TILE, STRIDE, threshold=0.3)
    monkeypatch.setitem(H.HEADS, 'tile_gate', real_head)
    seg = TiledSegmenter(m, TILE, STRIDE, threshold=0.3)
    with pytest.raises(ValueError, match='one threshold per gate'):
        seg.segment([torch.randn(3, 65, 129)], threshold=[0.1])
    with pytest.raises(ValueError, match='without a temperature'):
        seg.set_temperature(1.5)
    assert not dry['gather_tiles']
    with pytest.raises(addk.AddkError, match=re.escape(L.head_classes_text())):
        TiledSegmenter(_add(4, classes=7), TILE, STRIDE, threshold=0.3)


# ---------------- ABI ----------------
def _gate_args(**kw):
    a = L.GateTilesArgs()
    a.logits, a.ld, a.B, a.nb, a.h, a.w, a.C, a.th, a.tw = 64, 24, 3, 3, 9, 9, 19, 33, 33
    a.ext, a.max_thr, a.inv_temp, a.out, a.out_host, a.ws = 64, 64, None, 64, None, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _scatter_args(**kw):
    a = L.ScatterTileLogitsArgs()
    a.src, a.lds, a.B, a.store, a.ld, a.T, a.h, a.w, a.C, a.src_row, a.dst_tile, a.n = 64, 20, 3, 64, 20, 7, 9, 9, 19, 64, 64, 2
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_abi_declared_exported_bound_and_refusals(tmp_path):
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in ('addk_gate_tiles_upsample_supported', 'addk_gate_tiles_upsample_ws_bytes', 'addk_gate_tiles_upsample', 'addk_scatter_tile_logits'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    sup, wsb = lib.addk_gate_tiles_upsample_supported, lib.addk_gate_tiles_upsample_ws_bytes      # (B, h, w, th, tw, C), (B, th, tw)
    assert all(sup(3, 9, 9, 33, 33, c) == 1 for c in L.head_classes()) and sup(4, 193, 193, 769, 769, 19) == 1
    for bad in ((3, 9, 9, 33, 33, 20), (3, 9, 9, 33, 33, 7), (0, 9, 9, 33, 33, 19), (3, 0, 9, 33, 33, 19), (3, 9, 9, 33, -1, 19), (65536, 9, 9, 33, 33, 19)):
        assert sup(*bad) == 0, bad
    # [ticket, 16 bytes] + a float and a count per workgroup of 64 columns x 32 rows and slot
    assert wsb(3, 33, 33) == 16 + 8 * 3 * 1 * 2 and wsb(4, 769, 769) == 16 + 8 * 4 * 13 * 25 and wsb(0, 33, 33) == wsb(3, 0, 33) == 0
    # refused before anything is launched: needs no device
    assert lib.addk_gate_tiles_upsample(None, None) == -1 and lib.addk_scatter_tile_logits(None, None) == -1
    for kw in (dict(logits=None), dict(ext=None), dict(max_thr=None), dict(out=None), dict(ws=None), dict(nb=-1), dict(nb=4), dict(B=0),
               dict(h=0), dict(w=-2), dict(th=0), dict(tw=0), dict(ld=18), dict(C=20), dict(C=0)):
        assert lib.addk_gate_tiles_upsample(ctypes.byref(_gate_args(**kw)), None) == -1, kw
    assert 'gate_tiles_upsample' in lib.addk_last_error().decode()
    for kw in (dict(src=None), dict(store=None), dict(dst_tile=None), dict(n=-1), dict(n=4), dict(B=0), dict(T=0), dict(h=0), dict(w=0), dict(C=0),
               dict(lds=18), dict(ld=18)):
        assert lib.addk_scatter_tile_logits(ctypes.byref(_scatter_args(**kw)), None) == -1, kw
    assert 'scatter_tile_logits' in lib.addk_last_error().decode()
    # nothing to do is no error, and no launch: nb == 0, n == 0
    assert lib.addk_gate_tiles_upsample(ctypes.byref(_gate_args(nb=0)), None) == 0
    assert lib.addk_scatter_tile_logits(ctypes.byref(_scatter_args(n=0)), None) == 0
    # the mirrors against the header
    structs = {'addk_gate_tiles_args': 'GateTilesArgs', 'addk_scatter_tile_logits_args': 'ScatterTileLogitsArgs'}
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


# ---------------- the reference the kernel test uses ----------------
def test_reference_excuses_no_pixel_and_fp32_is_close():
    for case, (h, w, th, tw) in R.CASES.items():
        for C_ in R.CLASSES:
            for temp in range(len(R.INV_TEMP)):
                seen = set()
                for r in (0, 1):
                    ref = R.reference(case, C_, temp, r)
                    seen |= set(ref['ext'])
                    ent = ref['entropy']
                    print('%s/C%d/temp%d/r%d: entropy %s, e32 = %.2e (bound %.2e), e32p = %.2e, slots (pixels, hits, excused) %s'
                          % (case, C_, temp, r, [round(float(v), 6) for v in ent], ref['e32'], R.FACTOR * ref['e32'], ref['e32p'], ref['slots']))
                    assert 0 < ref['e32'] < 1e-5 and 0 < ref['e32p'] < 1e-5
                    assert bool(((ent > 0.05) & (ent < 1.0)).all()) and len(set(ent.tolist())) == R.B
                    for (npix, hits, excused), (vh, vw) in zip(ref['slots'], ref['ext']):
                        assert npix == vh * vw and excused <= R.CAP * npix                   # the cap, from the fp64 reference alone
                    assert any(0 < hits < npix for npix, hits, _ in ref['slots'])            # the threshold cuts through a window of every launch
                assert seen == set(R.clamp(R.EXTENTS, th, tw))                               # two rotations cover every extent
    assert R.clamp([(0, -5), (1000, 1000)], 17, 40) == [(1, 1), (17, 40)]
