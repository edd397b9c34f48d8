"""GPU tests of per-window early exits in the sliding window: addk_gate_tiles_upsample through the C ABI against the fp64 formula
(tests/_tile_gate_ref.py), addk_scatter_tile_logits against exact bytes, and segment.TiledSegmenter with `threshold` against the static
TiledSegmenter at the exit each window left at — bit for bit: the batch size never changes and no kernel of the plan looks at a row's
position in the batch.

The rule of the comparison with fp64 is tests/_views_ref.py's: e32 = the error of the fp32 torch formula on the CPU for these very inputs; the
entropy may differ from fp64 by 64 * e32; a pixel whose fp64 top probability lies within 64 * e32p of the threshold would be excused (at
most 0.2 % of a window's valid pixels) and the count over the others must be exact — with these inputs the reference excuses none
(tests/test_tile_gate_plan.py), so every share word is the fp64 one."""
import collections
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from _util import rand_tensor                                                              # noqa: E402
import _tile_gate_ref as R                                                                 # noqa: E402
from test_gpu_batched_gate import _force                                                   # noqa: E402
from test_gpu_tiles import STRIDE, TILE, _model                                            # noqa: E402

GUARD = 64
LD = 24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    import addk._lib as L
    return L.load(), L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """`n` bytes of `fill` between two guards of 64 bytes of 0xAB"""

    def __init__(self, n, dev, fill=0xAB):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=dev)
        self.raw[GUARD:GUARD + n] = fill

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def read(self):
        """the bytes on the host; the guards must be untouched"""
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == 0xAB).all()) and bool((raw[GUARD + self.n:] == 0xAB).all()), 'a guard byte was written'
        return raw[GUARD:GUARD + self.n].clone()


def _device_logits(x, ld, dev):
    """x [B,h,w,C] -> (tensor that owns the memory, address of the first pixel): ld == 24 with finite garbage in the padding channels, 16-byte
    aligned (the vector loader); ld == C dense, from a base offset by one float (the scalar loader)"""
    Cc = x.shape[3]
    if ld == LD:
        xa = (rand_tensor(1, 'tile_gate_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
        xa[..., :Cc] = x.to(dev)
        xa = xa.contiguous()
        assert xa.data_ptr() % 16 == 0
        return xa, xa.data_ptr()
    assert ld == Cc
    flat = torch.full((x.numel() + 1,), 1e30, device=dev)
    flat[1:] = x.to(dev).reshape(-1)
    assert (flat.data_ptr() + 4) % 16 != 0
    return flat, flat.data_ptr() + 4


class _Gate:
    """the buffers of addk_gate_tiles_upsample launches on one case: logits, a zero-initialised workspace, guarded output words"""

    def __init__(self, case, Cc, ld, temp, dev):
        lib, L = _lib()
        self.lib, self.L, self.dev = lib, L, dev
        self.h, self.w, self.th, self.tw = R.CASES[case]
        self.C, self.ld = Cc, ld
        self.keep, self.x = _device_logits(R.logits(case, Cc), ld, dev)
        self.ws = _Guarded(int(lib.addk_gate_tiles_upsample_ws_bytes(R.B, self.th, self.tw)), dev, fill=0)
        self.thr = torch.tensor([R.THR], dtype=torch.float32, device=dev)
        s = R.INV_TEMP[temp]
        self.it = None if s is None else torch.tensor([s], dtype=torch.float32, device=dev)
        self.host = torch.full((R.B, 2), -7.0).pin_memory()

    def launch(self, ext, nb, host=False):
        """-> (rc, float32 [B,2] words with the untouched ones still 0xAB bytes, the raw bytes)"""
        L = self.L
        out = _Guarded(R.B * 2 * 4, self.dev)
        e = torch.tensor(ext, dtype=torch.int32, device=self.dev)
        a = L.GateTilesArgs()
        a.logits, a.ld, a.B, a.nb, a.h, a.w, a.C, a.th, a.tw = self.x, self.ld, R.B, nb, self.h, self.w, self.C, self.th, self.tw
        a.ext, a.max_thr, a.inv_temp = e.data_ptr(), self.thr.data_ptr(), None if self.it is None else self.it.data_ptr()
        a.out, a.out_host, a.ws = out.ptr, self.host.data_ptr() if host else None, self.ws.ptr
        rc = self.lib.addk_gate_tiles_upsample(C.byref(a), _stream())
        torch.cuda.synchronize()
        raw = out.read()
        ticket = self.ws.read()[:4]
        assert bool((ticket == 0).all()), 'the ticket word was not put back to zero'
        return rc, raw.view(torch.float32).view(R.B, 2), raw


@pytest.mark.parametrize('temp', [0, 1], ids=['plain', 'tempered'])
@pytest.mark.parametrize('ld', [LD, 0], ids=['stride24', 'dense'])
@pytest.mark.parametrize('Cc', R.CLASSES)
@pytest.mark.parametrize('case', list(R.CASES))
def test_gate_tiles_upsample_is_the_fp64_formula(dev, case, Cc, ld, temp):
    lib, L = _lib()
    ld = ld or Cc
    h, w, th, tw = R.CASES[case]
    assert lib.addk_gate_tiles_upsample_supported(R.B, h, w, th, tw, Cc) == 1
    gate = _Gate(case, Cc, ld, temp, dev)
    for r in (0, 1):
        ref = R.reference(case, Cc, temp, r)
        bound = R.FACTOR * ref['e32']
        full = None
        for nb in (3, 2, 0):
            rc, words, raw = gate.launch(R.extents(r), nb, host=(nb == 3))
            assert rc == 0
            assert bool((raw[8 * nb:] == 0xAB).all()), 'a slot at or beyond nb was written'
            for b in range(nb):
                ent, share = float(words[b, 0]), float(words[b, 1])
                err = abs(ent - float(ref['entropy'][b]))
                print('%s/C%d/%d/temp%d/r%d/nb%d slot %d %s: entropy %.9g, fp64 %.9g, |diff| %.2e, e32 %.2e, bound %.2e; share %.9g'
                      % (case, Cc, ld, temp, r, nb, b, ref['ext'][b], ent, float(ref['entropy'][b]), err, ref['e32'], bound, share))
                assert err <= bound, (case, Cc, ld, temp, r, nb, b, err, bound)
                R.check_share(share, *ref['slots'][b], what=(case, Cc, ld, temp, r, nb, b))
            if nb == 3:
                full = words.clone()
                assert torch.equal(gate.host.view(torch.int32), words.view(torch.int32))             # the pinned words carry the same bits
                again = gate.launch(R.extents(r), nb)[1]
                assert torch.equal(again.view(torch.int32), full.view(torch.int32))                  # a second launch on the same workspace
            else:
                assert torch.equal(words[:nb].view(torch.int32), full[:nb].view(torch.int32))        # a slot's words do not depend on nb


def test_gate_tiles_upsample_clamps_extents_and_equals_the_image_gate(dev):
    lib, L = _lib()
    gate = _Gate('odd', 19, LD, 0, dev)
    wild = gate.launch([(0, -5), (1000, 1000), (33, 7)], 3)[1]
    tame = gate.launch([(1, 1), (17, 40), (17, 7)], 3)[1]
    assert torch.equal(wild.view(torch.int32), tame.view(torch.int32))
    # the whole window at 19 classes: addk_gate_upsample's words on the same logits
    whole = gate.launch([(17, 40)] * 3, 3)[1]
    out = torch.zeros((R.B, 2), device=dev)
    ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(R.B, 17, 40)), dtype=torch.uint8, device=dev)
    a = L.GateUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = gate.x, LD, R.B, 5, 9, 19, 17, 40
    a.max_thr, a.out, a.out_host, a.ws = gate.thr.data_ptr(), out.data_ptr(), None, ws.data_ptr()
    L.check(lib.addk_gate_upsample(C.byref(a), _stream()), 'gate_upsample')
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), whole.view(torch.int32))
    # refused without a launch
    for kw in (dict(nb=4), dict(nb=-1), dict(ld=18), dict(C=20)):
        out = _Guarded(R.B * 8, dev)
        a = L.GateTilesArgs()
        a.logits, a.ld, a.B, a.nb, a.h, a.w, a.C, a.th, a.tw = gate.x, LD, R.B, 3, 5, 9, 19, 17, 40
        a.ext, a.max_thr, a.out, a.ws = gate.thr.data_ptr(), gate.thr.data_ptr(), out.ptr, gate.ws.ptr
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.addk_gate_tiles_upsample(C.byref(a), _stream()) == -1, kw
        torch.cuda.synchronize()
        assert bool((out.read() == 0xAB).all())


# (lds, ld, C, aligned bases): the 16-byte form, the same at 21 classes, dense rows from a misaligned base, a padded source into a dense store
@pytest.mark.parametrize('lds,ld,Cc,aligned', [(20, 20, 19, True), (24, 24, 21, True), (19, 19, 19, False), (20, 19, 19, True)],
                         ids=['vec19', 'vec21', 'dense', 'mixed'])
def test_scatter_tile_logits_writes_exact_bytes(dev, lds, ld, Cc, aligned):
    lib, L = _lib()
    B, T, h, w = 3, 5, 9, 7
    off = 0 if aligned else 4
    src = rand_tensor(5, 'scatter_src:%d:%d' % (lds, Cc), (B, h, w, lds))
    before = rand_tensor(6, 'scatter_store:%d' % ld, (T, h, w, ld)) + 100
    s = _Guarded(src.numel() * 4 + off, dev)
    s.raw[GUARD + off:GUARD + off + src.numel() * 4] = src.view(torch.uint8).reshape(-1).to(dev)
    assert (s.ptr + off) % 16 == off
    # (rows, tiles, n): a permutation of every row, a partial set, rows 0..n-1 (src_row NULL), indices outside the store and the plan
    for rows, tiles in (([2, 0, 1], [4, 0, 2]), ([1, 2], [3, 1]), (None, [2, 4]), ([0, 1, 2], [T, -1, 2]), ([3, -1, 1], [0, 1, 4])):
        st = _Guarded(before.numel() * 4 + off, dev)
        st.raw[GUARD + off:GUARD + off + before.numel() * 4] = before.view(torch.uint8).reshape(-1).to(dev)
        n = len(tiles)
        a = L.ScatterTileLogitsArgs()
        a.src, a.lds, a.B, a.store, a.ld, a.T, a.h, a.w, a.C = s.ptr + off, lds, B, st.ptr + off, ld, T, h, w, Cc
        ri = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev)
        ti = torch.tensor(tiles, dtype=torch.int32, device=dev)
        a.src_row, a.dst_tile, a.n = None if ri is None else ri.data_ptr(), ti.data_ptr(), n
        assert lib.addk_scatter_tile_logits(C.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        got = st.read()[off:].view(torch.float32).view(T, h, w, ld)
        want = before.clone()
        for i, t in enumerate(tiles):
            r = i if rows is None else rows[i]
            if 0 <= t < T and 0 <= r < B:
                want[t, :, :, :Cc] = src[r, :, :, :Cc]
                want[t, :, :, Cc:] = 0                                       # the padding channels are written as zero
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (rows, tiles)
        assert bool((st.read()[:off] == 0xAB).all())
    s.read()


# ------------------------------------------------------------------------------------------------------------------------
# public path
# ------------------------------------------------------------------------------------------------------------------------
SIZES = ((97, 271), (40, 100))            # 2 x 3 windows, and one window that hangs over its image: 7 in all
VIEWS = dict(scales=(0.75, 1.0), flip=True)


@functools.lru_cache(maxsize=None)
def _images(dev):
    return [(rand_tensor(61 + i, 'tile_gate_img', (3,) + s) * 32.0).to(dev) for i, s in enumerate(SIZES)]


@functools.lru_cache(maxsize=None)
def _static(dev, views=False):
    """the static TiledSegmenter at every exit on the images -> {exit: (stored logits [T,h,w,C], maps, tiles)}; computed once, never modified"""
    from addk.segment import TiledSegmenter
    m, out = _model(dev), {}
    for e in range(m.num_exits()):
        seg = TiledSegmenter(m, TILE, STRIDE, exit=e, **(VIEWS if views else {}))
        maps = seg.segment(_images(dev))
        out[e] = (seg.tile_logits().clone(), [y.clone() for y in maps], list(seg.tiles))
        seg.close()
    assert not torch.equal(out[0][0], out[m.num_exits() - 1][0])
    return out


def _gap_threshold(v, rank=0):
    """the midpoint of the largest (rank 1: the second largest) gap of the values, and the gap"""
    s = sorted(float(x) for x in v)
    gap, i = sorted(((b - a, i) for i, (a, b) in enumerate(zip(s, s[1:]))), reverse=True)[rank]
    return 0.5 * (s[i] + s[i + 1]), gap


@pytest.mark.parametrize('kind', ['entropy', 'max'])
def test_all_windows_leave_and_all_stay(dev, kind):
    from addk.segment import TiledSegmenter
    m, imgs, want = _model(dev), _images(dev), _static(dev)
    G = m.num_exits() - 1
    force, forbid = _force(kind)
    seg = TiledSegmenter(m, TILE, STRIDE, threshold=force, confidence=kind)
    T = len(want[0][2])
    assert T >= 7 and TILE[0] == 3
    vals = []
    for thr, e in ((force, 0), (forbid, G)):
        for call in range(5):                                                # the stages run eagerly twice, are captured, then replay
            maps = seg.segment(imgs, threshold=thr)
            torch.cuda.synchronize()
            assert seg.tiles == want[e][2] and seg.exits.tolist() == [e] * T
            assert torch.equal(seg.tile_logits(), want[e][0]), (kind, e, call)
            assert all(torch.equal(a, b) for a, b in zip(maps, want[e][1])), (kind, e, call)
            assert not bool(seg.values[:, 0].isnan().any())
            vals.append(seg.values[:, 0].clone())
    assert seg.counts['park'] == seg.counts['unpark'] == 0 and seg.counts['scatter'] == 10 * math.ceil(T / 3)
    assert seg.counts[('seg', 0)] == 10 * math.ceil(T / 3) and seg.counts[('seg', G)] == 5 * math.ceil(T / 3)
    assert len(seg.plan.graphs) == G + 1                                     # every stage was captured and replayed
    if kind == 'entropy':
        assert all(torch.equal(v, vals[0]) for v in vals) and len(set(vals[0].tolist())) == T      # eager and replayed: the same words
    seg.close()


# rank 0: the threshold the windows' values suggest, in their largest gap — here it keeps one window, the zero-padded one of the last chunk,
# which goes straight on.  rank 1, in the second largest gap, keeps windows of several chunks: they are parked, pooled and run as one batch,
# so the bits below also pass through `addk_gather_rows` twice.  The launches are those of the schedule driven with the same decisions.
@pytest.mark.parametrize('rank', [0, 1], ids=['largest_gap', 'second_gap'])
def test_mixed_decisions(dev, rank):
    from addk.segment import TiledSegmenter, TileGateSchedule, tile_starts
    lib, L = _lib()
    m, imgs, want = _model(dev), _images(dev), _static(dev)
    G, B, (th, tw) = m.num_exits() - 1, TILE[0], TILE[2:]
    assert G == 1
    seg = TiledSegmenter(m, TILE, STRIDE, threshold=float('-inf'))
    seg.segment(imgs)
    v0 = seg.values[:, 0].clone()
    thr, gap = _gap_threshold(v0, rank)
    print('gate-0 values of the windows: %s; threshold %.6f in a gap of %.3e' % ([round(float(x), 6) for x in v0], thr, gap))
    assert gap >= 1e-3
    exits = [0 if float(x) < thr else 1 for x in v0]
    T, n1 = len(exits), sum(exits)
    assert 0 < n1 < T
    host = TileGateSchedule(B, G)
    host.run(T, lambda op: [exits[t] == 0 for t in op[2]] if op[0] == 'run' else None)
    ops = collections.Counter(op[0] for op in host.ops)
    assert rank == 0 or (ops['park'] >= 2 and ops['unpark'] >= 1)             # survivors of more than one chunk
    h, w = seg.low
    for call in range(4):
        before = collections.Counter(seg.counts)
        maps = seg.segment(imgs, threshold=thr)
        torch.cuda.synchronize()
        assert seg.exits.tolist() == exits                                   # the exits follow the values
        assert torch.equal(seg.values[:, 0], v0) and not bool(v0.isnan().any())
        got = seg.tile_logits()
        for t, e in enumerate(exits):
            assert torch.equal(got[t], want[e][0][t]), (call, t, e)          # bit for bit the static plan's logits at that window's exit
        assert seg.counts[('seg', 0)] - before[('seg', 0)] == math.ceil(T / B)
        assert seg.counts[('seg', 1)] - before[('seg', 1)] == math.ceil(n1 / B)
        assert all(seg.counts[k] - before[k] == ops[k] for k in ('park', 'unpark', 'scatter')) and seg.schedule.ops == host.ops
        assert [k for k, _ in seg.trace].count(1) == math.ceil(n1 / B) and sum(n for k, n in seg.trace if k == 1) == n1
        # the maps: addk_label_tiles_upsample on that mixed store
        store = torch.zeros((T, h, w, seg.ld), device=dev)
        for t, e in enumerate(exits):
            store[t, :, :, :seg.ncls] = want[e][0][t]
        t0 = 0
        for im, y in zip(imgs, maps):
            H, W = im.shape[1:]
            ys, xs = tile_starts(H, th, STRIDE[0]), tile_starts(W, tw, STRIDE[1])
            lab = torch.zeros((H, W), dtype=torch.uint8, device=dev)
            a = L.LabelTilesArgs()
            a.logits, a.ld, a.h, a.w, a.th, a.tw = store.data_ptr(), seg.ld, h, w, th, tw
            a.N, a.C, a.OH, a.OW, a.t0, a.ny, a.nx = 1, seg.ncls, H, W, t0, len(ys), len(xs)
            a.y0[:len(ys)], a.x0[:len(xs)] = ys, xs
            a.lut256, a.labels = None, lab.data_ptr()
            L.check(lib.addk_label_tiles_upsample(C.byref(a), _stream()), 'label_tiles_upsample')
            torch.cuda.synchronize()
            assert torch.equal(lab, y), call
            t0 += len(ys) * len(xs)
    seg.close()


def test_views_compose(dev):
    from addk.segment import TiledSegmenter
    m, imgs, want = _model(dev), _images(dev), _static(dev, views=True)
    G = m.num_exits() - 1
    seg = TiledSegmenter(m, TILE, STRIDE, threshold=float('-inf'), **VIEWS)
    T = len(want[0][2])
    for thr, e in ((float('inf'), 0), (float('-inf'), G)):
        maps = seg.segment(imgs, threshold=thr)
        torch.cuda.synchronize()
        assert seg.tiles == want[e][2] and seg.exits.tolist() == [e] * T
        assert torch.equal(seg.tile_logits(), want[e][0]) and all(torch.equal(a, b) for a, b in zip(maps, want[e][1]))
    v0 = seg.values[:, 0].clone()
    thr, gap = _gap_threshold(v0)
    print('views: %d windows, threshold %.6f in a gap of %.3e' % (T, thr, gap))
    assert gap >= 1e-3
    exits = [0 if float(x) < thr else 1 for x in v0]
    for call in range(3):
        seg.segment(imgs, threshold=thr)
        torch.cuda.synchronize()
        got = seg.tile_logits()
        assert seg.exits.tolist() == exits and torch.equal(seg.values[:, 0], v0)
        assert all(torch.equal(got[t], want[e][0][t]) for t, e in enumerate(exits))
    print('views: exits %s, launches %s' % (exits, dict(seg.counts)))
    seg.close()


def test_temperature(dev):
    from addk.segment import TiledSegmenter
    m, imgs, want = _model(dev), _images(dev), _static(dev)
    G = m.num_exits() - 1
    plain = TiledSegmenter(m, TILE, STRIDE, threshold=float('-inf'))
    plain.segment(imgs)
    v = plain.values.clone()
    seg = TiledSegmenter(m, TILE, STRIDE, threshold=float('-inf'), temperature=2.0)
    seg.segment(imgs)
    v2 = seg.values.clone()
    assert torch.equal(seg.tile_logits(), want[G][0])                         # only the gate is tempered
    assert bool((v2 != v).all()) and bool((v2 > v).all())                     # a flatter prediction: more entropy
    seg.set_temperature(1.3)
    seg.segment(imgs)
    fresh = TiledSegmenter(m, TILE, STRIDE, threshold=float('-inf'), temperature=1.3)
    fresh.segment(imgs)
    assert torch.equal(seg.values, fresh.values) and bool((seg.values != v2).all())
    for s in (plain, seg, fresh):
        s.close()
