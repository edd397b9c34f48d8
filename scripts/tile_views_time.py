"""Times of multi-scale + flip sliding-window label maps at Cityscapes size: a 1024 x 2048 image, scales 0.75 / 1.0 / 1.25 each plain and
mirrored, every view under 769 x 769 windows at stride 513; low-resolution grid as the decoder gives it for a 769 x 769 input.
  (a) the head launch (label_tile_views_upsample) for C = 19 and 21, against the materialised torch form on the same logits (per view and
      window: interpolate, softmax, add into the view's scaled-size buffer; divide by the cover count, flip back, resize to the image, weight
      and add; arg-max) and against six label_tiles_upsample launches (what six single views of the image cost the single-view head)
  (b) addk_gather_tile_views for one chunk of B windows of the mirrored 1.25 view, against torch's interpolate + flip + crop of the same
      windows, and against addk_gather_tiles (no resize) for the same number of bytes written
  (c) TiledSegmenter.segment with the six views end to end against the plain tiled call, on the F = 20 config-2 model (synthetic weights)
Device events around REPS passes, ROUNDS rounds, the forms of a comparison alternating in one process, warm; median (min ... max) per pass.
Run from the repository root on the MI355X:
    python scripts/tile_views_time.py [out.txt]          (default profiles/label_tile_views_head.txt)"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import torch
import torch.nn.functional as F
import addk._lib as L
from addk.segment import TiledSegmenter, tile_starts, view_size
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '20')), int(os.environ.get('ROUNDS', '10'))
B = int(os.environ.get('TILES_B', '4'))
OH, OW, TH, TW, SY, SX = 1024, 2048, 769, 769, 513, 513
SCALES = (0.75, 1.0, 1.25)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'label_tile_views_head.txt')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps=REPS, rounds=ROUNDS):
    """{name: [us per pass, one per round]}: the forms alternate inside every round"""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / reps)
    return times


def report(times, what=''):
    for k, v in times.items():
        say('%s%s: median %.1f us per pass (min %.1f ... max %.1f; %d rounds)' % (what, k, statistics.median(v), min(v), max(v), len(v)))
    return {k: statistics.median(v) for k, v in times.items()}


st = torch.cuda.current_stream().cuda_stream
views = [(s, m, 1.0 / 6) for s in SCALES for m in (False, True)]
grids, T = [], 0
for s, _, _ in views:
    Hv, Wv = view_size(OH, OW, s)
    ys, xs = tile_starts(Hv, TH, SY), tile_starts(Wv, TW, SX)
    grids.append((Hv, Wv, ys, xs, T))
    T += len(ys) * len(xs)

# ---- the front ends first: their plan says what the low-resolution grid is ----
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args
from addk.modeling.ADD import ADD
model = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), 0)
fill_params(model, 600)
model = model.to(dev).eval()
multi = TiledSegmenter(model, (B, 3, TH, TW), (SY, SX), scales=SCALES, flip=True)
plain = TiledSegmenter(model, (B, 3, TH, TW), (SY, SX))
h, w = multi.low
say('image %d x %d, windows %d x %d at stride (%d, %d), %d views: %s; %d windows; low-resolution grid of a window %d x %d'
    % (OH, OW, TH, TW, SY, SX, len(views), ', '.join('%g%s %dx%d: %dx%d windows' % (s, ' mirrored' if m else '', g[0], g[1], len(g[2]), len(g[3]))
                                                      for (s, m, _), g in zip(views, grids)), T, h, w))

# ---- (a) the head launch ----
g = torch.Generator().manual_seed(3)
ys1, xs1 = tile_starts(OH, TH, SY), tile_starts(OW, TW, SX)
for Cc in (19, 21):
    ld = (Cc + 3) // 4 * 4
    # one coarse scene behind every view (independent logits per window average to flat sums), plus noise
    scene = torch.randn((1, Cc, 5, 9), generator=g) * 3
    store = torch.zeros((T, h, w, ld))
    a_, b_ = torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5
    for (_, mirror, _), (Hv, Wv, ys, xs, t0) in zip(views, grids):
        for iy, y0 in enumerate(ys):
            for ix, x0 in enumerate(xs):
                v, u = (y0 + a_ * TH / h) / Hv, (x0 + b_ * TW / w) / Wv
                if mirror:
                    u = 1 - u
                grid = torch.stack([(2 * u - 1)[None, :].expand(h, w), (2 * v - 1)[:, None].expand(h, w)], 2)
                z = F.grid_sample(scene, grid[None], mode='bilinear', padding_mode='border', align_corners=True)[0].permute(1, 2, 0)
                store[t0 + iy * len(xs) + ix, :, :, :Cc] = z + torch.randn((h, w, Cc), generator=g) * 0.5
    store = store.to(dev)
    labels = torch.zeros((1, OH, OW), dtype=torch.uint8, device=dev)
    a = L.LabelTileViewsArgs()
    a.nview, a.logits, a.ld, a.h, a.w, a.th, a.tw = len(views), store.data_ptr(), ld, h, w, TH, TW
    a.N, a.C, a.OH, a.OW, a.lut256, a.labels = 1, Cc, OH, OW, None, labels.data_ptr()
    for v, (_, mirror, weight), (Hv, Wv, ys, xs, t0) in zip(a.view, views, grids):
        v.Hv, v.Wv, v.t0, v.ny, v.nx, v.mirror, v.weight = Hv, Wv, t0, len(ys), len(xs), int(mirror), weight
        v.y0[:len(ys)], v.x0[:len(xs)] = ys, xs
    # the single-view head on the scale-1 windows, six times
    lab1 = torch.zeros((1, OH, OW), dtype=torch.uint8, device=dev)
    b = L.LabelTilesArgs()
    b.logits, b.ld, b.h, b.w, b.th, b.tw = store.data_ptr(), ld, h, w, TH, TW
    b.N, b.C, b.OH, b.OW, b.t0, b.ny, b.nx = 1, Cc, OH, OW, grids[2][4], len(ys1), len(xs1)
    b.y0[:len(ys1)], b.x0[:len(xs1)] = ys1, xs1
    b.lut256, b.labels = None, lab1.data_ptr()
    nchw = store[..., :Cc].permute(0, 3, 1, 2)
    acc = torch.empty((Cc, OH, OW), device=dev)
    accv = [torch.empty((Cc, max(gr[0], TH), max(gr[1], TW)), device=dev) for gr in grids]
    cover = []
    for Hv, Wv, ys, xs, _ in grids:
        c = torch.zeros((max(Hv, TH), max(Wv, TW)))
        for y0 in ys:
            for x0 in xs:
                c[y0:y0 + TH, x0:x0 + TW] += 1
        cover.append(c.to(dev))
    result = {}

    def fused():
        L.check(lib.addk_label_tile_views_upsample(C.byref(a), st))

    def six():
        for _ in range(len(views)):
            L.check(lib.addk_label_tiles_upsample(C.byref(b), st))

    def materialised():
        acc.zero_()
        for (_, mirror, weight), (Hv, Wv, ys, xs, t0), av, cv in zip(views, grids, accv, cover):
            av.zero_()
            t = t0
            for y0 in ys:
                for x0 in xs:
                    av[:, y0:y0 + TH, x0:x0 + TW] += torch.softmax(F.interpolate(nchw[t:t + 1], (TH, TW), mode='bilinear', align_corners=False), 1)[0]
                    t += 1
            p = (av / cv)[None, :, :Hv, :Wv]
            if mirror:
                p = p.flip(3)
            acc.add_(F.interpolate(p, (OH, OW), mode='bilinear', align_corners=False)[0], alpha=weight)
        result['am'] = acc.argmax(0)

    fns = {'label_tile_views_upsample (fused, %d windows of 6 views)' % T: fused,
           'materialised (per view and window: interpolate + softmax + add; / cover, flip, resize back, add; arg-max; torch)': materialised,
           '6 x label_tiles_upsample (six single views at scale 1)': six}
    med = report(timed(fns), '(a) C=%d ' % Cc)
    same = float((result['am'].to(torch.uint8) == labels[0]).float().mean())
    say('(a) C=%d: the fused and the materialised form agree on %.3f %% of the pixels (the materialised form resamples every view twice)' % (Cc, 100 * same))
    k = list(fns)
    say('(a) C=%d ratios of the medians: materialised / fused %.2f; fused / six single views %.2f' % (Cc, med[k[1]] / med[k[0]], med[k[0]] / med[k[2]]))
    say('(a) C=%d bytes: the store %.1f MB; the fused form writes %.1f MB (the map)' % (Cc, store.numel() * 4 / 1e6, OH * OW / 1e6))

# ---- (b) the gather of one chunk ----
image = torch.randn((3, OH, OW), generator=g).to(dev)
Hv, Wv, ys, xs, _ = grids[5]
wins = [(y, x) for y in ys for x in xs][:B]
arr = (L.TileViewDesc * B)()
for d, (y0, x0) in zip(arr, wins):
    d.image, d.H, d.W, d.Hv, d.Wv, d.y0, d.x0, d.mirror = image.data_ptr(), OH, OW, Hv, Wv, y0, x0, 1
table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
arr1 = (L.TileDesc * B)()
for d, (y0, x0) in zip(arr1, [(y, x) for y in ys1 for x in xs1][:B]):
    d.image, d.H, d.W, d.y0, d.x0 = image.data_ptr(), OH, OW, y0, x0
table1 = torch.frombuffer(bytearray(bytes(arr1)), dtype=torch.uint8).to(dev)
xbuf, xtorch = torch.empty((B, 3, TH, TW), device=dev), torch.empty((B, 3, TH, TW), device=dev)


def torch_gather():
    S = F.interpolate(image[None], (Hv, Wv), mode='bilinear', align_corners=False)[0].flip(2)
    for i, (y0, x0) in enumerate(wins):
        xtorch[i].copy_(S[:, y0:y0 + TH, x0:x0 + TW])


med = report(timed({'gather_tile_views, %d windows of 3 x %d x %d of the mirrored %g view' % (B, TH, TW, views[5][0]):
                    lambda: L.check(lib.addk_gather_tile_views(table.data_ptr(), B, 3, TH, TW, xbuf.data_ptr(), B, st)),
                    'torch: interpolate to %d x %d, flip, %d crops' % (Hv, Wv, B): torch_gather,
                    'gather_tiles (scale 1, no resize), %d windows' % B:
                    lambda: L.check(lib.addk_gather_tiles(table1.data_ptr(), B, 3, TH, TW, xtorch.data_ptr(), B, st))}), '(b) ')
L.check(lib.addk_gather_tile_views(table.data_ptr(), B, 3, TH, TW, xbuf.data_ptr(), B, st))
torch_gather()
say('(b) largest difference between the two gathers: %.2e' % float((xbuf - xtorch).abs().max()))
k = list(med)
say('(b) ratio of the medians: torch / gather_tile_views %.2f; gather_tile_views / gather_tiles %.2f; %.1f MB written: %.0f GB/s'
    % (med[k[1]] / med[k[0]], med[k[0]] / med[k[2]], xbuf.numel() * 4 / 1e6, xbuf.numel() * 4 / 1e3 / med[k[0]]))

# ---- (c) end to end ----
img4 = image[None].contiguous()
t = timed({'TiledSegmenter.segment, 6 views (B = %d: %d windows, %d chunks)' % (B, T, -(-T // B)): lambda: multi.segment(img4),
           'TiledSegmenter.segment, plain (%d windows, %d chunks)' % (len(ys1) * len(xs1), -(-len(ys1) * len(xs1) // B)): lambda: plain.segment(img4)},
          reps=3, rounds=max(3, ROUNDS // 2))
med = report(t, '(c) ')
k = list(med)
say('(c) ratio of the medians (six views / plain): %.2f; windows through the network: %.2f x (%d against %d)'
    % (med[k[0]] / med[k[1]], T / (len(ys1) * len(xs1)), T, len(ys1) * len(xs1)))
say('(c) plan buffers: %.1f MB either way; store %.1f MB with views, %.1f MB plain' % (multi.nbytes / 1e6, multi._store.numel() * 4 / 1e6, plain._store.numel() * 4 / 1e6))
multi.close()
plain.close()
os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
