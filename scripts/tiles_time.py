"""Times of sliding-window label maps at Cityscapes size: a 1024 x 2048 image under 769 x 769 windows at stride 513 (2 x 4 windows, the last
of each axis clamped), low-resolution grid as the decoder gives it for a 769 x 769 input.
  (a) the head launch (label_tiles_upsample) for C = 19 and 21, against the materialised torch form on the same logits (interpolate each
      window, softmax, add into a full-size buffer, arg-max) and against ONE label_upsample of a whole-image logits map of the same pixel count
  (b) addk_gather_tiles for one chunk of B windows
  (c) TiledSegmenter.segment end to end against Segmenter.step at 1024 x 2048, on the F = 20 config-2 model (synthetic weights)
Device events around REPS passes, ROUNDS rounds, the forms of a comparison alternating in one process, warm; median (min ... max) per pass.
Run from the repository root on the MI355X:
    python scripts/tiles_time.py [out.txt]          (default profiles/label_tiles_head.txt)"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import torch
import torch.nn.functional as F
import addk._lib as L
from addk.segment import Segmenter, TiledSegmenter, tile_starts
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '20')), int(os.environ.get('ROUNDS', '10'))
B = int(os.environ.get('TILES_B', '4'))
OH, OW, TH, TW, SY, SX = 1024, 2048, 769, 769, 513, 513
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'label_tiles_head.txt')
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
ys, xs = tile_starts(OH, TH, SY), tile_starts(OW, TW, SX)
T = len(ys) * len(xs)

# ---- the two front ends first: their plans say what the low-resolution grids are ----
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args
from addk.modeling.ADD import ADD
model = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), 0)
fill_params(model, 600)
model = model.to(dev).eval()
tiled = TiledSegmenter(model, (B, 3, TH, TW), (SY, SX))
whole = Segmenter(model, (1, 3, OH, OW))
h, w = tiled.low
la = [c for c in whole.g.fwd if c.name == 'label_upsample'][0].args[0]._obj
HI, WI = la.H, la.W
say('image %d x %d, windows %d x %d at stride (%d, %d): origins %s x %s, %d windows; low-resolution grid of a window %d x %d, of the whole image %d x %d'
    % (OH, OW, TH, TW, SY, SX, ys, xs, T, h, w, HI, WI))

# ---- (a) the head launch ----
g = torch.Generator().manual_seed(3)
for Cc in (19, 21):
    ld = (Cc + 3) // 4 * 4
    store = torch.zeros((T, h, w, ld))
    store[..., :Cc] = torch.randn((T, h, w, Cc), generator=g) * 3
    store = store.to(dev)
    labels = torch.zeros((1, OH, OW), dtype=torch.uint8, device=dev)
    a = L.LabelTilesArgs()
    a.logits, a.ld, a.h, a.w, a.th, a.tw = store.data_ptr(), ld, h, w, TH, TW
    a.N, a.C, a.OH, a.OW, a.t0, a.ny, a.nx = 1, Cc, OH, OW, 0, len(ys), len(xs)
    a.y0[:len(ys)], a.x0[:len(xs)] = ys, xs
    a.lut256, a.labels = None, labels.data_ptr()
    # one whole-image map of the same pixel count through the plain label head
    img = torch.zeros((1, HI, WI, ld))
    img[..., :Cc] = torch.randn((1, HI, WI, Cc), generator=g) * 3
    img = img.to(dev)
    lab1 = torch.zeros((1, OH, OW), dtype=torch.uint8, device=dev)
    b = L.LabelUpsampleArgs()
    b.logits, b.ld, b.N, b.H, b.W, b.C, b.OH, b.OW, b.lut256, b.labels = img.data_ptr(), ld, 1, HI, WI, Cc, OH, OW, None, lab1.data_ptr()
    acc = torch.empty((Cc, OH, OW), device=dev)
    nchw = store[..., :Cc].permute(0, 3, 1, 2)
    result = {}

    def fused():
        L.check(lib.addk_label_tiles_upsample(C.byref(a), st))

    def plain():
        L.check(lib.addk_label_upsample(C.byref(b), st))

    def materialised():
        acc.zero_()
        t = 0
        for y0 in ys:
            for x0 in xs:
                p = torch.softmax(F.interpolate(nchw[t:t + 1], (TH, TW), mode='bilinear', align_corners=False), 1)[0]
                acc[:, y0:y0 + TH, x0:x0 + TW] += p
                t += 1
        result['am'] = acc.argmax(0)

    fns = {'label_tiles_upsample (fused)': fused, 'materialised (8 x interpolate + softmax + add, arg-max; torch)': materialised,
           'label_upsample of one whole-image map (no softmax, one cover)': plain}
    med = report(timed(fns), '(a) C=%d ' % Cc)
    same = float((result['am'].to(torch.uint8) == labels[0]).float().mean())
    say('(a) C=%d: the fused and the materialised form agree on %.4f %% of the pixels' % (Cc, 100 * same))
    assert same > 0.995
    k = list(fns)
    say('(a) C=%d ratios of the medians: materialised / fused %.2f; fused / label_upsample %.2f' % (Cc, med[k[1]] / med[k[0]], med[k[0]] / med[k[2]]))
    say('(a) C=%d bytes: the store both forms read %.1f MB; the fused form writes %.1f MB (the map); the materialised form writes and reads %d x '
        '[C,769,769] fp32 (%.1f MB each, several times) and a [C,1024,2048] accumulator (%.1f MB)'
        % (Cc, store.numel() * 4 / 1e6, OH * OW / 1e6, T, Cc * TH * TW * 4 / 1e6, Cc * OH * OW * 4 / 1e6))

# ---- (b) the gather of one chunk ----
image = torch.randn((3, OH, OW), generator=g).to(dev)
arr = (L.TileDesc * B)()
for d, (y0, x0) in zip(arr, [(y, x) for y in ys for x in xs][:B]):
    d.image, d.H, d.W, d.y0, d.x0 = image.data_ptr(), OH, OW, y0, x0
table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
xbuf = torch.empty((B, 3, TH, TW), device=dev)
med = report(timed({'gather_tiles, %d windows of 3 x %d x %d' % (B, TH, TW):
                    lambda: L.check(lib.addk_gather_tiles(table.data_ptr(), B, 3, TH, TW, xbuf.data_ptr(), B, st))}), '(b) ')
nbytes = 2 * xbuf.numel() * 4
say('(b) %.1f MB read + written: %.0f GB/s' % (nbytes / 1e6, nbytes / 1e3 / list(med.values())[0]))

# ---- (c) end to end ----
img4 = image[None].contiguous()
t = timed({'TiledSegmenter.segment (B = %d: %d chunks)' % (B, -(-T // B)): lambda: tiled.segment(img4),
           'Segmenter.step at 1024 x 2048': lambda: whole.step(img4)}, reps=5, rounds=ROUNDS)
med = report(t, '(c) ')
k = list(med)
say('(c) ratio of the medians (tiled / whole): %.2f; pixels through the network: %.2f x (%d windows of %d x %d against %d x %d)'
    % (med[k[0]] / med[k[1]], T * TH * TW / (OH * OW), T, TH, TW, OH, OW))
say('(c) plan buffers: tiled %.1f MB (+ store %.1f MB), whole image %.1f MB' % (tiled.nbytes / 1e6, tiled._store.numel() * 4 / 1e6, whole.nbytes / 1e6))
tiled.close()
whole.close()
os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
