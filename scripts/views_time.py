"""Per-launch time of the multi-view label head (label_views_upsample) against the materialised form of the same result, at config 2's
head shape with six views: (N,19,.,.) -> 1024 x 2048 from the scales 0.75 / 1 / 1.25 of a 128 x 256 map (96 x 192, 128 x 256, 160 x 320), each
plain and mirrored (the two halves of a batch-2N tensor), N = 1.  Materialised: six addk_resize_fwd to NCHW, then torch softmax, flip,
weighted sum and arg-max.  Device events around REPS passes, ROUNDS rounds, the two forms alternating in one process, warm; median (min ...
max) per pass, and the bytes each form allocates.  Run from the repository root on the MI355X:
    python scripts/views_time.py [out.txt]          (default profiles/label_views_heads.txt)"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
import addk._lib as L
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '20')), int(os.environ.get('ROUNDS', '10'))
N, OH, OW, LD = 1, 1024, 2048, 20
SIZES = ((96, 192), (128, 256), (160, 320))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'label_views_heads.txt')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


st = torch.cuda.current_stream().cuda_stream
g = torch.Generator().manual_seed(3)
maps = []
for h, w in SIZES:
    x = torch.zeros((2 * N, h, w, LD))
    x[..., :19] = torch.randn((2 * N, h, w, 19), generator=g) * 3
    maps.append(x.to(dev))
views = [(x, n0, mir) for x in maps for n0, mir in ((0, 0), (N, 1))]
wt = 1.0 / len(views)
# fused: one launch, one byte per pixel
labels = torch.zeros((N, OH, OW), dtype=torch.uint8, device=dev)
a = L.LabelViewsArgs()
for i, (x, n0, mir) in enumerate(views):
    v = a.view[i]
    v.logits, v.ld, v.n0, v.H, v.W, v.mirror, v.weight = x.data_ptr(), LD, n0, x.shape[1], x.shape[2], mir, wt
a.nview, a.N, a.C, a.OH, a.OW, a.lut256, a.labels = len(views), N, 19, OH, OW, None, labels.data_ptr()
# materialised: one [N,19,OH,OW] tensor per view, the accumulator and the int64 arg-max
ys = [torch.empty((N, 19, OH, OW), device=dev) for _ in views]
ras = []
for (x, n0, mir), y in zip(views, ys):
    ar = L.ResizeArgs()
    ar.src.x, ar.src.ld, ar.src.C = x[n0:].data_ptr(), LD, 19
    ar.N, ar.H, ar.W, ar.OH, ar.OW = N, x.shape[1], x.shape[2], OH, OW
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    ras.append(ar)
acc = torch.empty((N, 19, OH, OW), device=dev)
result = {}


def fused():
    L.check(lib.addk_label_views_upsample(C.byref(a), st))


def materialised():
    for ar in ras:
        L.check(lib.addk_resize_fwd(C.byref(ar), st))
    acc.zero_()
    for (x, n0, mir), y in zip(views, ys):
        p = torch.softmax(y, 1)
        acc.add_(p.flip(3) if mir else p, alpha=wt)
    result['am'] = acc.argmax(1)


fns = {'label_views_upsample (fused)': fused, 'materialised (6 resize_fwd + torch)': materialised}
for f in fns.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
same = float((result['am'].to(torch.uint8) == labels).float().mean())
say('views: %s, each plain + mirrored -> %d x %d, N = %d, weights 1/6; the two forms agree on %.4f %% of the pixels' % (SIZES, OH, OW, N, 100 * same))
assert same > 0.995
times = {k: [] for k in fns}
for _ in range(ROUNDS):
    for k, f in fns.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            f()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1000.0 / REPS)
for k, v in times.items():
    say('N=%d %s: median %.1f us per pass (min %.1f ... max %.1f; %d rounds of %d)' % (N, k, statistics.median(v), min(v), max(v), ROUNDS, REPS))
say('ratio of the medians (materialised / fused): %.1f' % (statistics.median(times[list(fns)[1]]) / statistics.median(times[list(fns)[0]])))
mb = lambda n: n / 1e6      # noqa: E731
say('allocated, fused: %.1f MB (the uint8 map)' % mb(labels.numel()))
say('allocated, materialised: %.1f MB (6 x [N,19,OH,OW] fp32 %.1f MB + accumulator %.1f MB + int64 arg-max %.1f MB), besides torch\'s softmax / flip temporaries'
    % (mb(sum(y.numel() for y in ys) * 4 + acc.numel() * 4 + N * OH * OW * 8), mb(sum(y.numel() for y in ys) * 4), mb(acc.numel() * 4), mb(N * OH * OW * 8)))
say('low-resolution logits both forms read: %.1f MB' % mb(sum(x.numel() for x in maps) * 4))
os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
