"""Per-window early exits of the sliding window against the static tile plans, alternating in ONE process.

    python scripts/tiled_gate_bench.py [--size 1024x2048] [--images 2] [--steps 3] [--repeats 5] [--F 20] [--out profiles/tiled_gate_bench.txt]

Set-up: synthetic images of different contrast, 769 x 769 windows at stride 513 (8 windows per 1024 x 2048 image), B = 4, config 2.
Forms:
  s/final, s/exit0 : the static TiledSegmenter at the last exit and at exit 0
  g/stay, g/leave  : the gated TiledSegmenter ('entropy') at a threshold no window passes / every window passes
  g/half           : the threshold at the median of the windows' gate-0 values, which the script reads first and requires to differ
  l/gate, l/scatter, l/park, l/unpark : the new launches alone on the plan's buffers at B rows — the gate of one chunk, the scatter of B
                     rows of logits into the store, the live state behind gate 0 of B rows into the pool and back (each `addk_gather_rows`
                     launch includes its host read-back of the item table); the bytes moved are printed beside them
Every form is warmed at the timed shape (the plans capture their hipGraphs on the third run of a stage); a window of `steps` calls is
timed with device events and ends in a synchronise; windows alternate over the forms `repeats` times; median and min .. max of the
per-call means are printed.  Nothing here is asserted but what the set-up needs."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import addk                                                      # noqa: E402,F401
from addk import _lib as L                                       # noqa: E402
from addk import plan as _plan                                   # noqa: E402
from addk.dynamic import gather_rows                             # noqa: E402
from addk.synth import fill_params, rand_tensor                  # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args       # noqa: E402

FORCE, FORBID = float('inf'), float('-inf')
TILE, STRIDE = (4, 3, 769, 769), (513, 513)


def build_model(F, dev):
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), ARCH_C2['low_level_layer'])
    fill_params(m, 600)
    return m.to(dev).eval()


def window(call, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='1024x2048')
    ap.add_argument('--images', type=int, default=2)
    ap.add_argument('--F', type=int, default=20)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--tile', type=int, default=TILE[2])
    ap.add_argument('--stride', type=int, default=STRIDE[0])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU: there is no CPU fallback'
    from addk.segment import TiledSegmenter
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    H, W = (int(v) for v in a.size.split('x'))
    tile, stride = (TILE[0], 3, a.tile, a.tile), (a.stride, a.stride)
    B = tile[0]
    model = build_model(a.F, dev)
    # images of different contrast, so that their windows' gate values differ
    x = [(rand_tensor(5 + i, 'tg_bench_x', (3, H, W)) * (0.5 * 2 ** i)).to(dev) for i in range(a.images)]
    say('tiled_gate_bench: %d images of %dx%d, windows %d at stride %d, B=%d F=%d steps=%d warmup=%d repeats=%d'
        % (a.images, H, W, a.tile, a.stride, B, a.F, a.steps, a.warmup, a.repeats))
    static = {e: TiledSegmenter(model, tile, stride, exit=e) for e in (-1, 0)}
    seg = TiledSegmenter(model, tile, stride, threshold=FORBID)
    seg.segment(x)
    T = len(seg.tiles)
    vals = sorted(float(v) for v in seg.values[:, 0])
    say('%d windows; gate values at exit 0: %s' % (T, ' '.join('%.6g' % v for v in vals)))
    assert vals[T // 2 - 1] < vals[T // 2], 'the two middle gate values coincide: no threshold lets half of the windows leave'
    mid = 0.5 * (vals[T // 2 - 1] + vals[T // 2])
    forms = {'s/final': lambda: static[-1].segment(x), 's/exit0': lambda: static[0].segment(x),
             'g/stay': lambda: seg.segment(x, threshold=FORBID), 'g/leave': lambda: seg.segment(x, threshold=FORCE),
             'g/half': lambda: seg.segment(x, threshold=mid)}
    for name, call in forms.items():
        for _ in range(max(a.warmup, 4)):
            call()
    torch.cuda.synchronize()
    seg.segment(x, threshold=mid)
    exits = seg.exits.tolist()
    assert exits.count(0) == T // 2, exits
    say('g/half exits: %s; trace (stage, rows): %s; plan %.1f MB + pools %.1f MB' % (exits, seg.trace, seg.g.nbytes / 1e6, seg.plan.pool_bytes / 1e6))
    # the new launches alone, at B rows
    plan = seg.plan
    gate = [plan.g.fwd[plan.cuts[0] - 1]]
    assert gate[0].name == 'gate_tiles_upsample'
    # index words of this script's own (rows 0..B-1 -> tiles / ring slots 0..B-1): the segmenter's ring of index words is rewritten by every
    # call of the gated forms, with tile indices that are no ring slot of a pool
    idx = torch.arange(B, dtype=torch.int32, device=dev).repeat(2, 1).contiguous()
    src = plan.outs[0].src.raw
    h, w = seg.low
    sa = L.ScatterTileLogitsArgs()
    sa.src, sa.lds, sa.B, sa.store, sa.ld, sa.T = src.ptr, src.ld, B, seg._store.data_ptr(), seg.ld, seg._store.shape[0]
    sa.h, sa.w, sa.C, sa.src_row, sa.dst_tile, sa.n = h, w, seg.ncls, idx[0].data_ptr(), idx[1].data_ptr(), B
    state = sum(4 * (b.n // B) for b in plan.pools[0][0]) + 8
    moved = {'l/scatter': 4 * h * w * seg.ncls * B, 'l/park': state * B, 'l/unpark': state * B}
    say('live state behind gate 0: %d buffers, %.3f MB per window; a window\'s logits: %.3f MB' % (len(plan.pools[0][0]), state / 1e6, 4 * h * w * seg.ncls / 1e6))
    forms['l/gate'] = lambda: plan.g.run(gate, _plan.current_stream())
    forms['l/scatter'] = lambda: seg._launch('scatter_tile_logits', C.byref(sa))
    forms['l/park'] = lambda: gather_rows(seg.g, plan.park[0], idx[0], idx[1], B)
    forms['l/unpark'] = lambda: gather_rows(seg.g, plan.unpark[0], idx[0], None, B)
    for name in ('l/gate', 'l/scatter', 'l/park', 'l/unpark'):
        for _ in range(4):
            forms[name]()
    times = {name: [] for name in forms}
    for rep in range(a.repeats):
        for name, call in forms.items():
            times[name].append(window(call, a.steps * (20 if name.startswith('l/') else 1)))
    for name, ts in times.items():
        extra = ''
        if name in moved:
            extra = '  = %.1f GB/s of rows moved (x2 for read + write traffic)' % (moved[name] / statistics.median(ts) / 1e6)
        say('%-9s %.3f ms per call (median of %d windows; min %.3f max %.3f)%s' % (name, statistics.median(ts), len(ts), min(ts), max(ts), extra))
    med = {k: statistics.median(v) for k, v in times.items()}
    say('g/stay - s/final = %+.3f ms (%+.2f %%: the cost of the feature when nobody leaves); g/leave - s/exit0 = %+.3f ms; g/half - s/final = %+.3f ms'
        % (med['g/stay'] - med['s/final'], 100 * (med['g/stay'] / med['s/final'] - 1), med['g/leave'] - med['s/exit0'], med['g/half'] - med['s/final']))
    for s in list(static.values()) + [seg]:
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
