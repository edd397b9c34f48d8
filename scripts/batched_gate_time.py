"""Batched dynamic inference against what a caller had before, alternating in ONE process.

    python scripts/batched_gate_time.py --size 1024x2048 --steps 10 --repeats 5 [--F 20] [--out profiles/batched_gate_time.txt]

Forms, config 2 at N = 4:
  a/exit, a/stay   : four sequential single-image ADD.dynamic_inference(x[i:i+1], thr, 'entropy', output='labels') calls at a threshold
                     that forces / forbids the early exit
  b/exit0, b/final : Segmenter at batch 4 for exit 0 and for the final exit
  c/4, c/2, c/0    : BatchedGate.run with 4, 2 and 0 of the 4 images leaving at gate 0 (c/2: the threshold sits between the second and
                     third of the four gate values, which the script reads first and requires to differ)
  d/gather, d/copy : the state transition 4 -> 2 alone: the ONE addk_gather_rows launch (its host read-back of the item table included),
                     and the same rows moved by one device-to-device copy per row and buffer (torch copy_ of a contiguous row: one
                     hipMemcpyAsync each); the bytes they move are printed beside them
Every form is warmed at the timed shape (the plans capture their hipGraphs on the third call); a window of `steps` calls is timed
with device events and ends in a synchronise; windows alternate over the forms `repeats` times; median and min .. max of the per-call
means are printed.  Nothing here is asserted."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import addk                                                      # noqa: E402,F401
from addk.synth import fill_params, rand_tensor                  # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args       # noqa: E402

FORCE, FORBID = float('inf'), float('-inf')


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
    ap.add_argument('--F', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU: there is no CPU fallback'
    from addk.dynamic import BatchedGate
    from addk.segment import Segmenter
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    H, W = (int(v) for v in a.size.split('x'))
    N = 4
    model = build_model(a.F, dev)
    # four images of different contrast, so that their gate values differ
    x = torch.cat([rand_tensor(5 + i, 'bg_time_x', (1, 3, H, W)) * c for i, c in enumerate((0.5, 1.0, 2.0, 4.0))]).to(dev)
    say('batched_gate_time: %dx%d N=%d F=%d steps=%d warmup=%d repeats=%d' % (H, W, N, a.F, a.steps, a.warmup, a.repeats))
    bg = BatchedGate(model, (N, 3, H, W), 'entropy')
    _, exits, values = bg.run(x, FORBID)
    vals = sorted(float(v) for v in values[:, 0])
    say('gate values at exit 0: %s' % ' '.join('%.9g' % v for v in vals))
    assert vals[1] < vals[2], 'the second and third gate value coincide: no threshold lets exactly two images leave'
    mid = 0.5 * (vals[1] + vals[2])
    assert vals[1] < mid < vals[2]
    segs = {0: Segmenter(model, (N, 3, H, W), exit=0), -1: Segmenter(model, (N, 3, H, W), exit=-1)}

    def singles(thr):
        for i in range(N):
            model.dynamic_inference(x[i:i + 1], thr, 'entropy', output='labels')
    forms = {'a/exit': lambda: singles(FORCE), 'a/stay': lambda: singles(FORBID),
             'b/exit0': lambda: segs[0].step(x), 'b/final': lambda: segs[-1].step(x),
             'c/4': lambda: bg.run(x, FORCE), 'c/2': lambda: bg.run(x, mid), 'c/0': lambda: bg.run(x, FORBID)}
    for name, call in forms.items():
        for _ in range(max(a.warmup, 4)):
            call()
    torch.cuda.synchronize()
    _, exits, _ = bg.run(x, mid)
    assert sorted(exits.tolist()) == [0, 0, 1, 1], exits
    say('c/2 exits: %s; sub-plan bytes: %s' % (exits.tolist(), bg.nbytes))
    # the transition of that call, alone
    (m_, n_, k_, stay), = bg.moves
    table = bg.tables[('state', m_, n_, k_)]
    pairs = table[2]
    moved = sum(4 * words for _, _, words in pairs) * len(stay)
    say('state transition %d -> %d behind gate %d: %d buffers, %.3f MB per image, %.3f MB moved (read once, written once)' % (
        m_, n_, k_, len(pairs), sum(4 * w for _, _, w in pairs) / 1e6, moved / 1e6))
    src_row = bg._idx.dev[k_][2]
    views = [(x_.t[:m_ * w].view(m_, w), y_.t[:n_ * w].view(n_, w)) for x_, y_, w in pairs]

    def copies():
        for s, d in views:
            for r, i in enumerate(stay):
                d[r].copy_(s[i], non_blocking=True)
    forms['d/gather'] = lambda: bg._gather('state', bg.sub(n_), table, src_row, None, len(stay))
    forms['d/copy'] = copies
    for name in ('d/gather', 'd/copy'):
        for _ in range(4):
            forms[name]()
    times = {name: [] for name in forms}
    for rep in range(a.repeats):
        for name, call in forms.items():
            times[name].append(window(call, a.steps * (10 if name.startswith('d/') else 1)))
    for name, ts in times.items():
        extra = ''
        if name.startswith('d/'):
            extra = '  = %.1f GB/s of rows moved (x2 for read + write traffic)' % (moved / statistics.median(ts) / 1e6)
        say('%-8s %.3f ms per call (median of %d windows; min %.3f max %.3f)%s' % (name, statistics.median(ts), len(ts), min(ts), max(ts), extra))
    med = {k: statistics.median(v) for k, v in times.items()}
    say('c/2 - b/final = %+.3f ms; c/0 - b/final = %+.3f ms; c/4 - b/exit0 = %+.3f ms; a/stay - c/0 = %+.3f ms; a/exit - c/4 = %+.3f ms' % (
        med['c/2'] - med['b/final'], med['c/0'] - med['b/final'], med['c/4'] - med['b/exit0'], med['a/stay'] - med['c/0'],
        med['a/exit'] - med['c/4']))
    bg.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
