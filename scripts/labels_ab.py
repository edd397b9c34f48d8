"""Label-map inference against logits + arg-max, alternating in ONE process.

    python scripts/labels_ab.py --sizes 1024x2048,1025x2049 --steps 20 --repeats 3 [--F 20] [--out profiles/labels_ab.txt]
    python scripts/labels_ab.py --sizes 1024x2048 --arm B --steps 10          # arm B only: the run to put under rocprofv3

Points, each at every size:
  dyn/exit, dyn/stay : ADD.dynamic_inference(x, thr, 'entropy') at bs = 1 with a threshold that forces / forbids the early exit
  seg                : the last exit at N = 2
Arms:
  A  : what a caller does today — output='logits' (dyn) or model(x)[-1] (seg), then addk_argmax_nchw on the result
  A0 : A without its arg-max launch (the bar the issue sets for B)
  B  : output='labels' (dyn) or Segmenter(exit=-1).step (seg)
Every arm is warmed at the timed shape (the plans capture their hipGraphs on the third call); a window of `steps` calls is timed
with device events and ends in a synchronise; windows alternate A A0 B `repeats` times; median and min .. max of the per-call
means are printed.  Peak allocated memory above the model is taken per arm with the other arms' plans released.  A's and B's
maps are compared before anything is timed."""
import argparse
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import addk                                                      # noqa: E402,F401
import addk._lib as L                                            # noqa: E402
from addk.synth import fill_params, rand_tensor                  # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args       # noqa: E402

FORCE, FORBID = float('inf'), float('-inf')


def build_model(F, dev):
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), ARCH_C2['low_level_layer'])
    fill_params(m, 600)
    return m.to(dev).eval()


class ArgMax:
    """addk_argmax_nchw into a resident int64 map: the launch a caller adds behind the logits"""

    def __init__(self):
        self.lib, self.out = L.load(), None

    def __call__(self, y):
        N, Cc, H, W = y.shape
        if self.out is None or tuple(self.out.shape) != (N, H, W):
            self.out = torch.empty((N, H, W), dtype=torch.int64, device=y.device)
        L.check(self.lib.addk_argmax_nchw(y.data_ptr(), N, Cc, H * W, self.out.data_ptr(), torch.cuda.current_stream().cuda_stream), 'argmax')
        return self.out


def make_arm(point, arm, model, x):
    """-> a callable that runs one call of (point, arm) and returns its map (or logits for A0)"""
    am = ArgMax()
    if point.startswith('dyn'):
        thr = FORCE if point == 'dyn/exit' else FORBID
        if arm == 'B':
            return lambda: model.dynamic_inference(x, thr, 'entropy', output='labels')[0]
        if arm == 'A0':
            return lambda: model.dynamic_inference(x, thr, 'entropy')[0]
        return lambda: am(model.dynamic_inference(x, thr, 'entropy')[0])
    if arm == 'B':
        from addk.segment import Segmenter
        seg = Segmenter(model, tuple(x.shape), exit=-1)
        return lambda: seg.step(x)

    def logits():
        with torch.no_grad():
            return model(x)[-1]
    return logits if arm == 'A0' else (lambda: am(logits()))


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
    ap.add_argument('--sizes', default='1024x2048,1025x2049')
    ap.add_argument('--points', default='dyn/exit,dyn/stay,seg')
    ap.add_argument('--F', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--arm', choices=['all', 'A', 'A0', 'B'], default='all')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU: there is no CPU fallback'
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    model = build_model(a.F, dev)
    arms = ['A', 'A0', 'B'] if a.arm == 'all' else [a.arm]
    say('labels_ab: sizes %s points %s F=%d steps=%d warmup=%d repeats=%d arms=%s' % (a.sizes, a.points, a.F, a.steps, a.warmup, a.repeats, arms))
    for size in a.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        for point in a.points.split(','):
            n = 1 if point.startswith('dyn') else 2
            x = rand_tensor(5, 'labels_x', (n, 3, H, W)).to(dev)
            tag = '%s %dx%d N=%d' % (point, H, W, n)

            def fresh(arm):
                model._plans().clear()
                gc.collect()
                torch.cuda.empty_cache()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                call = make_arm(point, arm, model, x)
                for _ in range(max(a.warmup, 4)):
                    call()
                torch.cuda.synchronize()
                return call, (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            # memory: each arm alone on the shared model
            for arm in arms:
                call, peak = fresh(arm)
                say('%s: peak allocated above the model, arm %-2s: %.1f MiB' % (tag, arm, peak))
                del call
            # all arms side by side (their plans have different cache keys), warmed
            model._plans().clear()
            calls = {}
            for arm in arms:
                calls[arm] = make_arm(point, arm, model, x)
                for _ in range(max(a.warmup, 4)):
                    calls[arm]()
            torch.cuda.synchronize()
            if 'A' in calls and 'B' in calls:
                ma, mb = calls['A']().clone(), calls['B']().clone()
                torch.cuda.synchronize()
                say('%s: maps of A and B differ in %d of %d pixels' % (tag, int((ma != mb.long()).sum()), ma.numel()))
            times = {arm: [] for arm in arms}
            for rep in range(a.repeats):
                for arm in arms:
                    times[arm].append(window(calls[arm], a.steps))
            for arm in arms:
                ts = times[arm]
                say('%s: arm %-2s %.3f ms per call (median of %d windows of %d calls; min %.3f max %.3f)' % (
                    tag, arm, statistics.median(ts), len(ts), a.steps, min(ts), max(ts)))
            if a.arm == 'all':
                ma_, m0, mb_ = (statistics.median(times[k]) for k in ('A', 'A0', 'B'))
                say('%s: A - B = %.3f ms, A0 - B = %.3f ms (%s the bar B <= A0)' % (tag, ma_ - mb_, m0 - mb_, 'meets' if mb_ <= m0 else 'MISSES'))
            del calls
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
