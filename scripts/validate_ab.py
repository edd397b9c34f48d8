"""Validation pass, fused against hand-assembled, alternating in ONE process (DESIGN.md 'Validation step').

    python scripts/validate_ab.py --shape 2,3,1024,2048 --steps 50 --repeats 3 [--F 20] [--out profiles/validate_ab.txt]
    python scripts/validate_ab.py --shape 2,3,1024,2048 --arm fused --steps 20      # one arm only: the run to put under rocprofv3

Arm `fused`: addk.validate.ValidationStep (one captured plan, one addk_score_upsample launch per exit).
Arm `hand` : the path a user assembles from the drop-in pieces — model.eval()(x), CrossEntropyLoss, argmax_logits, Evaluator,
             normalized_shannon_entropy (one host sync per exit and batch, as in the reference's loop).
Both arms are warmed at the timed shape (the plans capture their hipGraphs on the third call); a window of `steps` passes is
timed with device events and ends in a synchronise; windows alternate fused / hand `repeats` times and the spread (min .. max
of the per-step means) is printed beside the median.  Peak allocated memory is taken per arm with the other arm's objects
released.  The two arms' results on the timed batch are compared before anything is timed."""
import argparse
import gc
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import addk                                                      # noqa: E402,F401
from addk.synth import fill_params, rand_tensor                  # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args       # noqa: E402


def build_model(F, dev):
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), ARCH_C2['low_level_layer'])
    fill_params(m, 600)
    return m.to(dev).eval()


class Hand:
    def __init__(self, model, weight, dev):
        from addk.loss import CrossEntropyLoss
        from addk.metrics import Evaluator
        self.model, self.dev = model, dev
        self.crit = CrossEntropyLoss(weight=weight, ignore_index=255).to(dev)
        self.evs = None
        self.Evaluator = Evaluator
        self.reset()

    def reset(self):
        self.test_loss, self.conf = 0.0, None
        if self.evs:
            for e in self.evs:
                e.reset()

    def step(self, x, t):
        from addk.metrics import argmax_logits
        from addk.modeling.operations import normalized_shannon_entropy
        with torch.no_grad():
            outs = self.model(x)
        if self.evs is None:
            self.evs = [self.Evaluator(19, self.dev) for _ in outs]
        if self.conf is None:
            self.conf = [[] for _ in outs]
        self.test_loss += (sum(self.crit(o, t) for o in outs) / len(outs)).item()
        for i, o in enumerate(outs):
            self.evs[i].add_batch(t, argmax_logits(o))
            self.conf[i].append(normalized_shannon_entropy(o))

    def result(self):
        return dict(test_loss=self.test_loss, mIoU=[e.Mean_Intersection_over_Union() for e in self.evs],
                    confidence=[sum(c) / len(c) for c in self.conf], cm=[e._cm.clone() for e in self.evs])


def window(step, x, t, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        step(x, t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='2,3,1024,2048')
    ap.add_argument('--F', type=int, default=20)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--arm', choices=['both', 'fused', 'hand'], default='both')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU: there is no CPU fallback'
    dev = torch.device('cuda:0')
    shape = tuple(int(v) for v in a.shape.split(','))
    N, _, H, W = shape
    from addk.validate import ValidationStep
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    model = build_model(a.F, dev)
    x = rand_tensor(5, 'val_x', shape).to(dev)
    r = np.random.default_rng(5)
    t = torch.from_numpy(r.integers(0, 19, (N, H, W))).long()
    t[torch.from_numpy(r.random((N, H, W)) < 0.05)] = 255
    t = t.to(dev)
    w = (torch.rand(19, generator=torch.Generator().manual_seed(4)) + 0.5).to(dev)
    say('validate_ab: shape %s F=%d steps=%d warmup=%d repeats=%d arm=%s' % (shape, a.F, a.steps, a.warmup, a.repeats, a.arm))

    peak = {}

    def make(arm):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        obj = ValidationStep(model, shape, class_weight=w) if arm == 'fused' else Hand(model, w, dev)
        for _ in range(max(a.warmup, 3)):
            obj.step(x, t)
        torch.cuda.synchronize()
        peak[arm] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        return obj

    arms = ['fused', 'hand'] if a.arm == 'both' else [a.arm]
    # memory: each arm alone on the shared model
    objs = {}
    for arm in arms:
        objs[arm] = make(arm)
        say('peak allocated above the model, arm %-5s: %.1f MiB' % (arm, peak[arm]))
        if a.arm == 'both':
            if arm == 'hand':
                model._plans().clear()
            objs[arm] = None
    if a.arm == 'both':
        for arm in arms:
            objs[arm] = make(arm)
        # same figures first
        for o in objs.values():
            o.reset()
            o.step(x, t)
        rf, rh = objs['fused'].result(), objs['hand'].result()
        dcm = [int((e['confusion'] - c).abs().sum()) for e, c in zip(rf['exits'], rh['cm'])]
        say('agreement on the timed batch: test_loss %.8g vs %.8g (rel %.2g); confidence %s vs %s; sum|dcm| per exit %s; mIoU %s vs %s' % (
            rf['test_loss'], rh['test_loss'], abs(rf['test_loss'] - rh['test_loss']) / abs(rh['test_loss']),
            ['%.8g' % e['confidence'] for e in rf['exits']], ['%.8g' % c for c in rh['confidence']], dcm,
            [e['mIoU'] for e in rf['exits']], rh['mIoU']))
    times = {arm: [] for arm in arms}
    for rep in range(a.repeats):
        for arm in arms:
            objs[arm].reset()
            times[arm].append(window(objs[arm].step, x, t, a.steps))
            objs[arm].result()
    for arm in arms:
        ts = times[arm]
        say('arm %-5s: %.3f ms per validation step (median of %d windows of %d steps; min %.3f max %.3f)' % (
            arm, statistics.median(ts), len(ts), a.steps, min(ts), max(ts)))
    if a.arm == 'both':
        f, h = statistics.median(times['fused']), statistics.median(times['hand'])
        say('hand - fused = %.3f ms per step (%.2fx); run-to-run spread fused %.3f ms, hand %.3f ms' % (
            h - f, h / f, max(times['fused']) - min(times['fused']), max(times['hand']) - min(times['hand'])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
