"""Validation pass with and without the boundary-band (trimap) metric, alternating in ONE process.

    python scripts/trimap_ab.py --shape 2,3,1024,2048 --steps 50 --repeats 3 [--F 20] [--out profiles/trimap_ab.txt]
    python scripts/trimap_ab.py --shape 2,3,1024,2048 --arm trimap --steps 20      # one arm only: the run to put under rocprofv3

Arm `plain` : addk.validate.ValidationStep as before (its plan is command for command the one without the keyword).
Arm `trimap`: the same step built with trimap=(1, 2, 4, 8, 16, 32): one boundary_dist launch per batch and one confusion_banded
              launch per exit more.
Both arms are warmed at the timed shape through the capture of their hipGraphs; a window of `steps` passes is timed with device
events and ends in a synchronise; windows alternate plain / trimap `repeats` times and the spread (min .. max of the per-step
means) is printed beside the median.  The targets are seeded Voronoi blobs with an ignore patch (contours as a label map has
them: a per-pixel random target would make every pixel an edge).  Before anything is timed the two arms' whole-image figures on
the timed batch are compared (they must be the same bits) and the band sizes are printed."""
import argparse
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

WIDTHS = (1, 2, 4, 8, 16, 32)


def build_model(F, dev):
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), ARCH_C2['low_level_layer'])
    fill_params(m, 600)
    return m.to(dev).eval()


def voronoi_targets(N, H, W, seed, sites=60):
    """int64 [N,H,W]: every pixel takes the class of the nearest of `sites` seeded points; a 5 % patch of ignore labels per image"""
    r = np.random.default_rng(seed)
    out = np.empty((N, H, W), dtype=np.int64)
    xx = np.arange(W)[None, :, None]
    for n in range(N):
        sy, sx, cls = r.integers(0, H, sites), r.integers(0, W, sites), r.integers(0, 19, sites)
        for y0 in range(0, H, 64):
            yy = np.arange(y0, min(H, y0 + 64))[:, None, None]
            out[n, y0:y0 + 64] = cls[((yy - sy) ** 2 + (xx - sx) ** 2).argmin(-1)]
        out[n, H // 8:H // 8 + H // 5, W // 6:W // 6 + W // 4] = 255
    return torch.from_numpy(out)


def kernels_alone(t, launches, say):
    """The two entry points alone on an idle device, back to back on one stream: device events around `launches` calls each."""
    import ctypes as C
    import addk._lib as L
    lib = L.load()
    dev = t.device
    N, H, W = t.shape
    st = torch.cuda.current_stream().cuda_stream
    dist = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(lib.addk_boundary_dist_ws_bytes(N, H, W)), dtype=torch.uint8, device=dev)
    pred = torch.randint(0, 19, (N, H, W), dtype=torch.uint8, device=dev)
    cm = torch.zeros((len(WIDTHS), 19, 19), dtype=torch.int64, device=dev)
    a = L.BoundaryDistArgs()
    a.target, a.N, a.OH, a.OW, a.C, a.radius, a.dist, a.ws = t.data_ptr(), N, H, W, 19, WIDTHS[-1], dist.data_ptr(), ws.data_ptr()
    b = L.ConfusionBandedArgs()
    b.target, b.pred, b.dist, b.N, b.OH, b.OW, b.C, b.nw = t.data_ptr(), pred.data_ptr(), dist.data_ptr(), N, H, W, 19, len(WIDTHS)
    for j, w in enumerate(WIDTHS):
        b.width[j] = w
    b.cm, b.image_stride = cm.data_ptr(), 0

    def timed(fn, arg, what):
        for _ in range(5):
            L.check(fn(C.byref(arg), st), what)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            L.check(fn(C.byref(arg), st), what)
        e1.record()
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / launches
    for radius in (WIDTHS[-1], 64):
        a.radius = radius
        say('alone: addk_boundary_dist radius %d: %.1f us per call (two kernels, %d calls back to back)' % (
            radius, timed(lib.addk_boundary_dist, a, 'boundary_dist'), launches))
    a.radius = WIDTHS[-1]
    L.check(lib.addk_boundary_dist(C.byref(a), st), 'boundary_dist')
    inside = float((dist <= WIDTHS[-1]).float().mean())
    say('alone: addk_confusion_banded %d widths, %.1f %% of the pixels inside the widest band: %.1f us per call' % (
        len(WIDTHS), 100.0 * inside, timed(lib.addk_confusion_banded, b, 'confusion_banded')))


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
    ap.add_argument('--arm', choices=['both', 'plain', 'trimap'], default='both')
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
    t = voronoi_targets(N, H, W, 5).to(dev)
    w = (torch.rand(19, generator=torch.Generator().manual_seed(4)) + 0.5).to(dev)
    say('trimap_ab: shape %s F=%d steps=%d warmup=%d repeats=%d arm=%s widths=%s' % (shape, a.F, a.steps, a.warmup, a.repeats, a.arm, WIDTHS))
    if a.arm == 'both':
        kernels_alone(t, 200, say)
    arms = ['plain', 'trimap'] if a.arm == 'both' else [a.arm]
    objs = {}
    for arm in arms:
        objs[arm] = ValidationStep(model, shape, class_weight=w, trimap=WIDTHS if arm == 'trimap' else None)
        for _ in range(max(a.warmup, 3)):
            objs[arm].step(x, t)
        torch.cuda.synchronize()
        assert objs[arm].graph is not None
        say('arm %-6s: %d launches in the plan' % (arm, len(objs[arm].g.fwd)))
    res = {}
    for arm in arms:
        objs[arm].reset()
        objs[arm].step(x, t)
        res[arm] = objs[arm].result()
    if a.arm == 'both':
        same = all(torch.equal(p['confusion'], q['confusion']) and p['loss'] == q['loss'] and p['confidence'] == q['confidence']
                   for p, q in zip(res['plain']['exits'], res['trimap']['exits']))
        say('whole-image figures of the two arms on the timed batch: %s' % ('equal bits' if same else 'DIFFERENT'))
    if 'trimap' in res:
        for i, e in enumerate(res['trimap']['exits']):
            say('exit %d: mIoU %.4f; within %s px: pixels %s, mIoU %s' % (i, e['mIoU'], list(WIDTHS), [b['pixels'] for b in e['trimap']],
                                                                         ['%.4f' % b['mIoU'] for b in e['trimap']]))
    times = {arm: [] for arm in arms}
    for rep in range(a.repeats):
        for arm in arms:
            objs[arm].reset()
            times[arm].append(window(objs[arm].step, x, t, a.steps))
            objs[arm].result()
    for arm in arms:
        ts = times[arm]
        say('arm %-6s: %.3f ms per validation step (median of %d windows of %d steps; min %.3f max %.3f)' % (
            arm, statistics.median(ts), len(ts), a.steps, min(ts), max(ts)))
    if a.arm == 'both':
        p, q = statistics.median(times['plain']), statistics.median(times['trimap'])
        say('trimap - plain = %.3f ms per step (%.2f %%); run-to-run spread plain %.3f ms, trimap %.3f ms' % (
            q - p, 100.0 * (q - p) / p, max(times['plain']) - min(times['plain']), max(times['trimap']) - min(times['trimap'])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
