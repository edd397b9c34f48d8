"""Cost of the soft-Dice region term in the fused loss head.  (a) Per-call time of addk_dice_stats and of addk_ce_upsample_dice_fwd_bwd
(alone, with a kept set, with a teacher) against the plain addk_ce_upsample_fwd_bwd at config 2's head shape, (2,19,128,256) ->
1024 x 2048: device events around REPS calls, ROUNDS rounds, the forms alternating in one warm process; median (min, max) per call.
(b) STEP=1: the captured config-2 training step (bench.py's model, batch and hyper-parameters) with dice=(1.0, 1.0) against the same step
with dice=None, two TrainSteps alternating in one process.
Run from the repository root on the MI355X:  python scripts/dice_time.py"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import addk._lib as L
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '50')), int(os.environ.get('ROUNDS', '10'))
STEPS, STEP_ROUNDS = int(os.environ.get('STEPS', '10')), int(os.environ.get('STEP_ROUNDS', '7'))
N, H, W, OH, OW, LD = 2, 128, 256, 1024, 2048, 20
st = torch.cuda.current_stream().cuda_stream


def timed(fns, reps, rounds):
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


# ---- (a) the launches ---------------------------------------------------------------------------------------------------------------
g = torch.Generator().manual_seed(3)


def logits():
    x = torch.zeros((N, H, W, LD))
    x[..., :19] = torch.randn((N, H, W, 19), generator=g) * 3
    return x.to(dev)


x, y = logits(), logits()
t = torch.randint(0, 19, (N, OH, OW), generator=g)
t[torch.rand((N, OH, OW), generator=g) < 0.05] = 255
t = t.to(dev)
lmap, tau, wk = torch.zeros((N, OH, OW), device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
counts = torch.zeros(2, dtype=torch.int64, device=dev)
sws = torch.zeros(int(lib.addk_ohem_select_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
wsum, ws1 = torch.zeros(1, device=dev), torch.zeros(int(lib.addk_ce_ws_floats(N, OH * OW)), device=dev)
L.check(lib.addk_ce_count(t.data_ptr(), N * OH * OW, None, 255, 19, wsum.data_ptr(), ws1.data_ptr(), st))
loss, kd, gr = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.zeros((N, H, W, LD), device=dev)
hws = torch.zeros(int(lib.addk_ce_upsample_kd_ws_floats(N, H, W)), device=dev)
s = L.OhemSelectArgs()
s.logits, s.ld, s.N, s.H, s.W, s.C, s.OH, s.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW
s.target, s.class_w, s.ignore_index, s.thresh, s.min_kept_total = t.data_ptr(), None, 255, 0.7, 100000 * N
s.pix_loss, s.tau, s.wsum_kept, s.counts, s.ws = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr(), sws.data_ptr()
L.check(lib.addk_ohem_select(C.byref(s), st))
coef, dout = torch.zeros(38, device=dev), torch.zeros(20, device=dev)
dws = torch.zeros(int(lib.addk_dice_stats_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
q = L.DiceStatsArgs()
q.logits, q.ld, q.N, q.H, q.W, q.C, q.OH, q.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW
q.target, q.ignore_index, q.weight, q.smooth, q.scale = t.data_ptr(), 255, 1.0, 1.0, 0.5
q.coef, q.dice_out, q.loss_out, q.ws = coef.data_ptr(), dout.data_ptr(), loss.data_ptr(), dws.data_ptr()
d = L.CeUpsampleDiceArgs()
a = d.kd.ce
a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW
a.target, a.class_w, a.ignore_index, a.wsum, a.scale, a.loss_out = t.data_ptr(), None, 255, wsum.data_ptr(), 0.5, loss.data_ptr()
a.g, a.ldg, a.accumulate, a.ws = gr.data_ptr(), LD, 0, hws.data_ptr()
d.coef = coef.data_ptr()
p = L.CeUpsampleArgs.from_buffer_copy(d.kd.ce)
do = L.CeUpsampleDiceArgs.from_buffer_copy(d)
do.kd.ce.wsum, do.kd.pix_loss, do.kd.tau = wk.data_ptr(), lmap.data_ptr(), tau.data_ptr()
dk = L.CeUpsampleDiceArgs.from_buffer_copy(d)
dk.kd.teacher, dk.kd.ld_teacher, dk.kd.alpha, dk.kd.temperature, dk.kd.nvalid, dk.kd.kd_out = y.data_ptr(), LD, 1.0, 4.0, wsum.data_ptr(), kd.data_ptr()
fns = {'ce_upsample': lambda: L.check(lib.addk_ce_upsample_fwd_bwd(C.byref(p), st)),
       'ce_upsample_dice': lambda: L.check(lib.addk_ce_upsample_dice_fwd_bwd(C.byref(d), st)),
       'dice_stats': lambda: L.check(lib.addk_dice_stats(C.byref(q), st)),
       'ce_upsample_dice + kept set': lambda: L.check(lib.addk_ce_upsample_dice_fwd_bwd(C.byref(do), st)),
       'ce_upsample_dice + teacher': lambda: L.check(lib.addk_ce_upsample_dice_fwd_bwd(C.byref(dk), st))}
fns['dice_stats']()                                            # the table the heads read
for f in fns.values():
    for _ in range(20):
        f()
torch.cuda.synchronize()
print('head (2,19,128,256) -> 1024 x 2048, weight 1, smooth 1: dice %.6f, %d classes present, kept %d of %d valid pixels'
      % (float(dout[0]), int((dout[1:] >= 0).sum()), int(counts[1]), int(counts[0])))
for name, v in timed(fns, REPS, ROUNDS).items():
    print('  %s: median %.2f us per call (min %.2f, max %.2f; %d rounds of %d)' % (name, statistics.median(v), min(v), max(v), ROUNDS, REPS))

# ---- (b) the captured config-2 step ------------------------------------------------------------------------------------------------
if os.environ.get('STEP', '0') == '1':
    import bench
    from addk.modeling.ADD import ADD
    from addk.train import TrainStep
    genotype = np.load(os.path.join(bench.ROOT, 'searched_arch', 'autodeeplab', 'genotype.npy'))
    xb, tb = bench.synthetic_batch(2, 1024, 2048, 1, dev)
    steps = {}
    for name, dice in (('plain', None), ('dice', (1.0, 1.0))):
        m = ADD(bench.NETWORK_ARCH, bench.C_INDEX, genotype, 19, bench.make_args(20), 0)
        bench.init_weights(m)
        m.to(dev)
        ts = TrainStep(m, (2, 3, 1024, 2048), lr=0.05, momentum=0.9, weight_decay=4e-5, nesterov=True, dice=dice)
        ts.load_batch(xb, tb)
        for _ in range(4):                  # eager + capture, then replays
            ts.step()
        torch.cuda.synchronize()
        assert ts.graph is not None
        steps[name] = ts
    times = timed({n_: v.step for n_, v in steps.items()}, STEPS, STEP_ROUNDS)
    for n_, v in times.items():
        print('config-2 step, %s: median %.3f ms (min %.3f, max %.3f; %d rounds of %d captured steps)'
              % (n_, statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3, STEP_ROUNDS, STEPS))
    print('dice_stats (term per exit):', [v[0] for v in steps['dice'].dice_stats()])
    print('loss plain %.6f, dice %.6f' % (steps['plain'].loss.item(), steps['dice'].loss.item()))
