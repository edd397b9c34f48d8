"""Per-call time of the training heads and the label head at each class count they are compiled for (addk_head_classes: 19 and 21), at config 2's
head shape (2,C,128,256) -> 1024 x 2048 with the pixel stride the plan gives the classifier's output (C rounded up to a multiple of 4):
device events around REPS calls, ROUNDS rounds, the class counts of a head alternating in one warm process; median (min, max) per call
and the ratio to the first count.  Run from the repository root on the MI355X:  python scripts/heads_classes_time.py"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
import addk._lib as L
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '50')), int(os.environ.get('ROUNDS', '10'))
N, H, W, OH, OW = 2, 128, 256, 1024, 2048
st = torch.cuda.current_stream().cuda_stream
keep = []


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


def z(*shape, dtype=torch.float32):
    t = torch.zeros(shape, dtype=dtype, device=dev)
    keep.append(t)
    return t


def heads(nc):
    """name -> launch of every head at `nc` classes, on buffers of its own"""
    g = torch.Generator().manual_seed(3)
    ld = (nc + 3) // 4 * 4

    def logits(h=H, w=W, n=N):
        x = torch.zeros((n, h, w, ld))
        x[..., :nc] = torch.randn((n, h, w, nc), generator=g) * 3
        keep.append(x.to(dev))
        return keep[-1]

    def up(a, x):
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = x.data_ptr(), ld, N, H, W, nc, OH, OW
        keep.append(a)
        return a
    x, y = logits(), logits()
    t = torch.randint(0, nc, (N, OH, OW), generator=g)
    t[torch.rand((N, OH, OW), generator=g) < 0.05] = 255
    t = t.to(dev)
    keep.append(t)
    wsum, ws1 = z(1), z(int(lib.addk_ce_ws_floats(N, OH * OW)))
    L.check(lib.addk_ce_count(t.data_ptr(), N * OH * OW, None, 255, nc, wsum.data_ptr(), ws1.data_ptr(), st))
    loss, kd = z(1), z(1)
    # mining
    lmap, tau, wk, counts = z(N, OH, OW), z(1), z(1), z(2, dtype=torch.int64)
    s = up(L.OhemSelectArgs(), x)
    s.target, s.class_w, s.ignore_index, s.thresh, s.min_kept_total = t.data_ptr(), None, 255, 0.7, 100000 * N
    s.pix_loss, s.tau, s.wsum_kept, s.counts = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr()
    s.ws = z(int(lib.addk_ohem_select_ws_bytes(N, OH, OW)), dtype=torch.uint8).data_ptr()
    # the Dice reduction
    coef, dout = z(2 * nc), z(1 + nc)
    q = up(L.DiceStatsArgs(), x)
    q.target, q.ignore_index, q.weight, q.smooth, q.scale = t.data_ptr(), 255, 1.0, 1.0, 0.5
    q.coef, q.dice_out, q.loss_out = coef.data_ptr(), dout.data_ptr(), loss.data_ptr()
    q.ws = z(int(lib.addk_dice_stats_ws_bytes_classes(N, OH, OW, nc)), dtype=torch.uint8).data_ptr()
    # the loss heads

    def ce(a):
        up(a, x)
        a.target, a.class_w, a.ignore_index, a.wsum, a.scale, a.loss_out = t.data_ptr(), None, 255, wsum.data_ptr(), 0.5, loss.data_ptr()
        a.g, a.ldg, a.accumulate, a.ws = z(N, H, W, ld).data_ptr(), ld, 0, z(int(lib.addk_ce_upsample_kd_ws_floats(N, H, W))).data_ptr()
    p = L.CeUpsampleArgs()
    ce(p)
    po = L.CeUpsampleOhemArgs()
    ce(po.ce)
    po.ce.wsum, po.pix_loss, po.tau = wk.data_ptr(), lmap.data_ptr(), tau.data_ptr()
    pk = L.CeUpsampleKdArgs()
    ce(pk.ce)
    pk.teacher, pk.ld_teacher, pk.alpha, pk.temperature, pk.nvalid, pk.kd_out = y.data_ptr(), ld, 1.0, 4.0, wsum.data_ptr(), kd.data_ptr()
    pd = L.CeUpsampleDiceArgs()
    ce(pd.kd.ce)
    pd.coef = coef.data_ptr()
    keep.extend([po, pk, pd])
    # inference
    lab = z(N, OH, OW, dtype=torch.uint8)
    la = up(L.LabelUpsampleArgs(), x)
    la.lut256, la.labels = None, lab.data_ptr()

    def call(fn, a):
        return lambda: L.check(fn(C.byref(a), st))
    fns = {'ohem_select': call(lib.addk_ohem_select, s), 'dice_stats': call(lib.addk_dice_stats, q),
           'ce_upsample': call(lib.addk_ce_upsample_fwd_bwd, p), 'ce_upsample_ohem': call(lib.addk_ce_upsample_ohem_fwd_bwd, po),
           'ce_upsample_kd': call(lib.addk_ce_upsample_kd_fwd_bwd, pk), 'ce_upsample_dice': call(lib.addk_ce_upsample_dice_fwd_bwd, pd),
           'label_upsample': call(lib.addk_label_upsample, la)}
    fns['ohem_select'](), fns['dice_stats']()                      # the kept set and the table the heads read
    return fns


classes = L.head_classes()
per = {nc: heads(nc) for nc in classes}
for fns in per.values():
    for f in fns.values():
        for _ in range(10):
            f()
torch.cuda.synchronize()
print('heads at (2,C,128,256) -> 1024 x 2048, pixel stride C rounded up to 4; us per call, median (min, max) of %d rounds of %d' % (ROUNDS, REPS))
for name in per[classes[0]]:
    res = timed({nc: per[nc][name] for nc in classes}, REPS, ROUNDS)
    med = {nc: statistics.median(v) for nc, v in res.items()}
    print('  %-32s %s   ratio %s' % (name, '   '.join('C=%d: %.1f (%.1f, %.1f)' % (nc, med[nc], min(res[nc]), max(res[nc])) for nc in res),
                                     ' '.join('%.3f' % (med[nc] / med[classes[0]]) for nc in list(res)[1:])))
