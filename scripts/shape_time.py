"""Per-call time of the focal and label-smoothed loss heads (addk_ce_upsample_shaped_fwd_bwd) beside the heads they stand in for, at config
2's head shape (2,C,128,256) -> 1024 x 2048 with the pixel stride the plan gives the classifier's output (C rounded up to a multiple of 4),
the method of scripts/heads_classes_time.py: device events around REPS calls, ROUNDS rounds, all forms of a class count alternating in one
warm process; median (min, max) per call and the ratio to the unshaped head of the same row.  The unshaped kernels are the parent commit's,
instruction for instruction.  Run from the repository root on the MI355X:  python scripts/shape_time.py"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
import addk._lib as L
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '50')), int(os.environ.get('ROUNDS', '10'))
N, H, W, OH, OW = 2, 128, 256, 1024, 2048
GAMMA, EPS = 2.0, 0.1
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


def heads(nc, weighted):
    """(row, form) -> launch, on buffers of its own; rows: the head alone, with a kept set, with a Dice table, with both"""
    g = torch.Generator().manual_seed(3)
    ld = (nc + 3) // 4 * 4
    x = torch.zeros((N, H, W, ld))
    x[..., :nc] = torch.randn((N, H, W, nc), generator=g) * 3
    x = x.to(dev)
    t = torch.randint(0, nc, (N, OH, OW), generator=g)
    t[torch.rand((N, OH, OW), generator=g) < 0.05] = 255
    t = t.to(dev)
    cw = (torch.rand(nc, generator=g) + 0.5).to(dev) if weighted else None
    cwp = cw.data_ptr() if weighted else None
    keep.extend([x, t, cw])
    wsum, ws1 = z(1), z(int(lib.addk_ce_ws_floats(N, OH * OW)))
    L.check(lib.addk_ce_count(t.data_ptr(), N * OH * OW, cwp, 255, nc, wsum.data_ptr(), ws1.data_ptr(), st))
    loss = z(1)

    def up(a):
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = x.data_ptr(), ld, N, H, W, nc, OH, OW
        keep.append(a)
        return a
    lmap, tau, wk, counts = z(N, OH, OW), z(1), z(1), z(2, dtype=torch.int64)
    s = up(L.OhemSelectArgs())
    s.target, s.class_w, s.ignore_index, s.thresh, s.min_kept_total = t.data_ptr(), cwp, 255, 0.7, 100000 * N
    s.pix_loss, s.tau, s.wsum_kept, s.counts = lmap.data_ptr(), tau.data_ptr(), wk.data_ptr(), counts.data_ptr()
    s.ws = z(int(lib.addk_ohem_select_ws_bytes(N, OH, OW)), dtype=torch.uint8).data_ptr()
    coef, dout = z(2 * nc), z(1 + nc)
    q = up(L.DiceStatsArgs())
    q.target, q.ignore_index, q.weight, q.smooth, q.scale = t.data_ptr(), 255, 1.0, 1.0, 0.5
    q.coef, q.dice_out, q.loss_out = coef.data_ptr(), dout.data_ptr(), loss.data_ptr()
    q.ws = z(int(lib.addk_dice_stats_ws_bytes_classes(N, OH, OW, nc)), dtype=torch.uint8).data_ptr()
    L.check(lib.addk_ohem_select(C.byref(s), st))
    L.check(lib.addk_dice_stats(C.byref(q), st))

    def form(shape, mined, table):
        a = L.CeUpsampleShapedArgs()
        ce = a.dice.kd.ce
        up(ce)
        keep.append(a)
        ce.target, ce.class_w, ce.ignore_index, ce.scale, ce.loss_out = t.data_ptr(), cwp, 255, 0.5, loss.data_ptr()
        ce.wsum = (wk if mined else wsum).data_ptr()
        ce.g, ce.ldg, ce.accumulate, ce.ws = z(N, H, W, ld).data_ptr(), ld, 0, z(int(lib.addk_ce_upsample_ws_floats(N, H, W))).data_ptr()
        if mined:
            a.dice.kd.pix_loss, a.dice.kd.tau = lmap.data_ptr(), tau.data_ptr()
        if table:
            a.dice.coef = coef.data_ptr()
        a.shape, a.gamma, a.eps = shape, GAMMA, EPS
        return lambda: L.check(lib.addk_ce_upsample_shaped_fwd_bwd(C.byref(a), st))
    rows = {'alone': (False, False), 'kept set': (True, False), 'dice table': (False, True), 'kept set + dice table': (True, True)}
    shapes = {'unshaped': L.CE_SHAPE_NONE, 'focal': L.CE_SHAPE_FOCAL, 'smooth': L.CE_SHAPE_SMOOTH}
    return {(r, f): form(sh, *rows[r]) for r in rows for f, sh in shapes.items()}


for nc in L.head_classes():
    for weighted in (False, True):
        fns = heads(nc, weighted)
        for f in fns.values():
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        print('loss heads at (2,%d,128,256) -> 1024 x 2048, %s; gamma = %g, eps = %g; us per call, median (min, max) of %d rounds of %d'
              % (nc, 'class weights' if weighted else 'no class weights', GAMMA, EPS, ROUNDS, REPS))
        res = timed(fns, REPS, ROUNDS)
        med = {k: statistics.median(v) for k, v in res.items()}
        for row in dict.fromkeys(r for r, _ in fns):
            print('  %-22s %s' % (row, '   '.join('%s %.1f (%.1f, %.1f)%s' % (f, med[row, f], min(res[row, f]), max(res[row, f]),
                                                                               '' if f == 'unshaped' else ' x%.3f' % (med[row, f] / med[row, 'unshaped']))
                                                 for r, f in fns if r == row)))
        del keep[:]
