"""Per-launch time of the three heads on the low-resolution logits (score_upsample, gate_upsample, profile_upsample) at config 2's head
shape, (N,19,128,256) -> 1024 x 2048, N = 1 and 2, four thresholds: device events around REPS launches, ROUNDS rounds, the three
alternating in one process; median (min, max) per launch.  Run from the repository root on the MI355X:  python scripts/heads_profile_time.py"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
import addk._lib as L
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '50')), int(os.environ.get('ROUNDS', '10'))
H, W, OH, OW, LD = 128, 256, 1024, 2048, 20
st = torch.cuda.current_stream().cuda_stream
for N in (1, 2):
    g = torch.Generator().manual_seed(3)
    x = torch.zeros((N, H, W, LD))
    x[..., :19] = torch.randn((N, H, W, 19), generator=g) * 3
    x = x.to(dev)
    t = torch.randint(0, 19, (N, OH, OW), generator=g).to(dev)
    thr = torch.tensor([0.2, 0.35, 0.5, 0.8], device=dev)
    # score
    loss, ent1, wsum = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.ones(1, device=dev)
    cm1 = torch.zeros((19, 19), dtype=torch.int64, device=dev)
    ws_s = torch.zeros(int(lib.addk_score_upsample_ws_floats(N, OH, OW)), device=dev)
    a_s = L.ScoreUpsampleArgs()
    a_s.logits, a_s.ld, a_s.N, a_s.H, a_s.W, a_s.C, a_s.OH, a_s.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW
    a_s.target, a_s.class_w, a_s.ignore_index, a_s.wsum, a_s.scale = t.data_ptr(), None, 255, wsum.data_ptr(), 1.0
    a_s.loss_out, a_s.ent_out, a_s.cm, a_s.pred_out, a_s.ws = loss.data_ptr(), ent1.data_ptr(), cm1.data_ptr(), None, ws_s.data_ptr()
    # gate
    out_g = torch.zeros((N, 2), device=dev)
    ws_g = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    a_g = L.GateUpsampleArgs()
    a_g.logits, a_g.ld, a_g.N, a_g.H, a_g.W, a_g.C, a_g.OH, a_g.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW
    a_g.max_thr, a_g.out, a_g.out_host, a_g.ws = thr.data_ptr(), out_g.data_ptr(), None, ws_g.data_ptr()
    # profile
    ent_p, share_p = torch.zeros(N, device=dev), torch.zeros((N, 4), device=dev)
    cm_p = torch.zeros((N, 19, 19), dtype=torch.int64, device=dev)
    ws_p = torch.zeros(int(lib.addk_profile_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    a_p = L.ProfileUpsampleArgs()
    a_p.logits, a_p.ld, a_p.N, a_p.H, a_p.W, a_p.C, a_p.OH, a_p.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW
    a_p.target, a_p.thr, a_p.nthr = t.data_ptr(), thr.data_ptr(), 4
    a_p.ent_out, a_p.share_out, a_p.cm, a_p.pred_out, a_p.ws = ent_p.data_ptr(), share_p.data_ptr(), cm_p.data_ptr(), None, ws_p.data_ptr()
    fns = {'score_upsample': lambda: L.check(lib.addk_score_upsample(C.byref(a_s), st)),
           'gate_upsample': lambda: L.check(lib.addk_gate_upsample(C.byref(a_g), st)),
           'profile_upsample': lambda: L.check(lib.addk_profile_upsample(C.byref(a_p), st))}
    for f in fns.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    assert torch.equal(cm_p.sum(0) * 1, cm1) and float(out_g[0, 0]) == float(ent_p[0]) and float(out_g[0, 1]) == float(share_p[0, 0])
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
        print('N=%d %s: median %.2f us per launch (min %.2f, max %.2f; %d rounds of %d)' % (N, k, statistics.median(v), min(v), max(v), ROUNDS, REPS))
    print('N=%d score + gate medians: %.2f us' % (N, statistics.median(times['score_upsample']) + statistics.median(times['gate_upsample'])))
