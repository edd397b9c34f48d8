"""Per-launch time of the calibration head (calib_upsample, one and eight temperatures) against profile_upsample, and of the tempered gate
(gate_upsample_t, with and without the label map) against gate_upsample / gate_label_upsample, at config 2's head shape,
(N,19,128,256) -> 1024 x 2048, N = 1 and 2: device events around REPS launches, ROUNDS rounds, the launches alternating in one
process; median (min, max) per launch.  Two inputs: `spread` (random logits x 3: the confidences cover the bins) and `peaked` (x 10 with
one channel raised: nearly every pixel in the top bin, the case the per-thread runs and the wave sum are for).
Run from the repository root on the MI355X:  python scripts/calib_head_time.py [output file]"""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
import addk._lib as L
lib = L.load()
dev = torch.device('cuda:0')
REPS, ROUNDS = int(os.environ.get('REPS', '30')), int(os.environ.get('ROUNDS', '10'))
H, W, OH, OW, LD = 128, 256, 1024, 2048, 20
GRID = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0)
st = torch.cuda.current_stream().cuda_stream
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def prefix(a, x, N):
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = x.data_ptr(), LD, N, H, W, 19, OH, OW


for N in (1, 2):
    for kind in ('spread', 'peaked'):
        g = torch.Generator().manual_seed(3)
        z = torch.randn((N, H, W, 19), generator=g) * 3
        if kind == 'peaked':
            z = z * (10.0 / 3.0)
            z.scatter_add_(3, torch.randint(0, 19, (N, H, W, 1), generator=g), torch.full((N, H, W, 1), 30.0))
        x = torch.zeros((N, H, W, LD))
        x[..., :19] = z
        x = x.to(dev)
        t = torch.randint(0, 19, (N, OH, OW), generator=g).to(dev)
        thr = torch.tensor([0.2, 0.35, 0.5, 0.8], device=dev)
        one = torch.ones(1, device=dev)
        keep = []
        # profile
        ent_p, share_p = torch.zeros(N, device=dev), torch.zeros((N, 4), device=dev)
        cm_p = torch.zeros((N, 19, 19), dtype=torch.int64, device=dev)
        ws_p = torch.zeros(int(lib.addk_profile_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
        a_p = L.ProfileUpsampleArgs()
        prefix(a_p, x, N)
        a_p.target, a_p.thr, a_p.nthr = t.data_ptr(), thr.data_ptr(), 4
        a_p.ent_out, a_p.share_out, a_p.cm, a_p.pred_out, a_p.ws = ent_p.data_ptr(), share_p.data_ptr(), cm_p.data_ptr(), None, ws_p.data_ptr()
        # calibration, one and eight temperatures
        calib = {}
        for nt in (1, 8):
            inv = torch.tensor([1.0 / T for T in (GRID if nt == 8 else (1.0,))], dtype=torch.float32, device=dev)
            bins, nll = torch.zeros((nt, 16, 3), dtype=torch.int64, device=dev), torch.zeros(nt, dtype=torch.float64, device=dev)
            ws = torch.zeros(int(lib.addk_calib_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
            a = L.CalibUpsampleArgs()
            prefix(a, x, N)
            a.target, a.inv_temp, a.nt, a.bins, a.nll, a.ws = t.data_ptr(), inv.data_ptr(), nt, bins.data_ptr(), nll.data_ptr(), ws.data_ptr()
            keep += [inv, ws]
            calib[nt] = (a, bins, nll)
        # gates
        out_g, out_t = torch.zeros((N, 2), device=dev), torch.zeros((N, 2), device=dev)
        lab_g, lab_t = (torch.zeros((N, OH, OW), dtype=torch.uint8, device=dev) for _ in range(2))
        gates = {}
        for name, out, lab in (('gate_upsample', out_g, None), ('gate_label_upsample', out_g, lab_g)):
            ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
            a = L.GateUpsampleArgs()
            prefix(a, x, N)
            a.max_thr, a.out, a.out_host, a.ws = thr.data_ptr(), out.data_ptr(), None, ws.data_ptr()
            b = L.GateUpsampleTArgs()
            b.gate, b.inv_temp = a, one.data_ptr()
            b.gate.out = out_t.data_ptr()
            keep.append(ws)
            if lab is None:
                gates[name] = (lib.addk_gate_upsample, a)
            else:
                gl = L.GateLabelUpsampleArgs()
                gl.gate, gl.lut256, gl.labels = a, None, lab.data_ptr()
                b.lut256, b.labels = None, lab_t.data_ptr()
                gates[name] = (lib.addk_gate_label_upsample, gl)
            gates[name + ' tempered'] = (lib.addk_gate_upsample_t, b)
        fns = {'profile_upsample': lambda: L.check(lib.addk_profile_upsample(C.byref(a_p), st)),
               'calib_upsample nt=1': lambda: L.check(lib.addk_calib_upsample(C.byref(calib[1][0]), st)),
               'calib_upsample nt=8': lambda: L.check(lib.addk_calib_upsample(C.byref(calib[8][0]), st))}
        for name, (fn, a) in gates.items():
            fns[name] = (lambda fn=fn, a=a: L.check(fn(C.byref(a), st)))
        for f in fns.values():
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        assert torch.equal(out_g.view(torch.int32), out_t.view(torch.int32)) and torch.equal(lab_g, lab_t)      # the word 1.0: the same bits
        assert torch.equal(calib[1][1][0], calib[8][1][GRID.index(1.0)])
        top = int(calib[8][1][GRID.index(1.0), 15, 0]) / max(int(calib[8][1][GRID.index(1.0), :, 0].sum()), 1)
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
        say('N=%d %s (share of the pixels in the top bin at T = 1: %.3f)' % (N, kind, top))
        for k, v in times.items():
            say('  %s: median %.2f us per launch (min %.2f, max %.2f; %d rounds of %d)' % (k, statistics.median(v), min(v), max(v), ROUNDS, REPS))
        med = statistics.median(times['calib_upsample nt=8'])
        say('  calib_upsample nt=8: %.1f G exp/s (%d pixels x 8 x 19 exponentials)' % (N * OH * OW * 8 * 19 / med / 1e3, N * OH * OW))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(sys.argv[1]) or '.', exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
