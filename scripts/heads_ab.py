"""Two builds of libaddk.so on the gather heads of csrc/score_up.hip and csrc/label_up.hip, alternating in ONE process: addk_score_upsample (N = 2) and
addk_gate_upsample (N = 1) at config 2's head shape, (128, 256) -> (1024, 2048), pixel stride 24.

    python scripts/heads_ab.py --a /path/to/parent/libaddk.so [--b auto-dynamic-deeplab_amd/libaddk.so] [--iters 3000] [--repeats 5]
                               [--out profiles/heads_refactor_ab.txt]

Both libraries are loaded side by side (each handle resolves its own symbols).  Before anything is timed, every buffer the two
builds write on the timed inputs is compared bit for bit.  A window is `iters` back-to-back launches between two device events,
ending in a synchronise; per repetition the windows run A, B, A, so side A is also measured against itself: its run-to-run spread
(min .. max over its windows) is the margin, and B's median has to lie inside it."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import addk  # noqa: E402,F401
from addk import _lib as L  # noqa: E402

LO, HI, LD, NC = (128, 256), (1024, 2048), 24, 19


def bind(path):
    lib = C.CDLL(path)
    for name in ('addk_score_upsample', 'addk_gate_upsample', 'addk_score_upsample_ws_floats', 'addk_gate_upsample_ws_bytes'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGS[name]
    return lib


class Score:
    N = 2

    def __init__(self, lib, dev, x, t):
        self.lib = lib
        self.bufs = dict(loss=torch.zeros(1, device=dev), ent=torch.zeros(1, device=dev), cm=torch.zeros((NC, NC), dtype=torch.int64, device=dev),
                         pred=torch.zeros((self.N,) + HI, dtype=torch.uint8, device=dev),
                         ws=torch.zeros(int(lib.addk_score_upsample_ws_floats(self.N, *HI)), device=dev))
        self.wsum = torch.full((1,), float(((t >= 0) & (t < NC)).sum()), device=dev)
        a = self.a = L.ScoreUpsampleArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = x.data_ptr(), LD, self.N, LO[0], LO[1], NC, HI[0], HI[1]
        a.target, a.class_w, a.ignore_index, a.wsum, a.scale = t.data_ptr(), None, 255, self.wsum.data_ptr(), 1.0
        b = self.bufs
        a.loss_out, a.ent_out, a.cm, a.pred_out, a.ws = (b[k].data_ptr() for k in ('loss', 'ent', 'cm', 'pred', 'ws'))

    def launch(self, st):
        L.check(self.lib.addk_score_upsample(C.byref(self.a), st), 'score_upsample')


class Gate:
    N = 1

    def __init__(self, lib, dev, x, t):
        self.lib = lib
        self.bufs = dict(out=torch.zeros((self.N, 2), device=dev),
                         ws=torch.zeros(int(lib.addk_gate_upsample_ws_bytes(self.N, *HI)), dtype=torch.uint8, device=dev))
        self.thr = torch.full((1,), 0.5, device=dev)
        a = self.a = L.GateUpsampleArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = x.data_ptr(), LD, self.N, LO[0], LO[1], NC, HI[0], HI[1]
        a.max_thr, a.out, a.out_host, a.ws = self.thr.data_ptr(), self.bufs['out'].data_ptr(), None, self.bufs['ws'].data_ptr()

    def launch(self, st):
        L.check(self.lib.addk_gate_upsample(C.byref(self.a), st), 'gate_upsample')


def window(head, iters):
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        head.launch(st)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', required=True, help='side A: the library the margin is taken from (the parent build)')
    ap.add_argument('--b', default=L.LIB_PATH)
    ap.add_argument('--iters', type=int, default=3000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out')
    o = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    libs = {'A': bind(o.a), 'B': bind(o.b)}
    rs = np.random.RandomState(7)
    lines = ['A = %s' % o.a, 'B = %s' % o.b, '(%d, %d) -> (%d, %d), pixel stride %d, %d launches per window, %d repetitions of A B A; microseconds per launch'
             % (LO + HI + (LD, o.iters, o.repeats))]
    ok = True
    for cls in (Score, Gate):
        x = torch.from_numpy((3.0 * rs.standard_normal((cls.N,) + LO + (LD,))).astype(np.float32)).to(dev)
        t = rs.randint(0, NC, (cls.N,) + HI).astype(np.int64)
        t[rs.random_sample(t.shape) < 0.05] = 255
        td = torch.from_numpy(t).to(dev)
        heads = {k: cls(lib, dev, x, td) for k, lib in libs.items()}
        st = torch.cuda.current_stream().cuda_stream
        for h in heads.values():
            h.launch(st)
        torch.cuda.synchronize()
        same = all(torch.equal(heads['A'].bufs[k], heads['B'].bufs[k]) for k in heads['A'].bufs)
        for h in heads.values():                      # warm-up at the timed shape
            window(h, 200)
        times = {'A': [], 'B': []}
        for _ in range(o.repeats):
            for side in 'ABA':
                times[side].append(window(heads[side], o.iters))
        ma, mb = statistics.median(times['A']), statistics.median(times['B'])
        inside = mb <= max(times['A'])
        ok &= same and inside
        lines.append('%-5s N=%d  A median %.2f (min %.2f .. max %.2f, %d windows)   B median %.2f (min %.2f .. max %.2f, %d windows)   B/A %.4f   '
                     'outputs bit-identical: %s   B median within A\'s spread: %s'
                     % (cls.__name__.lower(), cls.N, ma, min(times['A']), max(times['A']), len(times['A']), mb, min(times['B']), max(times['B']),
                        len(times['B']), mb / ma, same, inside))
        lines.append('      A windows: %s' % ' '.join('%.2f' % v for v in times['A']))
        lines.append('      B windows: %s' % ' '.join('%.2f' % v for v in times['B']))
    print('\n'.join(lines))
    if o.out:
        with open(o.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
