"""Time the forward kernels that end in a statistics tail — the fused SepConv half (csrc/sepf.hip) and the pointwise kernels (csrc/pw.hip:
pw_kernel forward and data gradient, pwk_kernel) — through the C ABI at config 2's shapes, for one or more builds of the library:

    python scripts/fwd_tail_time.py [--launches 20] [--replays 10] [--rounds 7] LIB [LIB ...]

Each LIB is a path to a libaddk.so, optionally NAME=PATH; the libraries are timed alternately, round after round, in this one process, so a
parent build and a new build see the same device state.  A measurement is a chain of LAUNCHES launches on one stream captured into one
graph (the sepf launches ping-pong between two tensors, each reading what the one before wrote: the rows of
profiles/r05_sepf_boundary_accounting.txt), warmed by three replays and timed over REPLAYS more between two HIP events.  Printed per
launch and library: the median over the rounds in us per launch and, in brackets, the spread max - min of its rounds; last columns: first
library - last library in us, and whether that difference exceeds the first library's spread."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                                    # noqa: E402
from addk import _lib as L                                                      # noqa: E402

KEEP = []


def dev(*shape, scale=1.0, dtype=torch.float32):
    t = torch.randn(*shape, device='cuda', dtype=dtype) * scale
    KEEP.append(t)
    return t


def bind(path):
    lib = C.CDLL(path)
    for name in ('addk_sep_fwd', 'addk_conv_fwd', 'addk_conv_dgrad'):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p, C.c_void_p], C.c_int
    lib.addk_conv_rows.argtypes, lib.addk_conv_rows.restype = [C.c_int64, C.c_int32], C.c_int
    lib.addk_sep_rows.argtypes, lib.addk_sep_rows.restype = [C.c_void_p], C.c_int
    lib.addk_set_fast_paths.argtypes = [C.c_int]
    lib.addk_set_fast_paths(31)
    return lib


def sepf_chain(lib0, N, H, W, Cc, k, mode, n):
    """n argument structs: launch j reads buffer j % 2 and writes the other."""
    P = N * H * W
    bufs = [dev(P, Cc), dev(P, Cc)]
    tb, u1 = dev(P, Cc), dev(P, Cc)
    a, b = torch.rand(Cc, device='cuda') + 0.5, dev(Cc, scale=0.1)
    wdw, wpw = dev(Cc, k * k, scale=0.3), dev(Cc, Cc, scale=0.2)
    KEEP.append(a)
    out = []
    for j in range(n):
        ar = L.SepArgs()
        ar.src.x, ar.src.a, ar.src.b, ar.src.ld, ar.src.C, ar.src.relu = bufs[j % 2].data_ptr(), a.data_ptr(), b.data_ptr(), Cc, Cc, 1
        ar.N, ar.H, ar.W, ar.K, ar.Cout, ar.ldw = N, H, W, k, Cc, Cc
        ar.dw_w, ar.pw_w, ar.y, ar.ldy = wdw.data_ptr(), wpw.data_ptr(), bufs[(j + 1) % 2].data_ptr(), Cc
        if mode == 'train':
            rows = max(lib0.addk_conv_rows(P, Cc), lib0.addk_sep_rows(C.addressof(ar)))
            slab = dev(rows, Cc, 2, dtype=torch.float64)
            ar.t, ar.ldt, ar.stats, ar.stats_ld, ar.stats_rows = tb.data_ptr(), Cc, slab.data_ptr(), Cc, rows
        else:
            ar.ea, ar.eb, ar.nterm = a.data_ptr(), b.data_ptr(), 1
            ar.term[0].x, ar.term[0].ld, ar.term[0].C = u1.data_ptr(), Cc, Cc
        out.append(ar)
    KEEP.extend(out)
    return out


def conv_fwd_args(lib0, N, H, W, srcs, Cout):
    P, K = N * H * W, sum(srcs)
    ar = L.ConvArgs()
    for i, c in enumerate(srcs):
        ar.src[i].x, ar.src[i].a, ar.src[i].b, ar.src[i].ld, ar.src[i].C, ar.src[i].relu = dev(P, c).data_ptr(), dev(c).data_ptr(), dev(c).data_ptr(), c, c, 1
    ar.nsrc = len(srcs)
    ar.N, ar.H, ar.W, ar.OH, ar.OW, ar.KH, ar.KW, ar.stride, ar.pad, ar.dil, ar.Cout = N, H, W, H, W, 1, 1, 1, 0, 1, Cout
    ar.ldw, ar.cin_total, ar.w_choff, ar.ldy = K, K, 0, Cout
    rows = lib0.addk_conv_rows(P, Cout)
    ar.w, ar.y, ar.stats, ar.stats_ld = dev(Cout, K, scale=0.1).data_ptr(), dev(P, Cout).data_ptr(), dev(rows, Cout, 2, dtype=torch.float64).data_ptr(), Cout
    KEEP.append(ar)
    return ar


def conv_dgrad_args(lib0, N, H, W, K, Cout):
    """Data gradient of a K -> Cout pointwise conv: dy [P, Cout] -> g [P, K] with the (dA, dB) slab of the input's lazy BatchNorm."""
    P = N * H * W
    da = L.ConvDgradArgs()
    da.dy, da.lddy, da.Cout = dev(P, Cout).data_ptr(), Cout, Cout
    da.N, da.H, da.W, da.OH, da.OW, da.KH, da.KW, da.stride, da.pad, da.dil = N, H, W, H, W, 1, 1, 1, 0, 1
    da.w, da.ldw, da.cin_total, da.w_choff = dev(Cout, K, scale=0.1).data_ptr(), K, K, 0
    da.dst.x, da.dst.a, da.dst.b, da.dst.ld, da.dst.C, da.dst.relu = dev(P, K).data_ptr(), dev(K).data_ptr(), dev(K).data_ptr(), K, K, 1
    rows = lib0.addk_conv_rows(P, K)
    da.g, da.ldg, da.accumulate, da.dab = dev(P, K).data_ptr(), K, 0, dev(rows, K, 2, dtype=torch.float64).data_ptr()
    KEEP.append(da)
    return da


def graph_of(fn, structs, n):
    st = torch.cuda.current_stream().cuda_stream
    for j in range(min(n, 2)):
        assert fn(C.addressof(structs[j % len(structs)]), st) == 0, 'launch failed'
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for j in range(n):
            assert fn(C.addressof(structs[j % len(structs)]), st) == 0, 'launch failed'
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g, n, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (n * replays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('libs', nargs='+')
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--replays', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    o = ap.parse_args()
    assert torch.cuda.is_available(), 'fwd_tail_time needs the GPU'
    libs = []
    for spec in o.libs:
        name, _, path = spec.rpartition('=')
        libs.append((name or os.path.basename(os.path.dirname(os.path.abspath(path))), bind(os.path.abspath(path))))
    names = [n for n, _ in libs]
    lib0 = libs[0][1]
    torch.manual_seed(0)
    print('# us per launch: median of %d rounds of %d replays of a %d-launch graph [max - min of the rounds]' % (o.rounds, o.replays, o.launches))
    print('%-46s' % 'launch' + ''.join('%18s' % n for n in names) + '   %s - %s   beyond %s\'s spread' % (names[0], names[-1], names[0]))

    def run(label, entry, structs):
        graphs = {name: graph_of(getattr(lib, entry), structs, o.launches) for name, lib in libs}
        t = {n: [] for n in names}
        for _ in range(o.rounds):
            for n in names:                                   # alternate the libraries inside every round
                t[n].append(time_us(graphs[n], o.launches, o.replays))
        med = {n: statistics.median(v) for n, v in t.items()}
        spread = {n: max(v) - min(v) for n, v in t.items()}
        d = med[names[0]] - med[names[-1]]
        print('%-46s' % label + ''.join('%10.2f [%5.2f]' % (med[n], spread[n]) for n in names) + '   %+6.2f   %s' % (d, 'yes' if d > spread[names[0]] else 'no'), flush=True)
        del graphs
        KEEP.clear()
        torch.cuda.empty_cache()

    for N, H, W, Cc, k in ((2, 125, 253, 40, 3), (2, 125, 253, 40, 5), (2, 63, 127, 80, 3), (2, 63, 127, 80, 5)):
        for mode in ('eval', 'train'):
            run('sepf N=%d %dx%d C=%d k=%d %s' % (N, H, W, Cc, k, mode), 'addk_sep_fwd', sepf_chain(lib0, N, H, W, Cc, k, mode, o.launches))
    for N, H, W, K, Cout in ((2, 125, 253, 40, 40), (2, 125, 253, 80, 40), (2, 63, 127, 80, 80)):
        run('pw fwd %d->%d N=%d %dx%d' % (K, Cout, N, H, W), 'addk_conv_fwd', [conv_fwd_args(lib0, N, H, W, (K,), Cout) for _ in range(2)])
        run('pw dgrad %d<-%d N=%d %dx%d' % (K, Cout, N, H, W), 'addk_conv_dgrad', [conv_dgrad_args(lib0, N, H, W, K, Cout) for _ in range(2)])
    for N, H, W, srcs, Cout in ((2, 125, 253, (200,), 40), (2, 125, 253, (40, 40, 40), 40), (2, 63, 127, (400,), 80), (2, 32, 64, (800,), 160)):
        run('pwk %s->%d N=%d %dx%d' % ('+'.join(map(str, srcs)), Cout, N, H, W), 'addk_conv_fwd', [conv_fwd_args(lib0, N, H, W, srcs, Cout) for _ in range(2)])


if __name__ == '__main__':
    main()
