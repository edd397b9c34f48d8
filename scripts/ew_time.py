"""Time the elementwise links of a cell block (csrc/elementwise.hip: affine_sum_fwd, affine_sum_bwd, bn_bwd_apply and its batch form) through
the C ABI at every shape config 2's train plan runs them at (NET_AFFINE and NET_BN of tests/test_gpu_bn_kernels.py), for one or more builds
of the library:

    python scripts/ew_time.py [--launches 200] [--rounds 5] [--batch 3] LIB [LIB ...]

Each LIB is a path to a libaddk.so, optionally NAME=PATH; the libraries are timed alternately, round after round, in this one process, so a
parent build and a new build see the same device state.  A measurement is LAUNCHES launches captured into one graph (no host in the loop),
warmed by one replay and timed over one more between two HIP events; the launches walk round up to 8 copies of the tensors (fewer where a
copy is large: 2 GB per shape at most), so no launch finds its input in a cache the previous one filled.  The launches have the network's form:
two lazy-BatchNorm terms summed into one slot of the 5 C concat buffer, the backward writing g and the dab slab of both; bn_bwd_apply in place.
Printed per shape and form: the bytes the launch has to move, the streaming line 3.1 us + bytes / 5.6 TB/s (a dependent streaming launch on
MI355X, profiles/r04_persistent_vs_launch_chain.txt), then per library the median over the rounds in us per launch and, in brackets, the
spread max - min of its rounds; last column: first library / last library."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch                                                                    # noqa: E402
from addk import _lib as L                                                      # noqa: E402
from test_gpu_bn_kernels import NET_AFFINE, NET_BN                              # noqa: E402

MAX_COPIES, MAX_BYTES = 8, 2 << 30
KEEP = []                                                                       # every device buffer an argument struct points to


def dev(*shape, dtype=torch.float32):
    t = torch.randn(*shape, device='cuda', dtype=dtype)
    KEEP.append(t)
    return t


def src(x, Cc):
    s = L.Src()
    s.x, s.a, s.b, s.ld, s.C, s.relu, s.rs_hw = x.data_ptr(), dev(Cc).data_ptr(), dev(Cc).data_ptr(), x.stride(0), Cc, 0, 0
    return s


def affine_args(P, Cc, nterm, ldo, rows):
    """(forward args, backward args) of one branch sum: nterm lazy terms, slot ldo // C - 2 of the concat buffer and of its gradient."""
    xs = [dev(P, Cc) for _ in range(nterm)]
    col = (ldo // Cc - 2) * Cc
    out, dout = dev(P, ldo)[:, col:col + Cc], dev(P, ldo)[:, col:col + Cc]
    fa, ba = L.AffineSumArgs(), L.AffineSumBwdArgs()
    for i, x in enumerate(xs):
        fa.term[i] = ba.term[i] = src(x, Cc)
        g = dev(P, Cc)
        ba.g[i], ba.ldg[i], ba.accumulate[i], ba.dab[i] = g.data_ptr(), Cc, 0, dev(rows, Cc, 2, dtype=torch.float64).data_ptr()
    fa.nterm, fa.P, fa.C, fa.out, fa.ldo, fa.relu_out, fa.accumulate = nterm, P, Cc, out.data_ptr(), ldo, 0, 0
    ba.nterm, ba.P, ba.C, ba.dout, ba.lddo, ba.relu_out = nterm, P, Cc, dout.data_ptr(), ldo, 0
    KEEP.extend((fa, ba))
    return fa, ba


def apply_item(P, Cc):
    g, x = dev(P, Cc), dev(P, Cc)
    it = L.BnApplyItem()
    c1, c2 = dev(Cc).mul_(1e-3), dev(Cc).mul_(1e-3)             # small: the in-place launches repeat on the same tensors
    it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = g.data_ptr(), x.data_ptr(), c1.data_ptr(), c2.data_ptr(), dev(Cc).data_ptr(), g.data_ptr(), P
    it.ldg, it.ldx, it.ldo, it.C = Cc, Cc, Cc, Cc
    KEEP.append(it)
    return it


def table(structs):
    arr = (type(structs[0]) * len(structs))(*structs)
    t = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    KEEP.append(t)
    return t


def bind(path):
    lib = C.CDLL(path)
    for name in ('addk_affine_sum_fwd', 'addk_affine_sum_bwd'):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p, C.c_void_p], C.c_int
    # the lone entry takes the table's item since version 2 of the library, positional arguments before: `lib.apply(item, stream)` either way
    if lib.addk_version() >= 2:
        lib.addk_bn_bwd_apply.argtypes = [C.c_void_p, C.c_void_p]
        lib.apply = lambda it, st: lib.addk_bn_bwd_apply(C.addressof(it), st)
    else:
        lib.addk_bn_bwd_apply.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                          C.c_void_p, C.c_int32, C.c_void_p]
        lib.apply = lambda it, st: lib.addk_bn_bwd_apply(it.g, it.ldg, it.x, it.ldx, it.mean, it.c1, it.c2, it.P, it.C, it.out, it.ldo, st)
    lib.addk_bn_bwd_apply_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
    lib.addk_ew_rows.argtypes, lib.addk_ew_rows.restype = [C.c_int64, C.c_int32], C.c_int
    lib.addk_bn_bwd_apply.restype = lib.addk_bn_bwd_apply_batch.restype = C.c_int
    return lib


def graph_of(launch, n):
    """n launches (launch(j, stream)) captured into one graph, replayed once."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for j in range(n):
            rc = launch(j, st)
            assert rc == 0, 'launch failed: %d' % rc
    g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def copies_for(nbytes):
    return max(2, min(MAX_COPIES, MAX_BYTES // max(nbytes, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('libs', nargs='+')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=3)
    o = ap.parse_args()
    assert torch.cuda.is_available(), 'ew_time needs the GPU'
    libs = []
    for spec in o.libs:
        name, _, path = spec.rpartition('=')
        libs.append((name or os.path.basename(os.path.dirname(os.path.abspath(path))), bind(os.path.abspath(path))))
    names = [n for n, _ in libs]
    torch.manual_seed(0)
    print('# us per launch: median of %d rounds of %d graph-replayed launches [max - min of the rounds]; batch = one table of %d tensors'
          % (o.rounds, o.launches, o.batch))
    print('%-44s%9s%9s' % ('launch', 'MB', 'line us') + ''.join('%18s' % n for n in names) + '   %s/%s' % (names[0], names[-1]))
    tot = {n: 0.0 for n in names}

    def run(label, nbytes, make_graphs):
        graphs = {name: make_graphs(lib) for name, lib in libs}
        t = {n: [] for n in names}
        for _ in range(o.rounds):
            for n in names:                                   # alternate the libraries inside every round
                t[n].append(time_us(graphs[n], o.launches))
        med = {n: statistics.median(v) for n, v in t.items()}
        for n in names:
            tot[n] += med[n]
        print('%-44s%9.1f%9.1f' % (label, nbytes / 1e6, 3.1 + nbytes / 5.6e6)
              + ''.join('%10.2f [%5.2f]' % (med[n], max(t[n]) - min(t[n])) for n in names) + '   %5.2fx' % (med[names[0]] / med[names[-1]]), flush=True)
        del graphs
        KEEP.clear()
        torch.cuda.empty_cache()

    for P, Cc, nterm, ldo in NET_AFFINE:
        rows = libs[0][1].addk_ew_rows(P, Cc)
        t4 = P * Cc * 4
        nc = copies_for((2 * nterm + 2) * t4 * 5)
        args = [affine_args(P, Cc, nterm, ldo, rows) for _ in range(nc)]
        run('affine_sum_fwd P=%d C=%d terms=%d' % (P, Cc, nterm), (nterm + 1) * t4,
            lambda lib: graph_of(lambda j, st: lib.addk_affine_sum_fwd(C.addressof(args[j % nc][0]), st), o.launches))
        args = [affine_args(P, Cc, nterm, ldo, rows) for _ in range(nc)]
        run('affine_sum_bwd P=%d C=%d terms=%d' % (P, Cc, nterm), (2 * nterm + 1) * t4 + nterm * rows * Cc * 16,
            lambda lib: graph_of(lambda j, st: lib.addk_affine_sum_bwd(C.addressof(args[j % nc][1]), st), o.launches))
    for Cc, P in NET_BN:
        t4 = P * Cc * 4
        nc = copies_for(2 * t4)
        items = [apply_item(P, Cc) for _ in range(nc)]
        run('bn_bwd_apply P=%d C=%d' % (P, Cc), 3 * t4,
            lambda lib: graph_of(lambda j, st: lib.apply(items[j % nc], st), o.launches))
        nc = copies_for(2 * t4 * o.batch)
        tabs = [table([apply_item(P, Cc) for _ in range(o.batch)]) for _ in range(nc)]
        run('bn_bwd_apply_batch %d x (P=%d C=%d)' % (o.batch, P, Cc), 3 * t4 * o.batch,
            lambda lib: graph_of(lambda j, st: lib.addk_bn_bwd_apply_batch(tabs[j % nc].data_ptr(), o.batch, P, st), o.launches))
    print('%-62s' % 'sum over the launches' + ''.join('%10.2f        ' % tot[n] for n in names))


if __name__ == '__main__':
    main()
