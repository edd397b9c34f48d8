"""Time the BatchNorm slab kernels (csrc/bn.hip) through the C ABI at every shape config 2's train plan runs them at (NET_FIN and
NET_BWD of tests/test_gpu_bn_kernels.py; slab_reduce, the SyncBN form of the forward sums, at the slabs of NET_FIN), as single launches
and as batch tables, for one or more builds of the library:

    python scripts/bn_time.py [--launches 200] [--rounds 3] [--batch 4] LIB [LIB ...]

Each LIB is a path to a libaddk.so, optionally NAME=PATH; the libraries are timed alternately, round after round, in this one process,
so a parent build and a new build see the same device state.  A measurement is LAUNCHES launches captured into one graph (no host in
the loop), warmed by one replay and timed over one more between two HIP events; the launches walk round 8 copies of the slabs, so a 9-slab
list (3.9 MB) is not served from one XCD's L2 alone, as it is not in the step.  Printed: microseconds per launch, the median over the
rounds and, in brackets, the spread max - min of the rounds; `batch` is one table of BATCH entries of the shape (microseconds per launch
of the table).  Last column: first library / last."""
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
from test_gpu_bn_kernels import NET_BWD, NET_FIN                                # noqa: E402

COPIES = 8
f64 = torch.float64
KEEP = []                                                                       # every device buffer an argument struct points to


def dev(*shape, dtype=torch.float32):
    t = torch.randn(*shape, device='cuda', dtype=dtype)
    KEEP.append(t)
    return t


def fin_args(Cc, count, rows):
    a = L.BnFinalizeArgs()
    a.partial, a.rows, a.C, a.count = dev(rows, Cc, 2, dtype=f64).abs_().data_ptr(), rows, Cc, float(count)
    KEEP.append(a)
    a.gamma, a.beta, a.running_mean, a.running_var = (dev(Cc).data_ptr() for _ in range(4))
    a.momentum, a.eps = 0.1, 1e-5
    a.a, a.b, a.mean, a.invstd = (dev(Cc).data_ptr() for _ in range(4))
    return a


def reduce_args(Cc, count, rows):
    it = L.SlabReduceItem()
    it.partial, it.out, it.rows, it.C = dev(rows, Cc, 2, dtype=f64).data_ptr(), dev(Cc, 2, dtype=f64).data_ptr(), rows, Cc
    KEEP.append(it)
    return it


def bwd_args(Cc, count, rows):
    a = L.BnBwdArgs()
    for i, r in enumerate(rows):
        a.slab[i], a.rows[i] = dev(r, Cc, 2, dtype=f64).data_ptr(), r
    a.nslab, a.C, a.count = len(rows), Cc, float(count)
    a.gamma, a.mean, a.invstd, a.a, a.dgamma, a.dbeta, a.c1, a.c2 = (dev(Cc).data_ptr() for _ in range(8))
    a.accumulate, a.centered = 0, 1
    KEEP.append(a)
    return a


def table(structs):
    arr = (type(structs[0]) * len(structs))(*structs)
    t = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    KEEP.append(t)
    return t


def bind(path):
    lib = C.CDLL(path)
    for name in ('addk_bn_finalize', 'addk_bn_bwd'):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p, C.c_void_p], C.c_int
    for name in ('addk_bn_finalize_batch', 'addk_bn_bwd_batch', 'addk_slab_reduce_batch'):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], C.c_int
    # the lone slab_reduce takes the table's item since version 2 of the library, positional arguments before
    if lib.addk_version() >= 2:
        lib.addk_slab_reduce.argtypes = [C.c_void_p, C.c_void_p]
        reduce = lambda it, st: lib.addk_slab_reduce(C.addressof(it), st)                              # noqa: E731
    else:
        lib.addk_slab_reduce.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        reduce = lambda it, st: lib.addk_slab_reduce(it.partial, it.rows, it.C, it.out, st)            # noqa: E731
    by_address = lambda fn: lambda a, st: fn(C.addressof(a), st)                                       # noqa: E731
    lib.kinds = {'finalize': (by_address(lib.addk_bn_finalize), lib.addk_bn_finalize_batch), 'bwd': (by_address(lib.addk_bn_bwd), lib.addk_bn_bwd_batch),
                 'reduce': (reduce, lib.addk_slab_reduce_batch)}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('libs', nargs='+')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=4)
    o = ap.parse_args()
    assert torch.cuda.is_available(), 'bn_time needs the GPU'
    libs = []
    for spec in o.libs:
        name, _, path = spec.rpartition('=')
        libs.append((name or os.path.basename(os.path.dirname(os.path.abspath(path))), bind(os.path.abspath(path))))
    torch.manual_seed(0)
    rowsets = []                                              # (label, {lib name: {form: graph}})
    for kind, shapes, make in (('finalize', NET_FIN, fin_args), ('bwd', NET_BWD, bwd_args), ('reduce', NET_FIN, reduce_args)):
        for Cc, count, rows in shapes:
            copies = [make(Cc, count, rows) for _ in range(COPIES)]
            tabs = [table([copies[(j + i) % COPIES] for i in range(o.batch)]) for j in range(COPIES)] if kind == 'bwd' else \
                [table([make(Cc, count, rows) for _ in range(o.batch)]) for _ in range(COPIES)]     # finalize / reduce entries: outputs of their own
            graphs = {}
            for name, lib in libs:
                one, bat = lib.kinds[kind]
                graphs[name] = {
                    'single': graph_of(lambda j, st: one(copies[j % COPIES], st), o.launches),
                    'batch': graph_of(lambda j, st: bat(tabs[j % COPIES].data_ptr(), o.batch, Cc, st), o.launches)}
            rowsets.append(('%-8s C=%-3d rows=%s' % (kind, Cc, rows), graphs))
    names = [n for n, _ in libs]
    print('# us per launch, median of %d rounds of %d graph-replayed launches [max - min of the rounds]; batch = one table of %d entries' % (o.rounds, o.launches, o.batch))
    print('%-64s' % 'shape' + ''.join('%22s' % (n + ' ' + f) for f in ('single', 'batch') for n in names) + '   %s/%s single, batch' % (names[0], names[-1]))
    tot = {(n, f): 0.0 for n in names for f in ('single', 'batch')}
    for label, graphs in rowsets:
        t = {(n, f): [] for n in names for f in ('single', 'batch')}
        for _ in range(o.rounds):
            for n in names:                                   # alternate the libraries inside every round
                for f in ('single', 'batch'):
                    t[(n, f)].append(time_us(graphs[n][f], o.launches))
        med = {k: statistics.median(v) for k, v in t.items()}
        for k, v in med.items():
            tot[k] += v
        print('%-64s' % label + ''.join('%14.2f [%5.2f]' % (med[(n, f)], max(t[(n, f)]) - min(t[(n, f)])) for f in ('single', 'batch') for n in names)
              + '   %5.2fx %5.2fx' % (med[(names[0], 'single')] / med[(names[-1], 'single')], med[(names[0], 'batch')] / med[(names[-1], 'batch')]), flush=True)
    print('%-64s' % 'sum over the shapes' + ''.join('%14.2f        ' % tot[(n, f)] for f in ('single', 'batch') for n in names))


if __name__ == '__main__':
    main()
