#!/usr/bin/env python
"""Writes tests/golden/sepb_parent_bits.json: sha256 of every output of addk_sep_bwd (gradient first touch, gradient
accumulate, the (dA, dB) slab, the weight-gradient workspace) on seeded inputs, for every (KS, KG, KP, R) variant config 2
runs, their 56 / 72-stride siblings and two odd-sized maps.  Run it on the MI355X with the library of the commit whose bits
are to be pinned (ADDK_LIB selects another build of libaddk.so):

    ADDK_LIB=/path/to/parent/libaddk.so python tests/tools/make_sepb_bits.py

tests/test_gpu_sepb_waves.py imports CASES, make_inputs and run_case from here, so the test and the fixture cannot drift.
The inputs come from numpy.random.RandomState, whose stream is frozen; their hash is stored too, so that a changed input
shows up as such and not as a changed kernel."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'sepb_parent_bits.json')

CASES = [
    # name,           N,   H,   W,  C, k, seed      variant <KS, KG, KP, R>
    ('c80_k5',        2,  64, 128, 80, 5, 101),   # <5,5,88,1>  config 2, level 2
    ('c80_k3',        2,  64, 128, 80, 3, 102),   # <3,5,88,1>
    ('c40_k5',        2, 128, 256, 40, 5, 103),   # <5,3,40,2>  config 2, level 1
    ('c40_k3',        2, 128, 256, 40, 3, 104),   # <3,3,40,2>
    ('c72_k5',        2,  64, 128, 72, 5, 105),   # <5,5,72,1>  the 72-stride siblings
    ('c72_k3',        2,  64, 128, 72, 3, 106),   # <3,5,72,1>
    ('c48_k5',        2, 128, 256, 48, 5, 107),   # <5,3,56,2>  the 56-stride siblings
    ('c48_k3',        2, 128, 256, 48, 3, 108),   # <3,3,56,2>
    ('c80_k5_odd',    2,  63, 127, 80, 5, 109),   # partial tiles on both edges
    ('c40_k3_odd',    2, 125, 253, 40, 3, 110),
]
OUTPUTS = ('g_first', 'g_accumulate', 'dab', 'ws')


def sha(*arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def make_inputs(case):
    """(x, a, b, dw weights, pw weights, dy, g0) as float32 numpy arrays, and their sha256."""
    name, N, H, W, Cc, k, seed = case
    rs = np.random.RandomState(seed)
    P = N * H * W
    f = lambda scale, *s: (scale * rs.standard_normal(s)).astype(np.float32)
    arrs = (f(1.0, P, Cc), f(1.0, Cc), f(0.3, Cc), f(0.3, Cc, k * k), f(0.2, Cc, Cc), f(1.0, P, Cc), f(1.0, P, Cc))
    return arrs, sha(*arrs)


def run_case(L, case, arrs):
    """One first-touch and one accumulating launch of addk_sep_bwd; {output name: sha256}, and the kernel's cfg[1:5]."""
    import torch
    lb = L.load()
    name, N, H, W, Cc, k, seed = case
    dev = torch.device('cuda:0')
    x, a, b, wdw, wpw, dy, g0 = (torch.from_numpy(v).to(dev) for v in arrs)
    P = N * H * W
    ba = L.SepBwdArgs()
    ba.dy, ba.lddy, ba.N, ba.H, ba.W, ba.K = dy.data_ptr(), Cc, N, H, W, k
    ba.src.x, ba.src.a, ba.src.b, ba.src.ld, ba.src.C, ba.src.relu = x.data_ptr(), a.data_ptr(), b.data_ptr(), Cc, Cc, 1
    ba.Cout, ba.ldw, ba.dw_w, ba.pw_w = Cc, Cc, wdw.data_ptr(), wpw.data_ptr()
    rows = lb.addk_sep_bwd_rows(C.byref(ba))
    assert rows > 0, '%s: the fused backward does not take this shape' % name
    cfg = (C.c_int32 * 8)()
    L.check(lb.addk_sep_bwd_config(C.byref(ba), cfg), 'sep_bwd_config')
    st = torch.cuda.current_stream().cuda_stream
    got = {}
    for acc in (0, 1):
        g = g0.clone() if acc else torch.full((P, Cc), float('nan'), device=dev)
        dab = torch.full((rows, Cc, 2), float('nan'), device=dev, dtype=torch.float64)
        ws = torch.full((rows, Cc, k * k), float('nan'), device=dev)
        ba.g, ba.ldg, ba.accumulate, ba.dab, ba.ws = g.data_ptr(), Cc, acc, dab.data_ptr(), ws.data_ptr()
        L.check(lb.addk_sep_bwd(C.byref(ba), st), 'sep_bwd')
        torch.cuda.synchronize()
        h = {'g_accumulate' if acc else 'g_first': sha(g.cpu().numpy()), 'dab': sha(dab.cpu().numpy()), 'ws': sha(ws.cpu().numpy())}
        for key, v in h.items():
            assert got.setdefault(key, v) == v, '%s: %s differs between the first-touch and the accumulating launch' % (name, key)
    return got, [int(v) for v in cfg[1:5]]


def main():
    sys.path.insert(0, ROOT)
    import torch
    import addk  # noqa: F401
    from addk import _lib as L
    assert torch.cuda.is_available(), 'needs the MI355X'
    L.load().addk_set_fast_paths(31)
    doc = {'about': 'sha256 of addk_sep_bwd outputs on RandomState-seeded inputs; written by tests/tools/make_sepb_bits.py from the '
                    'parent of the commit that spread the kernel over more waves', 'cases': []}
    for case in CASES:
        arrs, hin = make_inputs(case)
        got, variant = run_case(L, case, arrs)
        name, N, H, W, Cc, k, seed = case
        doc['cases'].append({'name': name, 'shape': [N, H, W, Cc, k], 'seed': seed, 'variant': variant, 'inputs': hin, **got})
        print(name, variant, hin[:12], ' '.join(got[o][:12] for o in OUTPUTS), flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
