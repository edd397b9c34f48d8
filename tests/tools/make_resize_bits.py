#!/usr/bin/env python
"""Writes tests/golden/resize_parent_bits.json: sha256 of what addk_resize_fwd and addk_resize_bwd (csrc/resize.hip) write on seeded
inputs, one small case per code path.  The kernels are deterministic (the backward is a gather, the (dA, dB) sums are added in a fixed
order), so a hash of their outputs is well defined.  Per launch every buffer the launch writes is hashed whole, pixel-stride padding
included: y (prefilled NaN), or g (prefilled NaN, or a seeded gradient when accumulating) plus the (dA, dB) slab (prefilled NaN).

Backward cases run as  variant / accumulate 0, 1 / fast paths 31, 0:
  NHWC   relu_dab (lazy a*x+b with ReLU and the slab), relu (the ReLU mask without the sums), plain (lazy a, no ReLU);
         the sliced case has no slab (more than 1024 channels with one are refused)
  NCHW   scale: the logits gradient with dy_scale = 0.5 and a per-channel `a` (no prologue on this path)
Forward cases run with the ReLU prologue on and off.

Before anything is recorded the kind each backward case takes is asked of the tree's own library (addk_resize_bwd_config, no GPU needed):
a case whose kind is not the one it claims is refused.  Run it on the MI355X with the library of the commit whose bits are to be
pinned (the parent of the commit that gave resize.hip its one kernel choice; that library is bound here by hand, it has no
addk_resize_bwd_config):

    python tests/tools/make_resize_bits.py --lib /path/to/parent/libaddk.so [out.json]

tests/test_gpu_resize.py imports the cases, make_inputs and the run_* functions from here and compares the tree's library with the
fixture.  The inputs come from numpy.random.RandomState, whose stream is frozen; their hash is stored too, so that a changed input
shows up as such and not as a changed kernel."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'resize_parent_bits.json')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

NHWC, TAB, NCHW, TILE = range(4)           # addk_resize_bwd_config's kinds
# name, N, C, H, W, OH, OW, pixel stride (0: C; -1: NCHW gradient / destination), seed, kind with every fast path on, taps per axis
BWD = [
    ('tab5', 2, 40, 9, 17, 18, 33, 0, 700, TAB, 5),
    ('fit', 1, 40, 15, 31, 16, 32, 0, 701, TAB, 5),
    ('down', 1, 80, 16, 32, 8, 16, 0, 702, TAB, 5),
    ('tab9', 1, 160, 5, 9, 20, 36, 0, 703, TAB, 9),
    ('tab17', 1, 40, 4, 6, 32, 48, 0, 704, TAB, 17),
    ('beyond_x8', 1, 40, 3, 4, 32, 40, 0, 705, NHWC, 0),            # per-thread kernel, general branch
    ('three_lanes', 1, 260, 6, 10, 12, 20, 0, 706, TAB, 5),
    ('one_lane', 1, 516, 5, 7, 10, 14, 0, 707, NHWC, 0),            # per-thread kernel, 5-tap branch
    ('guarded', 1, 38, 7, 9, 14, 18, 38, 708, NHWC, 0),             # per-thread kernel, guarded loads and stores
    ('sliced', 1, 1100, 4, 6, 8, 12, 0, 709, NHWC, 0),              # 1024 + 76 channels
    ('nchw_tile', 1, 19, 8, 16, 64, 128, -1, 710, TILE, 0),
    ('nchw_ragged', 1, 19, 5, 9, 17, 33, -1, 711, TILE, 0),
    ('nchw_thread', 1, 6, 3, 4, 48, 64, -1, 712, NCHW, 0),
    ('nchw_down', 1, 6, 16, 16, 8, 8, -1, 713, NCHW, 0),
]
FWD = [('fwd_vec', 2, 40, 9, 17, 18, 33, 0, 720), ('fwd_guarded', 1, 38, 7, 9, 14, 18, 38, 721), ('fwd_sliced', 1, 1100, 4, 6, 8, 12, 0, 722),
       ('fwd_nchw', 1, 19, 8, 16, 64, 128, -1, 723)]
FAST = (31, 0)


def sha(*arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def _ld(case):
    Cc, ld = case[2], case[7]
    return (Cc + 3) // 4 * 4 if ld < 0 else ld or Cc


def variants(case):
    """(name, relu, dab) of a backward case"""
    if case[7] < 0:
        return [('scale', 0, False)]
    return [('relu', 1, False), ('plain', 0, False)] if case[2] > 1024 else [('relu_dab', 1, True), ('relu', 1, False), ('plain', 0, False)]


def make_inputs(case):
    """({name: array}, sha256 of all of them): x [P][ld], a, b [C], dy (NHWC [OP][ld] or NCHW [N][C][OH][OW]), g0 [P][ld]; forward cases: x, a, b"""
    name, N, Cc, H, W, OH, OW, ld, seed = case[:9]
    rs = np.random.RandomState(seed)
    ldx = _ld(case)
    arrs = {'x': rs.standard_normal((N * H * W, ldx)).astype(np.float32), 'a': rs.standard_normal(Cc).astype(np.float32),
            'b': (0.3 * rs.standard_normal(Cc)).astype(np.float32)}
    if case in BWD:
        arrs['dy'] = rs.standard_normal((N, Cc, OH, OW) if ld < 0 else (N * OH * OW, ldx)).astype(np.float32)
        arrs['g0'] = rs.standard_normal((N * H * W, ldx)).astype(np.float32)
    return arrs, sha(*[arrs[k] for k in sorted(arrs)])


def bwd_args(L, case, relu, dab, ptr):
    """addk_resize_bwd_args of a case on the pointers ptr[x, a, b, dy, g, dab, scale]"""
    name, N, Cc, H, W, OH, OW, ld = case[:8]
    ba = L.ResizeBwdArgs()
    ba.dy, ba.lddy, ba.nchw_in = ptr['dy'], 0 if ld < 0 else _ld(case), int(ld < 0)
    ba.dy_scale = ptr['scale'] if ld < 0 else None
    ba.src.x, ba.src.a, ba.src.b, ba.src.ld, ba.src.C, ba.src.relu = ptr['x'], ptr['a'], ptr['b'], _ld(case), Cc, relu
    ba.N, ba.H, ba.W, ba.OH, ba.OW = N, H, W, OH, OW
    ba.g, ba.ldg, ba.dab = ptr['g'], _ld(case), ptr['dab'] if dab else None
    return ba


def check_paths(L, lib):
    """Every backward case takes the kernel its entry claims (the tree's library, placeholder pointers, no GPU); raises otherwise"""
    from test_conv_dispatch import PTR
    ptr = dict(PTR, scale=PTR['stats'])
    fast = lib.addk_get_fast_paths()
    try:
        for case in BWD:
            for vname, relu, dab in variants(case):
                ba = bwd_args(L, case, relu, dab, ptr)
                for mask in FAST:
                    lib.addk_set_fast_paths(mask)
                    cfg = (C.c_int32 * 8)()
                    L.check(lib.addk_resize_bwd_config(C.byref(ba), cfg), 'resize_bwd_config')
                    want = (case[9], case[10]) if mask else (NCHW if case[7] < 0 else NHWC, 0)
                    if (cfg[0], cfg[1]) != want or cfg[6] != -(-min(case[2], 2048) // 1024):
                        raise AssertionError('%s/%s mask %d: kind, taps, slices %s, not %s' % (case[0], vname, mask, [cfg[0], cfg[1], cfg[6]], want))
    finally:
        lib.addk_set_fast_paths(fast)


def run_bwd(L, lib, case, arrs):
    """{variant/accN/fastM: {g: sha256, dab: sha256}} of a backward case"""
    import torch
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    name, N, Cc, H, W, OH, OW, ld = case[:8]
    d = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
    scale = torch.full((1,), 0.5, device=dev)
    rows = int(lib.addk_ew_rows(N * H * W, Cc))
    got = {}
    fast0 = lib.addk_get_fast_paths()
    try:
        for vname, relu, dab in variants(case):
            for acc in (0, 1):
                for fast in FAST:
                    lib.addk_set_fast_paths(fast)
                    g = d['g0'].clone() if acc else torch.full_like(d['g0'], float('nan'))
                    slab = torch.full((rows, Cc, 2), float('nan'), device=dev, dtype=torch.float64)
                    ptr = {'x': d['x'].data_ptr(), 'a': d['a'].data_ptr(), 'b': d['b'].data_ptr(), 'dy': d['dy'].data_ptr(),
                           'g': g.data_ptr(), 'dab': slab.data_ptr(), 'scale': scale.data_ptr()}
                    ba = bwd_args(L, case, relu, dab, ptr)
                    ba.accumulate = acc
                    rc = lib.addk_resize_bwd(C.byref(ba), st)
                    torch.cuda.synchronize()
                    assert rc == 0, (name, vname, acc, fast, lib.addk_last_error())
                    got['%s/acc%d/fast%d' % (vname, acc, fast)] = {'g': sha(g.cpu().numpy()), 'dab': sha(slab.cpu().numpy())}
    finally:
        lib.addk_set_fast_paths(fast0)
    return got


def run_fwd(L, lib, case, arrs):
    """{reluN: {y: sha256}} of a forward case"""
    import torch
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    name, N, Cc, H, W, OH, OW, ld = case[:8]
    d = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
    got = {}
    for relu in (1, 0):
        y = torch.full((N, Cc, OH, OW) if ld < 0 else (N * OH * OW, _ld(case)), float('nan'), device=dev)
        ar = L.ResizeArgs()
        ar.src.x, ar.src.a, ar.src.b, ar.src.ld, ar.src.C, ar.src.relu = d['x'].data_ptr(), d['a'].data_ptr(), d['b'].data_ptr(), _ld(case), Cc, relu
        ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
        ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0 if ld < 0 else _ld(case), int(ld < 0)
        rc = lib.addk_resize_fwd(C.byref(ar), st)
        torch.cuda.synchronize()
        assert rc == 0, (name, relu, lib.addk_last_error())
        got['relu%d' % relu] = {'y': sha(y.cpu().numpy())}
    return got


def main():
    import addk
    from addk import _lib as L
    import torch
    argv = [a for a in sys.argv[1:]]
    assert len(argv) >= 2 and argv[0] == '--lib', __doc__
    check_paths(L, addk.load())
    assert torch.cuda.is_available(), 'needs the MI355X'
    lib = C.CDLL(argv[1])
    for name in ('addk_resize_fwd', 'addk_resize_bwd', 'addk_set_fast_paths', 'addk_get_fast_paths', 'addk_ew_rows', 'addk_last_error'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGS[name]
    doc = {'about': 'sha256 of what addk_resize_fwd and addk_resize_bwd write on RandomState-seeded inputs; written by tests/tools/make_resize_bits.py '
                    'from the parent of the commit that gave csrc/resize.hip its one kernel choice',
           'cases': {}}
    for case in BWD + FWD:
        arrs, hin = make_inputs(case)
        runs = (run_bwd if case in BWD else run_fwd)(L, lib, case, arrs)
        doc['cases'][case[0]] = {'shape': list(case[1:9]), 'inputs': hin, 'runs': runs}
        print(case[0], hin[:12], len(runs), 'runs', flush=True)
    out = argv[2] if len(argv) > 2 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
