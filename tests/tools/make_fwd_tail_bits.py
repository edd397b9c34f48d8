#!/usr/bin/env python
"""Writes tests/golden/fwd_tail_parent_bits.json: sha256 of everything the forward kernels with a statistics tail write — the fused SepConv
half (csrc/sepf.hip: y, the stored depthwise output t, the whole statistics slab) for all twelve (KS, KG, KP, R) variants, lone, as a
two-member batch and with more slab rows than workgroups, and the pointwise kernels of csrc/pw.hip (pw_kernel forward and data gradient with
fp64 and fp32 lane sums, lone and batched, pwk_kernel, stem0_kernel; the cases, inputs and launches of tests/tools/make_pw_bits.py).  Every
output buffer is prefilled with NaN, so the own-row stores and the zero fill of the rows no workgroup owns are both in the hash.  Run it on
the MI355X with the library of the commit whose bits are to be pinned (ADDK_LIB selects another build of libaddk.so):

    ADDK_LIB=/path/to/parent/libaddk.so python tests/tools/make_fwd_tail_bits.py

tests/test_gpu_fwd_tail_bits.py imports the cases, make_inputs and the run functions from here, so the test and the fixture cannot drift.
The inputs come from numpy.random.RandomState, whose stream is frozen; their hash is stored too."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, 'tests', 'golden', 'fwd_tail_parent_bits.json')

_spec = importlib.util.spec_from_file_location('make_pw_bits', os.path.join(HERE, 'make_pw_bits.py'))
pwb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pwb)

# name, N, H, W, C, k, seed, slab rows beyond the workgroups, variant (KS, KG, KP, R).  R = 2 needs N ceil(H / 8) ceil(W / 16) >= 384 two-row
# tiles: 2 x 93 x 250 has 384 of them (and 2 x 89 x 250, the batch's second member, too), partial in both directions; R = 1 at 13 x 29:
# 4 x 2 tiles, the last row of tiles one pixel row deep, the last column 13 pixels wide.
SEPF_CASES = [
    ('c36_k3_r2',  2, 93, 250, 36, 3, 501, 0, (3, 3, 40, 2)),      # last channel group: 4 of 16 channels
    ('c36_k5_r2',  2, 93, 250, 36, 5, 502, 0, (5, 3, 40, 2)),
    ('c40_k3_r2',  2, 93, 250, 40, 3, 503, 0, (3, 3, 40, 2)),
    ('c40_k5_r2',  2, 93, 250, 40, 5, 504, 0, (5, 3, 40, 2)),
    ('c44_k3_r2',  2, 93, 250, 44, 3, 505, 0, (3, 3, 56, 2)),
    ('c44_k5_r2',  2, 93, 250, 44, 5, 506, 0, (5, 3, 56, 2)),
    ('c40_k3_r1',  1, 13, 29, 40, 3, 507, 0, (3, 3, 40, 1)),
    ('c40_k5_r1',  1, 13, 29, 40, 5, 508, 0, (5, 3, 40, 1)),
    ('c48_k3_r1',  1, 13, 29, 48, 3, 509, 0, (3, 3, 56, 1)),
    ('c48_k5_r1',  1, 13, 29, 48, 5, 510, 0, (5, 3, 56, 1)),
    ('c68_k3_r1',  1, 13, 29, 68, 3, 511, 0, (3, 5, 72, 1)),
    ('c68_k5_r1',  1, 13, 29, 68, 5, 512, 0, (5, 5, 72, 1)),
    ('c80_k3_r1',  1, 13, 29, 80, 3, 513, 0, (3, 5, 88, 1)),
    ('c80_k5_r1',  1, 13, 29, 80, 5, 514, 0, (5, 5, 88, 1)),
    ('c40_k3_r2_rows', 2, 93, 250, 40, 3, 515, 5, (3, 3, 40, 2)),   # rows > gx: every workgroup zeroes the rows behind its own
    ('c80_k5_r1_rows', 1, 13, 29, 80, 5, 516, 11, (5, 5, 88, 1)),   # ... more unowned rows than workgroups
]
SEPF_OUTPUTS = ('y', 't', 'slab')

# the cases of make_pw_bits.py this fixture takes: pw_kernel <CT, KG> = <3, 3> and <2, 5>, forward with statistics and data gradient with
# (dA, dB), grid a (P = 2145: fp64 lane sums) and b (P = 4160: fp32 lane sums), each lone and as a two-member batch; pwk_kernel with one and
# two sources; stem0_kernel with fp32 lane sums — and stem0 at 2 x 32 x 64 (P = 1024: fp64 lane sums), which that table does not hold
PW_NAMES = ['pw_fwd_40to40_a', 'pw_fwd_40to40_b', 'pw_fwd_80to40_a', 'pw_fwd_80to40_b',
            'pw_dgrad_40into40_a_acc0', 'pw_dgrad_40into40_b_acc0', 'pw_dgrad_80into40_a_acc1', 'pw_dgrad_80into40_b_acc1',
            'pwk_200to40_a', 'pwk_200to40_b', 'pwk_64+32to24_a', 'pwk_64+32to24_b', 'stem0_b']
STEM0_SMALL = ('stem0_2x32x64', 'fwd', dict(grid=(2, 32, 64), srcs=(3,), cout=64, k=3, stride=2, pad=1, rs=False, rs_y=False, bias=False, padded=False,
                                            accumulate=0, lazy=False), 390)
PW_CASES = [c for c in pwb.CASES if c[0] in PW_NAMES] + [STEM0_SMALL]
PW_PINS = dict({n: pwb.PINS[n] for n in PW_NAMES}, stem0_2x32x64=([2, 4, 0, 0, 0], -1))
assert len(PW_CASES) == len(PW_NAMES) + 1

sha = pwb.sha


def sepf_inputs(case):
    """(x, a, b, depthwise weights, pointwise weights) as float32 numpy arrays, and their sha256."""
    name, N, H, W, Cc, k, seed = case[:7]
    rs = np.random.RandomState(seed)
    f = lambda scale, *s: (scale * rs.standard_normal(s)).astype(np.float32)
    arrs = (f(1.0, N * H * W, Cc), (1.0 + 0.25 * rs.standard_normal(Cc)).astype(np.float32), f(0.3, Cc), f(0.3, Cc, k * k), f(0.2, Cc, Cc))
    return arrs, sha(*arrs)


def sepf_args(L, case, ptr, H=None, rows=0):
    """SepArgs of the training form (lazy BatchNorm + ReLU prologue, t stored, statistics slab of `rows` rows); H: another map height."""
    name, N, H0, W, Cc, k = case[:6]
    ar = L.SepArgs()
    ar.src.x, ar.src.a, ar.src.b, ar.src.ld, ar.src.C, ar.src.relu = ptr['x'], ptr['a'], ptr['b'], Cc, Cc, 1
    ar.N, ar.H, ar.W, ar.K, ar.Cout, ar.ldw = N, H or H0, W, k, Cc, Cc
    ar.dw_w, ar.pw_w, ar.y, ar.ldy = ptr['wdw'], ptr['wpw'], ptr['y'], Cc
    ar.t, ar.ldt, ar.stats, ar.stats_ld, ar.stats_rows = ptr['t'], Cc, ptr['slab'], Cc, rows
    return ar


def sepf_config(lb, L, case, H=None):
    """(variant [KS, KG, KP, R], workgroups, batch key) of a case's launch; needs no GPU (placeholder pointers, a large rows count)."""
    ar = sepf_args(L, case, {k: 0x10000000 * (i + 1) for i, k in enumerate(('x', 'a', 'b', 'wdw', 'wpw', 'y', 't', 'slab'))}, H=H, rows=1 << 20)
    cfg = (C.c_int32 * 8)()
    L.check(lb.addk_sep_fwd_config(C.byref(ar), cfg), 'sep_fwd_config')
    assert cfg[0] == 1, '%s: the fused kernel does not take this launch' % case[0]
    return [int(v) for v in cfg[1:5]], int(cfg[5]), int(cfg[7])


def run_sepf(L, case, arrs):
    """The lone launch and a two-member batch (the case, and the same map four rows shorter on its own outputs):
    ({launch: {buffer: sha256}}, variant)."""
    import torch
    lb = L.load()
    name, N, H, W, Cc, k, seed, extra, want = case
    variant, gx, key = sepf_config(lb, L, case)
    assert tuple(variant) == want, '%s runs variant %s, not %s' % (name, variant, want)
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    dv = dict(zip(('x', 'a', 'b', 'wdw', 'wpw'), (torch.from_numpy(v).to(dev) for v in arrs)))
    nan = lambda *sh, dt=torch.float32: torch.full(sh, float('nan'), device=dev, dtype=dt)

    def launch_args(Hm, rows):
        b = {'y': nan(N * Hm * W, Cc), 't': nan(N * Hm * W, Cc), 'slab': nan(rows, Cc, 2, dt=torch.float64)}
        ptr = {kk: v.data_ptr() for kk, v in dv.items()}
        ptr.update({kk: v.data_ptr() for kk, v in b.items()})
        return b, sepf_args(L, case, ptr, H=Hm, rows=rows)

    hashes = lambda b: {kk: sha(v.cpu().numpy()) for kk, v in sorted(b.items())}
    got = {}
    b, ar = launch_args(H, gx + extra)
    L.check(lb.addk_sep_fwd(C.byref(ar), stream), 'sep_fwd')
    torch.cuda.synchronize()
    got['lone'] = hashes(b)
    v1, gx1, key1 = sepf_config(lb, L, case, H=H - 4)
    assert (v1, key1) == (variant, key) and gx1 <= gx, '%s: the shorter map is another variant' % name      # (R = 1: fewer workgroups than the batch's grid)
    (b0, a0), (b1, a1) = launch_args(H, gx + extra), launch_args(H - 4, gx1 + 2)
    arr = (L.SepArgs * 2)(a0, a1)
    meta = (C.c_int64 * 8)()
    size = lb.addk_sep_fwd_batch_prepare(arr, 2, None, 0, meta)
    if size < 0:
        L.check(int(size), 'sep_fwd_batch_prepare')
    host = (C.c_uint8 * size)()
    rc = lb.addk_sep_fwd_batch_prepare(arr, 2, host, size, meta)
    if rc < 0:
        L.check(int(rc), 'sep_fwd_batch_prepare')
    assert [int(v) for v in meta[:4]] == [key, 2, gx, 1], '%s: batch meta %s' % (name, list(meta[:4]))
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    L.check(lb.addk_sep_batch_run(blob.data_ptr(), meta, stream), 'sep_batch_run')
    torch.cuda.synchronize()
    got['batch0'], got['batch1'] = hashes(b0), hashes(b1)
    return got, variant


def pins(L):
    """Variant and workgroups of every sepf case, kind / template values / batch key of every pw case, from placeholder pointers (no GPU)."""
    lb = L.load()
    out = {}
    for case in SEPF_CASES:
        out[case[0]] = sepf_config(lb, L, case) + (sepf_config(lb, L, case, H=case[2] - 4),)
    for case in PW_CASES:
        names = list(pwb.make_inputs(case)[0]) + ['y', 'slab', 'rs_y']
        ar = pwb.conv_args(L, case, {k: 0x10000000 * (i + 1) for i, k in enumerate(names)})
        cfg, gx, gy, key = pwb.config(lb, L, case, ar)
        rows = int(lb.addk_conv_rows(pwb.geometry(case)[5] if case[1] == 'fwd' else np.prod(case[2]['grid']), case[2]['cout'] if case[1] == 'fwd' else sum(case[2]['srcs'])))
        out[case[0]] = (cfg, key, gx, gy, rows)
    return out


def main():
    sys.path.insert(0, ROOT)
    import addk  # noqa: F401
    from addk import _lib as L
    lb = L.load()
    fast = lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(31)
    if '--pins' in sys.argv:
        for k, v in pins(L).items():
            print('    %r: %r,' % (k, v))
        lb.addk_set_fast_paths(fast)
        return
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    doc = {'about': 'sha256 of what the forward kernels with a statistics tail (csrc/sepf.hip, csrc/pw.hip) write on RandomState-seeded inputs; written by '
                    'tests/tools/make_fwd_tail_bits.py from the parent of the commit that moved the tail to a reduce-scatter in registers',
           'sepf': [], 'pw': []}
    for case in SEPF_CASES:
        arrs, hin = sepf_inputs(case)
        got, variant = run_sepf(L, case, arrs)
        doc['sepf'].append({'name': case[0], 'shape': list(case[1:6]), 'seed': case[6], 'extra_rows': case[7], 'variant': variant, 'inputs': hin, 'launches': got})
        print(case[0], variant, hin[:12], ' '.join('%s:%s' % (ln, '/'.join(h[:8] for h in hs.values())) for ln, hs in got.items()), flush=True)
    for case in PW_CASES:
        arrs, hin = pwb.make_inputs(case)
        got, (cfg, key) = pwb.run_case(L, case, arrs, PW_PINS[case[0]])
        doc['pw'].append({'name': case[0], 'op': case[1], 'seed': case[3], 'inputs': hin, 'cfg': cfg, 'key': key, 'launches': got})
        print(case[0], cfg, key, hin[:12], ' '.join('%s:%s' % (ln, '/'.join(h[:8] for h in hs.values())) for ln, hs in got.items()), flush=True)
    lb.addk_set_fast_paths(fast)
    out = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = out[0] if out else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
