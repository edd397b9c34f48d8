#!/usr/bin/env python
"""Writes tests/golden/wgrad_parent_bits.json: sha256 of what the dense weight gradient (csrc/wgrad*.hip) writes on seeded inputs,
for the smallest shapes that reach every kernel family, every NP, NT, NG, both register-streaming arithmetics and both the lone
and the batched launch.  Per case and arithmetic mode: dw of a lone launch (first touch; accumulate onto a seeded dw), the
NaN-prefilled workspace, and both dw of a two-conv batch of the same conv (op 0 first touch, op 1 accumulating).  Run it on the
MI355X with the library of the commit whose bits are to be pinned (ADDK_LIB selects another build of libaddk.so):

    ADDK_LIB=/path/to/parent/libaddk.so python tests/tools/make_wgrad_bits.py

tests/test_gpu_wgrad_bits.py imports CASES, make_inputs and run_case from here, and tests/test_wgrad_dispatch.py pins the launch
key of every (case, mode) without a GPU, so test, fixture and dispatch cannot drift.  The inputs come from
numpy.random.RandomState, whose stream is frozen; their hash is stored too, so that a changed input shows up as such and not as
a changed kernel."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'wgrad_parent_bits.json')

MODES = {'fp32': 0, 'f16x3': 1, 'bf16x6': 2}
FAST_ALL = 31
# name, (N, H, W, Cin, Cout, k, stride, dil), fast-path mask, padded strides (src.ld = C + 8, lddy = Cout + 4), seed,
# {mode: (kind, cty, ctz)} = addk_conv_wgrad_config's launch key; a mode that is absent has no kernel of that kind
CASES = [
    ('pix_tiny',     (1, 9, 11, 20, 24, 3, 1, 1),     FAST_ALL, False, 201, {'fp32': (0, 2, 1), 'f16x3': (0, 2, 1), 'bf16x6': (0, 2, 1)}),      # wgrad_kernel<2,1>
    ('pix_3x3',      (1, 70, 125, 40, 40, 3, 1, 2),   0,        False, 202, {'fp32': (0, 3, 3), 'f16x3': (0, 3, 3), 'bf16x6': (0, 3, 3)}),      # wgrad_kernel<3,3>
    ('os_128x64',    (1, 16, 32, 64, 128, 1, 1, 1),   FAST_ALL, False, 203, {'fp32': (1, 8, 4), 'f16x3': (1, 8, 4), 'bf16x6': (1, 8, 4)}),      # wgrad_os_kernel<4,2>
    ('os_96x96',     (2, 16, 32, 80, 80, 1, 1, 1),    FAST_ALL, True,  204, {'fp32': (2, 6, 6), 'f16x3': (2, 6, 6), 'bf16x6': (2, 6, 6)}),      # wgrad_os_kernel<3,3>
    ('os_64x64',     (2, 16, 32, 64, 64, 1, 1, 1),    FAST_ALL, False, 205, {'fp32': (3, 4, 4), 'f16x3': (3, 4, 4), 'bf16x6': (3, 4, 4)}),      # wgrad_os_kernel<2,2>
    ('h3_nt1_ng1',   (2, 33, 129, 24, 64, 3, 1, 2),   FAST_ALL, False, 206, {'fp32': (5, 4, 1), 'f16x3': (5, 4, 1), 'bf16x6': (5, 4, 1)}),      # wgrad_h3<1>, wgrad_h3b<1,NP,1>
    ('h3_nt2_ng1',   (1, 40, 256, 16, 128, 3, 1, 1),  FAST_ALL, False, 207, {'fp32': (5, 8, 1), 'f16x3': (5, 8, 1), 'bf16x6': (5, 8, 1)}),      # wgrad_h3<2>, wgrad_h3b<2,NP,1>
    ('h3_nt2_ng2',   (1, 40, 256, 32, 128, 3, 1, 1),  FAST_ALL, True,  208, {'fp32': (5, 8, 1), 'f16x3': (5, 8, 2), 'bf16x6': (5, 8, 2)}),      # wgrad_h3b<2,NP,2>
    ('h3_nt1_ng2',   (1, 65, 130, 32, 64, 3, 1, 1),   FAST_ALL, False, 209, {'fp32': (5, 4, 1), 'f16x3': (5, 4, 2), 'bf16x6': (5, 4, 2)}),      # wgrad_h3b<1,NP,2>
    ('h1_c200',      (1, 70, 130, 200, 128, 1, 1, 1), FAST_ALL, False, 210, {'f16x3': (9, 8, 4), 'bf16x6': (9, 8, 4)}),                       # wgrad_h1b<NP>
    ('hk_3x3_ct3',   (1, 70, 125, 40, 40, 3, 1, 2),   FAST_ALL, False, 211, {'fp32': (7, 3, 3), 'f16x3': (7, 3, 3), 'bf16x6': (7, 3, 3)}),      # wgrad_hk<3,3>, wgrad_hkb<3,3,NP>
    ('hk_5x5_ct3',   (1, 70, 125, 40, 40, 5, 1, 2),   FAST_ALL, False, 212, {'fp32': (7, 3, 5), 'f16x3': (7, 3, 5), 'bf16x6': (7, 3, 5)}),      # wgrad_hk<5,3>, wgrad_hkb<5,3,NP>
    ('hk_3x3_ct5',   (2, 40, 104, 32, 160, 3, 1, 2),  FAST_ALL, True,  213, {'fp32': (7, 5, 3), 'f16x3': (7, 5, 3), 'bf16x6': (7, 5, 3)}),      # wgrad_hk<3,5>, wgrad_hkb<3,5,NP>
    ('rs_33',        (1, 33, 125, 40, 40, 1, 1, 1),   FAST_ALL, False, 214, {'fp32': (6, 3, 3), 'f16x3': (6, 3, 3), 'bf16x6': (6, 3, 3)}),      # wgrad_rs<3,3>, fp32 and fp16 forms
    ('rs_44',        (1, 33, 125, 64, 64, 1, 1, 1),   FAST_ALL, False, 215, {'fp32': (6, 4, 4), 'f16x3': (6, 4, 4), 'bf16x6': (6, 4, 4)}),      # wgrad_rs<4,4>
    ('rs_34',        (1, 33, 125, 64, 40, 1, 1, 1),   FAST_ALL, True,  216, {'fp32': (6, 3, 4), 'f16x3': (6, 3, 4), 'bf16x6': (6, 3, 4)}),      # wgrad_rs<3,4>
    ('rs_43',        (1, 33, 125, 40, 64, 1, 1, 1),   FAST_ALL, False, 217, {'fp32': (6, 4, 3), 'f16x3': (6, 4, 3), 'bf16x6': (6, 4, 3)}),      # wgrad_rs<4,3>
    ('rs_3x3_s2',    (2, 97, 129, 48, 96, 3, 2, 1),   FAST_ALL, False, 218, {'fp32': (6, 3, 3), 'f16x3': (6, 3, 3), 'bf16x6': (6, 3, 3)}),      # strided tap walk
    ('st_stem0',     (2, 256, 511, 3, 64, 3, 2, 1),   FAST_ALL, False, 219, {'fp32': (8, 4, 2), 'f16x3': (8, 4, 2), 'bf16x6': (8, 4, 2)}),      # wgrad_st
]
OUTPUTS = ('dw_first', 'dw_accumulate', 'ws', 'batch_dw0', 'batch_dw1')


def sha(*arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def geometry(case):
    """(N, H, W, Ci, Cout, k, stride, dil, pad, OH, OW, ldx, lddy) of a case."""
    N, H, W, Ci, Cout, k, s, d = case[1]
    pad = d * (k // 2)
    OH, OW = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
    return N, H, W, Ci, Cout, k, s, d, pad, OH, OW, Ci + (8 if case[3] else 0), Cout + (4 if case[3] else 0)


def make_inputs(case):
    """(x, a, b, dy, dw0) as float32 numpy arrays (x and dy with their row strides), and their sha256."""
    N, H, W, Ci, Cout, k, s, d, pad, OH, OW, ldx, lddy = geometry(case)
    rs = np.random.RandomState(case[4])
    f = lambda scale, *sh: (scale * rs.standard_normal(sh)).astype(np.float32)
    arrs = (f(1.0, N * H * W, ldx), (1.0 + 0.25 * rs.standard_normal(Ci)).astype(np.float32), f(0.3, Ci), f(1.0, N * OH * OW, lddy), f(1.0, Cout, k * k * Ci))
    return arrs, sha(*arrs)


def wgrad_args(L, case, ptr):
    """ConvWgradArgs of a case; `ptr` maps dy, x, a, b, dw to addresses (ws and ws_floats are left to the caller)."""
    N, H, W, Ci, Cout, k, s, d, pad, OH, OW, ldx, lddy = geometry(case)
    wa = L.ConvWgradArgs()
    wa.dy, wa.lddy, wa.Cout = ptr['dy'], lddy, Cout
    wa.N, wa.H, wa.W, wa.OH, wa.OW, wa.KH, wa.KW, wa.stride, wa.pad, wa.dil = N, H, W, OH, OW, k, k, s, pad, d
    wa.src.x, wa.src.a, wa.src.b, wa.src.ld, wa.src.C, wa.src.relu = ptr['x'], ptr['a'], ptr['b'], ldx, Ci, 1
    wa.dw, wa.ldw, wa.cin_total, wa.w_choff, wa.accumulate = ptr['dw'], k * k * Ci, Ci, 0, 0
    return wa


def run_case(L, case, mode, arrs, key=None):
    """The lone launches and the two-conv batch of one case in one arithmetic mode: ({output name: sha256}, launch key).
    `key`: the launch key the conv must get, asserted before anything is launched.  Sets the case's fast-path mask and the mode;
    the caller restores them."""
    import torch
    lb = L.load()
    name = case[0]
    N, H, W, Ci, Cout, k, s, d, pad, OH, OW, ldx, lddy = geometry(case)
    lb.addk_set_fast_paths(case[2])
    L.check(lb.addk_set_conv_precision(MODES[mode]), 'set_conv_precision')
    dev = torch.device('cuda:0')
    x, a, b, dy, dw0 = (torch.from_numpy(v).to(dev) for v in arrs)
    st = torch.cuda.current_stream().cuda_stream
    ws_floats = int(lb.addk_conv_wgrad_ws(N * OH * OW, Cout, Ci, k * k))
    nan = lambda *sh: torch.full(sh, float('nan'), device=dev)

    def args(dw, ws, acc):
        wa = wgrad_args(L, case, {'dy': dy.data_ptr(), 'x': x.data_ptr(), 'a': a.data_ptr(), 'b': b.data_ptr(), 'dw': dw.data_ptr()})
        wa.accumulate, wa.ws, wa.ws_floats = acc, ws.data_ptr(), ws_floats
        return wa

    cfg = (C.c_int32 * 4)()
    L.check(lb.addk_conv_wgrad_config(C.byref(args(dw0, nan(1), 0)), cfg), 'conv_wgrad_config')
    assert key is None or [int(v) for v in cfg[:3]] == list(key), '%s [%s] gets launch key %s, expected %s' % (name, mode, list(cfg[:3]), list(key))
    got = {}
    for acc in (0, 1):
        dw, ws = (dw0.clone() if acc else nan(*dw0.shape)), nan(ws_floats)
        L.check(lb.addk_conv_wgrad(C.byref(args(dw, ws, acc)), st), 'conv_wgrad')
        torch.cuda.synchronize()
        got['dw_accumulate' if acc else 'dw_first'] = sha(dw.cpu().numpy())
        h = sha(ws.cpu().numpy())
        assert got.setdefault('ws', h) == h, '%s [%s]: the workspace differs between the first-touch and the accumulating launch' % (name, mode)
    # the same conv twice in one batch, into separate gradients and workspaces: op 0 first touch, op 1 accumulating
    dws, wss = [nan(*dw0.shape), dw0.clone()], [nan(ws_floats), nan(ws_floats)]
    arr = (L.ConvWgradArgs * 2)(args(dws[0], wss[0], 0), args(dws[1], wss[1], 1))
    meta = (C.c_int64 * 8)()
    size = lb.addk_conv_wgrad_batch_prepare(arr, 2, None, 0, meta)
    if size < 0:
        L.check(int(size), 'conv_wgrad_batch_prepare')
    host = (C.c_uint8 * size)()
    rc = lb.addk_conv_wgrad_batch_prepare(arr, 2, host, size, meta)
    if rc < 0:
        L.check(int(rc), 'conv_wgrad_batch_prepare')
    assert list(meta[:3]) == list(cfg[:3]), '%s [%s]: the batch carries another launch key than the lone launch' % (name, mode)
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    L.check(lb.addk_conv_wgrad_batch_run(blob.data_ptr(), meta, st), 'conv_wgrad_batch_run')
    torch.cuda.synchronize()
    got['batch_dw0'], got['batch_dw1'] = sha(dws[0].cpu().numpy()), sha(dws[1].cpu().numpy())
    return got, [int(v) for v in cfg[:3]]


def main():
    sys.path.insert(0, ROOT)
    import torch
    import addk  # noqa: F401
    from addk import _lib as L
    assert torch.cuda.is_available(), 'needs the MI355X'
    lb = L.load()
    prec = lb.addk_get_conv_precision()
    doc = {'about': 'sha256 of the dense weight gradient\'s outputs on RandomState-seeded inputs; written by tests/tools/make_wgrad_bits.py from '
                    'the parent of the commit that split csrc/wgrad.hip into a shared header and one file per kernel family', 'cases': []}
    for case in CASES:
        arrs, hin = make_inputs(case)
        rec = {'name': case[0], 'shape': list(case[1]), 'fast': case[2], 'padded': case[3], 'seed': case[4], 'inputs': hin, 'modes': {}}
        for mode in MODES:
            if mode not in case[5]:
                continue
            got, key = run_case(L, case, mode, arrs, case[5][mode])
            rec['modes'][mode] = {'key': key, **got}
            print(case[0], mode, key, hin[:12], ' '.join(got[o][:12] for o in OUTPUTS), flush=True)
        doc['cases'].append(rec)
    lb.addk_set_fast_paths(FAST_ALL)
    lb.addk_set_conv_precision(prec)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
