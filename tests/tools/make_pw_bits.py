#!/usr/bin/env python
"""Writes tests/golden/pw_parent_bits.json: sha256 of what the kernels of csrc/pw.hip write on seeded inputs, for the smallest shapes
that reach every variant: pw_kernel <CT, KG> x forward / resampled forward / data gradient x fp64 / fp32 lane sums (lone and as a
two-member batch), pwk_kernel CT 1..3 and a second channel block, plain and resampled, stem0_kernel and k1s_dgrad_kernel KMAX 20 / 32.
Per launch: y (or g), the statistics / (dA, dB) slab and, where present, the rs_y copy, every buffer prefilled with NaN (an
accumulating data gradient: with a seeded gradient) so that the own-row store and the zero-fill of the rows no workgroup owns are
both in the hash.  Run it on the MI355X with the library of the commit whose bits are to be pinned (ADDK_LIB selects another build of
libaddk.so):

    ADDK_LIB=/path/to/parent/libaddk.so python tests/tools/make_pw_bits.py

A GPU test that compares a library with the fixture imports CASES, make_inputs and run_case from here (run_case asserts the pins
before it launches), and tests/test_pw_dispatch.py pins the kernel kind, template values and batch key of every case without a GPU,
so fixture and dispatch cannot drift.  The inputs come from
numpy.random.RandomState, whose stream is frozen; their hash is stored too, so that a changed input shows up as such and not as a
changed kernel."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'pw_parent_bits.json')

STEM0, PW, PWK, K1S = 2, 3, 4, 5
GRID_A = (1, 33, 65)       # P = 2145: a partial last 16-pixel tile, fp64 lane sums
GRID_B = (2, 40, 52)       # P = 4160 >= 4096: fp32 lane sums
RS_MAP = (17, 33)          # the map a resampled source is sampled from
PAIRS = [(40, 12), (48, 24), (40, 40), (80, 16), (80, 40)]      # (K, channels out): <CT, KG> = <1,3>, <2,3>, <3,3>, <1,5>, <2,5> (two channel blocks)
PWK_SRCS = [((200,), 40), ((64, 32), 24), ((128,), 16), ((200,), 160)]      # CT 3, 2, 1 and gy = 4


def _cases():
    """name, op, spec, seed.  spec: grid (N, H, W) of the input, srcs (channels per source), cout, k / stride / pad, rs (source 0 is
    sampled from RS_MAP), rs_y, bias, padded (row strides = channels + 8), accumulate."""
    out = []

    def add(name, op, **kw):
        spec = dict(grid=GRID_A, srcs=(40,), cout=40, k=1, stride=1, pad=0, rs=False, rs_y=False, bias=False, padded=False, accumulate=0, lazy=True)
        spec.update(kw)
        spec['padded'] = len(out) % 2 == 1 if 'padded' not in kw else kw['padded']
        out.append((name, op, spec, 300 + len(out)))

    for gi, grid in (('a', GRID_A), ('b', GRID_B)):
        for K, co in PAIRS:
            add('pw_fwd_%dto%d_%s' % (K, co, gi), 'fwd', grid=grid, srcs=(K,), cout=co, bias=(K, co, gi) == (48, 24, 'a'))
            add('pw_fwd_rs_%dto%d_%s' % (K, co, gi), 'fwd', grid=grid, srcs=(K,), cout=co, rs=True, rs_y=(K, co, gi) == (40, 40, 'b'))
    for gi, grid in (('a', GRID_A), ('b', GRID_B)):
        for K, co in PAIRS:           # the forward pair's K is the gradient's channel count, its output channels the reduction
            for acc in (0, 1):
                add('pw_dgrad_%dinto%d_%s_acc%d' % (K, co, gi, acc), 'dgrad', grid=grid, srcs=(co,), cout=K, accumulate=acc)
    for gi, grid in (('a', GRID_A), ('b', GRID_B)):
        for srcs, co in PWK_SRCS:
            nm = '+'.join(map(str, srcs))
            add('pwk_%sto%d_%s' % (nm, co, gi), 'fwd', grid=grid, srcs=srcs, cout=co)
            add('pwk_rs_%sto%d_%s' % (nm, co, gi), 'fwd', grid=grid, srcs=srcs, cout=co, rs=True, rs_y=True)
    add('stem0_a', 'fwd', grid=(1, 33, 65), srcs=(3,), cout=64, k=3, stride=2, pad=1, lazy=False, padded=False)       # P = 561: fp64 sums
    add('stem0_b', 'fwd', grid=(2, 90, 95), srcs=(3,), cout=64, k=3, stride=2, pad=1, lazy=False, padded=True)        # P = 4320: fp32 sums
    for co, ch in ((19, 256), (24, 128)):        # KMAX 20 / 32
        for acc in (0, 1):
            add('k1s_%dinto%d_acc%d' % (co, ch, acc), 'dgrad', grid=GRID_A, srcs=(ch,), cout=co, accumulate=acc)
    return out


CASES = _cases()
# name -> ([kind, v0, v1, v2, v3] of addk_conv_fwd_config / addk_conv_dgrad_config, batch key (-1: not a batchable launch)), recorded from the
# parent of the commit that took the fused SepConv form out of csrc/pw.hip (`python tests/tools/make_pw_bits.py --pins`, no GPU needed)
PINS = {
    'pw_fwd_40to12_a': ([3, 1, 3, 0, 0], 304),
    'pw_fwd_rs_40to12_a': ([3, 1, 3, 1, 0], 306),
    'pw_fwd_48to24_a': ([3, 2, 3, 0, 0], 560),
    'pw_fwd_rs_48to24_a': ([3, 2, 3, 1, 0], 562),
    'pw_fwd_40to40_a': ([3, 3, 3, 0, 0], 816),
    'pw_fwd_rs_40to40_a': ([3, 3, 3, 1, 0], 818),
    'pw_fwd_80to16_a': ([3, 1, 5, 0, 0], 336),
    'pw_fwd_rs_80to16_a': ([3, 1, 5, 1, 0], 338),
    'pw_fwd_80to40_a': ([3, 2, 5, 0, 0], 592),
    'pw_fwd_rs_80to40_a': ([3, 2, 5, 1, 0], 594),
    'pw_fwd_40to12_b': ([3, 1, 3, 0, 1], 305),
    'pw_fwd_rs_40to12_b': ([3, 1, 3, 1, 1], 307),
    'pw_fwd_48to24_b': ([3, 2, 3, 0, 1], 561),
    'pw_fwd_rs_48to24_b': ([3, 2, 3, 1, 1], 563),
    'pw_fwd_40to40_b': ([3, 3, 3, 0, 1], 817),
    'pw_fwd_rs_40to40_b': ([3, 3, 3, 1, 1], 819),
    'pw_fwd_80to16_b': ([3, 1, 5, 0, 1], 337),
    'pw_fwd_rs_80to16_b': ([3, 1, 5, 1, 1], 339),
    'pw_fwd_80to40_b': ([3, 2, 5, 0, 1], 593),
    'pw_fwd_rs_80to40_b': ([3, 2, 5, 1, 1], 595),
    'pw_dgrad_40into12_a_acc0': ([3, 1, 3, 0, 0], 4400),
    'pw_dgrad_40into12_a_acc1': ([3, 1, 3, 0, 0], 4400),
    'pw_dgrad_48into24_a_acc0': ([3, 2, 3, 0, 0], 4656),
    'pw_dgrad_48into24_a_acc1': ([3, 2, 3, 0, 0], 4656),
    'pw_dgrad_40into40_a_acc0': ([3, 3, 3, 0, 0], 4912),
    'pw_dgrad_40into40_a_acc1': ([3, 3, 3, 0, 0], 4912),
    'pw_dgrad_80into16_a_acc0': ([3, 1, 5, 0, 0], 4432),
    'pw_dgrad_80into16_a_acc1': ([3, 1, 5, 0, 0], 4432),
    'pw_dgrad_80into40_a_acc0': ([3, 2, 5, 0, 0], 4688),
    'pw_dgrad_80into40_a_acc1': ([3, 2, 5, 0, 0], 4688),
    'pw_dgrad_40into12_b_acc0': ([3, 1, 3, 0, 1], 4401),
    'pw_dgrad_40into12_b_acc1': ([3, 1, 3, 0, 1], 4401),
    'pw_dgrad_48into24_b_acc0': ([3, 2, 3, 0, 1], 4657),
    'pw_dgrad_48into24_b_acc1': ([3, 2, 3, 0, 1], 4657),
    'pw_dgrad_40into40_b_acc0': ([3, 3, 3, 0, 1], 4913),
    'pw_dgrad_40into40_b_acc1': ([3, 3, 3, 0, 1], 4913),
    'pw_dgrad_80into16_b_acc0': ([3, 1, 5, 0, 1], 4433),
    'pw_dgrad_80into16_b_acc1': ([3, 1, 5, 0, 1], 4433),
    'pw_dgrad_80into40_b_acc0': ([3, 2, 5, 0, 1], 4689),
    'pw_dgrad_80into40_b_acc1': ([3, 2, 5, 0, 1], 4689),
    'pwk_200to40_a': ([4, 3, 0, 0, 0], -1),
    'pwk_rs_200to40_a': ([4, 3, 1, 0, 0], -1),
    'pwk_64+32to24_a': ([4, 2, 0, 0, 0], -1),
    'pwk_rs_64+32to24_a': ([4, 2, 1, 0, 0], -1),
    'pwk_128to16_a': ([4, 1, 0, 0, 0], -1),
    'pwk_rs_128to16_a': ([4, 1, 1, 0, 0], -1),
    'pwk_200to160_a': ([4, 3, 0, 0, 0], -1),
    'pwk_rs_200to160_a': ([4, 3, 1, 0, 0], -1),
    'pwk_200to40_b': ([4, 3, 0, 1, 0], -1),
    'pwk_rs_200to40_b': ([4, 3, 1, 1, 0], -1),
    'pwk_64+32to24_b': ([4, 2, 0, 1, 0], -1),
    'pwk_rs_64+32to24_b': ([4, 2, 1, 1, 0], -1),
    'pwk_128to16_b': ([4, 1, 0, 1, 0], -1),
    'pwk_rs_128to16_b': ([4, 1, 1, 1, 0], -1),
    'pwk_200to160_b': ([4, 3, 0, 1, 0], -1),
    'pwk_rs_200to160_b': ([4, 3, 1, 1, 0], -1),
    'stem0_a': ([2, 4, 0, 0, 0], -1),
    'stem0_b': ([2, 4, 1, 0, 0], -1),
    'k1s_19into256_acc0': ([5, 20, 0, 0, 0], -1),
    'k1s_19into256_acc1': ([5, 20, 0, 0, 0], -1),
    'k1s_24into128_acc0': ([5, 32, 0, 0, 0], -1),
    'k1s_24into128_acc1': ([5, 32, 0, 0, 0], -1),
}


def sha(*arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def geometry(case):
    """(N, H, W, OH, OW, P) of a case: input grid, output grid (P = N OH OW pixels of the forward output)."""
    s = case[2]
    N, H, W = s['grid']
    OH, OW = (H + 2 * s['pad'] - s['k']) // s['stride'] + 1, (W + 2 * s['pad'] - s['k']) // s['stride'] + 1
    return N, H, W, OH, OW, N * OH * OW


def strides(case):
    """Row strides of a case: per-source ld, ldw, ldy (forward) / lddy (gradient), ldg, stats_ld."""
    s = case[2]
    pad = 8 if s['padded'] else 0
    ctot = sum(s['srcs'])
    return {'ld': [4 if c == 3 else c + pad for c in s['srcs']], 'ldw': s['k'] * s['k'] * ctot + (pad if s['k'] == 1 else 0), 'ldy': s['cout'] + pad,
            'stats_ld': s['cout'] + pad, 'rs_ldy': s['srcs'][0] + pad}


def make_inputs(case):
    """({name: float32 array}, sha256 of all of them).  fwd: x<i>, a<i>, b<i>, w, bias; dgrad: dy, x0 (the forward input), a0, b0, w, g0."""
    s = case[2]
    N, H, W, OH, OW, P = geometry(case)
    st = strides(case)
    rs = np.random.RandomState(case[3])
    f = lambda scale, *sh: (scale * rs.standard_normal(sh)).astype(np.float32)
    ctot = sum(s['srcs'])
    arrs = {}
    for i, c in enumerate(s['srcs']):
        rows = N * RS_MAP[0] * RS_MAP[1] if (s['rs'] and i == 0) else N * H * W
        arrs['x%d' % i] = f(1.0, rows, st['ld'][i])
        arrs['a%d' % i] = (1.0 + 0.25 * rs.standard_normal(c)).astype(np.float32)
        arrs['b%d' % i] = f(0.3, c)
    arrs['w'] = f(1.0 / np.sqrt(s['k'] * s['k'] * ctot), s['cout'], st['ldw'])
    if case[1] == 'fwd':
        arrs['bias'] = f(0.5, s['cout'])
    else:
        arrs['dy'] = f(1.0, P, st['ldy'])
        arrs['g0'] = f(1.0, P, st['ld'][0])
    return arrs, sha(*[arrs[k] for k in sorted(arrs)])


def conv_args(L, case, ptr):
    """ConvArgs / ConvDgradArgs of a case; `ptr` maps buffer names (the inputs of make_inputs, y / g, slab, rs_y) to addresses."""
    s = case[2]
    N, H, W, OH, OW, P = geometry(case)
    st = strides(case)
    ctot = sum(s['srcs'])
    if case[1] == 'fwd':
        ar = L.ConvArgs()
        for i, c in enumerate(s['srcs']):
            ar.src[i].x, ar.src[i].ld, ar.src[i].C = ptr['x%d' % i], st['ld'][i], c
            if s['lazy']:
                ar.src[i].a, ar.src[i].b, ar.src[i].relu = ptr['a%d' % i], ptr['b%d' % i], 1
            if s['rs'] and i == 0:
                ar.src[i].rs_hw = (RS_MAP[0] << 16) | RS_MAP[1]
        ar.nsrc = len(s['srcs'])
        ar.N, ar.H, ar.W, ar.OH, ar.OW, ar.KH, ar.KW, ar.stride, ar.pad, ar.dil, ar.Cout = N, H, W, OH, OW, s['k'], s['k'], s['stride'], s['pad'], 1, s['cout']
        ar.ldw, ar.cin_total, ar.w_choff, ar.ldy = st['ldw'], ctot, 0, st['ldy']
        ar.w, ar.y, ar.stats, ar.stats_ld = ptr['w'], ptr['y'], ptr['slab'], st['stats_ld']
        if s['bias']:
            ar.bias = ptr['bias']
        if s['rs_y']:
            ar.rs_y, ar.rs_ldy = ptr['rs_y'], st['rs_ldy']
        return ar
    da = L.ConvDgradArgs()
    da.dy, da.lddy, da.Cout = ptr['dy'], st['ldy'], s['cout']
    da.N, da.H, da.W, da.OH, da.OW, da.KH, da.KW, da.stride, da.pad, da.dil = N, H, W, OH, OW, 1, 1, 1, 0, 1
    da.w, da.ldw, da.cin_total, da.w_choff = ptr['w'], st['ldw'], ctot, 0
    da.dst.x, da.dst.a, da.dst.b, da.dst.ld, da.dst.C, da.dst.relu = ptr['x0'], ptr['a0'], ptr['b0'], st['ld'][0], ctot, 1
    da.g, da.ldg, da.accumulate, da.dab = ptr['y'], st['ld'][0], s['accumulate'], ptr['slab']
    return da


def config(lb, L, case, ar):
    """([kind, v0..v3], gx, gy, batch key) of a case's launch."""
    t = 'dgrad' if case[1] == 'dgrad' else 'fwd'
    cfg = (C.c_int32 * 8)()
    L.check(getattr(lb, 'addk_conv_%s_config' % t)(C.byref(ar), cfg), 'conv_%s_config' % t)
    return [int(v) for v in cfg[:5]], int(cfg[5]), int(cfg[6]), int(getattr(lb, 'addk_conv_%s_batch_key' % t)(C.byref(ar)))


def run_case(L, case, arrs, pin=None):
    """The lone launch and, for the register-stationary kernel, a two-member batch of the same launch: ({launch: {buffer: sha256}},
    ([kind, v0..v3], key)).  `pin`: the kind, template values and batch key the launch must get, asserted before anything is launched."""
    import torch
    lb = L.load()
    s = case[2]
    t = 'dgrad' if case[1] == 'dgrad' else 'fwd'
    N, H, W, OH, OW, P = geometry(case)
    st = strides(case)
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    dv = {k: torch.from_numpy(v).to(dev) for k, v in arrs.items()}
    rows = int(lb.addk_conv_rows(P if t == 'fwd' else N * H * W, s['cout'] if t == 'fwd' else sum(s['srcs'])))
    nan = lambda *sh, dt=torch.float32: torch.full(sh, float('nan'), device=dev, dtype=dt)

    def buffers():
        b = {'slab': nan(rows, st['stats_ld'] if t == 'fwd' else sum(s['srcs']), 2, dt=torch.float64)}
        if t == 'fwd':
            b['y'] = nan(P, st['ldy'])
            if s['rs_y']:
                b['rs_y'] = nan(P, st['rs_ldy'])
        else:
            b['y'] = dv['g0'].clone() if s['accumulate'] else nan(P, st['ld'][0])
        return b

    def args(b):
        ptr = {k: v.data_ptr() for k, v in dv.items()}
        ptr.update({k: v.data_ptr() for k, v in b.items()})
        return conv_args(L, case, ptr)

    hashes = lambda b: {k: sha(v.cpu().numpy()) for k, v in sorted(b.items())}
    b = buffers()
    cfg, gx, gy, key = config(lb, L, case, args(b))
    assert pin is None or (cfg, key) == (list(pin[0]), pin[1]), '%s gets kind / template values %s and batch key %d, expected %s' % (case[0], cfg, key, pin)
    assert cfg[0] == K1S or gx < rows, '%s: every slab row is owned (gx %d, rows %d): the zero-fill would not be in the hash' % (case[0], gx, rows)
    got = {}
    L.check(getattr(lb, 'addk_conv_%s' % t)(C.byref(args(b)), stream), 'conv_%s' % t)
    torch.cuda.synchronize()
    got['lone'] = hashes(b)
    if cfg[0] == PW:
        bs = [buffers(), buffers()]
        a0, a1 = args(bs[0]), args(bs[1])
        arr = (type(a0) * 2)(a0, a1)
        meta = (C.c_int64 * 8)()
        prep = getattr(lb, 'addk_conv_%s_batch_prepare' % t)
        size = prep(arr, 2, None, 0, meta)
        if size < 0:
            L.check(int(size), 'conv_%s_batch_prepare' % t)
        host = (C.c_uint8 * size)()
        rc = prep(arr, 2, host, size, meta)
        if rc < 0:
            L.check(int(rc), 'conv_%s_batch_prepare' % t)
        assert int(meta[0]) == key and int(meta[1]) == 2, '%s: the batch carries key %d, the lone launch %d' % (case[0], int(meta[0]), key)
        blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
        L.check(lb.addk_conv_batch_run(blob.data_ptr(), meta, stream), 'conv_batch_run')
        torch.cuda.synchronize()
        got['batch0'], got['batch1'] = hashes(bs[0]), hashes(bs[1])
    return got, (cfg, key)


def pins(L):
    """The PINS table of the loaded library, from placeholder pointers: nothing is dereferenced before a launch."""
    lb = L.load()
    out = {}
    for case in CASES:
        names = list(make_inputs(case)[0]) + ['y', 'slab', 'rs_y']
        ar = conv_args(L, case, {k: 0x10000000 * (i + 1) for i, k in enumerate(names)})
        cfg, gx, gy, key = config(lb, L, case, ar)
        out[case[0]] = (cfg, key)
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
            print('    %r: (%r, %d),' % (k, v[0], v[1]))
        lb.addk_set_fast_paths(fast)
        return
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    doc = {'about': 'sha256 of what the kernels of csrc/pw.hip write on RandomState-seeded inputs; written by tests/tools/make_pw_bits.py from '
                    'the parent of the commit that took the fused SepConv form out of pw.hip', 'cases': []}
    for case in CASES:
        arrs, hin = make_inputs(case)
        got, (cfg, key) = run_case(L, case, arrs, PINS[case[0]])
        doc['cases'].append({'name': case[0], 'op': case[1], 'spec': {k: (list(v) if isinstance(v, tuple) else v) for k, v in case[2].items()},
                             'seed': case[3], 'inputs': hin, 'cfg': cfg, 'key': key, 'launches': got})
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
