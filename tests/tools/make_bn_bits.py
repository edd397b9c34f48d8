#!/usr/bin/env python
"""Writes tests/golden/bn_parent_bits.json: sha256 of every output of slab_reduce, bn_bwd_coeffs, bn_eval_affine and bn_bwd_apply
(csrc/bn.hip, csrc/elementwise.hip) on seeded inputs, at the smallest sizes at which these kernels can go wrong.  Run it on the
MI355X with the library of the commit whose bits are to be pinned (ADDK_LIB selects another build of libaddk.so):

    ADDK_LIB=/path/to/parent/libaddk.so python tests/tools/make_bn_bits.py

The hashes come from the four `_batch` entry points, whose signatures and table layouts are those of every version of the library:
each case as a table of one, then the cases of GROUPS as ONE table, which must give the same hashes.  The lone entry points took
positional arguments in version 1 of the library (addk_version()) and take the table's item since version 2; bind() binds what the
loaded library has, and this tool refuses to write unless the lone form gives the hashes of the table form.

tests/test_gpu_bn_bits.py imports CASES, GROUPS, inputs, run_table and run_lone from here, so the test and the fixture cannot
drift.  The inputs come from numpy.random.RandomState, whose stream is frozen; their hash is stored too, so that a changed input
shows up as such and not as a changed kernel.  Every output is pre-filled with NaN."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'bn_parent_bits.json')
EPS, COUNT = 1e-5, 63250.0

# slab_reduce: one row, the row-group boundary (64), the 512-row batch boundary, a third batch; C = 3 is a partial channel block.
# bn_bwd_coeffs: 257 is one channel past a 256-thread block.  bn_bwd_apply (vector-aligned): (8200, 256) is past 2048 blocks of 4 pixels
# (the table kernel's stride loop runs), (32771, 256) past 8192 blocks of 4 pixels (the lone kernel's stride loop runs).
_APPLY = ((1, 4), (5, 40), (3, 1024), (8200, 256), (32771, 256))
CASES = {
    'slab_reduce': [dict(rows=r, C=c) for r in (1, 65, 513, 1025) for c in (3, 40)],
    'bn_bwd_coeffs': [dict(C=c) for c in (1, 40, 257)],
    'bn_eval_affine': [dict(C=c, affine=a) for c in (1, 19, 257, 1000) for a in (1, 0)],
    'bn_bwd_apply': [dict(P=p, C=c, mean=m) for p, c in _APPLY for m in (1, 0)],
}
# the cases that also run as ONE table: blocks beyond a short item's C or P return
GROUPS = dict(CASES, bn_bwd_apply=[c for c in CASES['bn_bwd_apply'] if c['P'] != 32771])
OUTPUTS = {'slab_reduce': ('out',), 'bn_bwd_coeffs': ('c1', 'c2'), 'bn_eval_affine': ('a', 'b'), 'bn_bwd_apply': ('out',)}
FLAGS = ('affine', 'mean')             # what a case leaves NULL; the inputs do not depend on it


def case_id(op, case):
    return '%s-%s' % (op, '-'.join('%s%d' % kv for kv in case.items()))


def sha(*arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


_inputs = {}


def inputs(op, case):
    """({name: numpy array}, sha256 of them) of a case; cases that differ in a flag only share their arrays"""
    shape = tuple((k, v) for k, v in case.items() if k not in FLAGS)
    if (op, shape) not in _inputs:
        rs = np.random.RandomState(1000 + sum(map(ord, op)) + sum(v * (i + 3) for i, (_, v) in enumerate(shape)) % 100000)
        f = lambda scale, *s: (scale * rs.standard_normal(s)).astype(np.float32)           # noqa: E731
        Cc = case['C']
        if op == 'slab_reduce':      # magnitudes 2^-20 .. 2^19: a sum in another order has other bits
            arrs = {'partial': rs.standard_normal((case['rows'], Cc, 2)) * 2.0 ** rs.randint(-20, 20, (case['rows'], Cc, 2))}
        elif op == 'bn_bwd_coeffs':
            arrs = {'dmv': f(1.0, Cc, 2)}
        elif op == 'bn_eval_affine':
            arrs = {'gamma': 1 + f(0.3, Cc), 'beta': f(1.0, Cc), 'running_mean': f(1.0, Cc),
                    'running_var': (0.01 + 2 * rs.random_sample(Cc)).astype(np.float32)}
        else:                         # the two maps are multiples of 2^-13 (16-bit draws: the big case stays quick); the roundings come from the vectors
            m = lambda: rs.randint(-32768, 32768, (case['P'], Cc)).astype(np.float32) / 8192           # noqa: E731
            arrs = {'g': m(), 'x': m(), 'mean': f(1.0, Cc), 'c1': f(0.5, Cc), 'c2': f(0.5, Cc)}
        _inputs[(op, shape)] = (arrs, sha(*arrs.values()))
    return _inputs[(op, shape)]


_device = {}


def _dev(op, case):
    import torch
    arrs, h = inputs(op, case)
    if h not in _device:
        _device[h] = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
    return _device[h]


def _item(L, op, case):
    """(the item of a case, its NaN-filled outputs by name)"""
    import torch
    d, Cc = _dev(op, case), case['C']
    nan = lambda *s, dtype=torch.float32: torch.full(s, float('nan'), device='cuda', dtype=dtype)      # noqa: E731
    p = lambda t: t.data_ptr()                                                                          # noqa: E731
    if op == 'slab_reduce':
        it, o = L.SlabReduceItem(), {'out': nan(Cc, 2, dtype=torch.float64)}
        it.partial, it.out, it.rows, it.C = p(d['partial']), p(o['out']), case['rows'], Cc
    elif op == 'bn_bwd_coeffs':
        it, o = L.BnCoeffsItem(), {'c1': nan(Cc), 'c2': nan(Cc)}
        it.dmv, it.c1, it.c2, it.count, it.C = p(d['dmv']), p(o['c1']), p(o['c2']), COUNT, Cc
    elif op == 'bn_eval_affine':
        it, o = L.BnEvalItem(), {'a': nan(Cc), 'b': nan(Cc)}
        it.gamma, it.beta = (p(d['gamma']), p(d['beta'])) if case['affine'] else (None, None)
        it.running_mean, it.running_var, it.a, it.b, it.C, it.eps = p(d['running_mean']), p(d['running_var']), p(o['a']), p(o['b']), Cc, EPS
    else:
        it, o = L.BnApplyItem(), {'out': nan(case['P'], Cc)}
        it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = p(d['g']), p(d['x']), p(d['c1']), p(d['c2']), p(d['mean']) if case['mean'] else None, p(o['out']), case['P']
        it.ldg, it.ldx, it.ldo, it.C = Cc, Cc, Cc, Cc
    return it, o


def _hashes(op, outs):
    import torch
    torch.cuda.synchronize()
    return {k: sha(outs[k].cpu().numpy()) for k in OUTPUTS[op]}


def _check(lib, rc, what):
    if rc:
        raise RuntimeError('%s failed (%d): %s' % (what, rc, lib.addk_last_error().decode()))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_table(L, lib, op, cases):
    """`cases` as ONE table through the op's _batch entry point; [{output name: sha256}] in the order of `cases`"""
    import torch
    made = [_item(L, op, c) for c in cases]
    arr = (type(made[0][0]) * len(made))(*[it for it, _ in made])
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    size = () if op == 'bn_eval_affine' else (max(c['P' if op == 'bn_bwd_apply' else 'C'] for c in cases),)
    _check(lib, getattr(lib, 'addk_%s_batch' % op)(tab.data_ptr(), len(made), *size, _stream()), op + '_batch')
    return [_hashes(op, o) for _, o in made]


def run_lone(L, lib, op, case):
    """One case through the lone entry point: the item (library version 2), or the positional arguments it spells (version 1)"""
    it, o = _item(L, op, case)
    if lib.addk_version() >= 2:
        rc = getattr(lib, 'addk_' + op)(C.byref(it), _stream())
    elif op == 'slab_reduce':
        rc = lib.addk_slab_reduce(it.partial, it.rows, it.C, it.out, _stream())
    elif op == 'bn_bwd_coeffs':
        rc = lib.addk_bn_bwd_coeffs_from_dmv(it.dmv, it.C, it.count, it.c1, it.c2, _stream())
    elif op == 'bn_eval_affine':
        rc = lib.addk_bn_eval_affine(it.gamma, it.beta, it.running_mean, it.running_var, it.eps, it.C, it.a, it.b, _stream())
    else:
        rc = lib.addk_bn_bwd_apply(it.g, it.ldg, it.x, it.ldx, it.mean, it.c1, it.c2, it.P, it.C, it.out, it.ldo, _stream())
    _check(lib, rc, op)
    return _hashes(op, o)


def bind(path):
    """libaddk.so at `path` with the BatchNorm entry points bound: the lone ones by what addk_version() of that library says"""
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    lib = C.CDLL(path)
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    lib.addk_last_error.restype = C.c_char_p
    lone = {'addk_slab_reduce': [vp, vp], 'addk_bn_bwd_coeffs': [vp, vp], 'addk_bn_eval_affine': [vp, vp], 'addk_bn_bwd_apply': [vp, vp]}
    if lib.addk_version() < 2:
        lone = {'addk_slab_reduce': [vp, i32, i32, vp, vp], 'addk_bn_bwd_coeffs_from_dmv': [vp, i32, f64, vp, vp, vp],
                'addk_bn_eval_affine': [vp, vp, vp, vp, f32, i32, vp, vp, vp],
                'addk_bn_bwd_apply': [vp, i32, vp, i32, vp, vp, vp, i64, i32, vp, i32, vp]}
    table = {'addk_slab_reduce_batch': [vp, i32, i32, vp], 'addk_bn_bwd_coeffs_batch': [vp, i32, i32, vp],
             'addk_bn_eval_affine_batch': [vp, i32, vp], 'addk_bn_bwd_apply_batch': [vp, i32, i64, vp]}
    for name, args in {**lone, **table}.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, C.c_int
    return lib


def main():
    sys.path.insert(0, ROOT)
    import torch
    import addk  # noqa: F401
    from addk import _lib as L
    assert torch.cuda.is_available(), 'needs the MI355X'
    lib = bind(L.LIB_PATH)
    doc = {'about': 'sha256 of the outputs of the BatchNorm table launches on RandomState-seeded inputs; written by tests/tools/make_bn_bits.py '
                    'from the parent of the commit that gave the lone launches the tables\' items', 'library_version': int(lib.addk_version()), 'cases': []}
    for op, cases in CASES.items():
        single = {case_id(op, c): run_table(L, lib, op, [c])[0] for c in cases}
        for c, got in zip(GROUPS[op], run_table(L, lib, op, GROUPS[op])):
            assert got == single[case_id(op, c)], '%s: one table of all cases differs from a table of one' % case_id(op, c)
        for c in cases:
            got = run_lone(L, lib, op, c)
            assert got == single[case_id(op, c)], '%s: the lone launch differs from the table launch' % case_id(op, c)
            doc['cases'].append({'id': case_id(op, c), 'inputs': inputs(op, c)[1], **got})
            print(case_id(op, c), inputs(op, c)[1][:12], ' '.join(v[:12] for v in got.values()), flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
