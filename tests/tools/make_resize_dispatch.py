#!/usr/bin/env python
"""Writes tests/golden/resize_dispatch.json: what the host side of csrc/resize.hip answers for the resize backward of every shape in
SHAPES under every fast-path mask -- addk_resize_bwd_batch_key, and the return value and meta[0..3] of a one-item
addk_resize_bwd_batch_prepare.  No GPU: the library is called with aligned placeholder pointers, nothing is launched.

Run it with the library of the commit whose answers are to be pinned (the parent of the commit that gave resize.hip its one kernel
choice; that library has no addk_resize_bwd_config, so it is bound here by hand and not through addk._lib.load):

    python tests/tools/make_resize_dispatch.py --lib /path/to/parent/libaddk.so

tests/test_resize_dispatch.py imports SHAPES, bwd_args and record from here and compares the tree's library with the fixture."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'resize_dispatch.json')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

NHWC, TAB, NCHW, TILE = range(4)           # addk_resize_bwd_config's kinds
# name, N, C, H, W, OH, OW, pixel stride (0: C; NCHW gradient input: C rounded up to 4), kind with every fast path on, taps per axis
SHAPES = [
    # tests/test_gpu_resize.py, test_table_driven_resize_backward_matches_fp64_autograd
    ('up_32_63', 2, 40, 32, 64, 63, 127, 0, TAB, 5), ('fit_63_64', 1, 40, 63, 127, 64, 128, 0, TAB, 5), ('down4', 2, 64, 64, 128, 16, 32, 0, TAB, 5),
    ('down2', 1, 80, 64, 128, 32, 64, 0, TAB, 5), ('up2_c256', 2, 256, 16, 32, 32, 64, 0, TAB, 5), ('fit_128_125', 1, 40, 128, 256, 125, 253, 0, TAB, 5),
    ('up4_c160', 2, 160, 32, 64, 128, 256, 0, TAB, 9), ('up4_odd', 1, 80, 31, 63, 125, 253, 0, TAB, 9), ('up8_c160', 1, 160, 16, 32, 128, 256, 0, TAB, 17),
    ('up2_c400', 2, 400, 32, 64, 64, 128, 0, TAB, 5),
    # test_logits_upsample_backward_tiled_matches_autograd
    ('logits_x4', 2, 19, 64, 128, 256, 512, -1, TILE, 0), ('logits_odd', 1, 19, 33, 65, 129, 257, -1, TILE, 0), ('logits_c6', 1, 6, 40, 50, 80, 100, -1, TILE, 0),
    # the edges of the up-sampling rules, each just inside and just outside: OH <= 2H + 1, OW <= 4W + 1, OH <= 8H + 1
    ('oh_2h1', 1, 40, 16, 32, 33, 65, 0, TAB, 5), ('oh_2h2', 1, 40, 16, 32, 34, 65, 0, TAB, 9),
    ('ow_4w1', 1, 40, 16, 32, 64, 129, 0, TAB, 9), ('ow_4w2', 1, 40, 16, 32, 64, 130, 0, TAB, 17),
    ('oh_8h1', 1, 40, 8, 16, 65, 128, 0, TAB, 17), ('oh_8h2', 1, 40, 8, 16, 66, 128, 0, NHWC, 0),
    # channel counts: one pixel lane (generic), three lanes (segments of npl * 8 pixels), four lanes, not vector-aligned, sliced
    ('c516', 1, 516, 8, 12, 16, 24, 0, NHWC, 0), ('c260', 1, 260, 8, 30, 16, 60, 0, TAB, 5), ('c256', 1, 256, 8, 30, 16, 60, 0, TAB, 5),
    ('c38', 1, 38, 8, 12, 16, 24, 38, NHWC, 0), ('c1100', 1, 1100, 4, 6, 8, 12, 0, NHWC, 0),
    ('w_lt_tw', 1, 40, 16, 5, 32, 10, 0, TAB, 5),                      # 25 pixel lanes: segments of 100 pixels, clamped to the row
    # NCHW gradient input: x8 (LDS-tiled), x16 (too large for the tile), down-sampling (per-thread)
    ('nchw_x8', 1, 19, 8, 16, 64, 128, -1, TILE, 0), ('nchw_x16', 1, 19, 4, 8, 64, 128, -1, NCHW, 0), ('nchw_down', 1, 6, 16, 16, 8, 8, -1, NCHW, 0),
]
IDS = [s[0] for s in SHAPES]


def bwd_args(L, shape, ptr, relu=1):
    """addk_resize_bwd_args of a shape on placeholder pointers `ptr` (tests/test_conv_dispatch.py PTR); NHWC: lazy ReLU source and (dA, dB) slab"""
    name, N, Cc, H, W, OH, OW, ld = shape[:8]
    nchw = ld < 0
    ld = (Cc + 3) // 4 * 4 if nchw else ld or Cc
    ba = L.ResizeBwdArgs()
    ba.dy, ba.lddy, ba.nchw_in = ptr['dy'], 0 if nchw else ld, int(nchw)
    ba.src.x, ba.src.a, ba.src.b, ba.src.ld, ba.src.C, ba.src.relu = ptr['x'], ptr['a'], ptr['b'], ld, Cc, 0 if nchw else relu
    ba.N, ba.H, ba.W, ba.OH, ba.OW = N, H, W, OH, OW
    ba.g, ba.ldg, ba.dab = ptr['g'], ld, None if nchw or Cc > 1024 else ptr['dab']
    return ba


def prepare(lib, items):
    """(return value, meta[0..3]) of addk_resize_bwd_batch_prepare without a blob"""
    arr = (type(items[0]) * len(items))(*items)
    meta = (C.c_int64 * 8)()
    size = int(lib.addk_resize_bwd_batch_prepare(arr, len(items), None, 0, meta))
    return size, list(meta[:4])


def record(lib, ba):
    size, meta = prepare(lib, [ba])
    return {'key': int(lib.addk_resize_bwd_batch_key(C.byref(ba))), 'size': size, 'meta': meta if size > 0 else None}


def main():
    from addk import _lib as L
    from test_conv_dispatch import MASKS, PTR
    assert len(sys.argv) == 3 and sys.argv[1] == '--lib', __doc__
    lib = C.CDLL(sys.argv[2])
    for name in ('addk_resize_bwd_batch_key', 'addk_resize_bwd_batch_prepare', 'addk_set_fast_paths', 'addk_get_fast_paths'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGS[name]
    doc = {'about': 'addk_resize_bwd_batch_key and a one-item addk_resize_bwd_batch_prepare (return value, meta[0..3]) per shape and fast-path mask; written by '
                    'tests/tools/make_resize_dispatch.py from the parent of the commit that gave csrc/resize.hip its one kernel choice',
           'masks': MASKS, 'shapes': {}}
    for shape in SHAPES:
        ba = bwd_args(L, shape, PTR)
        doc['shapes'][shape[0]] = {'shape': list(shape[1:8]), 'masks': {}}
        for mask in MASKS:
            lib.addk_set_fast_paths(mask)
            doc['shapes'][shape[0]]['masks'][str(mask)] = record(lib, ba)
        print(shape[0], doc['shapes'][shape[0]]['masks']['31'], doc['shapes'][shape[0]]['masks']['0'])
    with open(OUT, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', OUT)


if __name__ == '__main__':
    main()
