#!/usr/bin/env python
"""Writes tests/golden/conv_dispatch.json: what the host side of the forward / data-gradient convolutions (csrc/conv.hip conv_choose_*) answers
for every launch of a sweep -- cfg[0..7] of addk_conv_*_config, addk_conv_*_pack_floats and addk_conv_*_batch_key.  A launch is a map x a channel
pair x a geometry x a direction x an arithmetic mode, every fast path on (mask 31), with a weight-pack workspace large enough for any kernel.
No GPU: the library is called with aligned placeholder pointers, nothing is launched.

Run it with the library of the commit whose answers are to be pinned:

    python tests/tools/make_conv_dispatch.py --lib /path/to/libaddk.so

Encoding.  `rows` lists the distinct (cfg[0..4], cfg[6], cfg[7], batch key); `launches` holds one entry per (map, channel pair, geometry,
direction) in the order of launches(), and each entry one item per mode of MODES: [row, cfg[5]] or [row, cfg[5], pack floats] (no pack floats:
0), or the index of an earlier mode of the entry with the same answer.  tests/test_conv_variants.py imports the sweep and the decoder from here
and compares the tree's library with the fixture."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'conv_dispatch.json')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

MODES = ['fp32', 'f16x3', 'bf16x6', 'tail_x3']                 # addk_set_conv_precision 0..3
MAPS = [(1, 16, 48), (1, 33, 65), (2, 32, 64), (1, 50, 100), (1, 64, 128), (2, 63, 127), (1, 128, 256), (2, 65, 300), (2, 125, 253), (2, 128, 256),
        (2, 256, 512), (1, 512, 1024), (2, 512, 1024)]
# input -> output channels: the forward's kernel follows the output count, the data gradient's the input count
CHANNELS = [(16, 16), (16, 256), (32, 32), (32, 128), (40, 40), (64, 48), (64, 64), (80, 80), (96, 96), (128, 64), (160, 160), (192, 208), (208, 192),
            (256, 256), (256, 304), (304, 256), (400, 256), (256, 400), (512, 128), (640, 640)]
# kernel size, stride, dilation ('same' padding; the stride-2 3x3 pads 1)
GEOMETRIES = [(1, 1, 1), (3, 1, 1), (3, 1, 2), (3, 1, 3), (3, 1, 6), (3, 1, 18), (5, 1, 1), (5, 1, 2), (3, 2, 1)]
WPACK_FLOATS = 1 << 40


def launches():
    """(shape in the form of tests/test_conv_dispatch.py, 'fwd' | 'dgrad') of every entry, in the fixture's order"""
    for mi, (N, H, W) in enumerate(MAPS):
        for cin, cout in CHANNELS[1 - mi % 2::2]:          # every second pair, alternating from map to map: half the cross product, every value in it
            for k, s, d in GEOMETRIES:
                shape = ('%dx%dx%d_%d_%d_k%ds%dd%d' % (N, H, W, cin, cout, k, s, d), N, H, W, (cin,), cout, k, s, d * (k // 2), d, 0, True)
                yield shape, 'fwd'
                yield shape, 'dgrad'


def args_of(shape, t, ptr):
    import test_conv_dispatch as T
    a = T._fwd(shape) if t == 'fwd' else T._dgrads(shape)[0]
    a.wpack, a.wpack_floats = ptr['wpack'], WPACK_FLOATS
    return a


def record(lib, a, t):
    """[cfg[0..7], pack floats, batch key] of one launch under the library's current mode and mask"""
    cfg = (C.c_int32 * 8)()
    rc = getattr(lib, 'addk_conv_%s_config' % t)(C.byref(a), cfg)
    assert rc == 0, rc
    return list(cfg) + [int(getattr(lib, 'addk_conv_%s_pack_floats' % t)(C.byref(a))), int(getattr(lib, 'addk_conv_%s_batch_key' % t)(C.byref(a)))]


def decode(doc):
    """one list per entry: the records of MODES"""
    out = []
    for entry in doc['launches']:
        recs = []
        for item in entry:
            if isinstance(item, int):
                recs.append(recs[item])
                continue
            r = doc['rows'][item[0]]
            recs.append(r[:5] + [item[1], r[5], r[6], item[2] if len(item) > 2 else 0, r[7]])
        out.append(recs)
    return out


def sweep(lib, ptr):
    """the records of every entry, mode by mode (the library's mode and mask are the caller's to restore)"""
    lib.addk_set_fast_paths(31)
    items = [(args_of(shape, t, ptr), t) for shape, t in launches()]
    out = [[] for _ in items]
    for m in range(len(MODES)):
        assert lib.addk_set_conv_precision(m) == 0
        for i, (a, t) in enumerate(items):
            out[i].append(record(lib, a, t))
    return out


def main():
    from addk import _lib as L
    from test_conv_dispatch import PTR
    assert len(sys.argv) == 3 and sys.argv[1] == '--lib', __doc__
    lib = C.CDLL(sys.argv[2])
    for name in ('addk_conv_fwd_config', 'addk_conv_dgrad_config', 'addk_conv_fwd_pack_floats', 'addk_conv_dgrad_pack_floats', 'addk_conv_fwd_batch_key',
                 'addk_conv_dgrad_batch_key', 'addk_set_conv_precision', 'addk_set_fast_paths'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGS[name]
    rows, entries = {}, []
    for recs in sweep(lib, PTR):
        entry = []
        for m, r in enumerate(recs):
            if r in recs[:m]:
                entry.append(recs.index(r))
                continue
            row = rows.setdefault(tuple(r[:5] + [r[6], r[7], r[9]]), len(rows))
            entry.append([row, r[5], r[8]] if r[8] else [row, r[5]])
        entries.append(entry)
    doc = {'about': 'cfg[0..7] of addk_conv_*_config, addk_conv_*_pack_floats and addk_conv_*_batch_key per launch of the sweep in '
                    'tests/tools/make_conv_dispatch.py (which documents the encoding), fast-path mask 31, a large enough wpack; written from a build of '
                    'the parent of the commit that made the convolution choice resolve its kernel, with ONLY that commit\'s fp32 column-block fix '
                    'applied (csrc/conv3.hip c3_bct: a 5x5 never takes the 128-channel block, which has no 5x5 kernel) -- the parent alone answers '
                    'a block of 8 tiles for some fp32 5x5 launches, which then failed',
           'modes': MODES, 'maps': MAPS, 'channels': CHANNELS, 'geometries': GEOMETRIES,
           'rows': [list(r) for r in rows], 'launches': entries}
    with open(OUT, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(entries), 'entries,', len(rows), 'rows')


if __name__ == '__main__':
    main()
