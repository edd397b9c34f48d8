#!/usr/bin/env python
"""Writes tests/_conv_cases.py: for every halo-patch kernel the lookups of csrc/conv3b.h offer (c3_variant_fp32, c3b_variant_*, c3n_variant), the
cheapest launch of a small search space that the library's own choice (addk_conv_*_config, fast-path mask 31, split minimum 0, a large enough wpack)
sends to it, and for a variant that admits both parities of the dilation one launch per parity (d = 1 and 2; d = 3 and 6 on the `bigd` rows).  No GPU:
nothing is launched.

A launch is a map x an output-side channel count x a K-side channel count x a geometry x a direction x an arithmetic mode.  Among the launches of a
variant the one that meets most of the four shape constraints of tests/_conv_ref.constraints wins, then one whose output-side channel count is no
multiple of 16 (a partly filled last tile), then the one with the fewest multiply-adds; the constraints that the winner does not meet, so that no
launch of the space meets them together with the others, are recorded as the case's `ruled out`.

    python tests/tools/find_conv_cases.py          (after a build; then run tests/test_conv_ref.py)"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', '_conv_cases.py')
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

MAPS = [(1, 33, 65), (1, 41, 53), (3, 33, 65), (1, 65, 127), (1, 83, 101), (1, 193, 50), (1, 129, 257), (2, 63, 255), (1, 171, 193), (1, 65, 193), (2, 33, 130)]
CN = [32, 36, 40, 44, 48, 52, 64, 80, 96, 100, 128, 136, 160, 192, 200, 208, 256, 272, 304, 320, 384, 400]      # output side: Cout of a forward, channels of a gradient
CK = [20, 24, 40]                                                                                               # K side: source channels of a forward, dy channels of a gradient
GEOMETRIES = [(1, 1, 1), (3, 1, 1), (3, 1, 2), (3, 1, 3), (3, 1, 6), (5, 1, 1), (5, 1, 2), (3, 2, 1)]           # kernel size, stride, dilation
SEARCH_MODES = ['fp32', 'f16x3', 'bf16x6']

HEAD = '''"""The launches of tests/test_gpu_conv_fp64.py: one per instantiated halo-patch kernel of the forward / data-gradient convolution and per parity of the
dilation it admits.  Written by tests/tools/find_conv_cases.py (which documents the search); tests/test_conv_ref.py checks without a GPU that the library's
choice sends every launch to the variant named here and that the variants are exactly the instantiated ones.

(lookup, lookup arguments, map N x H x W, source channels, output channels, kernel size, stride, dilation, direction, mode, ruled out), the lookup arguments as
in tests/test_conv_variants.LOOKUPS.  `ruled out`: the shape constraints (tests/_conv_ref.constraints: W no multiple of the tile row, H odd against the row
pairs, K with a tail chunk, C no multiple of the block's columns) that no launch of the search space meets together with the others for this variant."""
CASES = [
'''


def main():
    import addk
    from addk import _lib as L
    import _conv_ref as R
    lib = addk.load()
    lib.addk_set_fast_paths(31)
    lib.addk_set_split_min_channels(0)
    best = {}
    for mode in SEARCH_MODES:
        assert lib.addk_set_conv_precision(R.MODES[mode]) == 0
        for (N, H, W), Cn, K, (k, s, d), direction in itertools.product(MAPS, CN, CK, GEOMETRIES, ('fwd', 'dgrad')):
            Cs, Cout = ((K,), Cn) if direction == 'fwd' else ((Cn,), K)
            op = R.make_op(N, H, W, Cs, Cout, k, s, d)
            lookup, args = R.variant_of(R.config(L, lib, R.host_args(L, op, direction)), op, direction, mode)
            if lookup == 'kind' or (lookup == 'c3_variant_fp32' and d > 2):      # (the fp32 kernel has one form for every dilation: d = 1 and 2)
                continue
            unmet = ''.join(sorted(c for c, ok in R.constraints(lookup, args, op, direction).items() if not ok))
            cost = op.N * op.OH * op.OW * Cn * K * k * k
            entry = (len(unmet), Cn % 16 == 0, cost, (lookup, args, (N, H, W), Cs[0], Cout, k, s, d, direction, mode, unmet))
            key = (lookup, args, d)
            if key not in best or entry[:3] < best[key][:3]:
                best[key] = entry
    lib.addk_set_split_min_channels(-1)
    rows = [best[key] for key in sorted(best)]
    with open(OUT, 'w') as f:
        f.write(HEAD)
        for _, _, cost, e in rows:
            f.write('    %r,\n' % (e,))
        f.write(']\n')
    nvar = len({(r[3][0], r[3][1]) for r in rows})
    print('wrote %s: %d launches of %d variants, %.2f GMAC, the largest %.2f GMAC; constraints ruled out in %d launches'
          % (OUT, len(rows), nvar, sum(r[2] for r in rows) / 1e9, max(r[2] for r in rows) / 1e9, sum(1 for r in rows if r[0])))


if __name__ == '__main__':
    main()
