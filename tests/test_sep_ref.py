"""The fused SepConv suite's case list, reference and bound (tests/_sep_ref.py), checked without a GPU:

* the 24 cases take, through addk_sep_fwd_config and addk_sep_bwd_config with placeholder pointers, the variant each names, the same in both
  directions, with 24 and 384 workgroups, and between them exactly the twelve entries of ADDK_SEP_VARIANTS as csrc/sep.h lists them; the batch members
  (1 x 1 x 1, 3 x 5 x 16, the second two-row shape) take the case's variant with 1, 6 and 392 workgroups;
* the reference equals explicit tap-by-tap Python loops (no conv2d, no autograd) on 1 x 5 x 7 with 8 channels in all four source forms: t, y, the
  statistics, the finalize, two inference epilogues, dx, (dA, dB) and dW_dw; backward_taps equals the autograd reference at every case;
* the bound can fail: at every case, eleven subtly wrong results lie at least 10 x TOL from the right one in the measure the GPU suite uses (max|got -
  ref| / max|ref|, statistics and (dA, dB) as one array each).  The smallest ratio over the 24 cases x 11 mistakes is 1502 x TOL (the sum of squares
  without the last tile row, 1 of 13 rows, at k3_g3_p40_r1-c36-2x13x37); every other mistake is beyond 7000 x TOL at every case."""
import ctypes as C

import numpy as np
import pytest

import addk
from addk import _lib as L
import _sep_ref as R

TOL = R.TOL
MISTAKES = ('1 taps not flipped', '2 border row from the neighbouring image', '3 ReLU mask from x', '4 last channel quad of t zero', '5 pw_w not transposed',
            '6 sumsq misses the last tile row', '7 dA without x', '8 accumulate overwrites', '9 dW_dw misses pixel lane 15', "10 term 1's ReLU dropped",
            '11 ea applied to the terms')


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    fast = lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(R.FAST_ALL)
    yield lb
    lb.addk_set_fast_paths(fast)


def _both(lib, op):
    ar = R.fwd_args(L, op, R.PTR, t=True, stats_rows=4096)
    f, b = R.config(L, lib, ar), R.config(L, lib, R.bwd_args(L, op, R.PTR))
    assert f[0] == b[0] == 1 and f[1:7] == b[1:7], (op, f, b)
    assert f[5] == int(lib.addk_sep_rows(C.byref(ar)))
    return tuple(f[1:5]), f[5]


def test_the_cases_reach_exactly_the_built_variants(lib):
    built = R.built_variants()
    assert len(built) == len(set(built)) == 12
    assert len(R.CASES) == 24
    reached = set()
    for c in R.CASES:
        variant, gx = _both(lib, c.op)
        assert variant == c.variant, (R.case_id(c), variant)
        assert gx == (24 if c.variant[3] == 1 else 384), (R.case_id(c), gx)
        reached.add(variant)
        grids = [_both(lib, m) for m in R.batch_members(c)]
        assert all(v == c.variant for v, _ in grids), (R.case_id(c), grids)
        assert [g for _, g in grids] == ([24, 6, 1] if c.variant[3] == 1 else [384, 384, 392]), (R.case_id(c), grids)
    assert reached == set(built)
    # every padded stride once with a partial last quad group and once at its upper end; the last group holds 4, 8, 12 or 16 channels
    assert {(c.variant[2], (c.op.C - 1) % 16 + 1) for c in R.CASES} == {(40, 4), (40, 8), (56, 12), (56, 16), (72, 4), (72, 8), (88, 12), (88, 16)}


# ---------------------------------------------------------------------------------------------------------------- explicit loops

def _loops(op, inp, form):
    """everything from the definition, pixel by pixel and tap by tap, in Python floats (float64)"""
    aff, relu = R.FORMS[form]
    N, H, W, Cc, K, p = op.N, op.H, op.W, op.C, op.K, op.K // 2
    P = N * H * W
    f8 = lambda v: np.asarray(v, dtype=np.float64)
    x, dwv, pw, dy = f8(R.x_of(op, inp)), f8(inp['dw_w']), f8(R.pw_of(op, inp)), f8(inp['dy'][:, :Cc])
    a = f8(inp['a']) if aff else np.ones(Cc)
    b = f8(inp['b']) if aff else np.zeros(Cc)
    pix = lambda n, h, w: (n * H + h) * W + w
    z, m = np.zeros((P, Cc)), np.zeros((P, Cc))
    for q in range(P):
        for c in range(Cc):
            v = a[c] * x[q, c] + b[c]
            m[q, c] = 1.0 if (not relu or v > 0) else 0.0
            z[q, c] = v if (not relu or v > 0) else 0.0
    t, y, dt, dz, dW = np.zeros((P, Cc)), np.zeros((P, Cc)), np.zeros((P, Cc)), np.zeros((P, Cc)), np.zeros((Cc, K * K))
    for q in range(P):
        for c in range(Cc):
            s = 0.0
            for co in range(Cc):
                s += dy[q, co] * pw[co, c]
            dt[q, c] = s
    for n in range(N):
        for h in range(H):
            for w in range(W):
                q = pix(n, h, w)
                for c in range(Cc):
                    s = 0.0
                    for ky in range(K):
                        for kx in range(K):
                            ih, iw = h + ky - p, w + kx - p
                            if 0 <= ih < H and 0 <= iw < W:
                                s += dwv[c, ky * K + kx] * z[pix(n, ih, iw), c]
                                dW[c, ky * K + kx] += dt[q, c] * z[pix(n, ih, iw), c]
                                dz[pix(n, ih, iw), c] += dwv[c, ky * K + kx] * dt[q, c]
                    t[q, c] = s
    for q in range(P):
        for co in range(Cc):
            s = 0.0
            for c in range(Cc):
                s += pw[co, c] * t[q, c]
            y[q, co] = s
    stats, dab, dx = np.zeros((Cc, 2)), np.zeros((Cc, 2)), np.zeros((P, Cc))
    for q in range(P):
        for c in range(Cc):
            stats[c, 0] += y[q, c]
            stats[c, 1] += y[q, c] * y[q, c]
            dab[c, 0] += m[q, c] * dz[q, c] * x[q, c]
            dab[c, 1] += m[q, c] * dz[q, c]
            dx[q, c] = a[c] * m[q, c] * dz[q, c]
    fin = []
    for c in range(Cc):
        mean = stats[c, 0] / P
        var = stats[c, 1] / P - mean * mean
        inv = 1.0 / (var + R.EPS) ** 0.5
        g = float(inp['gamma'][c])
        fin.append((g * inv, float(inp['beta'][c]) - mean * g * inv, mean, inv, 0.9 * float(inp['rm0'][c]) + 0.1 * mean,
                    0.9 * float(inp['rv0'][c]) + 0.1 * var * P / (P - 1)))
    eps = {}
    for j in (3, 5):
        nterm, ea = R.EPILOGUES[j]
        out = np.zeros((P, Cc))
        for q in range(P):
            for c in range(Cc):
                s = float(inp['ea'][c]) * y[q, c] + float(inp['eb'][c]) if ea else y[q, c]
                for i, f in enumerate(R.term_forms(j)):
                    taff, trelu = R.FORMS[f]
                    u = float(inp['term'][i][q, c])
                    if taff:
                        u = float(inp['ta'][i][c]) * u + float(inp['tb'][i][c])
                    s += max(u, 0.0) if trelu else u
                out[q, c] = s
        eps[j] = out
    return {'t': t, 'y': y, 'stats': stats, 'fin': np.array(fin).T, 'ep3': eps[3], 'ep5': eps[5], 'dx': dx, 'dab': dab, 'dW': dW}


@pytest.mark.parametrize('K', (3, 5))
def test_the_reference_equals_explicit_loops_in_every_source_form(K):
    op = R.make_op((1, 5, 7), 8, K)
    inp = R.make_inputs(op)
    for form in range(4):
        want = _loops(op, inp, form)
        t, y = R.forward_fp64(op, inp, form)
        dx, dab, dW = R.backward_fp64(op, inp, form)
        got = {'t': t, 'y': y, 'stats': R.stats_fp64(op, y), 'fin': np.array(R.finalize_fp64(op, inp, y)), 'ep3': R.epilogue_fp64(op, inp, y, 3),
               'ep5': R.epilogue_fp64(op, inp, y, 5), 'dx': dx, 'dab': dab, 'dW': dW}
        for k in want:
            assert got[k].shape == want[k].shape and R.rel_err(got[k], want[k]) < 1e-13, (K, R.FORM_NAMES[form], k, R.rel_err(got[k], want[k]))
        for k, v in zip(('dx', 'dab', 'dW'), R.backward_taps(op, inp, form)):
            assert R.rel_err(v, want[k]) < 1e-13, (K, R.FORM_NAMES[form], k)
    assert (R.apply_form(R.x_of(op, inp), inp['a'], inp['b'], 0).numpy() == 0).mean() > 0.25 and (inp['a'] < 0).any()      # masks off, negative a


# ---------------------------------------------------------------------------------------------------------------- the bound

def _ratios(c):
    """how far each wrong result lies from the right one, in units of TOL"""
    op, r = c.op, c.variant[3]
    inp = R.make_inputs(op)
    t, y = R.forward_fp64(op, inp, 0)
    dx, dab, dW = R.backward_taps(op, inp, 0)
    for k, (v, ref) in enumerate(zip((dx, dab, dW), R.backward_fp64(op, inp, 0))):
        assert R.rel_err(v, ref) < 1e-11, (R.case_id(c), k)
    wrong = lambda mistake: R.backward_taps(op, inp, 0, mistake)
    t2, y2 = R.forward_fp64(op, inp, 0, pad_from_neighbour=True)
    t4, y4 = R.forward_fp64(op, inp, 0, zero_last_quad=True)
    g0 = inp['g0'][:, :op.C].astype(np.float64)
    e = [R.rel_err(wrong('taps_not_flipped')[0], dx), min(R.rel_err(t2, t), R.rel_err(y2, y)), R.rel_err(wrong('mask_from_x')[0], dx),
         min(R.rel_err(t4, t), R.rel_err(y4, y)), R.rel_err(wrong('pw_not_transposed')[0], dx),
         R.rel_err(R.stats_fp64(op, y, skip_last_tile_row_in_sumsq=r), R.stats_fp64(op, y)), R.rel_err(wrong('dA_without_x')[1], dab),
         R.rel_err(dx, dx + g0), R.rel_err(wrong('dw_skips_lane_15')[2], dW),
         R.rel_err(R.epilogue_fp64(op, inp, y, 3, drop_relu_of=1), R.epilogue_fp64(op, inp, y, 3)),
         R.rel_err(R.epilogue_fp64(op, inp, y, 4, ea_on_terms=True), R.epilogue_fp64(op, inp, y, 4))]
    return [v / TOL for v in e]


@pytest.mark.parametrize('case', R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_the_bound_separates_eleven_wrong_results(case):
    assert R.FORMS[0] == (True, 1) and R.FORMS[R.term_forms(3)[1]][1] == 1 and R.EPILOGUES[4] == (3, True)
    ratios = _ratios(case)
    print('%s smallest %.0f x TOL: %s' % (R.case_id(case), min(ratios), ' '.join('%.0f' % v for v in ratios)))
    bad = ['%s: %.1f x TOL' % (n, v) for n, v in zip(MISTAKES, ratios) if not v >= 10.0]
    assert not bad, '%s: within 10 x TOL of the right result: %s' % (R.case_id(case), '; '.join(bad))
