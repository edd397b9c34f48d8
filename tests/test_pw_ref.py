"""The fp64 reference of the kernels of csrc/pw.hip (tests/_pw_ref.py) and the case table of tests/test_gpu_pw_fp64.py checked without a GPU: the
reference against the definition written with torch in float64 (F.interpolate -> affine -> ReLU -> F.conv2d, autograd for g, dA, dB); the bound of the GPU
test against fourteen subtly wrong results a kernel could compute and against the right result computed in float32; and the case table and the mixed
batches against the library's own choice."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import addk
from addk import _lib as L
import _pw_ref as R

FLOOR = 10 * R.TOL


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(R.FAST_ALL)
    yield lb
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


# ---------------------------------------------------------------------------------------------------------------- the reference

_t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64))


def _torch_forward(op, inp, forms, bias):
    zs, raw0 = [], None
    for i, c in enumerate(op.Cs):
        aff, relu = R.FORMS[forms[i]]
        h, w = op.maps[i] or (op.H, op.W)
        z = _t(inp['x'][i][:, :c]).view(op.N, h, w, c).permute(0, 3, 1, 2)
        if op.maps[i]:
            z = F.interpolate(z, size=(op.H, op.W), mode='bilinear', align_corners=False)
            raw0 = z.permute(0, 2, 3, 1).reshape(-1, c).numpy() if i == 0 else raw0
        if aff:
            z = _t(inp['a'][i]).view(1, c, 1, 1) * z + _t(inp['b'][i]).view(1, c, 1, 1)
        zs.append(F.relu(z) if relu else z)
    ctot = sum(op.Cs)
    wt = _t(inp['w'][:, R.W_CHOFF:R.W_CHOFF + ctot]).view(op.Cout, ctot, 1, 1)
    y = F.conv2d(torch.cat(zs, 1), wt, _t(inp['bias']) if bias else None)
    return y.permute(0, 2, 3, 1).reshape(-1, op.Cout).numpy(), raw0


def _torch_dgrad(op, inp, form):
    aff, relu = R.FORMS[form]
    c, K = op.Cs[0], op.Cout
    x = _t(inp['x'][0][:, :c]).view(op.N, op.H, op.W, c).permute(0, 3, 1, 2).requires_grad_()
    a = (_t(inp['a'][0]) if aff else torch.ones(c, dtype=torch.float64)).requires_grad_()
    b = (_t(inp['b'][0]) if aff else torch.zeros(c, dtype=torch.float64)).requires_grad_()
    z = a.view(1, c, 1, 1) * x + b.view(1, c, 1, 1)
    y = F.conv2d(F.relu(z) if relu else z, _t(inp['w'][:K, R.W_CHOFF:R.W_CHOFF + c]).view(K, c, 1, 1))
    (y * _t(inp['dy'][:, :K]).view(op.N, op.H, op.W, K).permute(0, 3, 1, 2)).sum().backward()
    return x.grad.permute(0, 2, 3, 1).reshape(-1, c).numpy(), torch.stack([a.grad, b.grad], 1).numpy()


DEFINITION = ['pw_fwd_36to12_s', 'pw_fwd_rs_36to24_s', 'pw_fwd_rs_80to80_l', 'pwk_rs1_64+32to24_s', 'pwk_64+8+24to16_l', 'pwk_rs_64+8+24to12_l', 'pwk_rs_200to40_s',
              'pw_dgrad_36into12_s', 'pw_dgrad_68into40_l', 'k1s_21into132', 'k1s_19into256_tiny', 'pw_fwd_36to24_tiny', 'stem0_s', 'stem0_l']


@pytest.mark.parametrize('name', DEFINITION)
def test_reference_equals_the_definition(name):
    """to 1e-12 of max-abs: y, the statistics and rs_y of every forward launch of the case (both maps of an RS case), g and (dA, dB) of every form of a
    data gradient, first touch and accumulating"""
    case = R.BY_NAME[name]
    op, e = case.op, R.rel_err
    if op.kind == 'stem0':
        inp = R.make_inputs(op)
        x = _t(inp['x'][0][:, :3]).view(op.N, op.H, op.W, 3).permute(0, 3, 1, 2)
        y = F.conv2d(x, _t(inp['w'][:, :27]).view(64, 3, 3, 3).permute(0, 3, 1, 2), stride=2, padding=1)
        assert y.shape[2:] == R.out_hw(op)
        assert e(R.reference(R.default_launch(op))['y'], y.permute(0, 2, 3, 1).reshape(-1, 64).numpy()) <= 1e-12
        return
    for label, la, _ in R.case_launches(case):
        inp, ref = R.make_inputs(la.op), R.reference(la)
        if op.kind == 'dgrad':
            g, dab = _torch_dgrad(la.op, inp, la.forms[0])
            g = g * la.dy_scale + (inp['g0'][:, :op.Cs[0]].astype(np.float64) if la.accumulate else 0.0)
            assert e(ref['g'], g) <= 1e-12, (label, e(ref['g'], g))
            assert ref['dab'] is None or e(ref['dab'], dab * la.dy_scale) <= 1e-12, label
        else:
            y, raw = _torch_forward(la.op, inp, la.forms, la.bias)
            assert e(ref['y'], y) <= 1e-12, (label, e(ref['y'], y))
            assert ref['stats'] is None or e(ref['stats'], np.stack([y.sum(0), (y * y).sum(0)], 1)) <= 1e-12, label
            assert (ref['rs_y'] is None) == (not la.rs_y) and (ref['rs_y'] is None or e(ref['rs_y'], raw) <= 1e-12), label


def test_scaled_gradient_is_exact():
    op = R.BY_NAME['pw_dgrad_36into12_s'].op
    one, tiny = R.reference(R.dgrad_launch(op, 0)), R.reference(R.dgrad_launch(op, 0, dy_scale=R.TINY_DY))
    assert np.array_equal(tiny['g'] * 2.0 ** 30, one['g']) and np.array_equal(tiny['dab'] * 2.0 ** 30, one['dab'])
    g, dab = R.dgrad(op, R.make_inputs(op), 0, dy_scale=R.TINY_DY)
    assert np.array_equal(g, tiny['g']) and np.array_equal(dab, tiny['dab'])


# ---------------------------------------------------------------------------------------------------------------- the bound

def test_bound_separates_right_from_subtly_wrong(lib):
    """Each of fourteen mistakes a kernel of pw.hip could make moves the reference by more than 10 x TOL in the GPU test's own error measure (the largest
    over the buffers the launch writes), in every case it applies to and at the case's own shape and data, so a kernel that makes it cannot pass.
    Measured, the smallest over the cases as multiples of TOL:
     1 last live K quad dropped (K = 36 / 68) 1.0e+04      2 w_choff off by 4 3.5e+04 (forward), 5.2e+04 (gradient)
     3 gradient weight not transposed 5.4e+04              4 ReLU mask from x, not a x + b 2.3e+04
     5 dA without its x factor 1.4e+04                     6 accumulate overwrites 1.5e+04
     7 bias missing from the statistics 1.6e+04            8 partial last tile missing from the statistics 2.6e+02
     9 RS with align_corners = True 5.3e+03               10 RS affine + ReLU before the interpolation 5.9e+03 (ReLU forms: an affine alone commutes)
    11 RS reads image 0 for every image 1.8e+04           12 second pwk source at weight offset 0 1.9e+04
    13 stem0 with pad 0 6.8e+04                           14 k1s second pixel of a trip missing from (dA, dB) 2.5e+04"""
    worst = {}

    def hold(what, name, err):
        worst[what] = min(worst.get(what, err), err)
        assert err >= FLOOR, '%s: %s moves the reference by %.2e only (< %.0e)' % (name, what, err, FLOOR)

    e = R.rel_err
    for case in R.CASES:
        op, inp, name = case.op, R.make_inputs(case.op), case.name
        if op.kind == 'stem0':
            hold('13 stem0 pad 0', name, e(R.stem0(op, inp, pad=0), R.stem0(op, inp)))
            continue
        if op.kind == 'fwd':
            n = len(op.Cs)
            for f in range(4):
                forms = [(f + i) % 4 for i in range(n)]
                y, raw = R.forward(op, inp, forms, bias=True)
                if case.cfg[0] == R.PW and op.Cs[0] in (36, 68):
                    hold('1 last K quad dropped', name, e(R.forward(op, inp, forms, True, drop_last_quad=True)[0], y))
                hold('2 w_choff + 4 (forward)', name, e(R.forward(op, inp, forms, True, w_choff_shift=4)[0], y))
                hold('7 bias missing from the statistics', name, e(R.stats(y, without=inp['bias']), R.stats(y)))
                if len(y) % 16:
                    hold('8 partial tile missing from the statistics', name, e(R.stats(y, drop_partial_tile=True), R.stats(y)))
                if n > 1:
                    hold('12 second source at weight offset 0', name, e(R.forward(op, inp, forms, True, second_source_offset0=True)[0], y))
                if any(op.maps):
                    both = lambda got: max(e(got[0], y), e(got[1], raw) if raw is not None else 0.0)
                    hold('9 align_corners = True', name, both(R.forward(op, inp, forms, True, align_corners=True)))
                    hold('11 image 0 for every image', name, both(R.forward(op, inp, forms, True, image0=True)))
                    rs = [i for i in range(n) if op.maps[i]][0]
                    if R.FORMS[forms[rs]][1]:
                        hold('10 affine + ReLU before the interpolation', name, e(R.forward(op, inp, forms, True, affine_first=True)[0], y))
            continue
        nw = 4 * R.config(lib, L, R.default_launch(op))[1]
        for f, (aff, relu) in enumerate(R.FORMS):
            for acc in (0, 1):
                g, dab = R.dgrad(op, inp, f, acc)
                both = lambda got: max(e(got[0], g), e(got[1], dab))
                hold('2 w_choff + 4 (gradient)', name, both(R.dgrad(op, inp, f, acc, w_choff_shift=4)))
                if name in ('pw_dgrad_40into40_l', 'pw_dgrad_80into80_s'):
                    hold('3 weight not transposed', name, both(R.dgrad(op, inp, f, acc, no_transpose=True)))
                if aff and relu:
                    hold('4 mask from x', name, both(R.dgrad(op, inp, f, acc, mask_from_x=True)))
                hold('5 dA without x', name, both(R.dgrad(op, inp, f, acc, da_without_x=True)))
                if acc:
                    hold('6 accumulate overwrites', name, both(R.dgrad(op, inp, f, acc, overwrite=True)))
                if case.cfg[0] == R.K1S and nw < R.pixels(op):
                    hold('14 second pixel missing', name, both(R.dgrad(op, inp, f, acc, second_pixel_stride=nw)))
    assert len(worst) == 15, sorted(worst)
    print('\n'.join('%s %.1e' % (k, v / R.TOL) for k, v in sorted(worst.items(), key=lambda kv: int(kv[0].split()[0]))))


def test_float32_arithmetic_stays_under_the_bound():
    """The right answer in float32 numpy (fp32 matmul, numpy's pairwise sums: another summation order than the kernels') is within TOL of the reference for
    every launch of every case, so the bound is not tight for correct fp32 arithmetic at these reduction lengths (K <= 224).  Worst measured: 3.5e-06,
    a sixth of TOL."""
    worst = 0.0
    for case in R.CASES:
        for label, la, _ in R.case_launches(case):
            op, inp, ref = la.op, R.make_inputs(la.op), R.reference(la)
            f32 = np.float32
            if op.kind == 'dgrad':
                g, dab = R.dgrad(op, inp, la.forms[0], la.accumulate, la.dy_scale, dt=f32)
                errs = [R.rel_err(g, ref['g']), R.rel_err(dab, ref['dab']) if la.stats else 0.0]
            else:
                y, raw = (R.stem0(op, inp, dt=f32), None) if op.kind == 'stem0' else R.forward(op, inp, la.forms, la.bias, dt=f32)
                assert y.dtype == f32
                errs = [R.rel_err(y, ref['y']), R.rel_err(R.stats(y), ref['stats']) if la.stats else 0.0, R.rel_err(raw, ref['rs_y']) if la.rs_y else 0.0]
            assert max(errs) <= R.TOL, (case.name, label, errs)
            worst = max(worst, max(errs))
    print('worst float32 error %.2e' % worst)


# ---------------------------------------------------------------------------------------------------------------- the case table

def test_every_launch_of_every_case_takes_the_variant_it_names(lib):
    """kind, template values and batch key, in every form, bias form, map and slab / rs_y presence the GPU test launches; outside the tiny map and k1s
    (one workgroup per slab row) fewer workgroups than slab rows, so the zero-fill of the rows no workgroup owns is part of every check"""
    bad = []
    for case in R.CASES:
        for label, la, ldy in R.case_launches(case):
            cfg, gx, gy, key = R.bits.config(lib, L, (None, 'dgrad' if la.op.kind == 'dgrad' else 'fwd'), R.launch_args(L, la, R.host_ptr(la.op), ldy))
            if (cfg, key) != (case.cfg, case.key):
                bad.append((case.name, label, cfg, key))
            rows = lib.addk_conv_rows(R.pixels(la.op), la.op.Cout if la.op.kind != 'dgrad' else la.op.Cs[0])
            assert gx < rows or case.cfg[0] == R.K1S or R.pixels(la.op) == 5, (case.name, gx, rows)
    assert not bad, bad[:5]
    assert len({c.name for c in R.CASES}) == len(R.CASES)


def test_cases_reach_exactly_the_46_variants():
    """the `want` set of tests/test_pw_dispatch.py, one case per variant among the first 46"""
    seen = [('dgrad' if c.op.kind == 'dgrad' else 'fwd',) + tuple(c.cfg) for c in R.CASES]
    want = {('fwd', R.PW, ct, kg, rs, r32) for ct, kg in ((1, 3), (2, 3), (3, 3), (1, 5), (2, 5)) for rs in (0, 1) for r32 in (0, 1)}
    want |= {('dgrad', R.PW, ct, kg, 0, r32) for ct, kg in ((1, 3), (2, 3), (3, 3), (1, 5), (2, 5)) for r32 in (0, 1)}
    want |= {('fwd', R.PWK, ct, rs, r32, 0) for ct in (1, 2, 3) for rs in (0, 1) for r32 in (0, 1)}
    want |= {('fwd', R.STEM0, 4, r32, 0, 0) for r32 in (0, 1)} | {('dgrad', R.K1S, kmax, 0, 0, 0) for kmax in (20, 32)}
    assert len(want) == 46 == R.N_VARIANTS
    assert set(seen) == want and len(set(seen[:46])) == 46, (sorted(want - set(seen)), sorted(set(seen) - want))
    for c in R.CASES:
        if c.cfg[0] == R.PW:
            assert c.key == R.pw_key(int(c.op.kind == 'dgrad'), *c.cfg[1:]) and c.key >= 0
        else:
            assert c.key == -1


def test_red32_flips_at_4096_pixels(lib):
    for kind, slot in (('fwd', 4), ('dgrad', 4)):
        got = []
        for grid in ((1, 63, 65), (1, 64, 64)):          # 4095 and 4096 pixels
            op = R.Op(kind, grid[0], grid[1], grid[2], (40,), 40, (None,), 1)
            got.append(R.config(lib, L, R.default_launch(op))[0])
        assert [g[0] for g in got] == [R.PW, R.PW] and [g[slot] for g in got] == [0, 1], got
    got = [R.config(lib, L, R.default_launch(R.Op('fwd', 1, h, w, (128,), 16, (None,), 1)))[0] for h, w in ((63, 65), (64, 64))]
    assert [g[0] for g in got] == [R.PWK, R.PWK] and [g[3] for g in got] == [0, 1], got
    got = [R.config(lib, L, R.default_launch(R.Op('stem0', 1, h, w, (3,), 64, (None,), 1)))[0] for h, w in ((125, 129), (127, 127))]      # 63 x 65, 64 x 64
    assert [g[0] for g in got] == [R.STEM0, R.STEM0] and [g[2] for g in got] == [0, 1], got


@pytest.mark.parametrize('v', R.BATCH_VARIANTS, ids=[R.batch_id(v) for v in R.BATCH_VARIANTS])
def test_mixed_batch_has_one_key_and_unequal_grids(lib, v):
    """every member gets the variant's key on its own, the batch carries it with the largest grid, and the members differ in (gx, gy) (in gx alone where CT
    leaves the output width no choice), in reduction length, form, bias / accumulate and slab presence; RS members in map and rs_y too"""
    mode, ct, kg, rs, r32 = v
    ms = R.batch_members(v)
    cfgs = [R.config(lib, L, la) for la in ms]
    key = R.pw_key(*v)
    assert all(c[0] == [R.PW, ct, kg, rs, r32] and c[3] == key for c in cfgs), cfgs
    grids = [(c[1], c[2]) for c in cfgs]
    assert len({g[0] for g in grids}) == 3, grids
    assert len({g[1] for g in grids}) == (3 if ct == 3 or (ct, kg) == (2, 5) else 1), grids
    meta, _ = R.batch_meta(lib, L, ms)
    assert list(meta[:4]) == [key, 3, max(g[0] for g in grids), max(g[1] for g in grids)]
    assert len({la.op.Cout if mode else la.op.Cs[0] for la in ms}) >= 2 and len({la.forms for la in ms}) == 3
    assert [la.stats for la in ms] == [True, True, False]
    assert len({(la.op.N, la.op.H, la.op.W) for la in ms}) == 3 and all((R.pixels(la.op) >= 4096) == bool(r32) for la in ms)
    if mode == 0:
        assert [la.bias for la in ms] == [False, True, False]
        assert not rs or (len({la.op.maps for la in ms}) == 3 and [la.rs_y for la in ms] == [True, False, True] and all(la.op.N > 1 for la in ms[::2]))
    else:
        assert [la.accumulate for la in ms] == [0, 1, 1]
