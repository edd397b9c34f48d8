"""The fp64 reference of the convolution's forward and data gradient (tests/_conv_ref.py) and the case list of tests/test_gpu_conv_fp64.py checked
without a GPU: the reference against a direct tap-by-tap evaluation of the definition in include/addk.h; the bound of the GPU test against the subtly
wrong results a kernel could compute; and the case list against the library's own choice: every launch of CASES takes the variant it names, and the
variants of CASES are exactly the halo-patch kernels that are instantiated."""
import itertools

import numpy as np
import pytest

import addk
from addk import _lib as L
import _conv_ref as R
from test_conv_variants import LOOKUPS, Variant

ALL = [R.case_of(e) for e in R.CASES]
FLOOR = 50 * R.TOL


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(R.FAST_ALL)
    lb.addk_set_split_min_channels(0)
    for name, domain in LOOKUPS.items():
        getattr(lb, name).restype, getattr(lb, name).argtypes = Variant, [R.C.c_int] * len(domain)
    yield lb
    lb.addk_set_split_min_channels(-1)
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


# ---------------------------------------------------------------------------------------------------------------- the reference

# two sources, the second without an affine; stride 2 and dilation 2 among them; the weight slice starts at channel 8 of cin_total = C + 12
TINY = [('k3_s2_d2', (2, 9, 11, (5, 3), 4, 3, 2, 2)), ('k5_d2', (1, 10, 9, (4, 6), 3, 5, 1, 2)), ('k3_s2', (1, 9, 12, (3, 2), 5, 3, 2, 1)), ('k1', (2, 5, 7, (6, 2), 4, 1, 1, 1))]
TINY_FORMS = (0, 3), (2, 1)


def _padded(op, inp, i, form):
    aff, relu = R.FORMS[form]
    z = inp['x'][i].astype(np.float64).reshape(op.N, op.H, op.W, -1)
    if aff:
        z = inp['a'][i].astype(np.float64) * z + inp['b'][i].astype(np.float64)
    if relu:
        z = np.maximum(z, 0.0)
    zp = np.zeros((op.N, op.H + 2 * op.pad, op.W + 2 * op.pad, op.Cs[i]))
    zp[:, op.pad:op.pad + op.H, op.pad:op.pad + op.W] = z
    return zp


def _taps(op):
    s, d = op.stride, op.dil
    for ky in range(op.k):
        for kx in range(op.k):
            yield (ky * op.k + kx) * op.cin_total, slice(ky * d, ky * d + (op.OH - 1) * s + 1, s), slice(kx * d, kx * d + (op.OW - 1) * s + 1, s)


def _direct_forward(op, inp, forms, bias_form):
    """y[n,oy,ox,co] = bias + sum_{tap,ci} w[co][tap*cin_total + w_choff + ci] * z[n, oy*s - pad + ky*d, ox*s - pad + kx*d, ci], tap by tap"""
    w = inp['w'].astype(np.float64)
    y = np.zeros((op.N, op.OH, op.OW, op.Cout))
    for i in range(len(op.Cs)):
        zp = _padded(op, inp, i, forms[i])
        for t0, ys, xs in _taps(op):
            y += np.einsum('nyxc,oc->nyxo', zp[:, ys, xs], w[:, t0 + R.choff(op, i): t0 + R.choff(op, i) + op.Cs[i]])
    if bias_form == 1:
        y += inp['bias'].astype(np.float64)
    if bias_form == 2:
        y += inp['bias_n'].astype(np.float64)[:, None, None, :]
    return y.reshape(-1, op.Cout)


def _direct_dgrad(op, inp, i, form):
    """every (output pixel, tap) scatters dy * w into the padded input pixel it read; then mask and scale"""
    aff, relu = R.FORMS[form]
    w, Ci = inp['w'].astype(np.float64), op.Cs[i]
    dy = inp['dy'].astype(np.float64).reshape(op.N, op.OH, op.OW, op.Cout)
    dzp = np.zeros((op.N, op.H + 2 * op.pad, op.W + 2 * op.pad, Ci))
    for t0, ys, xs in _taps(op):
        dzp[:, ys, xs] += np.einsum('nyxo,oc->nyxc', dy, w[:, t0 + R.choff(op, i): t0 + R.choff(op, i) + Ci])
    dz = dzp[:, op.pad:op.pad + op.H, op.pad:op.pad + op.W].reshape(-1, Ci)
    x = inp['x'][i].astype(np.float64)
    a = inp['a'][i].astype(np.float64) if aff else 1.0
    b = inp['b'][i].astype(np.float64) if aff else 0.0
    m = dz * (a * x + b > 0) if relu else dz
    return a * m, np.stack([(m * x).sum(0), m.sum(0)], 1)


@pytest.mark.parametrize('forms', TINY_FORMS, ids=['ab_relu+plain', 'relu+ab'])
@pytest.mark.parametrize('name,shape', TINY, ids=[t[0] for t in TINY])
def test_reference_equals_the_definition(name, shape, forms):
    """conv2d / conv_transpose2d in fp64 against the tap-by-tap sums over explicitly zero-padded maps, to fp64 rounding: forward in the three bias forms,
    the statistics, and every source's gradient with its own w_choff, first touch and accumulating, in the wider rows the GPU test uses."""
    op = R.make_op(*shape, seed=31)
    assert (op.w_choff, op.cin_total, op.ldw, op.ldy) == (8, sum(op.Cs) + 12, op.k * op.k * (sum(op.Cs) + 12) + 4, op.Cout + 12)
    inp = R.make_inputs(op)
    for bf in range(3):
        got, want = R.ref_forward(op, forms, bf), _direct_forward(op, inp, forms, bf)
        assert R.rel_err(got, want) <= 1e-13, (name, bf, R.rel_err(got, want))
        assert R.rel_err(R.stats_fp64(got), np.stack([want.sum(0), (want ** 2).sum(0)], 1)) <= 1e-13
    for i in range(len(op.Cs)):
        (g, dab), (wg, wdab) = R.ref_dgrad(op, i, forms[i]), _direct_dgrad(op, inp, i, forms[i])
        assert R.rel_err(g, wg) <= 1e-13 and R.rel_err(dab, wdab) <= 1e-13, (name, i, R.rel_err(g, wg), R.rel_err(dab, wdab))
        g0 = inp['g0'][i]
        for acc in (0, 1):
            full = R.widen(g, g0, R.ldg(op, i), acc)
            assert np.array_equal(full[:, op.Cs[i]:], g0.astype(np.float64)[:, op.Cs[i]:])
            assert R.rel_err(full[:, :op.Cs[i]], wg + (g0[:, :op.Cs[i]] if acc else 0.0)) <= 1e-13


def test_scaled_gradient_is_exact():
    op = R.make_op(*TINY[0][1], seed=31)
    g, dab = R.ref_dgrad(op, 0, 0)
    gs, dabs = R.ref_dgrad(op, 0, 0, 2.0 ** -30)
    assert np.array_equal(gs * 2.0 ** 30, g) and np.array_equal(dabs * 2.0 ** 30, dab)


MISTAKE_CASES = [c for c in ALL if (c.lookup, c.args[:-1]) in {('c3b_variant_tr3', (3, 32, 0)), ('c3b_variant_tr3', (3, 32, 1)), ('c3n_variant', (5, 0)), ('c3n_variant', (5, 1)),
                                                               ('c3b_variant_row', (4, 1, 0, 128, 0)), ('c3b_variant_row', (4, 1, 0, 128, 1)), ('c3b_variant_s2f', (4, 64)),
                                                               ('c3b_variant_s2d', ()), ('c3b_variant_row', (3, 3, 1, 128, 0)), ('c3b_variant_row', (3, 3, 1, 128, 1))}
                 and c.args[-1] == 2]


@pytest.mark.parametrize('case', MISTAKE_CASES, ids=[R.case_id(c) for c in MISTAKE_CASES])
def test_bound_separates_right_from_subtly_wrong(case):
    """Each mistake a kernel could make moves the reference by at least 50 x TOL in the GPU test's own error measure, at a case's own shape and data
    and in every form it applies to, so a kernel that makes one cannot pass.  Forward: a tap dropped at the last output column; the affine applied to the
    padding; w_choff + 1; one tap's sign flipped (what a wrong checkerboard factor in the weight pack does); bias_n of the wrong image.  Data gradient:
    the ReLU mask ignored; accumulate ignored; w_choff + 1; the taps not mirrored; one tap's sign flipped.  Measured over these cases, as multiples of
    TOL, the smallest: dropped tap 7.0e+03, affine on the padding 5.0e+03, w_choff + 1 5.4e+04 (forward) and 6.2e+04 (gradient), flipped tap 2.4e+04
    in both directions, bias_n of the wrong image 3.0e+04, ReLU mask ignored 3.7e+04, accumulate ignored 3.0e+04, taps not mirrored 6.1e+04."""
    op, inp = R.case_op(case), R.make_inputs(R.case_op(case))
    worst = {}

    def hold(what, e):
        worst[what] = min(worst.get(what, e), e)
        assert e >= FLOOR, '%s: %s moves the reference by %.2e only (< %.0e)' % (R.case_id(case), what, e, FLOOR)

    if case.direction == 'fwd':
        for form, (aff, relu) in enumerate(R.FORMS):
            ref = R.ref_forward(op, [form])
            hold('dropped tap', R.rel_err(R.forward_fp64(op, inp, [form], drop_tap=True), ref))
            if aff and op.k > 1:
                hold('affine on the padding', R.rel_err(R.forward_fp64(op, inp, [form], affine_on_padding=True), ref))
            if form == 0:
                hold('w_choff + 1', R.rel_err(R.forward_fp64(op, inp, [form], w_choff=op.w_choff + 1), ref))
                hold('flipped tap', R.rel_err(R.forward_fp64(op, inp, [form], flip_tap=True), ref))
                if op.N > 1:
                    hold('bias_n of the wrong image', R.rel_err(R.forward_fp64(op, inp, [form], 2, bias_n_shift=1), R.ref_forward(op, [form], 2)))
    else:
        dz, C0 = R.ref_dz(op, 0), op.Cs[0]
        hold('w_choff + 1', R.rel_err(R.dz_fp64(op, inp, 0, w_choff=op.w_choff + 1), dz))
        hold('flipped tap', R.rel_err(R.dz_fp64(op, inp, 0, flip_tap=True), dz))
        if op.k > 1:
            hold('taps not mirrored', R.rel_err(R.dz_fp64(op, inp, 0, no_mirror=True), dz))
        for form, (aff, relu) in enumerate(R.FORMS):
            g, dab = R.ref_dgrad(op, 0, form)
            if relu:
                gm, dabm = R.dgrad_fp64(op, inp, 0, form, dz, ignore_relu_mask=True)
                hold('ReLU mask ignored', min(R.rel_err(gm, g), R.rel_err(dabm, dab)))
            hold('accumulate ignored', R.rel_err(R.widen(g, inp['g0'][0], R.ldg(op, 0), 0)[:, :C0], R.widen(g, inp['g0'][0], R.ldg(op, 0), 1)[:, :C0]))
    print(R.case_id(case), ' '.join('%s %.1e' % (k, v / R.TOL) for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------------------------- the case list

def _chosen(lib, case, form=0, bias_form=0):
    L.check(lib.addk_set_conv_precision(R.MODES[case.mode]), 'set_conv_precision')
    op = R.case_op(case)
    return R.variant_of(R.config(L, lib, R.host_args(L, op, case.direction, form, bias_form)), op, case.direction, case.mode)


def test_every_case_takes_the_variant_it_names(lib):
    """with a large enough wpack, mask 31, the case's mode and split minimum 0, in every source / destination form and bias form of the GPU test"""
    bad = []
    for c in ALL:
        for form, bf in itertools.product(range(4), range(3) if c.direction == 'fwd' else (0,)):
            got = _chosen(lib, c, form, bf)
            if got != (c.lookup, c.args):
                bad.append((R.case_id(c), R.FORM_NAMES[form], R.BIAS_FORMS[bf], got))
    assert not bad, '%d launches take another kernel than their case names, the first: %s' % (len(bad), bad[:5])


def test_cases_reach_exactly_the_instantiated_variants(lib):
    offered = {(name, args) for name, domain in LOOKUPS.items() for args in itertools.product(*domain) if getattr(lib, name)(*args).fn}
    named = {(c.lookup, c.args) for c in ALL}
    assert offered - named == set(), 'instantiated without a numeric test: %s' % sorted(offered - named)
    assert named - offered == set(), 'cases of kernels that do not exist: %s' % sorted(named - offered)
    assert len(offered) == 110
    assert len(set(ALL)) == len(ALL) and len({R.case_id(c) for c in ALL}) == len(ALL)


def test_dilation_parities(lib):
    """Every variant that takes a dilated 3x3 / 5x5 has a launch at an odd and at an even dilation (d = 1 and 2; 3 and 6 on the `bigd` rows), and
    both launches take that one variant; 1x1 and stride-2 variants have their only dilation."""
    by = {}
    for c in ALL:
        by.setdefault((c.lookup, c.args), []).append(c)
    for (lookup, args), cs in by.items():
        dils = sorted(c.dil for c in cs)
        if cs[0].k == 1 or cs[0].stride == 2:
            assert dils == [1], (lookup, args, dils)
            continue
        bigd = lookup == 'c3b_variant_row' and args[2] == 1
        assert dils == ([3, 6] if bigd else [1, 2]), (lookup, args, dils)
        assert {_chosen(lib, c) for c in cs} == {(lookup, args)}
        assert len({(c.k, c.stride, c.direction, c.mode) for c in cs}) == 1


def test_ruled_out_constraints_are_the_ones_the_shape_misses(lib):
    """a case says which of the four shape constraints its variant's gates rule out: exactly those its shape does not have.  Only the fp32 kernel's
    128-channel block misses one: its gate asks for a multiple of 128 channels."""
    for c in ALL:
        unmet = ''.join(sorted(k for k, ok in R.constraints(c.lookup, c.args, R.case_op(c), c.direction).items() if not ok))
        assert unmet == c.ruled_out, (R.case_id(c), unmet, c.ruled_out)
    assert {(c.lookup, c.args[:2], c.ruled_out) for c in ALL if c.ruled_out} == {('c3_variant_fp32', (8, 3), 'C')}
    assert all(c.Cout % 4 == 0 and all(ci % 4 == 0 for ci in c.Cs) for c in ALL)
    cost = [c.N * R.case_op(c).OH * R.case_op(c).OW * c.Cs[0] * c.Cout * c.k * c.k for c in ALL]
    assert max(cost) <= 1.6e9, max(cost)


def test_derived_launches_take_their_variants(lib):
    """the launches tests/test_gpu_conv_fp64.py derives from the cases: three sources in the forward, three destinations, tail_x3 on either side of 192 channels"""
    assert len(R.LAYOUTS) == 11 and all(f is not None and d is not None for f, d in R.LAYOUTS)
    for f, d in R.LAYOUTS:
        L.check(lib.addk_set_conv_precision(R.MODES[f.mode]), 'set_conv_precision')
        op = R.case_op(R.three_sources(f))
        for forms, bf in (((0, 3, 2), 0), ((1, 2, 0), 2)):
            ar = R.fwd_args(L, op, list(forms), bf, R.host_ptr(op))
            assert R.variant_of(R.config(L, lib, ar), op, 'fwd', f.mode) == (f.lookup, f.args), R.case_id(f)
        op = R.case_op(R.three_destinations(d))
        for i, form in enumerate((0, 3, 2)):
            assert R.variant_of(R.config(L, lib, R.host_args(L, op, 'dgrad', form, i=i)), op, 'dgrad', d.mode, i) == (d.lookup, d.args), R.case_id(d)
    sides = {(c.lookup, c.direction, R.out_channels(c) >= 192) for c in R.TAIL}
    for lk in ('c3b_variant_row', 'c3b_variant_tr3', 'c3b_variant_tr5'):
        assert {(lk, di, hi) for di in ('fwd', 'dgrad') for hi in (False, True)} <= sides
    assert {('c3b_variant_s2f', 'fwd', False), ('c3b_variant_s2f', 'fwd', True), ('c3b_variant_s2d', 'dgrad', False), ('c3n_variant', 'fwd', False),
            ('c3n_variant', 'dgrad', False)} <= sides
    L.check(lib.addk_set_conv_precision(3), 'set_conv_precision')
    for c in R.TAIL:
        op = R.case_op(c)
        assert R.variant_planes(c.lookup, c.args) == (2 if R.out_channels(c) >= 192 else 3), R.case_id(c)
        assert R.variant_of(R.config(L, lib, R.host_args(L, op, c.direction)), op, c.direction, 'tail_x3') == (c.lookup, c.args), R.case_id(c)
