"""Host-side tests of the boundary-band ("trimap") metric (CPU, no GPU): the numpy reference checks itself (separable form against
brute force, the rounding rule), the dry-built plans of ValidationStep / ExitProfile carry one `boundary_dist` launch and one
`confusion_banded` launch per exit in the right order, the C ABI of the two entry points, and exit_curve's band matrices.
Arithmetic on the GPU is tests/test_gpu_trimap.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import addk
import addk._lib as L
import _trimap_ref as R
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 65, 129)
WIDTHS = (1, 2, 4, 8)


def _add(F=4, ncls=19):
    from addk.modeling.ADD import ADD
    return ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, ncls, make_args(F), ARCH_C2['low_level_layer'])


# ---- the yardstick checks itself -------------------------------------------------------------------------------------------------
def test_separable_reference_equals_brute_force():
    r = np.random.default_rng(5)
    small = r.integers(0, 3, (1, 5, 7)).astype(np.int64)
    assert np.array_equal(R.dist_sep(small, 19, 64), R.dist_brute(small, 19, 64))
    assert R.edges(small, 19).any()
    b = R.case_b()
    got = R.dist_sep(b, 19, 8)
    assert np.array_equal(got, R.dist_brute(b, 19, 8))
    assert (got == R.FAR).any() and (got == 0).any() and ((got > 0) & (got <= 8)).any()


def test_rounding_rule():
    """dist = the smallest k with k*k >= D2"""
    assert R.k_of(np.array([0, 1, 2, 4, 5, 4096, 4097])).tolist() == [0, 1, 2, 2, 3, 64, 65]
    # ... and FAR beyond the radius: one foreign pixel in a uniform field gives discs (Euclidean), not squares or diamonds
    t = R.case_c()[1:]
    d = R.dist_sep(t, 19, 64)
    assert d[0, 43, 74] == 5 and d[0, 45, 75] == 7 and d[0, 40, 134] == 63
    assert d[0, 40, 70] == 0 and d[0, 40, 71] == 0 and d[0, 41, 71] == 1 and d[0, 40, 136] == R.FAR
    assert np.array_equal(d, R.dist_brute(t, 19, 64))


def test_edges_ignore_invalid_neighbours_and_borders():
    t = R.case_e()
    e = R.edges(t, 19)[0]
    v = R.valid(t, 19)[0]
    assert not e[~v].any()                                   # an invalid pixel is never an edge
    assert not e[2, 1:9].any() and not e[1, 3] and not e[3, 3]      # a run of different invalid values inside one class: no edge
    assert e[:, 11].all() and e[:, 12].all()                 # the contour between class 2 and class 5
    assert e[12, 3] and e[11, 3] and e[13, 3] and not e[12, 2] and not e[12, 4] and not e[12, 1] and not e[12, 5]
    assert not R.edges(R.case_d(), 19)[1].any() and R.edges(R.case_d(), 19)[0, 38:].all()


# ---- dry-built plans -------------------------------------------------------------------------------------------------------------
def _struct(c):
    return c.args[0]._obj                                     # the argument struct behind ctypes.byref


def _check_order(g, nex, head):
    """one boundary_dist, and per exit one confusion_banded behind that exit's head launch (matched by the uint8 map) and behind it"""
    order = [c.name for c in g.fwd]
    assert order.count('boundary_dist') == 1 and order.count('confusion_banded') == nex and order.count(head) == nex
    bd = order.index('boundary_dist')
    heads = {}
    for i, c in enumerate(g.fwd):
        if c.name == head:
            a = _struct(c)
            heads[(a.profile if head.endswith('_t') else a).pred_out] = i
    assert len(heads) == nex and None not in heads
    banded = [(i, _struct(c)) for i, c in enumerate(g.fwd) if c.name == 'confusion_banded']
    assert sorted(b.pred for _, b in banded) == sorted(heads)
    for i, b in banded:
        assert heads[b.pred] < i and bd < i
        assert b.dist == _struct(g.fwd[bd]).dist


def test_validation_step_plan(dry):
    from addk.validate import ValidationStep
    m = _add()
    vs = ValidationStep(m, SHAPE, trimap=WIDTHS)
    assert vs.nex == 2
    _check_order(vs.g, vs.nex, 'score_upsample')
    assert tuple(vs.rings.shape) == (2, 4, 19, 19) and vs.rings.dtype == torch.int64
    assert tuple(vs.pred.shape) == (2, 2, 65, 129) and vs.pred.dtype == torch.uint8      # allocated without keep_predictions
    with pytest.raises(addk.AddkError):
        vs.predictions()                                                                 # ... and handed out by its present rule only
    bd = next(c for c in vs.g.fwd if c.name == 'boundary_dist')
    a = _struct(bd)
    assert (a.N, a.OH, a.OW, a.C, a.radius) == (2, 65, 129, 19, 8) and a.dist == vs.dist.data_ptr() and a.target == vs.target.data_ptr()
    for i, c in enumerate(c for c in vs.g.fwd if c.name == 'confusion_banded'):
        b = _struct(c)
        assert (b.N, b.OH, b.OW, b.C, b.nw, b.image_stride) == (2, 65, 129, 19, 4, 0) and list(b.width)[:4] == list(WIDTHS)
        assert b.dist == vs.dist.data_ptr() and b.cm in (vs.rings[0].data_ptr(), vs.rings[1].data_ptr())
        assert b.pred in (vs.pred[0].data_ptr(), vs.pred[1].data_ptr())
    vs.step(torch.randn(SHAPE), torch.zeros((2, 65, 129), dtype=torch.int64))
    assert dry['boundary_dist'] == 1 and dry['confusion_banded'] == 2
    r = vs.result()
    assert r['trimap_widths'] == WIDTHS
    for e in r['exits']:
        assert [b['width'] for b in e['trimap']] == list(WIDTHS)
        assert all(tuple(b['confusion'].shape) == (19, 19) and b['pixels'] == 0 for b in e['trimap'])
    vs.rings.fill_(3)
    vs.reset()
    assert int(vs.rings.abs().sum()) == 0
    # without the keyword the plan names neither launch and the result has no band entries
    plain = ValidationStep(m, SHAPE)
    names = [c.name for c in plain.g.fwd]
    assert 'boundary_dist' not in names and 'confusion_banded' not in names and plain.pred is None
    assert 'trimap_widths' not in plain.result() and 'trimap' not in plain.result()['exits'][0]


def test_exit_profile_plan(dry):
    from addk.exit_profile import ExitProfile
    m = _add()
    prof = ExitProfile(m, SHAPE, trimap=WIDTHS)
    _check_order(prof.g, prof.nex, 'profile_upsample')
    order = [c.name for c in prof.g.fwd]
    assert order.count('trimap_zero') == 1 and order.index('trimap_zero') < order.index('confusion_banded')
    assert tuple(prof.rings.shape) == (2, 2, 4, 19, 19)
    for c in prof.g.fwd:
        if c.name == 'confusion_banded':
            assert _struct(c).image_stride == 4 * 19 * 19
    prof.step(torch.randn(SHAPE), torch.zeros((2, 65, 129), dtype=torch.int64))
    prof.step(count=1)
    rec = prof.records()
    assert tuple(rec['band_confusion'].shape) == (2, 3, 4, 19, 19) and rec['trimap_widths'] == WIDTHS
    assert [b['width'] for b in rec['static'][1]['trimap']] == list(WIDTHS)
    pt = prof.curve('entropy', [0.5])[0]
    assert [b['width'] for b in pt['trimap']] == list(WIDTHS)
    tempered = ExitProfile(m, SHAPE, trimap=WIDTHS, temperature=1.5)
    _check_order(tempered.g, tempered.nex, 'profile_upsample_t')
    plain = ExitProfile(m, SHAPE)
    names = [c.name for c in plain.g.fwd]
    assert 'boundary_dist' not in names and 'confusion_banded' not in names and 'trimap_zero' not in names
    plain.step()
    assert 'band_confusion' not in plain.records() and 'trimap' not in plain.curve('entropy', [0.5])[0]


def test_exit_without_the_fused_head_is_refused(dry):
    """7 classes: addk_score_upsample_supported == 0, the stand-alone path keeps an int64 map"""
    from addk.validate import ValidationStep
    with pytest.raises(ValueError):
        ValidationStep(_add(ncls=7), (1, 3, 33, 65), trimap=WIDTHS)
    ValidationStep(_add(ncls=7), (1, 3, 33, 65))                # and is built as before without the keyword


@pytest.mark.parametrize('bad', [(), (0, 1), (2, 2), (4, 2), (1, 65), (-1,), (1, 2, 3, 4, 5, 6, 7, 8, 9), (1.5, 2), 8])
def test_width_list_errors(dry, bad):
    from addk.exit_profile import ExitProfile
    from addk.trimap import check_widths
    from addk.validate import ValidationStep
    with pytest.raises(ValueError):
        check_widths(bad)
    m = _add()
    with pytest.raises(ValueError):
        ValidationStep(m, SHAPE, trimap=bad)
    with pytest.raises(ValueError):
        ExitProfile(m, SHAPE, trimap=bad)


def test_width_list_accepts_its_limits():
    from addk.trimap import check_widths
    assert check_widths([1, 64]) == (1, 64) and check_widths(range(1, 9)) == tuple(range(1, 9)) and check_widths(np.array([3])) == (3,)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cname,cls', [('addk_boundary_dist_args', L.BoundaryDistArgs), ('addk_confusion_banded_args', L.ConfusionBandedArgs)])
def test_trimap_args_layout_matches_header(tmp_path, cname, cls):
    fields = [f for f, _ in cls._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){',
             'printf("size %%zu\\n", sizeof(%s));' % cname,
             'printf("consts %d %d %d\\n", ADDK_TRIMAP_MAX_RADIUS, ADDK_TRIMAP_MAX_WIDTHS, ADDK_TRIMAP_FAR);']
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f in fields] + ['return 0;}']
    c = tmp_path / 'abi.c'
    c.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    got = dict(l.split(None, 1) for l in out)
    assert int(got['size']) == ctypes.sizeof(cls)
    assert got['consts'].split() == [str(L.TRIMAP_MAX_RADIUS), str(L.TRIMAP_MAX_WIDTHS), str(L.TRIMAP_FAR)] == ['64', '8', '255']
    for f in fields:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_supported_predicates_at_their_limits():
    lib = addk.load()
    bd, cb = lib.addk_boundary_dist_supported, lib.addk_confusion_banded_supported
    assert bd(2, 65, 129, 19, 1) == 1 and bd(2, 65, 129, 19, 64) == 1 and bd(1, 1, 1, 1, 1) == 1 and bd(1, 5, 7, 32, 64) == 1
    assert bd(2, 65, 129, 19, 0) == 0 and bd(2, 65, 129, 19, 65) == 0 and bd(2, 65, 129, 0, 8) == 0 and bd(2, 65, 129, 33, 8) == 0
    assert bd(0, 65, 129, 19, 8) == 0 and bd(2, 0, 129, 19, 8) == 0 and bd(2, 65, -1, 19, 8) == 0
    assert bd(1, 32768, 65535, 19, 8) == 1 and bd(1, 32768, 65536, 19, 8) == 0 and bd(2, 32768, 32768, 19, 8) == 0      # N*OH*OW < 2^31
    assert cb(2, 65, 129, 19, 1) == 1 and cb(2, 65, 129, 19, 8) == 1 and cb(2, 65, 129, 32, 8) == 1
    assert cb(2, 65, 129, 19, 0) == 0 and cb(2, 65, 129, 19, 9) == 0 and cb(2, 65, 129, 33, 4) == 0 and cb(2, 65, 129, 0, 4) == 0
    assert cb(0, 65, 129, 19, 4) == 0 and cb(1, 32768, 65536, 19, 4) == 0
    assert lib.addk_boundary_dist_ws_bytes(2, 65, 129) >= 2 * 65 * 129
    # an error code and no launch for what the predicates refuse and for null pointers (no device is touched)
    assert lib.addk_boundary_dist(ctypes.byref(L.BoundaryDistArgs()), None) == -1
    assert lib.addk_confusion_banded(ctypes.byref(L.ConfusionBandedArgs()), None) == -1
    assert lib.addk_boundary_dist(None, None) == -1 and lib.addk_confusion_banded(None, None) == -1


# ---- exit_curve ------------------------------------------------------------------------------------------------------------------
def test_exit_curve_sums_the_chosen_exits_band_matrices():
    from addk.exit_profile import exit_curve
    from addk.metrics import mean_iou
    nex, M, nw, C = 3, 6, 3, 19
    r = np.random.default_rng(1)
    ent = torch.from_numpy(r.random((nex, M)).astype(np.float32))
    share = torch.zeros((nex, M, 0))
    cm = torch.from_numpy(r.integers(0, 1000, (nex, M, C, C)))
    band = torch.from_numpy(r.integers(0, 100, (nex, M, nw, C, C))).cumsum(2)
    pts = exit_curve(ent, share, cm, 'entropy', [float('inf'), float('-inf'), 0.5], band_confusion=band, widths=(1, 3, 9))
    for pt, k in zip(pts[:2], (0, nex - 1)):                 # all leave at exit 0 / none leaves
        assert pt['exit_counts'][k] == M
        for j, b in enumerate(pt['trimap']):
            want = band[k, :, j].sum(0)
            assert b['width'] == (1, 3, 9)[j] and torch.equal(b['confusion'], want) and b['confusion'].dtype == torch.int64
            assert b['mIoU'] == float(mean_iou(want)) and b['pixels'] == int(want.sum())
    mixed = pts[2]
    want = sum(band[int(k), i] for i, k in enumerate(mixed['exit_of_image']))
    assert 0 < mixed['exit_counts'][0] < M
    assert all(torch.equal(b['confusion'], want[j]) for j, b in enumerate(mixed['trimap']))
    assert 'trimap' not in exit_curve(ent, share, cm, 'entropy', [0.5])[0]
    with pytest.raises(ValueError):
        exit_curve(ent, share, cm, 'entropy', [0.5], band_confusion=band, widths=(1, 3))
