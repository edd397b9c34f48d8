"""Host arithmetic of the early-exit operating curve (CPU, no GPU): addk.exit_profile.exit_curve on synthetic per-image records
against a loop that restates the decision rule of dynamic.GatePlan.run.  The records themselves are tests/test_gpu_exit_profile.py."""
import math

import numpy as np
import pytest
import torch

from addk.exit_profile import exit_curve
from addk.metrics import mean_iou

NEX, M, NT, C = 3, 12, 3, 19
MAX_T = (0.25, 0.5, 0.75)
EXIT_MS = (3.0, 5.0, 11.0)


def _records(seed=0):
    r = np.random.default_rng(seed)
    ent = torch.from_numpy(r.random((NEX, M)).astype(np.float32))
    share = torch.from_numpy(r.random((NEX, M, NT)).astype(np.float32))
    cm = torch.from_numpy(r.integers(0, 1000, (NEX, M, C, C)))
    # values exactly ON a threshold: both comparisons are strict, so these images stay
    ent[0, 0], ent[1, 0] = 0.5, 0.125
    share[0, 1, 1], share[1, 1, 1] = 0.5, 0.75
    share[0, 2, 0] = 0.25
    return ent, share, cm


def _loop(ent, share, cm, kind, thr, j=None):
    """the rule, restated: early exits in order, Python-float comparison, the last gate evaluated is the confidence"""
    exit_of, conf = [], []
    for i in range(M):
        chosen = NEX - 1
        for k in range(NEX - 1):
            v = float(ent[k, i]) if kind == 'entropy' else float(share[k, i, j])
            if (v < thr) if kind == 'entropy' else (v > thr):
                chosen = k
                break
        exit_of.append(chosen)
        conf.append(v)
    total = sum(cm[k, i] for i, k in enumerate(exit_of))
    return exit_of, conf, total


ENT_THRESHOLDS = [float('-inf'), 0.125, 0.3, 0.5, 0.5000001, 0.9, float('inf')]


def _check_point(pt, ent, share, cm, kind, thr, j=None):
    exit_of, conf, total = _loop(ent, share, cm, kind, thr, j)
    assert pt['threshold'] == thr
    assert pt['exit_of_image'].dtype == torch.int64 and pt['exit_of_image'].tolist() == exit_of
    assert pt['exit_counts'] == [exit_of.count(k) for k in range(NEX)] and sum(pt['exit_counts']) == M
    assert torch.equal(pt['confusion'], total) and pt['confusion'].dtype == torch.int64
    assert pt['mIoU'] == float(mean_iou(total))
    assert pt['num_earlier_exit'] == 100.0 * sum(1 for k in exit_of if k < NEX - 1) / M
    assert pt['avg_confidence'] == pytest.approx(sum(conf) / M, rel=1e-12, abs=0)
    assert pt['expected_ms'] == pytest.approx(sum(EXIT_MS[k] for k in exit_of) / M, rel=1e-12)
    assert pt['fps'] == pytest.approx(1000.0 / pt['expected_ms'], rel=1e-12)
    return exit_of


def test_entropy_curve_equals_the_restated_rule():
    ent, share, cm = _records()
    pts = exit_curve(ent, share, cm, 'entropy', ENT_THRESHOLDS, MAX_T, EXIT_MS)
    assert len(pts) == len(ENT_THRESHOLDS)
    got = {thr: _check_point(pt, ent, share, cm, 'entropy', thr) for pt, thr in zip(pts, ENT_THRESHOLDS)}
    assert got[float('inf')] == [0] * M and got[float('-inf')] == [NEX - 1] * M          # every image early / none
    assert pts[-1]['num_earlier_exit'] == 100.0 and pts[0]['num_earlier_exit'] == 0.0
    assert pts[0]['expected_ms'] == EXIT_MS[-1] and pts[-1]['expected_ms'] == EXIT_MS[0]
    # image 0 sits exactly on 0.5 at exit 0 and on 0.125 at exit 1: `<` is strict, it stays; one ulp above, it leaves
    assert got[0.5][0] != 0 and got[0.5000001][0] == 0
    assert got[0.125][0] == NEX - 1
    # -inf: nobody leaves, the last gate evaluated is exit NEX-2's
    assert pts[0]['avg_confidence'] == pytest.approx(float(ent[NEX - 2].double().sum()) / M, rel=1e-12)
    assert pts[-1]['avg_confidence'] == pytest.approx(float(ent[0].double().sum()) / M, rel=1e-12)
    assert len(set(got[0.3])) > 1                                                          # a finite threshold splits the images


def test_max_curve_equals_the_restated_rule():
    ent, share, cm = _records(1)
    pts = exit_curve(ent, share, cm, 'max', MAX_T, MAX_T, EXIT_MS)
    got = [_check_point(pt, ent, share, cm, 'max', thr, j) for j, (pt, thr) in enumerate(zip(pts, MAX_T))]
    # image 1: share exactly 0.5 at exit 0 (`>` is strict: stays), 0.75 > 0.5 at exit 1 (leaves there)
    assert got[1][1] == 1
    # image 2: share exactly 0.25 at threshold 0.25: stays at exit 0
    assert got[0][2] != 0
    assert any(len(set(e)) > 1 for e in got)
    # a subset, in any order, and one point per threshold asked for
    sub = exit_curve(ent, share, cm, 'max', [0.75, 0.25], MAX_T)
    assert [p['threshold'] for p in sub] == [0.75, 0.25]
    assert sub[0]['exit_of_image'].tolist() == got[2] and sub[1]['exit_of_image'].tolist() == got[0]
    assert 'expected_ms' not in sub[0] and 'fps' not in sub[0]


def test_value_errors():
    ent, share, cm = _records()
    with pytest.raises(ValueError, match='0.25'):                                          # names the recorded thresholds
        exit_curve(ent, share, cm, 'max', [0.6], MAX_T)
    with pytest.raises(ValueError):
        exit_curve(ent, share, cm, 'max', [0.5], None)                                     # shares without their thresholds
    with pytest.raises(ValueError):
        exit_curve(ent, share, cm, 'edm', [0.5], MAX_T)
    with pytest.raises(ValueError):
        exit_curve(ent, share, cm, 'entropy', [0.5], MAX_T, exit_ms=(1.0, 2.0))           # one latency per exit
    with pytest.raises(ValueError):
        exit_curve(ent, share, cm[:, :5], 'entropy', [0.5], MAX_T)


def test_single_exit_and_empty_records():
    ent, share, cm = _records()
    pt = exit_curve(ent[:1], share[:1], cm[:1], 'entropy', [0.5], MAX_T, (4.0,))[0]       # no early exit: everything is final
    assert pt['exit_of_image'].tolist() == [0] * M and pt['num_earlier_exit'] == 0.0 and math.isnan(pt['avg_confidence'])
    assert torch.equal(pt['confusion'], cm[0].sum(0)) and pt['expected_ms'] == 4.0
    pt = exit_curve(ent[:, :0], share[:, :0], cm[:, :0], 'entropy', [0.5], MAX_T)[0]
    assert pt['exit_counts'] == [0] * NEX and int(pt['confusion'].sum()) == 0


def test_threshold_validation_of_the_class():
    from addk.exit_profile import _check_thresholds
    assert _check_thresholds((0.5, 0.9)) == (0.5, 0.9) and _check_thresholds(()) == ()
    assert len(_check_thresholds([i / 16 for i in range(16)])) == 16
    for bad in ((0.9, 0.5), (0.5, 0.5), [i / 17 for i in range(17)], (0.1, float('nan'))):
        with pytest.raises(ValueError):
            _check_thresholds(bad)
