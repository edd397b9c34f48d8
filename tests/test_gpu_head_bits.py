"""GPU test of the logits heads (csrc/loss_up.hip, score_up.hip, label_up.hip; first the fused loss head, the validation scoring head and the exit gate) after they were put
on one pixel loader and one up-sampling walk: every buffer a launch writes, bit for bit against the hashes recorded from the parent
commit's library (tests/golden/head_parent_bits.json, written by tests/tools/make_head_bits.py).  The refactor names shared pieces;
every floating-point operation stays the same operation in the same order, so no difference at all is allowed.  The heads that came
later (mining, distillation, label map, gate with labels, exit profile, multi-view labels) are pinned the same way, recorded from the
parent of the commit that split csrc/loss.hip by head family."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location('make_head_bits', os.path.join(HERE, 'tools', 'make_head_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

RUNS = [(case, ld, kernel) for case in bits.CASES for ld in bits.LDS for kernel in bits.KERNELS]
LAUNCHES = {'score': 4, 'gate': 4, 'ce': 2, 'ce_ohem': 2, 'ce_kd': 4, 'label': 2, 'gate_label': 4, 'profile': 6, 'views': 2}


@functools.lru_cache(maxsize=None)
def _golden():
    """The fixture's records by case name; it must list exactly the tool's cases, each with its input hash and every run."""
    with open(os.path.join(HERE, 'golden', 'head_parent_bits.json')) as f:
        rec = json.load(f)['cases']
    assert [(r['name'], tuple(r['lo']), tuple(r['hi']), r['seed']) for r in rec] == [tuple(c) for c in bits.CASES], \
        'fixture and tool list different cases'
    for r in rec:
        assert len(r['inputs']) == 64 and len(r['inputs2']) == 64, r['name']
        assert sorted(r['runs']) == sorted('ld%d/%s' % (ld, k) for ld in bits.LDS for k in bits.KERNELS), r['name']
        for key, launches in r['runs'].items():
            assert len(launches) == LAUNCHES[key.split('/')[1]], (r['name'], key)
            assert all(len(h) == 64 for bufs in launches.values() for h in bufs.values()), (r['name'], key)
    return {r['name']: r for r in rec}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """One case's seeded inputs, made once and shared by its runs (never modified: run_case copies them to the device): the arrays of
    make_inputs and make_inputs2 in one dict, and the two hashes."""
    case = next(c for c in bits.CASES if c[0] == name)
    (arrs, hin), (arrs2, hin2) = bits.make_inputs(case), bits.make_inputs2(case)
    return {**arrs, **arrs2}, hin, hin2


@pytest.mark.parametrize('case,ld,kernel', RUNS, ids=['%s-ld%d-%s' % (c[0], ld, k) for c, ld, k in RUNS])
def test_head_outputs_are_bit_identical_to_the_parent(case, ld, kernel):
    """sha256 of every buffer each launch of the kernel writes (outputs, workspace, ticket word) equals what the parent commit's
    library wrote on the same inputs."""
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    rec = _golden()[case[0]]
    arrs, hin, hin2 = _inputs(case[0])
    assert (hin, hin2) == (rec['inputs'], rec['inputs2']), '%s: the seeded INPUTS differ from the fixture (numpy RandomState stream or dtype handling changed)' % case[0]
    got = bits.run_case(L, case, ld, kernel, arrs)
    want = rec['runs']['ld%d/%s' % (ld, kernel)]
    assert sorted(got) == sorted(want)
    diff = ['%s:%s' % (ln, b) for ln in sorted(want) for b in sorted(set(want[ln]) | set(got[ln])) if got[ln].get(b) != want[ln].get(b)]
    assert not diff, '%s ld %d %s: %s differ from the parent commit bit for bit' % (case[0], ld, kernel, ', '.join(diff))
