"""GPU test of the dense weight gradient after csrc/wgrad.hip was split into a shared header (wgrad.h) and one file per kernel
family (wgrad_pix.hip, wgrad_h3.hip, wgrad_hk.hip, wgrad_rs.hip): every output bit for bit against the hashes recorded from the
parent commit's library (tests/golden/wgrad_parent_bits.json, written by tests/tools/make_wgrad_bits.py).  The split moves code
between files and names shared pieces; no lane computes anything else, so no difference at all is allowed."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location('make_wgrad_bits', os.path.join(HERE, 'tools', 'make_wgrad_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

RUNS = [(case, mode) for case in bits.CASES for mode in bits.MODES if mode in case[5]]
_INPUTS = {}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    lb = L.load()
    prec, fast = lb.addk_get_conv_precision(), lb.addk_get_fast_paths()
    yield L
    lb.addk_set_fast_paths(fast)
    lb.addk_set_conv_precision(prec)


def _golden():
    """The fixture's records by case name; it must list exactly the tool's cases, each with its input hash and, per mode, the launch
    key CASES gives and all five output hashes."""
    with open(os.path.join(HERE, 'golden', 'wgrad_parent_bits.json')) as f:
        rec = json.load(f)['cases']
    assert [(r['name'], r['shape'], r['fast'], r['padded'], r['seed']) for r in rec] == [(c[0], list(c[1]), c[2], c[3], c[4]) for c in bits.CASES], \
        'fixture and tool list different cases'
    for r, c in zip(rec, bits.CASES):
        assert len(r['inputs']) == 64 and {m: tuple(v['key']) for m, v in r['modes'].items()} == c[5], r['name']
        assert all(len(v[o]) == 64 for v in r['modes'].values() for o in bits.OUTPUTS), r['name']
    return {r['name']: r for r in rec}


def _inputs(case):
    """One case's seeded inputs, made once and shared by its modes (never modified: run_case copies them to the device)."""
    if case[0] not in _INPUTS:
        _INPUTS.clear()
        _INPUTS[case[0]] = bits.make_inputs(case)
    return _INPUTS[case[0]]


@pytest.mark.parametrize('case,mode', RUNS, ids=['%s-%s' % (c[0], m) for c, m in RUNS])
def test_wgrad_outputs_are_bit_identical_to_the_parent(lib, case, mode):
    """sha256 of dw (first touch and accumulate), the workspace and both dw of a two-conv batch equals what the parent commit's
    library wrote on the same inputs, under the launch key the fixture was recorded on."""
    rec = _golden()[case[0]]
    arrs, hin = _inputs(case)
    assert hin == rec['inputs'], '%s: the seeded INPUTS differ from the fixture (numpy RandomState stream or dtype handling changed)' % case[0]
    got, key = bits.run_case(lib, case, mode, arrs, rec['modes'][mode]['key'])      # asserts the launch key before it launches
    diff = [o for o in bits.OUTPUTS if got[o] != rec['modes'][mode][o]]
    assert not diff, '%s [%s]: %s differ from the parent commit bit for bit' % (case[0], mode, ', '.join(diff))
