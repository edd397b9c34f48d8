"""GPU test of the BatchNorm launches that exist as a lone and as a table-driven `_batch` entry point over ONE item type (slab_reduce,
bn_bwd_coeffs, bn_eval_affine, bn_bwd_apply): every output bit for bit against the hashes recorded from the parent commit's library
(tests/golden/bn_parent_bits.json, written by tests/tools/make_bn_bits.py), through the table entry and through the lone entry.  Giving
the lone launches the tables' items moved arguments, never arithmetic, so no difference at all is allowed."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_bn_bits', os.path.join(HERE, 'tools', 'make_bn_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

ALL = [(op, c) for op, cases in bits.CASES.items() for c in cases]
IDS = [bits.case_id(op, c) for op, c in ALL]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    return L, L.load()


def _golden():
    """The fixture's records by case id: exactly the tool's cases, each with its input hash and every output's hash."""
    with open(os.path.join(HERE, 'golden', 'bn_parent_bits.json')) as f:
        rec = json.load(f)['cases']
    assert [r['id'] for r in rec] == IDS, 'fixture and tool list different cases'
    for r in rec:
        assert all(len(r[k]) == 64 for k in ('inputs',) + bits.OUTPUTS[r['id'].split('-')[0]]), r['id']
    return {r['id']: r for r in rec}


def _compare(op, case, got, how):
    rec = _golden()[bits.case_id(op, case)]
    assert bits.inputs(op, case)[1] == rec['inputs'], '%s: the seeded INPUTS differ from the fixture' % rec['id']
    diff = [o for o in bits.OUTPUTS[op] if got[o] != rec[o]]
    assert not diff, '%s, %s: %s differ from the parent commit bit for bit' % (rec['id'], how, ', '.join(diff))


@pytest.mark.parametrize('op,case', ALL, ids=IDS)
def test_bn_table_launch_is_bit_identical_to_the_parent(lib, op, case):
    _compare(op, case, bits.run_table(*lib, op, [case])[0], 'a table of one')


@pytest.mark.parametrize('op,case', ALL, ids=IDS)
def test_bn_lone_launch_is_bit_identical_to_the_parent(lib, op, case):
    _compare(op, case, bits.run_lone(*lib, op, case), 'the lone launch')


@pytest.mark.parametrize('op', list(bits.GROUPS))
def test_bn_cases_in_one_table_are_bit_identical_to_the_parent(lib, op):
    """items of different C / P in one table: the blocks beyond a short item return"""
    for case, got in zip(bits.GROUPS[op], bits.run_table(*lib, op, bits.GROUPS[op])):
        _compare(op, case, got, 'one table of %d' % len(bits.GROUPS[op]))
