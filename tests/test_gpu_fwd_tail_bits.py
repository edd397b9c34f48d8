"""GPU test of the statistics tail of the forward kernels (csrc/sepf.hip, csrc/pw.hip) after the per-channel totals over the 16 pixel lanes
moved from an all-reduce butterfly of LDS permutes to a reduce-scatter in registers (csrc/common.h, rs16): everything each launch writes —
y, the stored depthwise output t, the whole statistics / (dA, dB) slab including the rows no workgroup owns — bit for bit against the hashes
recorded from the parent commit's library (tests/golden/fwd_tail_parent_bits.json, written by tests/tools/make_fwd_tail_bits.py).  The
reduce-scatter adds the same partial sums at every level of the same tree (tests/test_stats_tail_tree.py), so no difference is allowed."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FAST_ALL = 31
HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location('make_fwd_tail_bits', os.path.join(HERE, 'tools', 'make_fwd_tail_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    L.load().addk_set_fast_paths(FAST_ALL)
    yield L
    L.load().addk_set_fast_paths(FAST_ALL)


@pytest.fixture(scope='module')
def golden():
    """The fixture's records by family and case name; it lists exactly the tool's cases, every launch with all of its buffers, and between
    them all twelve sepf variants."""
    with open(os.path.join(HERE, 'golden', 'fwd_tail_parent_bits.json')) as f:
        doc = json.load(f)
    assert [(r['name'], r['shape'], r['seed'], r['extra_rows']) for r in doc['sepf']] == [(c[0], list(c[1:6]), c[6], c[7]) for c in bits.SEPF_CASES]
    assert [(r['name'], r['seed']) for r in doc['pw']] == [(c[0], c[3]) for c in bits.PW_CASES]
    for r in doc['sepf']:
        assert sorted(r['launches']) == ['batch0', 'batch1', 'lone'], r['name']
        assert all(sorted(h) == sorted(bits.SEPF_OUTPUTS) and all(len(v) == 64 for v in h.values()) for h in r['launches'].values()), r['name']
    assert len({tuple(r['variant']) for r in doc['sepf']}) == 12
    for r in doc['pw']:
        assert sorted(r['launches']) == (['batch0', 'batch1', 'lone'] if r['cfg'][0] == bits.pwb.PW else ['lone']), r['name']
        assert all({'y', 'slab'} <= set(h) and all(len(v) == 64 for v in h.values()) for h in r['launches'].values()), r['name']
    return {'sepf': {r['name']: r for r in doc['sepf']}, 'pw': {r['name']: r for r in doc['pw']}}


def _differences(got, rec):
    return ['%s.%s' % (ln, buf) for ln in sorted(rec) for buf in sorted(rec[ln]) if got.get(ln, {}).get(buf) != rec[ln][buf]]


@pytest.mark.parametrize('case', bits.SEPF_CASES, ids=[c[0] for c in bits.SEPF_CASES])
def test_sepf_writes_the_parents_bits(lib, golden, case):
    """addk_sep_fwd (training form) lone and as a two-member batch: y, t and the whole slab equal the parent's, NaN prefill included."""
    rec = golden['sepf'][case[0]]
    arrs, hin = bits.sepf_inputs(case)
    assert hin == rec['inputs'], '%s: the seeded INPUTS differ from the fixture (numpy RandomState stream or dtype handling changed)' % case[0]
    got, variant = bits.run_sepf(lib, case, arrs)
    assert variant == rec['variant'] == list(case[8]), '%s runs variant %s, the fixture was recorded on %s' % (case[0], variant, rec['variant'])
    diff = _differences(got, rec['launches'])
    assert not diff, '%s: %s differ from the parent commit bit for bit' % (case[0], ', '.join(diff))


@pytest.mark.parametrize('case', bits.PW_CASES, ids=[c[0] for c in bits.PW_CASES])
def test_pw_kernels_write_the_parents_bits(lib, golden, case):
    """pw_kernel (forward statistics, data gradient (dA, dB); fp64 and fp32 lane sums; lone and batched), pwk_kernel and stem0_kernel."""
    rec = golden['pw'][case[0]]
    arrs, hin = bits.pwb.make_inputs(case)
    assert hin == rec['inputs'], '%s: the seeded INPUTS differ from the fixture' % case[0]
    got, (cfg, key) = bits.pwb.run_case(lib, case, arrs, bits.PW_PINS[case[0]])
    assert (cfg, key) == (rec['cfg'], rec['key']), '%s: launch %s / key %d, the fixture was recorded on %s / %d' % (case[0], cfg, key, rec['cfg'], rec['key'])
    diff = _differences(got, rec['launches'])
    assert not diff, '%s: %s differ from the parent commit bit for bit' % (case[0], ', '.join(diff))
