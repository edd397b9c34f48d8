"""Host-side choice of the kernels of csrc/pw.hip (pw_choose_*, pw_key / pw_key_decode and the one launch table), no GPU: the library is
called with aligned placeholder pointers (nothing is dereferenced before a launch).  Every case of the bit-for-bit fixture
(tests/tools/make_pw_bits.py) gets the kernel kind and template values recorded from the parent commit, the batch key a lone launch
reports is the one a batch of it carries in meta[0], and between them the cases reach every variant of the launch table."""
import ctypes as C
import importlib.util
import os

import pytest

import addk
from addk import _lib as L

_spec = importlib.util.spec_from_file_location('make_pw_bits', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'make_pw_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope='module')
def lib():
    lb = addk.load()
    fast = lb.addk_get_fast_paths()
    lb.addk_set_fast_paths(31)
    yield lb
    lb.addk_set_fast_paths(fast)


def _args(case):
    names = list(bits.make_inputs(case)[0]) + ['y', 'slab', 'rs_y']
    return bits.conv_args(L, case, {k: 0x10000000 * (i + 1) for i, k in enumerate(names)})      # 16-byte aligned, never dereferenced


def test_every_case_has_a_pin():
    assert [c[0] for c in bits.CASES] == list(bits.PINS)


@pytest.mark.parametrize('case', bits.CASES, ids=[c[0] for c in bits.CASES])
def test_bit_fixture_cases_get_their_kind_template_values_and_batch_key(lib, case):
    """addk_conv_*_config's kind and template values and the batch key are the parent's; a batch of the launch (one and two members)
    carries that key in meta[0] with the lone launch's grid, i.e. the key survives pw_key -> prepare -> pw_key_decode's input."""
    cfg0, key0 = bits.PINS[case[0]]
    ar = _args(case)
    cfg, gx, gy, key = bits.config(lib, L, case, ar)
    assert (cfg, key) == (cfg0, key0), case[0]
    t = 'dgrad' if case[1] == 'dgrad' else 'fwd'
    prep = getattr(lib, 'addk_conv_%s_batch_prepare' % t)
    for n in (1, 2):
        arr = (type(ar) * n)(*([ar] * n))
        meta = (C.c_int64 * 8)()
        size = prep(arr, n, None, 0, meta)
        if cfg[0] != bits.PW:
            assert key == -1 and size < 0, (case[0], 'only the register-stationary kernel is batched')
            continue
        assert size > 0 and list(meta[:4]) == [key, n, gx, gy], (case[0], list(meta[:4]), lib.addk_last_error())
        # the key's fields are the template values: (mode, CT, KG, RS, red32)
        assert [key >> 12, (key >> 8) & 15, (key >> 4) & 15, (key >> 1) & 1, key & 1] == [int(t == 'dgrad')] + cfg[1:5], case[0]


def test_cases_reach_every_variant_of_the_launch_tables(lib):
    seen = {(c[1],) + tuple(bits.PINS[c[0]][0]) for c in bits.CASES}
    want = {('fwd', bits.PW, ct, kg, rs, r32) for ct, kg in ((1, 3), (2, 3), (3, 3), (1, 5), (2, 5)) for rs in (0, 1) for r32 in (0, 1)}
    want |= {('dgrad', bits.PW, ct, kg, 0, r32) for ct, kg in ((1, 3), (2, 3), (3, 3), (1, 5), (2, 5)) for r32 in (0, 1)}
    want |= {('fwd', bits.PWK, ct, rs, r32, 0) for ct in (1, 2, 3) for rs in (0, 1) for r32 in (0, 1)}
    want |= {('fwd', bits.STEM0, 4, r32, 0, 0) for r32 in (0, 1)} | {('dgrad', bits.K1S, kmax, 0, 0, 0) for kmax in (20, 32)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
