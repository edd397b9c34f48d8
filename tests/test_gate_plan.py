"""Host-logic tests (CPU, no GPU) of dynamic inference gated by exit entropy / top-probability share: the segments of the
launch plan, the untouched 'edm' plan, the error paths and the C layout of the gate launch's argument struct.  Launches are
stubbed as in tests/test_plan_dryrun.py; the arithmetic is checked in tests/test_gpu_gate.py."""
import collections
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import addk  # noqa: F401
from addk import _lib as L
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _add(F=20, arch=ARCH_C2):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), arch['low_level_layer']).eval()


def _names(plan, i0, i1):
    return [c.name for c in plan.g.fwd[i0:i1]]


def _check_segments(plan, gates):
    n = len(plan.g.fwd)
    assert len(plan.trunk_end) == len(plan.heads) == len(plan.head_rng) == gates and plan.final is not None
    pos = 0
    for k in range(gates):
        t, (cut, end) = plan.trunk_end[k], plan.head_rng[k]
        assert pos < t < cut < end < n                                   # trunk < head < resize < rest
        trunk, head, resize = _names(plan, pos, t), _names(plan, t, cut), _names(plan, cut, end)
        assert 'gate_upsample' not in trunk and 'resize_nchw' not in trunk
        assert head.count('gate_upsample') == 1 and head[-1] == 'gate_upsample' and 'resize_nchw' not in head
        assert any(nm.startswith('conv_fwd') for nm in head)             # the head itself (ASPP, decoder) sits before its gate
        assert resize == ['resize_nchw']
        assert plan.heads[k].gate_fused and tuple(plan.heads[k].y.shape) == (1, 19, 65, 129)
        pos = end
    rest = _names(plan, pos, n)
    assert rest.count('resize_nchw') == 1 and rest[-1] == 'resize_nchw' and 'gate_upsample' not in rest
    assert not any(c.name == 'edm_head' for c in plan.g.fwd)
    assert sum(1 for c in plan.g.fwd if c.name == 'gate_upsample') == gates
    assert tuple(plan.final.y.shape) == (1, 19, 65, 129)


@pytest.mark.parametrize('kind', ['entropy', 'max'])
def test_gate_plan_segments_c2(dry, kind):
    m = _add(20, ARCH_C2)
    x = torch.randn(1, 3, 65, 129)
    plan = m._gate_plan(x, kind)
    _check_segments(plan, 1)
    assert m._gate_plan(x, kind) is plan                                 # cached per (kind, shape, precision)
    assert m._gate_plan(x, 'max' if kind == 'entropy' else 'entropy') is not plan


def test_gate_plan_segments_c3(dry):
    m = _add(20, ARCH_C3)
    plan = m._gate_plan(torch.randn(1, 3, 65, 129), 'entropy')
    _check_segments(plan, 2)


def test_gate_head_is_forward_head(dry, monkeypatch):
    """Exit k's launches are those of forward(): the gated plan holds forward()'s launches (compared un-batched) and one gate."""
    monkeypatch.setenv('ADDK_LEVEL_BATCH', '0')
    m = _add(20, ARCH_C2)
    x = torch.randn(1, 3, 65, 129)
    plan = m._gate_plan(x, 'entropy')
    with torch.no_grad():
        m(x)
    fwd = next(p for k, p in m._plans().items() if not (isinstance(k, tuple) and k and k[0] == 'dyn'))
    full = collections.Counter(c.name for c in fwd.g.fwd)
    gated = collections.Counter(c.name for c in plan.g.fwd)
    gated.pop('gate_upsample')
    assert gated == full                                                 # the gated plan = forward()'s launches + one gate


def test_public_path_replays_segments(dry):
    m = _add(20, ARCH_C2)
    x = torch.randn(1, 3, 65, 129)
    y, ex, sec, val = m.dynamic_inference(x, float('inf'), confidence='entropy')
    assert ex == 1 and isinstance(val, float) and isinstance(sec, float) and tuple(y.shape) == (1, 19, 65, 129)
    assert dry['gate_upsample'] == 1 and dry['resize_nchw'] == 1
    y, ex, sec, val = m.dynamic_inference(x, float('-inf'), confidence='entropy')
    assert ex == 0 and isinstance(val, float) and tuple(y.shape) == (1, 19, 65, 129)
    assert dry['gate_upsample'] == 2 and dry['resize_nchw'] == 2         # the exit's resize did not run for the image that stays


def test_stand_alone_kernels_when_fused_form_is_off(dry, monkeypatch):
    monkeypatch.setenv('ADDK_FUSE_GATE', '0')
    m = _add(20, ARCH_C2)
    x = torch.randn(1, 3, 65, 129)
    for kind, tail in (('entropy', 'entropy_sum'), ('max', 'gate_count_torch')):
        plan = m._gate_plan(x, kind)
        t, (cut, end) = plan.trunk_end[0], plan.head_rng[0]
        head = _names(plan, t, cut)
        assert cut == end and head[-2:] == ['resize_nchw', tail] and not plan.heads[0].gate_fused
        assert not any(c.name == 'gate_upsample' for c in plan.g.fwd)


def test_edm_plan_is_untouched(dry):
    from addk.dynamic import DynamicPlan
    from addk.modeling.ADD import EDM
    x = torch.randn(1, 3, 65, 129)
    m, edm = _add(20, ARCH_C2), EDM().eval()
    old = DynamicPlan(m, edm, x)                                         # the old call
    m._gate_plan(x, 'entropy')                                           # gate plans in the cache change nothing for 'edm'
    m.dynamic_inference(x, 1.0, confidence='edm', edm=edm)
    new = m._dynamic_plan(x, edm)
    assert type(new) is DynamicPlan
    assert [c.name for c in new.g.fwd] == [c.name for c in old.g.fwd]
    assert (new.trunk_end, new.head_rng) == (old.trunk_end, old.head_rng)
    names = collections.Counter(c.name for c in new.g.fwd)
    assert names['gate_upsample'] == 0 and names['resize_nchw'] == 2
    assert names['edm_head'] == 1 or names['gap_fwd'] == 1


def test_errors(dry):
    m = _add(4, ARCH_C2)
    for kind in ('entropy', 'max', 'edm'):
        with pytest.raises(RuntimeError):
            from addk.modeling.ADD import EDM
            m.dynamic_inference(torch.randn(2, 3, 65, 129), 0.5, confidence=kind, edm=EDM().eval())
    with pytest.raises(ValueError):
        m.dynamic_inference(torch.randn(1, 3, 65, 129), 0.5, confidence='pool')


def test_gate_struct_layout_matches_header():
    cname, cls = 'addk_gate_upsample_args', L.GateUpsampleArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f, _ in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['return 0;}']
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'abi.c')
        open(c, 'w').write('\n'.join(lines))
        exe = os.path.join(d, 'abi')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, f
    assert [f for f, _ in cls._fields_] == ['logits', 'ld', 'N', 'H', 'W', 'C', 'OH', 'OW', 'max_thr', 'out', 'out_host', 'ws']
    for sym in ('addk_gate_upsample_supported', 'addk_gate_upsample_ws_bytes', 'addk_gate_upsample'):
        assert sym in L.EXPORTED_SYMBOLS
    lib = addk.load()
    assert lib.addk_gate_upsample_supported(1, 8, 16, 64, 128, 19) == 1
    assert lib.addk_gate_upsample_supported(1, 8, 16, 64, 128, 21) == 0
    assert lib.addk_gate_upsample_supported(1, 0, 16, 64, 128, 19) == 0
    assert lib.addk_gate_upsample_supported(1, 8, 16, 65536 * 32 + 1, 1, 19) == 0
    assert lib.addk_gate_upsample_ws_bytes(2, 41, 67) == 16 + 8 * 2 * 2 * 2
