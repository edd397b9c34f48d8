"""Host-logic tests of the exit profile (CPU, no GPU): addk.exit_profile.ExitProfile is built with the kernel launches stubbed out
(the `dry` pattern of tests/test_validate_plan.py) and the launch list is inspected — one profile launch per exit, no scoring, gate
or resize launch and no full-resolution logits anywhere — plus the C ABI of the profile entry points.  Arithmetic is
tests/test_gpu_exit_profile.py."""
import collections
import ctypes
import os
import re
import subprocess

import pytest
import torch

import addk
import addk._lib as L
import addk.plan as P
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 65, 129)
NAMES = ('addk_profile_upsample', 'addk_profile_upsample_supported', 'addk_profile_upsample_ws_bytes')


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer'])


def _has_full_resolution_buffer(g, shape):
    """a [N,C,OH,OW] tensor, or its NHWC form (dense or with the padded pixel stride), among what the plan owns"""
    N, Cc, OH, OW = shape
    sizes = {N * OH * OW * Cc, N * OH * OW * ((Cc + 3) // 4 * 4)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    return any(b.n in sizes for b in g._bufs) or any(tuple(t.shape) == tuple(shape) or t.numel() in sizes for t in owned)


@pytest.mark.parametrize('arch,nex', [(ARCH_C2, 2), (ARCH_C3, 3)], ids=['c2', 'c3'])
def test_one_profile_launch_per_exit_and_no_full_resolution_logits(dry, arch, nex):
    from addk.exit_profile import ExitProfile
    m = _add(4, arch)
    prof = ExitProfile(m, SHAPE, max_thresholds=(0.5, 0.9, 0.99))
    order = [c.name for c in prof.g.fwd]
    names = collections.Counter(order)
    assert names['profile_upsample'] == nex == prof.nex == len(prof.outs)
    assert names['resize_nchw'] == names['score_upsample'] == names['gate_upsample'] == 0
    assert names['profile_zero'] == 1 and order.index('profile_zero') < order.index('profile_upsample')
    assert names['bn_eval_affine_batch'] == 1 and names['bn_finalize'] == 0   # inference form
    assert not prof.g.bwd
    assert all(o.y is None and o.head == 'profile' and o.binding is not None and tuple(o.shape) == (2, 19, 65, 129) for o in prof.outs)
    assert not _has_full_resolution_buffer(prof.g, (2, 19, 65, 129))
    launches = [c for c in prof.g.fwd if c.name == 'profile_upsample']
    assert all(c.tag == 'decoder' for c in launches)                          # tagged like the scoring launch
    assert m.training                                                         # the model's mode is not touched
    assert tuple(prof.ent.shape) == (nex, 2) and tuple(prof.share.shape) == (nex, 2, 3) and tuple(prof.cm.shape) == (nex, 2, 19, 19)
    # two full batches and a short one; the stubbed launches leave zeros, the bookkeeping is what is checked
    x, t = torch.randn(SHAPE), torch.zeros((2, 65, 129), dtype=torch.int64)
    prof.step(x, t)
    prof.step(x, t)
    prof.step(x, t, count=1)
    assert dry['profile_upsample'] == 3 * nex and dry['profile_zero'] == 3 and prof.batches == 3
    r = prof.records()
    assert tuple(r['entropy'].shape) == (nex, 5) and tuple(r['share'].shape) == (nex, 5, 3)
    assert tuple(r['confusion'].shape) == (nex, 5, 19, 19) and r['confusion'].dtype == torch.int64
    assert len(r['static']) == nex and tuple(r['static'][0]['confusion'].shape) == (19, 19)
    pts = prof.curve('max')
    assert [p['threshold'] for p in pts] == [0.5, 0.9, 0.99] and all(sum(p['exit_counts']) == 5 for p in pts)
    assert len(prof.curve('entropy', [0.1, 0.2])) == 2
    with pytest.raises(ValueError):
        prof.curve('entropy')
    with pytest.raises(ValueError):
        prof.step(x, t, count=3)
    prof.reset()
    assert prof.batches == 0 and tuple(prof.records()['entropy'].shape) == (nex, 0)


def test_thresholds_live_in_a_device_buffer(dry):
    from addk.exit_profile import ExitProfile
    prof = ExitProfile(_add(4), SHAPE, max_thresholds=(float('-inf'), 0.5, float('inf')))
    assert prof.thr.dtype == torch.float32 and prof.thr.tolist() == [-1.0, 0.5, 2.0]       # GatePlan.run's clamp
    g0 = prof.g
    prof.set_max_thresholds((0.25, 0.75, 0.875))
    assert prof.g is g0 and prof.thr.tolist() == [0.25, 0.75, 0.875] and prof.max_thresholds == (0.25, 0.75, 0.875)
    a = [c for c in g0.fwd if c.name == 'profile_upsample'][0].args[0]._obj
    assert a.thr == prof.thr.data_ptr() and a.nthr == 3
    with pytest.raises(ValueError):
        prof.set_max_thresholds((0.25, 0.75))                                 # another length is another plan
    for bad in ((0.9, 0.5), (0.5, 0.5), tuple(i / 17 for i in range(17))):
        with pytest.raises(ValueError):
            ExitProfile(_add(4), SHAPE, max_thresholds=bad)
    none = ExitProfile(_add(4), SHAPE, max_thresholds=())                     # the entropy gate alone
    a = [c for c in none.g.fwd if c.name == 'profile_upsample'][0].args[0]._obj
    assert a.nthr == 0 and not a.thr and not a.share_out


def test_plain_eval_plan_keeps_its_resizes(dry):
    """The flag is per plan: a model(x) call before and after an ExitProfile was built on the model still materialises its logits."""
    from addk.exit_profile import ExitProfile
    m = _add(4).eval()
    with torch.no_grad():
        before = m(torch.randn(SHAPE))
    assert all(tuple(o.shape) == (2, 19, 65, 129) for o in before)
    ExitProfile(m, SHAPE)
    with torch.no_grad():
        outs = m(torch.randn(SHAPE))
    assert all(tuple(o.shape) == (2, 19, 65, 129) for o in outs)
    plan = next(iter(m._plans().values()))
    names = collections.Counter(c.name for c in plan.g.fwd)
    assert names['resize_nchw'] == 2 and names['profile_upsample'] == 0
    assert P.Graph(torch.device('cpu'), False, False).head is None


def test_unsupported_class_count_is_an_error(dry):
    from addk.exit_profile import ExitProfile
    with pytest.raises(addk.AddkError, match='19 classes.*16 thresholds'):
        ExitProfile(_add(4, classes=7), (1, 3, 33, 65))


def test_rebuilds_when_the_parameters_move(dry):
    from addk.exit_profile import ExitProfile
    m = _add(4)
    prof = ExitProfile(m, SHAPE)
    g0 = prof.g
    prof.step()
    assert prof.g is g0
    p = next(m.parameters())
    p.data = p.data.clone()
    prof.step()
    assert prof.g is not g0 and prof.batches == 2 and prof.records()['entropy'].shape[1] == 4
    # after a capture: the rebuild drops the captured graph with the plan it replayed and starts the eager calls again
    prof = ExitProfile(m, SHAPE, use_graph=True)
    g0, prof.graph, prof.calls = prof.g, object(), 7
    p.data = p.data.clone()
    prof.step()
    assert prof.g is not g0 and prof.graph is None and prof.calls == 1 and prof.batches == 1


def test_profile_abi_declared_and_exported():
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert 'addk_profile_upsample_args' in src
    fields = [f for f, _ in L.ProfileUpsampleArgs._fields_]
    assert fields[:8] == [f for f, _ in L.GateUpsampleArgs._fields_][:8]      # the prefix the heads share
    assert fields[8:] == ['target', 'thr', 'nthr', 'ent_out', 'share_out', 'cm', 'pred_out', 'ws']
    sup = lib.addk_profile_upsample_supported
    assert sup(2, 9, 17, 65, 129, 19, 0) == 1 and sup(2, 9, 17, 65, 129, 19, 16) == 1
    assert sup(1, 4, 4, 128, 128, 19, 4) == 1
    assert sup(2, 9, 17, 65, 129, 19, 17) == 0 and sup(2, 9, 17, 65, 129, 19, -1) == 0
    assert sup(2, 9, 17, 65, 129, 21, 4) == 0
    assert sup(2, 0, 17, 65, 129, 19, 4) == 0
    # the ticket, then per 64 x 32 tile one entropy partial and sixteen counts
    assert lib.addk_profile_upsample_ws_bytes(2, 65, 129) == 16 + 68 * 2 * 3 * 3
    assert lib.addk_profile_upsample_ws_bytes(0, 65, 129) == 0


def test_profile_args_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.ProfileUpsampleArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(addk_profile_upsample_args));']
    lines += ['printf("%s %%zu\\n", offsetof(addk_profile_upsample_args, %s));' % (f, f) for f in fields] + ['return 0;}']
    c = tmp_path / 'abi.c'
    c.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got['size']) == ctypes.sizeof(L.ProfileUpsampleArgs)
    for f in fields:
        assert int(got[f]) == getattr(L.ProfileUpsampleArgs, f).offset, f
