"""Host-logic tests of the validation step (CPU, no GPU): addk.validate.ValidationStep is built with the kernel launches stubbed
out (the `dry` pattern of tests/test_plan_dryrun.py) and the launch list is inspected — one fused scoring launch per exit, no
full-resolution logits anywhere — plus the C ABI of the scoring entry points.  Arithmetic is tests/test_gpu_validate.py."""
import collections
import ctypes
import os
import re

import torch

import addk
import addk._lib as L
import addk.plan as P
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, GENOTYPE_BASELINE_2, NETWORK_PATH_BASELINE, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 65, 129)


def _add(F=4, arch=ARCH_C2):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), arch['low_level_layer'])


def _names(step):
    return collections.Counter(c.name for c in step.g.fwd)


def _has_full_resolution_buffer(g, shape):
    """a [N,C,OH,OW] tensor, or its NHWC form (dense or with the padded pixel stride), among what the plan owns"""
    N, Cc, OH, OW = shape
    sizes = {N * OH * OW * Cc, N * OH * OW * ((Cc + 3) // 4 * 4)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    return any(b.n in sizes for b in g._bufs) or any(tuple(t.shape) == tuple(shape) or t.numel() in sizes for t in owned)


def test_validation_step_scores_every_exit_without_full_resolution_logits(dry):
    from addk.validate import ValidationStep
    m = _add(4)
    vs = ValidationStep(m, SHAPE)
    names = _names(vs)
    assert names['score_upsample'] == 2 and names['resize_nchw'] == 0
    assert names['ce_count'] == 1 and names['score_zero'] == 1               # one target count shared by the exits
    assert names['bn_eval_affine_batch'] == 1 and names['bn_finalize'] == 0   # inference form
    assert not vs.g.bwd
    assert all(o.y is None and o.head == 'score' and tuple(o.shape) == (2, 19, 65, 129) for o in vs.outs)
    assert not _has_full_resolution_buffer(vs.g, (2, 19, 65, 129))
    # every scoring launch follows the zeroing of its scalars and the shared count in the scheduled list
    order = [c.name for c in vs.g.fwd]
    first_score = order.index('score_upsample')
    assert order.index('score_zero') < first_score and order.index('ce_count') < first_score
    assert m.training                                                         # the model's mode is not touched
    vs.step(torch.randn(SHAPE), torch.zeros((2, 65, 129), dtype=torch.int64))
    assert dry['score_upsample'] == 2 and vs.batches == 1
    r = vs.result()
    assert len(r['exits']) == 2 and r['batches'] == 1 and tuple(r['exits'][0]['confusion'].shape) == (19, 19)
    vs.reset()
    assert vs.batches == 0


def test_three_exits_and_baseline(dry):
    from addk.modeling.baseline_model import Baselin_Model
    from addk.validate import ValidationStep
    vs = ValidationStep(_add(4, ARCH_C3), SHAPE, class_weight=torch.rand(19) + 0.5, keep_predictions=True)
    assert _names(vs)['score_upsample'] == 3 and _names(vs)['resize_nchw'] == 0
    assert tuple(vs.pred.shape) == (3, 2, 65, 129) and vs.pred.dtype == torch.uint8
    b = Baselin_Model(NETWORK_PATH_BASELINE, [5], GENOTYPE_BASELINE_2, 19, make_args(4), 1)
    vb = ValidationStep(b, SHAPE)
    assert _names(vb)['score_upsample'] == 2 and _names(vb)['resize_nchw'] == 0


def test_plain_eval_plan_keeps_its_resizes(dry):
    """The flag is per plan: a model(x) call in the same process, before and after a ValidationStep was built on the model,
    still materialises its logits."""
    from addk.validate import ValidationStep
    m = _add(4).eval()
    ValidationStep(m, SHAPE)
    with torch.no_grad():
        outs = m(torch.randn(SHAPE))
    assert all(tuple(o.shape) == (2, 19, 65, 129) for o in outs)
    plan = next(iter(m._plans().values()))
    names = collections.Counter(c.name for c in plan.g.fwd)
    assert names['resize_nchw'] == 2 and names['score_upsample'] == 0
    assert P.Graph(torch.device('cpu'), False, False).head is None


def test_unsupported_class_count_falls_back_inside_the_plan(dry):
    """addk_score_upsample_supported == 0 (here: 7 classes): resize + cross-entropy without a gradient + argmax + confusion +
    entropy, in the same plan."""
    from addk.modeling.ADD import ADD
    from addk.validate import ValidationStep
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 7, make_args(4), 0)
    vs = ValidationStep(m, (1, 3, 33, 65), keep_predictions=True)
    names = _names(vs)
    assert names['score_upsample'] == 0
    assert names['resize_nchw'] == names['ce_fwd_bwd'] == names['argmax_nchw'] == names['confusion'] == names['entropy_sum'] == 2
    ce = [c for c in vs.g.fwd if c.name == 'ce_fwd_bwd']
    assert all(c.args[10] is None for c in ce)                                # null gradient pointer
    assert not vs.g.bwd


def test_rebuilds_when_the_parameters_move(dry):
    """A TrainStep built later re-points the parameters into its flat buffer: the validation plan holds raw pointers and has to be
    emitted again."""
    from addk.validate import ValidationStep
    m = _add(4)
    vs = ValidationStep(m, SHAPE)
    g0 = vs.g
    vs.step()
    assert vs.g is g0
    p = next(m.parameters())
    p.data = p.data.clone()
    vs.step()
    assert vs.g is not g0 and vs.batches == 2
    # after a capture: the rebuild drops the captured graph with the plan it replayed and starts the eager calls again
    vs = ValidationStep(m, SHAPE, use_graph=True)
    g0, vs.graph, vs.calls = vs.g, object(), 7
    p.data = p.data.clone()
    vs.step()
    assert vs.g is not g0 and vs.graph is None and vs.calls == 1 and vs.batches == 1


def test_score_abi_declared_and_exported():
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in ('addk_score_upsample', 'addk_score_upsample_supported', 'addk_score_upsample_ws_floats'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert 'addk_score_upsample_args' in src
    f = dict(L.ScoreUpsampleArgs._fields_)
    assert f['cm'] is ctypes.c_void_p and f['pred_out'] is ctypes.c_void_p and f['ent_out'] is ctypes.c_void_p
    # host-side queries: 19 classes only; the gather form has no rows-per-input-row limit (addk_ce_upsample_supported has)
    assert lib.addk_score_upsample_supported(2, 9, 17, 65, 129, 19) == 1
    assert lib.addk_score_upsample_supported(1, 4, 4, 128, 128, 19) == 1 and lib.addk_ce_upsample_supported(1, 4, 4, 128, 128, 19) == 0
    assert lib.addk_score_upsample_supported(2, 9, 17, 65, 129, 7) == 0
    assert lib.addk_score_upsample_supported(2, 0, 17, 65, 129, 19) == 0
    assert lib.addk_score_upsample_ws_floats(2, 65, 129) == 2 * 2 * 3 * 3      # two partials per 64 x 32 tile


def test_score_args_layout_matches_header(tmp_path):
    import subprocess
    fields = [f for f, _ in L.ScoreUpsampleArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(addk_score_upsample_args));']
    lines += ['printf("%s %%zu\\n", offsetof(addk_score_upsample_args, %s));' % (f, f) for f in fields] + ['return 0;}']
    c = tmp_path / 'abi.c'
    c.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got['size']) == ctypes.sizeof(L.ScoreUpsampleArgs)
    for f in fields:
        assert int(got[f]) == getattr(L.ScoreUpsampleArgs, f).offset, f
