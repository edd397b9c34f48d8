"""Host-logic tests of self-distillation from the final exit in the training step (CPU, no GPU): train.TrainStep(distill=...) is built with
the kernel launches stubbed out (the `dry` pattern of tests/test_plan_dryrun.py) and the launch list is inspected, plus the C ABI of the
entry point.  Arithmetic is tests/test_gpu_distill.py."""
import collections
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import addk
import addk._lib as L
import addk.heads as H
import addk.plan as P
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 65, 129)


def _add(F=4, arch=ARCH_C2):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), arch['low_level_layer'])


def _has_full_resolution_buffer(g, shape):
    """a [N,C,OH,OW] tensor, or its NHWC form (dense or with the padded pixel stride), among what the plan owns"""
    N, Cc, OH, OW = shape
    sizes = {N * OH * OW * Cc, N * OH * OW * ((Cc + 3) // 4 * 4)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    return any(b.n in sizes for b in g._bufs) or any(tuple(t.shape) == tuple(shape) or t.numel() in sizes for t in owned)


def _names(ts):
    return collections.Counter(c.name for c in ts.g.fwd), collections.Counter(c.name for c in ts.g.bwd)


def test_struct_layout_matches_header():
    cname, cls = 'addk_ce_upsample_kd_args', L.CeUpsampleKdArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
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
    assert cls.ce.offset == 0 and cls.pix_loss.offset == ctypes.sizeof(L.CeUpsampleArgs)
    # the mining head's block is a prefix: ce, pix_loss, tau
    assert cls.pix_loss.offset == L.CeUpsampleOhemArgs.pix_loss.offset and cls.tau.offset == L.CeUpsampleOhemArgs.tau.offset


def test_host_side_queries():
    lib = addk.load()
    for shp in ((2, 17, 33, 65, 129, 19), (2, 17, 33, 65, 129, 7), (0, 17, 33, 65, 129, 19), (2, 4, 8, 128, 256, 19), (2, 128, 256, 1024, 2048, 19)):
        assert lib.addk_ce_upsample_kd_supported(*shp) == lib.addk_ce_upsample_supported(*shp), shp
    assert lib.addk_ce_upsample_kd_supported(2, 17, 33, 65, 129, 19) == 1 and lib.addk_ce_upsample_kd_supported(2, 4, 8, 128, 256, 19) == 0
    # two partial-sum regions: the loss and the KL
    assert lib.addk_ce_upsample_kd_ws_floats(2, 17, 33) == 2 * lib.addk_ce_upsample_ws_floats(2, 17, 33) > 0
    # a null argument block is refused on the host, before any launch
    assert lib.addk_ce_upsample_kd_fwd_bwd(None, None) == -1


def test_train_step_with_distill_has_one_student_head_and_the_plain_last_exit(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, distill=(1.0, 4.0), use_graph=False)
    fwd, bwd = _names(ts)
    assert len(ts.outs) == 2 and bwd['ce_upsample_kd'] == 1 and bwd['ce_upsample'] == 1
    assert bwd['ohem_select'] == 0 and bwd['ce_upsample_ohem'] == 0 and fwd['ce_count'] == 1 and fwd['ce_count_valid'] == 0
    assert (fwd + bwd)['resize_nchw'] == 0 and (fwd + bwd)['resize_nchw_bwd'] == 0
    assert all(o.y is None and o.head == 'ce' and tuple(o.shape) == (2, 19, 65, 129) and o.src is not None for o in ts.outs)
    assert not _has_full_resolution_buffer(ts.g, (2, 19, 65, 129))
    kd = [c for c in ts.g.bwd if c.name == 'ce_upsample_kd'][0]
    last = [c for c in ts.g.bwd if c.name == 'ce_upsample'][0]
    k, a = kd.args[0]._obj, last.args[0]._obj
    # the student's block: its own logits, the LAST exit's logits as the teacher, the step's count word, no kept set
    assert k.teacher == a.logits and k.ld_teacher == a.ld and k.ce.logits != a.logits
    assert k.ce.logits == ts.g.src(ts.outs[0].src).x and a.logits == ts.g.src(ts.outs[1].src).x
    assert k.alpha == 1.0 and k.temperature == 4.0 and not k.pix_loss and not k.tau
    assert k.nvalid == ts.wsum.data_ptr() == k.ce.wsum and k.ce.scale == 0.5 and k.ce.loss_out == ts.loss.data_ptr()
    assert k.kd_out == ts.outs[0].binding['distill_state']['kd'].data_ptr() and k.ce.ws != a.ws
    assert 'distill' not in ts.outs[1].binding
    # regions: the command reads the teacher's logits and the count word, writes kd_out and the workspace
    treg = [P._region(r) for r in ts.g.lz(ts.outs[1].src)]
    assert all(r in kd.rd for r in treg) and P._region(ts.wsum) in kd.rd
    assert P._region(ts.outs[0].binding['distill_state']['kd']) in kd.wr and not any(r in kd.wr for r in treg)
    # the hazard tracker over the whole step orders the student's head after the launch that produced the teacher's logits
    cmds = ts.g.fwd + ts.g.bwd
    deps = list(P.deps(cmds))
    prod = [i for i, c in enumerate(cmds) if any(r in c.wr for r in treg)]
    ikd = cmds.index(kd)
    assert prod and prod[-1] < ikd and prod[-1] in deps[ikd]
    ts.g.run_parallel(ts.g.bwd, None)
    assert dry['ce_upsample_kd'] == 1 and dry['ce_upsample'] == 1
    assert ts.distill_stats() == [0.0]                               # nothing ran: the zero-initialised word


def test_distill_with_ohem_and_with_class_weights(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, distill=(1.0, 4.0), ohem=(0.7, 1000), use_graph=False)
    fwd, bwd = _names(ts)
    assert bwd['ohem_select'] == 2 and bwd['ce_upsample_kd'] == 1 and bwd['ce_upsample_ohem'] == 1 and bwd['ce_upsample'] == 0
    assert fwd['ce_count'] == 0 and fwd['ce_count_valid'] == 1      # ONE extra count for all exits, unweighted
    cnt = [c for c in ts.g.fwd if c.name == 'ce_count_valid'][0]
    assert cnt.args[2] is None and cnt.args[5] == ts.nvalid.data_ptr() != ts.wsum.data_ptr()      # class_w, wsum of addk_ce_count
    kd = [c for c in ts.g.bwd if c.name == 'ce_upsample_kd'][0]
    k = kd.args[0]._obj
    sel = [c.args[0]._obj for c in ts.g.bwd if c.name == 'ohem_select']
    mine = [s for s in sel if s.pix_loss == k.pix_loss]
    assert len(mine) == 1 and k.tau == mine[0].tau and k.ce.wsum == mine[0].wsum_kept and k.ce.logits == mine[0].logits
    assert k.nvalid == ts.nvalid.data_ptr() and P._region(ts.nvalid) in kd.rd
    order = [c.name for c in ts.g.bwd]
    deps = list(P.deps(ts.g.bwd))
    i = ts.g.bwd.index(kd)
    assert [ts.g.bwd[j].args[0]._obj.pix_loss for j in deps[i] if ts.g.bwd[j].name == 'ohem_select'] == [k.pix_loss]
    assert order.index('ohem_select') < i
    assert not _has_full_resolution_buffer(ts.g, (2, 19, 65, 129))
    assert len(ts.ohem_stats()) == 2 and ts.distill_stats() == [0.0]
    # class weights without mining: wsum is a weighted sum, so the term gets the count word of its own
    w = torch.rand(19) + 0.5
    ts = TrainStep(_add(4), SHAPE, distill=(0.5, 2.0), class_weight=w, use_graph=False)
    fwd, bwd = _names(ts)
    assert fwd['ce_count'] == 1 and fwd['ce_count_valid'] == 1 and bwd['ce_upsample_kd'] == 1 and bwd['ce_upsample'] == 1
    k = [c for c in ts.g.bwd if c.name == 'ce_upsample_kd'][0].args[0]._obj
    assert k.nvalid == ts.nvalid.data_ptr() and k.ce.wsum == ts.wsum.data_ptr() and k.ce.class_w and k.alpha == 0.5 and k.temperature == 2.0


def test_without_distill_the_plan_is_the_parents(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, use_graph=False)
    fwd, bwd = _names(ts)
    assert bwd['ce_upsample'] == 2 and bwd['ce_upsample_kd'] == 0 and fwd['ce_count'] == 1 and fwd['ce_count_valid'] == 0
    assert all('distill' not in o.binding and 'nvalid' not in o.binding for o in ts.outs)
    with pytest.raises(ValueError):
        ts.distill_stats()
    # command for command the names of a step that has the parameter at its default
    ts2 = TrainStep(_add(4), SHAPE, use_graph=False, distill=None)
    assert [c.name for c in ts2.g.fwd] == [c.name for c in ts.g.fwd] and [c.name for c in ts2.g.bwd] == [c.name for c in ts.g.bwd]
    # and a distilling step differs from it in the student's loss head only
    ts3 = TrainStep(_add(4), SHAPE, use_graph=False, distill=(1.0, 4.0))
    assert [c.name for c in ts3.g.fwd] == [c.name for c in ts.g.fwd]
    strip = lambda lst: sorted(c.name for c in lst if c.name not in ('ce_upsample', 'ce_upsample_kd'))   # noqa: E731
    assert strip(ts3.g.bwd) == strip(ts.g.bwd) and len(ts3.g.bwd) == len(ts.g.bwd)


@pytest.mark.parametrize('distill', [(0, 4), (-1, 4), (1, 0), (float('nan'), 4), (1, float('inf')), (1,), 1.0, ('a', 'b'), (1, 4, 2)])
def test_bad_parameters_raise_before_a_plan_is_built(dry, distill, monkeypatch):
    from addk.train import TrainStep
    built = []
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: built.append(1))
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, distill=distill, use_graph=False)
    assert not built


def test_unfused_head_single_exit_or_unsupported_exit_raises(dry, monkeypatch):
    from addk.train import TrainStep
    built = []
    real = P.Graph.finalize
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    monkeypatch.setenv('ADDK_FUSE_CE', '0')
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, distill=(1.0, 4.0), use_graph=False)
    monkeypatch.setenv('ADDK_FUSE_CE', '1')

    # a model with a single exit has nobody to teach
    class OneExit(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = _add(4)

        def emit(self, g, a):
            return self.net.emit(g, a)[-1:]
    with pytest.raises(ValueError):
        TrainStep(OneExit(), SHAPE, distill=(1.0, 4.0), use_graph=False)
    # exits whose low-resolution logits differ in shape
    real_head = H.HEADS['ce']

    def odd_head(g, src, OH, OW):
        out = real_head(g, src, OH, OW)
        if not seen:                                                 # the first exit claims a map one row shorter
            r = src.raw
            out.src = P.Act(P.TRef(r.buf, r.off, r.N, r.H - 1, r.W, r.C, r.ld), needs_grad=True)
        seen.append(1)
        return out
    seen = []
    monkeypatch.setitem(H.HEADS, 'ce', odd_head)
    try:
        with pytest.raises(ValueError):
            TrainStep(_add(4), SHAPE, distill=(1.0, 4.0), use_graph=False)
    finally:
        monkeypatch.setitem(H.HEADS, 'ce', real_head)
    # an exit whose shape the fused head does not take (more than 16 output rows per input row): no materialised fallback
    lib = addk.load()
    monkeypatch.setattr(lib, 'addk_ce_upsample_supported', lambda *a: 0)
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, distill=(1.0, 4.0), use_graph=False)
    assert not built
    TrainStep(_add(4), SHAPE, use_graph=False)                     # the plain step still takes the three-kernel form there
    assert built
