"""Host-logic tests of the soft-Dice region term in the training step (CPU, no GPU): train.TrainStep(dice=...) is built with the kernel
launches stubbed out (the `dry` pattern of tests/test_plan_dryrun.py) and the launch list is inspected, plus the C ABI of the two entry
points.  Arithmetic is tests/test_gpu_dice.py."""
import collections
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import addk
import addk._lib as L
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


def test_struct_layouts_match_header():
    structs = {'addk_dice_stats_args': L.DiceStatsArgs, 'addk_ce_upsample_dice_args': L.CeUpsampleDiceArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    for cname, cls in structs.items():
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
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    # the head's block wraps the distillation head's, which wraps the plain head's: all at offset 0
    assert L.CeUpsampleDiceArgs.kd.offset == 0 and L.CeUpsampleDiceArgs.coef.offset == ctypes.sizeof(L.CeUpsampleKdArgs)
    # the reduction's block starts with the prefix every *_upsample block shares
    for f in ('logits', 'ld', 'N', 'H', 'W', 'C', 'OH', 'OW', 'target'):
        assert getattr(L.DiceStatsArgs, f).offset == getattr(L.CeUpsampleArgs, f).offset, f


def test_host_side_queries():
    lib = addk.load()
    for shp in ((2, 17, 33, 65, 129, 19), (2, 17, 33, 65, 129, 7), (0, 17, 33, 65, 129, 19), (2, 4, 8, 128, 256, 19), (2, 128, 256, 1024, 2048, 19)):
        assert lib.addk_dice_stats_supported(*shp) == lib.addk_ohem_select_supported(*shp), shp
    assert lib.addk_dice_stats_supported(2, 17, 33, 65, 129, 19) == 1 and lib.addk_dice_stats_supported(2, 17, 33, 65, 129, 20) == 0
    assert lib.addk_dice_stats_supported(2, 128, 256, 32768, 32768, 19) == 0          # 2^31 pixels: the 32-bit counters
    # 96 words of tables, then one row of 38 fp32 partials per 64 x 32 tile and image
    assert lib.addk_dice_stats_ws_bytes(2, 65, 129) == 4 * (96 + 38 * 2 * 3 * 3)
    assert lib.addk_dice_stats_ws_bytes(2, 1024, 2048) == 4 * (96 + 38 * 2 * 32 * 32)
    assert lib.addk_dice_stats_ws_bytes(0, 65, 129) == 0
    # null argument blocks are refused on the host, before any launch
    assert lib.addk_dice_stats(None, None) == -1 and lib.addk_ce_upsample_dice_fwd_bwd(None, None) == -1
    assert lib.addk_dice_stats(ctypes.byref(L.DiceStatsArgs()), None) == -1
    assert lib.addk_ce_upsample_dice_fwd_bwd(ctypes.byref(L.CeUpsampleDiceArgs()), None) == -1


def _pairs(ts):
    """(dice_stats command, the head that reads its table) per exit; in the scheduled backward list the reduction comes first"""
    bwd = ts.g.bwd
    res = []
    for i, c in enumerate(bwd):
        if c.name == 'dice_stats':
            heads = [j for j, h in enumerate(bwd) if h.name == 'ce_upsample_dice' and h.args[0]._obj.coef == c.args[0]._obj.coef]
            assert len(heads) == 1 and heads[0] > i
            res.append((c, bwd[heads[0]]))
    return res


@pytest.fixture()
def emitted(monkeypatch):
    """the names of the loss-head commands in the order emit_ce appends them (finalize then schedules the list over the streams)"""
    names, real = [], P.Graph._add

    def add(self, lst, name, *a, **k):
        if name in ('ohem_select', 'dice_stats') or name.startswith('ce_upsample'):
            names.append(name)
        return real(self, lst, name, *a, **k)
    monkeypatch.setattr(P.Graph, '_add', add)
    return names


def test_train_step_with_dice_has_stats_directly_in_front_of_every_head(dry, emitted):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, dice=(0.5, 1.0), use_graph=False)
    fwd, bwd = _names(ts)
    assert len(ts.outs) == 2 and bwd['dice_stats'] == 2 and bwd['ce_upsample_dice'] == 2
    assert bwd['ce_upsample'] == 0 and bwd['ce_upsample_kd'] == 0 and bwd['ce_upsample_ohem'] == 0 and bwd['ohem_select'] == 0
    assert fwd['ce_count'] == 1 and fwd['ce_count_valid'] == 0 and fwd['dice_stats'] == 0
    assert (fwd + bwd)['resize_nchw'] == 0 and (fwd + bwd)['resize_nchw_bwd'] == 0
    assert not _has_full_resolution_buffer(ts.g, (2, 19, 65, 129))
    assert emitted == ['dice_stats', 'ce_upsample_dice'] * 2
    pairs = _pairs(ts)
    assert len(pairs) == 2
    lib = addk.load()
    by_table = {st.args[0]._obj.coef: (st, hd) for st, hd in pairs}
    for o in ts.outs:
        state = o.binding['dice_state']
        st, hd = by_table[state['coef'].data_ptr()]
        s, h = st.args[0]._obj, hd.args[0]._obj
        coef, dout = state['coef'], state['dice']
        assert o.binding['dice'] == (0.5, 1.0) and coef.numel() == 38 and dout.numel() == 20
        # the reduction: the exit's own logits and grids, the step's target, the term's parameters, the step's loss word
        src = ts.g.src(o.src)
        assert (s.logits, s.ld, s.N, s.H, s.W, s.C, s.OH, s.OW) == (src.x, src.ld, 2, o.src.H, o.src.W, 19, 65, 129)
        assert s.target == ts.target.data_ptr() and s.ignore_index == 255 and (s.weight, s.smooth, s.scale) == (0.5, 1.0, 0.5)
        assert s.coef == coef.data_ptr() and s.dice_out == dout.data_ptr() and s.loss_out == ts.loss.data_ptr() and s.ws
        # the head: the plain head's block, no kept set, no teacher, the table
        assert h.coef == coef.data_ptr() and not h.kd.teacher and not h.kd.pix_loss and not h.kd.tau and not h.kd.nvalid
        assert h.kd.ce.logits == s.logits and h.kd.ce.wsum == ts.wsum.data_ptr() and h.kd.ce.scale == 0.5 and h.kd.ce.loss_out == ts.loss.data_ptr()
        assert h.kd.ce.ws and h.kd.ce.g
        # regions: the reduction reads the logits and the target and writes table, term, loss and workspace; the head reads the table
        lreg = [P._region(r) for r in ts.g.lz(o.src)]
        assert all(r in st.rd for r in lreg) and P._region(ts.target) in st.rd
        assert P._region(coef) in st.wr and P._region(dout) in st.wr and P._region(ts.loss) in st.wr and len(st.wr) == 4
        assert P._region(coef) in hd.rd and P._region(coef) not in hd.wr and P._region(ts.loss) in hd.wr
        # the hazard tracker orders the pair
        deps = list(P.deps(ts.g.bwd))
        assert ts.g.bwd.index(st) in deps[ts.g.bwd.index(hd)]
    ts.g.run_parallel(ts.g.bwd, None)
    assert dry['dice_stats'] == 2 and dry['ce_upsample_dice'] == 2
    stats = ts.dice_stats()                                          # nothing ran: the zero-initialised words
    assert stats == [(0.0, [0.0] * 19)] * 2
    assert lib.addk_dice_stats_ws_bytes(2, 65, 129) > 0


def test_dice_with_ohem(dry, emitted):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, dice=(1.0, 1.0), ohem=(0.7, 1000), use_graph=False)
    fwd, bwd = _names(ts)
    assert bwd['ohem_select'] == 2 and bwd['dice_stats'] == 2 and bwd['ce_upsample_dice'] == 2 and bwd['ce_upsample_ohem'] == 0
    assert fwd['ce_count'] == 0 and fwd['ce_count_valid'] == 0
    assert emitted == ['ohem_select', 'dice_stats', 'ce_upsample_dice'] * 2
    deps = list(P.deps(ts.g.bwd))
    for st, hd in _pairs(ts):
        h = hd.args[0]._obj
        sel = [c for c in ts.g.bwd if c.name == 'ohem_select' and c.args[0]._obj.pix_loss == h.kd.pix_loss]
        assert len(sel) == 1
        s = sel[0].args[0]._obj
        assert h.kd.tau == s.tau and h.kd.ce.wsum == s.wsum_kept and h.kd.ce.logits == s.logits and not h.kd.teacher
        i = ts.g.bwd.index(hd)
        assert ts.g.bwd.index(sel[0]) in deps[i] and ts.g.bwd.index(st) in deps[i]
        # mining never reaches the reduction: it reads neither the map nor tau
        assert not any(r in st.rd for r in sel[0].wr)
    assert not _has_full_resolution_buffer(ts.g, (2, 19, 65, 129))
    assert len(ts.ohem_stats()) == 2 and len(ts.dice_stats()) == 2


def test_dice_with_distill(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, dice=(2, 0), distill=(1.0, 4.0), use_graph=False)      # smooth = 0 is a good value
    assert ts.dice == (2.0, 0.0)
    fwd, bwd = _names(ts)
    assert bwd['dice_stats'] == 2 and bwd['ce_upsample_dice'] == 2 and bwd['ce_upsample_kd'] == 0 and bwd['ce_upsample'] == 0
    assert fwd['ce_count'] == 1 and fwd['ce_count_valid'] == 0
    heads = {hd.args[0]._obj.kd.ce.logits: (st, hd) for st, hd in _pairs(ts)}
    (st0, hd0), (st1, hd1) = (heads[ts.g.src(o.src).x] for o in ts.outs)
    k0, k1 = hd0.args[0]._obj, hd1.args[0]._obj
    # the student keeps its teacher wiring, the last exit has none; both have the table
    assert k0.kd.teacher == k1.kd.ce.logits and k0.kd.alpha == 1.0 and k0.kd.temperature == 4.0 and k0.kd.nvalid == ts.wsum.data_ptr()
    assert k0.kd.kd_out == ts.outs[0].binding['distill_state']['kd'].data_ptr()
    assert not k1.kd.teacher and not k1.kd.nvalid and not k1.kd.kd_out
    assert k0.coef == ts.outs[0].binding['dice_state']['coef'].data_ptr() and k1.coef == ts.outs[1].binding['dice_state']['coef'].data_ptr()
    treg = [P._region(r) for r in ts.g.lz(ts.outs[1].src)]
    assert all(r in hd0.rd for r in treg) and P._region(ts.outs[0].binding['distill_state']['kd']) in hd0.wr
    assert ts.distill_stats() == [0.0] and len(ts.dice_stats()) == 2
    # the student's workspace holds the two partial-sum regions of the distillation head
    lib = addk.load()
    o = ts.outs[0].src
    ws = [t for t in ts.g.keep if isinstance(t, torch.Tensor) and t.data_ptr() == k0.kd.ce.ws]
    assert len(ws) == 1 and ws[0].numel() == lib.addk_ce_upsample_kd_ws_floats(o.N, o.H, o.W)


def test_dice_with_ohem_distill_and_class_weights(dry, emitted):
    from addk.train import TrainStep
    w = torch.rand(19) + 0.5
    ts = TrainStep(_add(4), SHAPE, dice=(0.25, 1e-3), ohem=(0.7, 1000), distill=(0.5, 2.0), class_weight=w, use_graph=False)
    fwd, bwd = _names(ts)
    assert bwd['ohem_select'] == 2 and bwd['dice_stats'] == 2 and bwd['ce_upsample_dice'] == 2
    assert bwd['ce_upsample_kd'] == 0 and bwd['ce_upsample_ohem'] == 0 and bwd['ce_upsample'] == 0
    assert fwd['ce_count'] == 0 and fwd['ce_count_valid'] == 1
    assert emitted == ['ohem_select', 'dice_stats', 'ce_upsample_dice'] * 2
    for st, hd in _pairs(ts):
        s, h = st.args[0]._obj, hd.args[0]._obj
        assert h.kd.ce.class_w and h.kd.pix_loss and h.kd.tau and h.coef == s.coef
        assert abs(s.weight - 0.25) < 1e-7 and abs(s.smooth - 1e-3) < 1e-9          # the fp32 words
    student = [hd.args[0]._obj for _, hd in _pairs(ts) if hd.args[0]._obj.kd.teacher]
    assert len(student) == 1 and student[0].kd.nvalid == ts.nvalid.data_ptr() and student[0].kd.alpha == 0.5
    assert not _has_full_resolution_buffer(ts.g, (2, 19, 65, 129))


def test_without_dice_the_plan_is_the_parents(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, use_graph=False)
    fwd, bwd = _names(ts)
    assert bwd['ce_upsample'] == 2 and bwd['dice_stats'] == 0 and bwd['ce_upsample_dice'] == 0
    assert all('dice' not in o.binding and 'dice_state' not in o.binding for o in ts.outs)
    with pytest.raises(ValueError):
        ts.dice_stats()
    # command for command the names of a step that has the parameter at its default
    ts2 = TrainStep(_add(4), SHAPE, use_graph=False, dice=None)
    assert [c.name for c in ts2.g.fwd] == [c.name for c in ts.g.fwd] and [c.name for c in ts2.g.bwd] == [c.name for c in ts.g.bwd]
    # a step with the term has the same forward list; its backward list has the reductions and the other heads (the reductions add a
    # dependency level, so the level-batched launches behind them may group differently: the list is not compared name for name)
    ts3 = TrainStep(_add(4), SHAPE, use_graph=False, dice=(1.0, 1.0))
    assert [c.name for c in ts3.g.fwd] == [c.name for c in ts.g.fwd]
    _, b3 = _names(ts3)
    assert b3['dice_stats'] == 2 and b3['ce_upsample_dice'] == 2 and b3['ce_upsample'] == 0
    # mining and distillation without the term keep their own heads
    ts4 = TrainStep(_add(4), SHAPE, use_graph=False, ohem=(0.7, 1000), distill=(1.0, 4.0))
    _, b4 = _names(ts4)
    assert b4['ce_upsample_kd'] == 1 and b4['ce_upsample_ohem'] == 1 and b4['dice_stats'] == 0 and b4['ce_upsample_dice'] == 0


@pytest.mark.parametrize('dice', [(0, 1), (-1, 1), (1, -1e-3), (float('nan'), 1), (1, float('nan')), (float('inf'), 1), (1, float('inf')),
                                  (1e-50, 1), (1,), 1.0, ('a', 'b'), (1, 1, 2)])
def test_bad_parameters_raise_before_a_plan_is_built(dry, dice, monkeypatch):
    from addk.train import TrainStep
    built = []
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: built.append(1))
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, dice=dice, use_graph=False)
    assert not built


def test_unfused_head_or_unsupported_exit_raises(dry, monkeypatch):
    from addk.train import TrainStep
    built = []
    real = P.Graph.finalize
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    monkeypatch.setenv('ADDK_FUSE_CE', '0')
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, dice=(1.0, 1.0), use_graph=False)
    monkeypatch.setenv('ADDK_FUSE_CE', '1')
    # an exit whose shape the fused head does not take (more than 16 output rows per input row): no materialised fallback
    lib = addk.load()
    monkeypatch.setattr(lib, 'addk_ce_upsample_supported', lambda *a: 0)
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, dice=(1.0, 1.0), use_graph=False)
    assert not built
    TrainStep(_add(4), SHAPE, use_graph=False)                     # the plain step still takes the three-kernel form there
    assert built
