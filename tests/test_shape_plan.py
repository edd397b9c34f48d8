"""Host-logic tests of the focal and label-smoothed loss heads in the training step (CPU, no GPU): train.TrainStep(focal=..., label_smoothing=...)
is built with the kernel launches stubbed out (the `dry` pattern of tests/test_plan_dryrun.py) and the launch list is inspected, plus the C
ABI of the entry point and the torch references of tests/_shape_ref.py against torch itself.  Arithmetic on the device is
tests/test_gpu_shape.py."""
import collections
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import addk
import addk._lib as L
import addk.plan as P
import _shape_ref as R
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, dry_run, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
import plan_fingerprint as FP     # noqa: E402

SHAPE = (2, 3, 65, 129)


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer'])


def _names(ts):
    return collections.Counter(c.name for c in ts.g.fwd), collections.Counter(c.name for c in ts.g.bwd)


def _has_full_resolution_buffer(g, shape):
    N, Cc, OH, OW = shape
    sizes = {N * OH * OW * Cc, N * OH * OW * ((Cc + 3) // 4 * 4)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    return any(b.n in sizes for b in g._bufs) or any(tuple(t.shape) == tuple(shape) or t.numel() in sizes for t in owned)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_struct_layout_matches_header():
    structs = {'addk_ce_upsample_shaped_args': L.CeUpsampleShapedArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("shapes %d %d %d\\n", ADDK_CE_SHAPE_NONE, ADDK_CE_SHAPE_FOCAL, ADDK_CE_SHAPE_SMOOTH);')
    lines += ['return 0;}']
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'abi.c')
        open(c, 'w').write('\n'.join(lines))
        exe = os.path.join(d, 'abi')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = [l.split() for l in out.strip().splitlines()]
    got = {r[0]: r[1:] for r in rows}
    for cname, cls in structs.items():
        assert int(got[cname][0]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)][0]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    assert [int(v) for v in got['shapes']] == [L.CE_SHAPE_NONE, L.CE_SHAPE_FOCAL, L.CE_SHAPE_SMOOTH] == [0, 1, 2]
    # the block wraps the widest existing one at offset 0, which wraps the distillation head's, which wraps the plain head's
    S = L.CeUpsampleShapedArgs
    assert S.dice.offset == 0 and S.shape.offset == ctypes.sizeof(L.CeUpsampleDiceArgs)
    assert (S.gamma.offset, S.eps.offset) == (S.shape.offset + 4, S.shape.offset + 8)
    assert L.STRUCTS['addk_ce_upsample_shaped_args'] is S
    assert S.dice.offset == L.CeUpsampleDiceArgs.kd.offset == L.CeUpsampleKdArgs.ce.offset == 0


def test_host_side_queries():
    lib = addk.load()
    for C_, ok in ((7, 0), (19, 1), (20, 0), (21, 1), (22, 0)):
        assert lib.addk_ce_upsample_shaped_supported(2, 17, 33, 65, 129, C_) == ok, C_
        assert lib.addk_ce_upsample_shaped_supported(2, 17, 33, 65, 129, C_) == lib.addk_ce_upsample_supported(2, 17, 33, 65, 129, C_)
    assert sorted(L.head_classes()) == [19, 21]
    assert lib.addk_ce_upsample_shaped_supported(0, 17, 33, 65, 129, 19) == 0
    assert lib.addk_ce_upsample_shaped_supported(2, 4, 8, 128, 256, 19) == 0           # 32 output rows per input row
    # refused on the host, before any launch: a null block, an empty block in each shape, a shape outside the three
    assert lib.addk_ce_upsample_shaped_fwd_bwd(None, None) == -1
    for shape in (L.CE_SHAPE_NONE, L.CE_SHAPE_FOCAL, L.CE_SHAPE_SMOOTH, 3, -1):
        a = L.CeUpsampleShapedArgs()
        a.shape, a.gamma, a.eps = shape, 2.0, 0.1
        assert lib.addk_ce_upsample_shaped_fwd_bwd(ctypes.byref(a), None) == -1, shape
    assert b'shape' in lib.addk_last_error()


# ---- the references against torch ----------------------------------------------------------------------------------------------------
# Two fp64 evaluations of one formula in different operation orders: a softmax over 19 - 21 classes, a power and a mean are some hundred
# rounded operations of 1.1e-16 each.  1e-13 of the largest element leaves room for them and is ten orders below a wrong factor.
TOL = 1e-13

def _ref_case(C=19, seed=3):
    g = torch.Generator().manual_seed(seed)
    up = (torch.randn(2, C, 9, 11, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    r = np.random.default_rng(seed)
    t = torch.from_numpy(r.integers(0, C, (2, 9, 11))).long()
    t[torch.from_numpy(r.random((2, 9, 11)) < 0.15)] = 255
    w = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return up, t, w


@pytest.mark.parametrize('C_', [19, 21])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'class_weights'])
@pytest.mark.parametrize('eps', [0.1, 0.3])
def test_smooth_reference_is_torch_cross_entropy(eps, weighted, C_):
    up, t, w = _ref_case(C_)
    w = w if weighted else None
    want = Fn.cross_entropy(up, t, weight=w, ignore_index=255, label_smoothing=eps)
    got = R.smooth_loss(up, t, eps, class_w=w)
    assert int((t == 255).sum()) > 0
    assert abs(float(got.detach()) - float(want.detach())) <= TOL * abs(float(want.detach())), (got, want)
    gw, = torch.autograd.grad(want, up)
    ga, = torch.autograd.grad(got, up)
    gf = R.smooth_grad(up.detach(), t, eps, class_w=w)
    scale = float(gw.abs().max())
    assert float((ga - gw).abs().max()) <= TOL * scale and float((gf - gw).abs().max()) <= TOL * scale
    # eps -> the plain cross-entropy is the other end of the same formula
    plain = Fn.cross_entropy(up.detach(), t, weight=w, ignore_index=255)
    assert abs(float(R.smooth_loss(up.detach(), t, 0.0, class_w=w)) - float(plain)) <= TOL * abs(float(plain))


@pytest.mark.parametrize('C_', [19, 21])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'class_weights'])
@pytest.mark.parametrize('gamma', [1.0, 2.0, 3.5])
def test_focal_reference_gradient_is_autograd(gamma, weighted, C_):
    up, t, w = _ref_case(C_, seed=4)
    w = w if weighted else None
    loss = R.focal_loss(up, t, gamma, class_w=w)
    ga, = torch.autograd.grad(loss, up)
    gf = R.focal_grad(up.detach(), t, gamma, class_w=w)
    assert float(ga.abs().max()) > 0 and float((gf - ga).abs().max()) <= TOL * float(ga.abs().max())
    # the definition, written the plain way: w_t (1 - p_t)^gamma (-log p_t) over the valid pixels, normalised by their weight sum
    valid = t != 255
    tc = torch.where(valid, t, torch.zeros_like(t))
    logpt = torch.log_softmax(up.detach(), 1).gather(1, tc[:, None]).squeeze(1)
    wt = (w[tc] if w is not None else torch.ones_like(logpt)) * valid
    want = (wt * (1 - logpt.exp()) ** gamma * -logpt).sum() / wt.sum()
    assert abs(float(loss.detach()) - float(want)) <= 10 * TOL * abs(float(want))          # 1 - p_t the plain way: its cancellation on top
    # a kept mask filters pixels and the normaliser; nothing kept is exactly 0
    mask = torch.zeros_like(valid)
    assert float(R.focal_loss(up.detach(), t, gamma, class_w=w, mask=mask)) == 0.0 and float(R.focal_grad(up.detach(), t, gamma, class_w=w, mask=mask).abs().max()) == 0.0


# ---- the plan ------------------------------------------------------------------------------------------------------------------------

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


def _heads(ts):
    """the shaped launches of the backward list, by the logits they read"""
    res = {}
    for c in ts.g.bwd:
        if c.name == 'ce_upsample_shaped':
            res[c.args[0]._obj.dice.kd.ce.logits] = c
    return res


def _check_heads(ts, ncls, shape, value, ohem=False, dice=False, weighted=False):
    """one shaped launch per exit in the place of the other heads, at the head of the backward list, with their arguments, reads and writes"""
    fwd, bwd = _names(ts)
    nex = len(ts.outs)
    assert nex == 2 and bwd['ce_upsample_shaped'] == nex
    assert bwd['ce_upsample'] == bwd['ce_upsample_ohem'] == bwd['ce_upsample_dice'] == bwd['ce_upsample_kd'] == 0
    assert bwd['ohem_select'] == (nex if ohem else 0) and bwd['dice_stats'] == (nex if dice else 0)
    assert fwd['ce_count'] == (0 if ohem else 1) and fwd['ce_count_valid'] == 0
    assert (fwd + bwd)['resize_nchw'] == 0 and (fwd + bwd)['resize_nchw_bwd'] == 0
    assert not _has_full_resolution_buffer(ts.g, (2, ncls) + SHAPE[2:])
    heads = _heads(ts)
    assert len(heads) == nex
    deps = list(P.deps(ts.g.bwd))
    # at the head of the backward list: the list starts with a head's command, and a head waits for nothing in it but the heads'
    # own commands — its selection and reduction, and the exit before it on the loss word (the scheduler interleaves the exits' chains)
    assert ts.g.bwd[0].name in ('ce_upsample_shaped', 'ohem_select', 'dice_stats')
    for hd in heads.values():
        assert all(ts.g.bwd[j].name in ('ce_upsample_shaped', 'ohem_select', 'dice_stats') for j in deps[ts.g.bwd.index(hd)])
    for o in ts.outs:
        src = ts.g.src(o.src)
        hd = heads[src.x]
        s = hd.args[0]._obj
        kd, ce = s.dice.kd, s.dice.kd.ce
        assert s.shape == shape
        assert (s.gamma if shape == L.CE_SHAPE_FOCAL else s.eps) == ctypes.c_float(value).value
        assert (ce.logits, ce.ld, ce.N, ce.H, ce.W, ce.C, ce.OH, ce.OW) == (src.x, src.ld, 2, o.src.H, o.src.W, ncls, 65, 129)
        assert ce.target == ts.target.data_ptr() and ce.ignore_index == 255 and ce.scale == 0.5 and ce.loss_out == ts.loss.data_ptr()
        assert ce.g and ce.ws and bool(ce.class_w) == weighted
        assert not kd.teacher and not kd.nvalid and not kd.kd_out                      # no distillation form
        i = ts.g.bwd.index(hd)
        if ohem:
            st = o.binding['ohem_state']
            assert (kd.pix_loss, kd.tau, ce.wsum) == (st['pix_loss'].data_ptr(), st['tau'].data_ptr(), st['wsum_kept'].data_ptr())
            sel = [c for c in ts.g.bwd if c.name == 'ohem_select' and c.args[0]._obj.pix_loss == kd.pix_loss]
            assert len(sel) == 1 and ts.g.bwd.index(sel[0]) in deps[i]
            assert all(P._region(st[k]) in hd.rd for k in ('pix_loss', 'tau', 'wsum_kept'))
        else:
            assert not kd.pix_loss and not kd.tau and ce.wsum == ts.wsum.data_ptr() and P._region(ts.wsum) in hd.rd
        if dice:
            st = o.binding['dice_state']
            assert s.dice.coef == st['coef'].data_ptr() and P._region(st['coef']) in hd.rd and P._region(st['coef']) not in hd.wr
            red = [c for c in ts.g.bwd if c.name == 'dice_stats' and c.args[0]._obj.coef == s.dice.coef]
            assert len(red) == 1 and ts.g.bwd.index(red[0]) in deps[i]
        else:
            assert not s.dice.coef
        # reads and writes: the logits, the target and the normaliser in; the gradient, the loss word and the workspace out
        assert all(P._region(r) in hd.rd for r in ts.g.lz(o.src)) and P._region(ts.target) in hd.rd
        assert P._region(ts.loss) in hd.wr and len(hd.wr) == 3
    return heads


def test_focal_alone(dry, emitted):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, focal=2.0, use_graph=False)
    assert ts.focal == 2.0 and ts.label_smoothing is None
    _check_heads(ts, 19, L.CE_SHAPE_FOCAL, 2.0)
    assert emitted == ['ce_upsample_shaped'] * 2
    assert all(o.binding['focal'] == 2.0 and 'smooth' not in o.binding for o in ts.outs)
    ts.g.run_parallel(ts.g.bwd, None)
    assert dry['ce_upsample_shaped'] == 2
    # the plain step's launch lists with the one name exchanged: same forward list, same backward names in the same order
    t0 = TrainStep(_add(4), SHAPE, use_graph=False)
    assert [c.name for c in ts.g.fwd] == [c.name for c in t0.g.fwd]
    assert [c.name.replace('ce_upsample_shaped', 'ce_upsample') for c in ts.g.bwd] == [c.name for c in t0.g.bwd]
    assert ts.g.nbytes == t0.g.nbytes and len(ts.g._bufs) == len(t0.g._bufs)


def test_focal_with_ohem(dry, emitted):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, focal=2.0, ohem=(0.7, 1000), use_graph=False)
    _check_heads(ts, 19, L.CE_SHAPE_FOCAL, 2.0, ohem=True)
    assert emitted == ['ohem_select', 'ce_upsample_shaped'] * 2
    t0 = TrainStep(_add(4), SHAPE, ohem=(0.7, 1000), use_graph=False)
    assert [c.name.replace('ce_upsample_shaped', 'ce_upsample_ohem') for c in ts.g.bwd] == [c.name for c in t0.g.bwd]
    assert len(ts.ohem_stats()) == 2


def test_focal_with_dice(dry, emitted):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, focal=2.0, dice=(0.5, 1.0), use_graph=False)
    _check_heads(ts, 19, L.CE_SHAPE_FOCAL, 2.0, dice=True)
    assert emitted == ['dice_stats', 'ce_upsample_shaped'] * 2
    t0 = TrainStep(_add(4), SHAPE, dice=(0.5, 1.0), use_graph=False)
    assert [c.name.replace('ce_upsample_shaped', 'ce_upsample_dice') for c in ts.g.bwd] == [c.name for c in t0.g.bwd]
    assert len(ts.dice_stats()) == 2


@pytest.mark.parametrize('ncls', [19, 21])
@pytest.mark.parametrize('kind', ['focal', 'label_smoothing'])
def test_with_ohem_dice_and_class_weights(dry, emitted, kind, ncls):
    from addk.train import TrainStep
    w = torch.rand(ncls) + 0.5
    kw = dict(focal=2.0) if kind == 'focal' else dict(label_smoothing=0.1)
    ts = TrainStep(_add(4, classes=ncls), SHAPE, ohem=(0.7, 1000), dice=(0.25, 1e-3), class_weight=w, use_graph=False, **kw)
    shape, value = (L.CE_SHAPE_FOCAL, 2.0) if kind == 'focal' else (L.CE_SHAPE_SMOOTH, 0.1)
    _check_heads(ts, ncls, shape, value, ohem=True, dice=True, weighted=True)
    assert emitted == ['ohem_select', 'dice_stats', 'ce_upsample_shaped'] * 2
    assert all(o.binding['dice_state']['coef'].numel() == 2 * ncls for o in ts.outs)


def test_label_smoothing_alone(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, label_smoothing=0.1, use_graph=False)
    assert ts.label_smoothing == 0.1 and ts.focal is None
    _check_heads(ts, 19, L.CE_SHAPE_SMOOTH, 0.1)
    assert all(o.binding['smooth'] == 0.1 and 'focal' not in o.binding for o in ts.outs)


def _fingerprint(name, **kw):
    """the fingerprint of tests/tools/plan_fingerprint.py for one of its train steps, built here with more keywords"""
    lib = addk.load()
    mode, fast = lib.addk_get_conv_precision(), lib.addk_get_fast_paths()
    build = {'train_step_ohem': dict(ohem=(0.7, 1000)), 'train_step_dice': dict(dice=(0.5, 1.0)), 'syncbn_forced_train_step': dict(sync=True)}[name]
    try:
        L.check(lib.addk_set_conv_precision(1), 'set_conv_precision')
        lib.addk_set_fast_paths(31)
        with dry_run():
            g, lists, extra, front = FP._train_step(4, SHAPE, **build, **kw)
            return FP._fingerprint(g, lists, extra, None, name + '/default')
    finally:
        lib.addk_set_conv_precision(mode)
        lib.addk_set_fast_paths(fast)


def test_without_the_arguments_the_plan_is_the_parents(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, use_graph=False)
    fwd, bwd = _names(ts)
    assert bwd['ce_upsample'] == 2 and bwd['ce_upsample_shaped'] == 0
    assert all('focal' not in o.binding and 'smooth' not in o.binding for o in ts.outs)
    assert ts.focal is None and ts.label_smoothing is None
    ts2 = TrainStep(_add(4), SHAPE, use_graph=False, focal=None, label_smoothing=None)
    assert [c.name for c in ts2.g.fwd] == [c.name for c in ts.g.fwd] and [c.name for c in ts2.g.bwd] == [c.name for c in ts.g.bwd]
    # the recorded fingerprints of the parent's plans (every command, stream, wait, region and argument byte), with the keywords at None
    with open(FP.OUT) as f:
        want = json.load(f)
    for name in ('train_step_ohem', 'train_step_dice', 'syncbn_forced_train_step'):
        got = _fingerprint(name, focal=None, label_smoothing=None)
        assert not FP.differences({name + '/default': got}, {name + '/default': want[name + '/default']}), name
    # and a shape does change it
    got = _fingerprint('train_step_ohem', focal=2.0)
    assert FP.differences({'x': got}, {'x': want['train_step_ohem/default']})


# ---- the refusals --------------------------------------------------------------------------------------------------------------------

def _refused(monkeypatch, match, **kw):
    from addk.train import TrainStep
    built = []
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: built.append(1))
    with pytest.raises(ValueError, match=match):
        TrainStep(_add(4), SHAPE, use_graph=False, **kw)
    assert not built


@pytest.mark.parametrize('focal', [0.999, 0.0, -2.0, float('nan'), float('inf'), float('-inf'), 1e39, 'a', (2.0,)])
def test_bad_gamma_raises_before_a_plan_is_built(dry, focal, monkeypatch):
    _refused(monkeypatch, 'focal', focal=focal)


@pytest.mark.parametrize('eps', [0.0, 1.0, -0.1, 1.5, float('nan'), float('inf'), 1e-50, 1.0 - 1e-9, 'a', (0.1,)])
def test_bad_eps_raises_before_a_plan_is_built(dry, eps, monkeypatch):
    _refused(monkeypatch, 'label_smoothing', label_smoothing=eps)


def test_the_fp32_word_decides(dry):
    """the checks read the fp32 word the library receives, as _check_dice does: 1 - 1e-9 is 1.0f, a gamma the library takes and an eps it
    refuses (above), 1e39 is inf and 1e-50 is 0 (above); a small eps that the word can hold is taken"""
    from addk.train import TrainStep
    assert TrainStep(_add(4), SHAPE, use_graph=False, focal=1).focal == 1.0
    assert TrainStep(_add(4), SHAPE, use_graph=False, focal=1.0 - 1e-9).focal == 1.0 - 1e-9
    assert TrainStep(_add(4), SHAPE, use_graph=False, label_smoothing=1e-30).label_smoothing == 1e-30


def test_both_shapes_or_a_shape_with_distill_raise(dry, monkeypatch):
    _refused(monkeypatch, 'one of them', focal=2.0, label_smoothing=0.1)
    _refused(monkeypatch, 'focal.*distill', focal=2.0, distill=(1.0, 4.0))
    _refused(monkeypatch, 'label_smoothing.*distill', label_smoothing=0.1, distill=(1.0, 4.0))
    _refused(monkeypatch, 'distill', label_smoothing=0.1, distill=(1.0, 4.0), ohem=(0.7, 1000), dice=(1.0, 1.0))


@pytest.mark.parametrize('kw', [dict(focal=2.0), dict(label_smoothing=0.1)], ids=['focal', 'label_smoothing'])
def test_unfused_head_or_unsupported_exit_raises(dry, monkeypatch, kw):
    from addk.train import TrainStep
    name = next(iter(kw))
    built = []
    real = P.Graph.finalize
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    monkeypatch.setenv('ADDK_FUSE_CE', '0')
    with pytest.raises(ValueError, match=name + ' needs the fused loss head'):
        TrainStep(_add(4), SHAPE, use_graph=False, **kw)
    monkeypatch.setenv('ADDK_FUSE_CE', '1')
    # an exit whose shape the fused head does not take: no materialised fallback
    lib = addk.load()
    monkeypatch.setattr(lib, 'addk_ce_upsample_supported', lambda *a: 0)
    with pytest.raises(ValueError, match=name + ': an exit of this model has no fused loss head'):
        TrainStep(_add(4), SHAPE, use_graph=False, **kw)
    assert not built
    TrainStep(_add(4), SHAPE, use_graph=False)                     # the plain step still takes the three-kernel form there
    assert built
