"""Host-logic tests (CPU, no GPU) of the fused logits heads at 21 classes (Pascal VOC, the reference's second dataset): the library names
the class counts each group of heads is compiled for, and the training step and the Segmenter build at 21 classes the plans they build
at 19.  Launches are stubbed as in the other *_plan.py files; the
arithmetic is tests/test_gpu_heads21.py."""
import collections
import ctypes

import pytest
import torch

import addk
from addk import _lib as L
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

HW = (33, 65)
X1, X2 = (1, 3) + HW, (2, 3) + HW
C21 = 21


def _add(classes=C21, F=4, arch=ARCH_C2):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer'])


def _count(cmds):
    return collections.Counter(c.name for c in cmds)


def _has_logits_buffer(g, n, classes=C21):
    """a [N,C,OH,OW] tensor, or its NHWC form (dense or with the padded pixel stride), among what the plan owns (tests/test_label_plan.py)"""
    px = n * HW[0] * HW[1]
    sizes = {px * classes, px * ((classes + 3) // 4 * 4)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    return any(b.n in sizes for b in g._bufs) or any(t.numel() in sizes for t in owned)


# ---------------- the class-count lists ----------------
def test_the_library_names_its_class_counts():
    lib = addk.load()
    assert lib.addk_head_classes(None, 0) == 2 and lib.addk_gate_head_classes(None, 0) >= 1
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    assert lib.addk_head_classes(out, 1) == 2 and list(out) == [19, -1, -1, -1]            # never beyond cap
    assert lib.addk_head_classes(out, 4) == 2 and set(out[:2]) == {19, 21} and list(out[2:]) == [-1, -1]
    assert set(L.head_classes()) == {19, 21} and 19 in L.gate_head_classes() and set(L.gate_head_classes()) <= set(L.head_classes())
    assert 'addk_head_classes' in L.EXPORTED_SYMBOLS and 'addk_gate_head_classes' in L.EXPORTED_SYMBOLS
    assert all('%d' % c in L.head_classes_text() for c in L.head_classes()) and L.head_classes_text().startswith('19 classes')
    assert L.gate_head_classes_text().startswith('19 classes')


def _supported(lib, C_):
    """(the training and label heads, the scoring / profile / calibration / gate / multi-view heads) at C_ classes"""
    shape = (2, 9, 17, 65, 129)                                                           # N, H, W, OH, OW
    head = {
        'ce_upsample': lib.addk_ce_upsample_supported(*shape, C_),
        'ce_upsample_kd': lib.addk_ce_upsample_kd_supported(*shape, C_),
        'ohem_select': lib.addk_ohem_select_supported(*shape, C_),
        'dice_stats': lib.addk_dice_stats_supported(*shape, C_),
        'label_upsample': lib.addk_label_upsample_supported(*shape, C_),
    }
    gate = {
        'score_upsample': lib.addk_score_upsample_supported(*shape, C_),
        'profile_upsample': lib.addk_profile_upsample_supported(*shape, C_, 4),
        'calib_upsample': lib.addk_calib_upsample_supported(*shape, C_, 3),
        'gate_upsample': lib.addk_gate_upsample_supported(*shape, C_),
        'label_views_upsample': lib.addk_label_views_upsample_supported(3, 2, 65, 129, C_),
    }
    return head, gate


def test_every_head_takes_the_counts_of_its_list():
    lib = addk.load()
    for c in (19, 21, 7, 20, 22):
        head, gate = _supported(lib, c)
        assert set(head.values()) == {1 if c in (19, 21) else 0}, (c, head)
        assert set(gate.values()) == {1 if c in L.gate_head_classes() else 0}, (c, gate)      # 19; never 7, 20 or 22
    assert not {7, 20, 22} & set(L.gate_head_classes())
    assert lib.addk_dice_stats_ws_bytes_classes(2, 65, 129, 21) == 4 * (96 + 42 * 2 * 3 * 3)
    assert lib.addk_dice_stats_ws_bytes_classes(2, 65, 129, 19) == lib.addk_dice_stats_ws_bytes(2, 65, 129)
    assert lib.addk_dice_stats_ws_bytes_classes(2, 65, 129, 20) == 0


# ---------------- training ----------------
def test_train_step_has_the_fused_head(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(), X2, use_graph=False)
    assert len(ts.outs) == 2 and all(o.head == 'ce' for o in ts.outs)
    fwd, bwd = _count(ts.g.fwd), _count(ts.g.bwd)
    assert bwd['ce_upsample'] == 2 and (fwd + bwd)['resize_nchw'] == 0 and (fwd + bwd)['ce_fwd_bwd'] == 0
    assert not _has_logits_buffer(ts.g, 2)
    for o in ts.outs:
        # the plan pads the classifier's pixels to 24 floats on a 16-byte-aligned base: the heads' 16-byte loads (px_vec_ok)
        s = ts.g.src(o.src)
        assert (o.src.C, s.ld) == (21, 24) and s.x % 16 == 0


def test_train_step_with_every_term(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(), X2, use_graph=False, ohem=(0.7, 100), dice=(0.5, 1.0), distill=(0.5, 2.0))
    fwd, bwd = _count(ts.g.fwd), _count(ts.g.bwd)
    assert bwd['ohem_select'] == 2 and bwd['dice_stats'] == 2 and bwd['ce_upsample_dice'] == 2
    assert (fwd + bwd)['resize_nchw'] == 0 and (fwd + bwd)['ce_fwd_bwd'] == 0
    student = ts.outs[0].binding
    assert student['dice_state']['coef'].numel() == 42 and student['dice_state']['dice'].numel() == 22
    assert 'distill_state' in student and 'distill_state' not in ts.outs[-1].binding
    heads = [c.args[0]._obj for c in ts.g.bwd if c.name == 'ce_upsample_dice']
    assert all(h.kd.ce.C == 21 for h in heads) and sum(1 for h in heads if h.kd.teacher) == 1
    stats = [c.args[0]._obj for c in ts.g.bwd if c.name == 'dice_stats']
    assert all(s.C == 21 and s.ws for s in stats)


# ---------------- label maps ----------------
def test_segmenter_has_the_label_head(dry):
    from addk.segment import Segmenter
    seg = Segmenter(_add().eval(), X2)
    names = _count(seg.g.fwd)
    assert [c.name for c in seg.g.fwd][-1] == 'label_upsample' and names['argmax_nchw'] == 0 and names['resize_nchw'] == 0
    assert not _has_logits_buffer(seg.g, 2) and seg.out.y.dtype == torch.uint8 and tuple(seg.out.y.shape) == (2,) + HW
    a = [c for c in seg.g.fwd if c.name == 'label_upsample'][0].args[0]._obj
    assert (a.C, a.ld) == (21, 24) and a.logits % 16 == 0


def test_dynamic_inference_labels_final_exit_has_the_label_head(dry):
    from addk.dynamic import GatePlan
    plan = GatePlan(_add().eval(), torch.randn(X1), 'entropy', output='labels')
    names = _count(plan.g.fwd)
    assert names['label_upsample'] == 1 and [c.name for c in plan.g.fwd][-1] == 'label_upsample'
    assert tuple(plan.final.y.shape) == (1,) + HW and plan.final.y.dtype == torch.uint8


# ---------------- refusals ----------------
def test_refusals_name_the_counts_of_the_library(dry):
    """a count in neither list (7): the messages carry the words the library's lists give"""
    from addk.segment import MultiViewSegmenter
    from addk.train import TrainStep
    with pytest.raises(addk.AddkError) as e:
        MultiViewSegmenter(_add(7).eval(), X1, scales=(1.0,))
    assert L.gate_head_classes_text() in str(e.value)
    with pytest.raises(ValueError) as e:
        TrainStep(_add(7), X2, use_graph=False, dice=(0.5, 1.0))
    assert L.head_classes_text() in str(e.value) and '(or 21)' in str(e.value)
