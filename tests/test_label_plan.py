"""Host-logic tests (CPU, no GPU) of label-map inference: the C ABI of the two label heads, the decode table, the launch plans of
dynamic inference with output='labels' (gated and 'edm'), the cold path for a class count the fused heads do not take, the static
Segmenter and the error paths.  Launches are stubbed as in tests/test_gate_plan.py; the arithmetic is tests/test_gpu_labels.py."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import addk
from addk import _lib as L
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (65, 129)
X = (1, 3) + HW


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer']).eval()


def _names(g, i0=0, i1=None):
    return [c.name for c in g.fwd[i0:i1]]


def _count(g):
    return collections.Counter(_names(g))


def _has_logits_buffer(g, classes=19, n=1):
    """a [N,C,OH,OW] tensor, or its NHWC form (dense or with the padded pixel stride), among what the plan owns"""
    px = n * HW[0] * HW[1]
    sizes = {px * classes, px * ((classes + 3) // 4 * 4)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    return any(b.n in sizes for b in g._bufs) or any(t.numel() in sizes for t in owned)


# ---------------- ABI and tables ----------------
FUNCS = ('addk_label_upsample_supported', 'addk_label_upsample', 'addk_gate_label_upsample')
STRUCTS = {'addk_label_upsample_args': 'LabelUpsampleArgs', 'addk_gate_label_upsample_args': 'GateLabelUpsampleArgs'}


def test_label_abi_declared_exported_and_bound():
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in FUNCS:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    for cname, pyname in STRUCTS.items():
        assert re.search(r'\}\s*%s\s*;' % cname, src), cname
        assert hasattr(L, pyname)
    # == addk_score_upsample_supported
    for args in ((2, 9, 17, 65, 129, 19), (1, 4, 4, 128, 128, 19), (2, 9, 17, 65, 129, 7), (2, 0, 17, 65, 129, 19),
                 (1, 8, 16, 65536 * 32 + 1, 1, 19)):
        assert lib.addk_label_upsample_supported(*args) == lib.addk_score_upsample_supported(*args), args
    assert lib.addk_label_upsample_supported(2, 9, 17, 65, 129, 19) == 1 and lib.addk_label_upsample_supported(2, 9, 17, 65, 129, 7) == 0


def test_label_struct_layouts_match_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    for cname, pyname in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in getattr(L, pyname)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['return 0;}']
    c, exe = tmp_path / 'abi.c', tmp_path / 'abi'
    c.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, pyname in STRUCTS.items():
        cls = getattr(L, pyname)
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    assert [f for f, _ in L.LabelUpsampleArgs._fields_] == ['logits', 'ld', 'N', 'H', 'W', 'C', 'OH', 'OW', 'lut256', 'labels']
    assert [f for f, _ in L.GateLabelUpsampleArgs._fields_] == ['gate', 'lut256', 'labels']
    assert dict(L.GateLabelUpsampleArgs._fields_)['gate'] is L.GateUpsampleArgs


def test_decode_segmap_lut_inverts_the_encoder():
    from addk.data import VALID_CLASSES, decode_segmap_lut, encode_segmap_lut
    dec, enc = decode_segmap_lut(), encode_segmap_lut()
    assert dec.dtype == np.uint8 and dec.shape == (256,)
    for v in VALID_CLASSES:
        assert dec[enc[v]] == v
    assert list(dec[:19]) == list(VALID_CLASSES)
    assert not dec[19:].any()


# ---------------- gated plans ----------------
@pytest.mark.parametrize('arch,gates', [(ARCH_C2, 1), (ARCH_C3, 2)])
def test_gate_plan_with_labels(dry, arch, gates):
    from addk.dynamic import GatePlan
    m = _add(4, arch)
    x = torch.randn(X)
    plan = GatePlan(m, x, 'entropy', output='labels')
    ref = GatePlan(m, x, 'entropy')
    g, n = plan.g, len(plan.g.fwd)
    assert len(plan.trunk_end) == len(plan.heads) == len(plan.head_rng) == gates
    pos = 0
    for k in range(gates):
        t, (cut, end) = plan.trunk_end[k], plan.head_rng[k]
        assert pos < t < cut == end < n                                  # nothing behind the cut
        head = _names(g, t, cut)
        assert head.count('gate_label_upsample') == 1 and head[-1] == 'gate_label_upsample'
        assert 'gate_label_upsample' not in _names(g, pos, t)
        assert plan.heads[k].gate_fused and plan.heads[k].gate_cut == cut
        pos = end
    rest = _names(g, pos, n)
    assert rest.count('label_upsample') == 1 and rest[-1] == 'label_upsample' and 'gate_label_upsample' not in rest
    names = _count(g)
    assert names['resize_nchw'] == 0 and names['gate_upsample'] == 0
    assert names['gate_label_upsample'] == gates and names['label_upsample'] == 1
    for h in plan.heads + [plan.final]:
        assert h.y.dtype == torch.uint8 and tuple(h.y.shape) == (1,) + HW and h.head == 'labels'
    assert not _has_logits_buffer(g)
    assert g.nbytes <= ref.g.nbytes - (gates + 1) * (19 * 4 - 1) * HW[0] * HW[1]
    # the plan without the mode, built next to it, is what it was
    assert _count(ref.g)['resize_nchw'] == gates + 1 and _count(ref.g)['gate_upsample'] == gates
    assert _count(ref.g)['label_upsample'] == _count(ref.g)['gate_label_upsample'] == 0
    assert all(tuple(h.y.shape) == (1, 19) + HW for h in ref.heads + [ref.final])
    # ... and the two share every other launch
    a, b = _count(g), _count(ref.g)
    for nm in ('resize_nchw', 'gate_upsample', 'label_upsample', 'gate_label_upsample'):
        a.pop(nm, None), b.pop(nm, None)
    assert a == b


def test_dynamic_plan_with_labels(dry):
    from addk.dynamic import DynamicPlan
    from addk.modeling.ADD import EDM
    m, edm = _add(20, ARCH_C2), EDM().eval()
    x = torch.randn(X)
    plan, ref = DynamicPlan(m, edm, x, output='labels'), DynamicPlan(m, edm, x)
    g = plan.g
    (h0, h1), = plan.head_rng
    assert _names(g, h0, h1)[-1] == 'label_upsample' and _names(g)[-1] == 'label_upsample'
    assert _count(g)['label_upsample'] == 2 and _count(g)['resize_nchw'] == 0 and _count(g)['gate_label_upsample'] == 0
    assert all(h.y.dtype == torch.uint8 and tuple(h.y.shape) == (1,) + HW for h in plan.heads + [plan.final])
    assert g.nbytes <= ref.g.nbytes - 2 * (19 * 4 - 1) * HW[0] * HW[1]
    # the EDM segment is unchanged
    assert plan.trunk_end == ref.trunk_end and plan.head_rng == ref.head_rng and plan.conf_fused == ref.conf_fused
    assert _names(g, 0, plan.trunk_end[0]) == _names(ref.g, 0, ref.trunk_end[0])
    assert _count(ref.g)['resize_nchw'] == 2 and _count(ref.g)['label_upsample'] == 0


def test_logits_and_labels_plans_coexist_in_the_cache(dry):
    from addk.data import decode_segmap_lut
    from addk.modeling.ADD import EDM
    m, edm = _add(20, ARCH_C2), EDM().eval()
    x = torch.randn(X)
    y, ex, sec, val = m.dynamic_inference(x, float('inf'), confidence='entropy', output='labels')
    assert ex == 1 and isinstance(val, float) and y.dtype == torch.uint8 and tuple(y.shape) == (1,) + HW
    assert dry['gate_label_upsample'] == 1 and dry['label_upsample'] == 0 and dry['resize_nchw'] == 0
    y, ex, sec, val = m.dynamic_inference(x, float('-inf'), confidence='entropy', output='labels')
    assert ex == 0 and y.dtype == torch.uint8 and tuple(y.shape) == (1,) + HW
    assert dry['gate_label_upsample'] == 2 and dry['label_upsample'] == 1 and dry['resize_nchw'] == 0
    y, ex, _, _ = m.dynamic_inference(x, float('inf'), confidence='entropy')
    assert tuple(y.shape) == (1, 19) + HW and dry['resize_nchw'] == 1 and dry['gate_upsample'] == 1
    key = m.dynamic_inference.__func__.__defaults__                      # (threshold, confidence, edm, output, label_lut)
    assert key == (1.0, 'edm', False, 'logits', None)
    lab, log = m._gate_plan(x, 'entropy', 'labels'), m._gate_plan(x, 'entropy')
    assert lab is not log and m._gate_plan(x, 'entropy', 'labels') is lab and m._gate_plan(x, 'entropy') is log
    assert _count(log.g)['resize_nchw'] == 2 and _count(lab.g)['resize_nchw'] == 0
    lut = decode_segmap_lut()
    m.dynamic_inference(x, 0.5, confidence='max', output='labels', label_lut=lut)
    withlut = m._gate_plan(x, 'max', 'labels', lut.tobytes())
    assert withlut is not m._gate_plan(x, 'max', 'labels') and withlut.g.lut.tolist() == lut.tolist()
    y, ex, _, conf = m.dynamic_inference(x, 1.0, confidence='edm', edm=edm, output='labels')
    assert y.dtype == torch.uint8 and m._dynamic_plan(x, edm, 'labels') is not m._dynamic_plan(x, edm)
    assert _count(m._dynamic_plan(x, edm).g)['resize_nchw'] == 2


def test_seven_classes_take_the_stand_alone_kernels(dry):
    from addk.dynamic import GatePlan
    from addk.segment import Segmenter
    m = _add(4, ARCH_C2, classes=7)
    plan = GatePlan(m, torch.randn(X), 'entropy', output='labels')
    names = _count(plan.g)
    assert names['resize_nchw'] == names['argmax_nchw'] == names['label_cast_torch'] == 2
    assert names['label_upsample'] == names['gate_label_upsample'] == names['gate_upsample'] == 0 and names['entropy_sum'] == 1
    t, (cut, end) = plan.trunk_end[0], plan.head_rng[0]
    assert _names(plan.g, t, cut)[-2:] == ['resize_nchw', 'entropy_sum'] and _names(plan.g, cut, end) == ['argmax_nchw', 'label_cast_torch']
    assert not plan.heads[0].gate_fused
    assert all(h.y.dtype == torch.uint8 and tuple(h.y.shape) == (1,) + HW for h in plan.heads + [plan.final])
    seg = Segmenter(m, X)
    assert _names(seg.g)[-3:] == ['resize_nchw', 'argmax_nchw', 'label_cast_torch'] and _count(seg.g)['label_upsample'] == 0


def test_gated_labels_with_the_fused_gate_off(dry, monkeypatch):
    monkeypatch.setenv('ADDK_FUSE_GATE', '0')
    from addk.dynamic import GatePlan
    plan = GatePlan(_add(4), torch.randn(X), 'max', output='labels')
    t, (cut, end) = plan.trunk_end[0], plan.head_rng[0]
    assert _names(plan.g, t, cut)[-2:] == ['resize_nchw', 'gate_count_torch']
    assert _names(plan.g, cut, end) == ['argmax_nchw', 'label_cast_torch']
    assert _names(plan.g)[-1] == 'label_upsample' and _count(plan.g)['gate_label_upsample'] == 0


# ---------------- Segmenter ----------------
def test_segmenter_emits_the_trunk_only_up_to_its_exit(dry):
    from addk.segment import Segmenter
    m = _add(4).train()
    first, last = Segmenter(m, (2, 3) + HW, exit=0), Segmenter(m, (2, 3) + HW, exit=-1)
    assert last.exit == 1 and Segmenter(m, (2, 3) + HW, exit=1).exit == 1
    for s in (first, last):
        names = _count(s.g)
        assert names['label_upsample'] == 1 and names['resize_nchw'] == 0 and _names(s.g)[-1] == 'label_upsample'
        assert names['bn_eval_affine_batch'] == 1 and names['bn_finalize'] == 0      # inference form
        assert not s.g.bwd and not _has_logits_buffer(s.g, n=2)
        assert s.out.y.dtype == torch.uint8 and tuple(s.out.y.shape) == (2,) + HW
    assert len(first.g.fwd) < len(last.g.fwd)
    c0 = m.C_index[0]
    behind = {id(p) for cell in list(m.cells)[c0 + 1:] for p in cell.parameters()}
    upto = {id(p) for cell in list(m.cells)[:c0 + 1] for p in cell.parameters()}
    touched = {id(p) for p in first.g.params}
    assert not (touched & behind) and (touched & upto)
    assert {id(p) for p in last.g.params} & behind
    assert m.training                                                                # the model's mode is not touched
    y = first.step(torch.randn((2, 3) + HW))
    assert y is first.out.y and dry['label_upsample'] == 1


def test_segmenter_rebuilds_when_the_parameters_move(dry):
    from addk.segment import Segmenter
    m = _add(4)
    seg = Segmenter(m, (2, 3) + HW)
    g0 = seg.g
    seg.step()
    assert seg.g is g0
    p = next(m.parameters())
    p.data = p.data.clone()
    seg.step()
    assert seg.g is not g0 and seg.calls == 1
    # after a capture: the rebuild drops the captured graph with the plan it replayed and starts the eager calls again
    seg = Segmenter(m, (2, 3) + HW, use_graph=True)
    g0, seg.graph, seg.calls = seg.g, object(), 7
    p.data = p.data.clone()
    seg.step()
    assert seg.g is not g0 and seg.graph is None and seg.calls == 1


# ---------------- error paths ----------------
def test_errors(dry):
    from addk.dynamic import DynamicPlan, GatePlan
    from addk.modeling.ADD import EDM
    from addk.modeling.baseline_model import Baselin_Model
    from addk.segment import Segmenter
    from _util import GENOTYPE_BASELINE_2, NETWORK_PATH_BASELINE
    m, x = _add(4), torch.randn(X)
    for kind in ('edm', 'entropy', 'max'):
        with pytest.raises(ValueError):
            m.dynamic_inference(x, 0.5, confidence=kind, edm=EDM().eval(), output='probabilities')
        for bad in (np.zeros(255, np.uint8), np.zeros(256, np.int64), torch.zeros((2, 256), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                m.dynamic_inference(x, 0.5, confidence=kind, edm=EDM().eval(), output='labels', label_lut=bad)
    with pytest.raises(ValueError):
        GatePlan(m, x, 'entropy', output='map')
    with pytest.raises(ValueError):
        DynamicPlan(m, EDM().eval(), x, output='map')
    with pytest.raises(ValueError):
        Segmenter(m, X, label_lut=np.zeros(19, np.uint8))
    with pytest.raises(TypeError):
        Segmenter(Baselin_Model(NETWORK_PATH_BASELINE, [5], GENOTYPE_BASELINE_2, 19, make_args(4), 1), X)
    with pytest.raises(TypeError):
        Segmenter(torch.nn.Conv2d(3, 19, 1), X)
    for bad in (2, -3):
        with pytest.raises(IndexError):
            Segmenter(m, X, exit=bad)
