"""Host-logic tests (CPU, no GPU) of multi-scale + flip label maps: the C ABI of the multi-view label head, the launch plan of
segment.MultiViewSegmenter (one `label_views_upsample`, no full-resolution logits), its rebuild and its error paths, and the fp32-against-
fp64 check of the torch formula that tests/test_gpu_views.py holds the kernel to.  Launches are stubbed as in tests/test_label_plan.py.

The reference check (tests/_views_ref.py): on the four kernel-test cases with N(0, 3^2) logits the fp32 formula differs from the fp64 one
by e32 = 9.4e-8 (three_scales), 6.3e-7 (odd), 5.3e-7 (down_one), 1.8e-5 (eight: its weights sum to 18).  tau = 64 * e32, per case (6.0e-6,
4.0e-5, 3.4e-5, 1.1e-3: the reason is in tests/_views_ref.py), excuses 0.006 %, 0.08 %, 0 and 0.04 % of the pixels, within the cap of
0.2 %, and fp32's arg-max equals fp64's on every other pixel."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import addk
import addk.plan as P
from addk import _lib as L
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)
import _views_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HW = 2, (64, 128)
X = (N, 3) + HW


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer']).eval()


def _names(g):
    return [c.name for c in g.fwd]


# ---------------- ABI ----------------
def test_views_abi_declared_exported_and_bound():
    lib = addk.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'addk.h')).read(), flags=re.S)
    for name in ('addk_label_views_upsample_supported', 'addk_label_views_upsample'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert int(re.search(r'#define ADDK_MAX_VIEWS (\d+)', src).group(1)) == L.MAX_VIEWS == 8
    # (nview, N, OH, OW, C)
    assert lib.addk_label_views_upsample_supported(6, 2, 64, 128, 19) == 1
    assert lib.addk_label_views_upsample_supported(1, 1, 5, 5, 19) == 1 and lib.addk_label_views_upsample_supported(8, 1, 40, 70, 19) == 1
    assert lib.addk_label_views_upsample_supported(6, 2, 64, 128, 21) == 0
    assert lib.addk_label_views_upsample_supported(0, 2, 64, 128, 19) == 0
    assert lib.addk_label_views_upsample_supported(9, 2, 64, 128, 19) == 0
    assert lib.addk_label_views_upsample_supported(2, 0, 64, 128, 19) == 0 and lib.addk_label_views_upsample_supported(2, 2, 64, 0, 19) == 0
    assert lib.addk_label_views_upsample_supported(2, 65536, 64, 128, 19) == 0          # grid limits
    assert lib.addk_label_views_upsample_supported(2, 1, 65536 * 16 + 1, 1, 19) == 0
    # refused before anything is launched: needs no device
    assert lib.addk_label_views_upsample(ctypes.byref(L.LabelViewsArgs()), None) == -1
    assert lib.addk_label_views_upsample(None, None) == -1


def test_views_struct_layouts_match_header(tmp_path):
    structs = {'addk_view': 'View', 'addk_label_views_args': 'LabelViewsArgs'}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    for cname, pyname in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in getattr(L, pyname)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['return 0;}']
    c, exe = tmp_path / 'abi.c', tmp_path / 'abi'
    c.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, pyname in structs.items():
        cls = getattr(L, pyname)
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    assert [f for f, _ in L.View._fields_] == ['logits', 'ld', 'n0', 'H', 'W', 'mirror', 'weight']
    assert [f for f, _ in L.LabelViewsArgs._fields_] == ['view', 'nview', 'N', 'C', 'OH', 'OW', 'lut256', 'labels']
    assert dict(L.LabelViewsArgs._fields_)['view']._type_ is L.View and dict(L.LabelViewsArgs._fields_)['view']._length_ == 8


# ---------------- plan structure ----------------
def _launch_args(g):
    """the argument struct of the plan's one label_views_upsample launch"""
    cmds = [c for c in g.fwd if c.name == 'label_views_upsample']
    assert len(cmds) == 1
    return cmds[0], cmds[0].args[0]._obj


def test_three_scales_with_flip_end_in_one_launch(dry):
    from addk.segment import MultiViewSegmenter
    m = _add(4).train()
    seg = MultiViewSegmenter(m, X, scales=(0.75, 1.0, 1.25), flip=True)
    g, names = seg.g, collections.Counter(_names(seg.g))
    assert names['label_views_upsample'] == 1 and _names(g)[-1] == 'label_views_upsample'
    assert names['resize_nchw'] == names['label_upsample'] == names['argmax_nchw'] == 0
    assert names['nchw_to_nhwc'] == 1 and names['bn_eval_affine_batch'] == 1 and names['bn_finalize'] == 0     # one staged input; inference form
    assert not g.bwd and m.training
    # the six views, in kernel order
    assert [(s, mir, hw) for s, mir, hw, _ in seg.views] == [(0.75, False, (48, 96)), (0.75, True, (48, 96)), (1.0, False, (64, 128)),
                                                              (1.0, True, (64, 128)), (1.25, False, (80, 160)), (1.25, True, (80, 160))]
    cmd, a = _launch_args(g)
    assert (a.nview, a.N, a.C, a.OH, a.OW) == (6, N, 19, 64, 128) and a.labels == g.view_labels.data_ptr() and not a.lut256
    for i, (s, mir, hw, low) in enumerate(seg.views):
        v, src = a.view[i], seg.outs[i // 2].src.raw
        assert (v.H, v.W) == low == (src.H, src.W) and v.mirror == int(mir) and v.n0 == (N if mir else 0)
        assert v.logits == src.ptr and v.ld == src.ld and src.N == 2 * N and abs(v.weight - 1 / 6) < 1e-7
        assert low[0] < hw[0] and low[1] < hw[1]                               # the decoder's grid, not the view's size
    # the launch reads every view's source and writes the map
    assert all(P._region(o.src.raw) in cmd.rd for o in seg.outs) and cmd.wr == [P._region(g.view_labels)]
    assert all(o.y is None and o.head == 'views' for o in seg.outs)
    assert [tuple(o.shape) for o in seg.outs] == [(2 * N, 19, 48, 96), (2 * N, 19, 64, 128), (2 * N, 19, 80, 160)]
    # no [.,19,.,.] tensor of any view at its own or at the output size, in either layout
    sizes = {n * h * w * c for n in (N, 2 * N) for (h, w) in [HW] + [hw for _, _, hw, _ in seg.views] for c in (19, 20)}
    owned = [t for t in g.keep if isinstance(t, torch.Tensor)]
    assert not any(b.n in sizes for b in g._bufs) and not any(t.numel() in sizes for t in owned)
    assert tuple(seg.x.shape) == (2 * N, 3) + HW and tuple(g.view_labels.shape) == (N,) + HW and g.view_labels.dtype == torch.uint8
    # step: the images and their mirror are loaded, one replay, the plan-owned map comes back
    img = torch.randn(X)
    y = seg.step(img)
    assert y is g.view_labels and dry['label_views_upsample'] == 1
    assert torch.equal(seg.x[:N], img) and torch.equal(seg.x[N:], img.flip(3))
    logits = seg.view_logits()
    assert [tuple(t.shape) for t in logits] == [(N,) + low + (19,) for _, _, _, low in seg.views]


def test_without_flip_and_with_weights_and_lut(dry):
    from addk.data import decode_segmap_lut
    from addk.segment import MultiViewSegmenter
    seg = MultiViewSegmenter(_add(4), X, scales=(1.0, 0.5), flip=False, weights=(3, 1), label_lut=decode_segmap_lut())
    assert tuple(seg.x.shape) == X and [(s, mir, hw) for s, mir, hw, _ in seg.views] == [(1.0, False, (64, 128)), (0.5, False, (32, 64))]
    cmd, a = _launch_args(seg.g)
    assert a.nview == 2 and [a.view[i].n0 for i in range(2)] == [0, 0] and [a.view[i].weight for i in range(2)] == [3.0, 1.0]
    assert a.lut256 == seg.g.lut.data_ptr() and seg.g.lut.tolist() == decode_segmap_lut().tolist()
    names = collections.Counter(_names(seg.g))
    assert names['label_views_upsample'] == 1 and names['resize_nchw'] == 0
    # default scales: three scales with flip
    assert len(MultiViewSegmenter(_add(4), X).views) == 6


def test_exit_zero_emits_no_cell_behind_the_first_exit(dry):
    from addk.segment import MultiViewSegmenter
    m = _add(4)
    first, last = MultiViewSegmenter(m, X, exit=0), MultiViewSegmenter(m, X, exit=-1)
    assert first.exit == 0 and last.exit == 1 and len(first.g.fwd) < len(last.g.fwd)
    c0 = m.C_index[0]
    behind = {id(p) for cell in list(m.cells)[c0 + 1:] for p in cell.parameters()}
    upto = {id(p) for cell in list(m.cells)[:c0 + 1] for p in cell.parameters()}
    touched = {id(p) for p in first.g.params}
    assert not (touched & behind) and (touched & upto)
    assert {id(p) for p in last.g.params} & behind
    for s in (first, last):
        assert collections.Counter(_names(s.g))['label_views_upsample'] == 1 and _names(s.g)[-1] == 'label_views_upsample'


def test_rebuilds_when_the_parameters_move(dry):
    from addk.segment import MultiViewSegmenter
    m = _add(4)
    seg = MultiViewSegmenter(m, X, scales=(1.0,))
    g0 = seg.g
    seg.step()
    assert seg.g is g0
    p = next(m.parameters())
    p.data = p.data.clone()
    y = seg.step()
    assert seg.g is not g0 and seg.calls == 1 and y is seg.g.view_labels and len(seg.views) == 2
    seg = MultiViewSegmenter(m, X, scales=(1.0,), use_graph=True)
    g0, seg.graph, seg.calls = seg.g, object(), 7
    p.data = p.data.clone()
    seg.step()
    assert seg.g is not g0 and seg.graph is None and seg.calls == 1


# ---------------- error paths ----------------
def test_errors(dry, monkeypatch):
    from addk.modeling.baseline_model import Baselin_Model
    from addk.segment import MultiViewSegmenter
    from _util import GENOTYPE_BASELINE_2, NETWORK_PATH_BASELINE
    m = _add(4)
    built = []
    monkeypatch.setattr(MultiViewSegmenter, '_build', lambda self: built.append(self))
    with pytest.raises(TypeError):
        MultiViewSegmenter(Baselin_Model(NETWORK_PATH_BASELINE, [5], GENOTYPE_BASELINE_2, 19, make_args(4), 1), X)
    with pytest.raises(TypeError):
        MultiViewSegmenter(torch.nn.Conv2d(3, 19, 1), X)
    for kw in (dict(scales=()), dict(scales=(1.0, 0.0)), dict(scales=(-0.5,)), dict(scales=(float('nan'),)),
               dict(scales=(0.5, 0.75, 1.0, 1.25, 1.5), flip=True),            # ten views
               dict(scales=tuple(0.5 + 0.1 * i for i in range(9)), flip=False),  # nine
               dict(scales=(0.75, 1.0), flip=True, weights=(1, 1, 1)), dict(scales=(1.0,), flip=False, weights=()),
               dict(scales=(1.0,), weights=(1.0, 0.0)), dict(scales=(1.0,), weights=(1.0, float('inf'))),
               dict(label_lut=np.zeros(19, np.uint8))):
        with pytest.raises(ValueError):
            MultiViewSegmenter(m, X, **kw)
    with pytest.raises(ValueError, match='scale 0.001.*0x0'):                  # a view the plan cannot build, named
        MultiViewSegmenter(m, X, scales=(1.0, 0.001))
    with pytest.raises(ValueError, match='scale 600'):
        MultiViewSegmenter(m, X, scales=(600.0,))
    for bad in (2, -3):
        with pytest.raises(IndexError):
            MultiViewSegmenter(m, X, exit=bad)
    assert not built                                                           # every error came before any plan was built
    MultiViewSegmenter(m, X, scales=(0.5, 0.75, 1.0, 1.25), flip=True)         # eight views are taken
    assert len(built) == 1


def test_seven_classes_and_nine_views_raise_addk_error(dry):
    from addk.segment import MultiViewSegmenter
    with pytest.raises(addk.AddkError, match='19 classes'):
        MultiViewSegmenter(_add(4, classes=7), X, scales=(1.0,))
    # the plan's own limit, behind the front end's: nine views bound to one output
    m = _add(4)
    seg = MultiViewSegmenter(m, X, scales=(1.0,), flip=False)

    def nine(g, a):
        out = m._emit_exit(g, a, seg.exit)
        out.binding = {'N': N, 'size': HW, 'views': [(0, 0, 1.0)] * 9}
        seg.outs = [out]
    seg._emit = nine
    with pytest.raises(addk.AddkError, match='views'):
        seg._build()


# ---------------- the reference the kernel test uses ----------------
def test_reference_fp32_agrees_with_fp64():
    seen = {}
    for case, (n, _, size) in R.CASES.items():
        a64, want, excused, e32, tau = R.reference(case)
        a32 = R.formula(R.views(case), n, size, torch.float32)
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and tuple(a64.shape) == (n, 19) + size
        assert e32 == float((a32.double() - a64).abs().max()) and tau == 64 * e32
        assert len(want.unique()) > 4
        print('%s: e32 = %.2e, tau = %.2e' % (case, e32, tau))
        R.check_map(a32.argmax(1).to(torch.uint8), want, excused, case)      # the cap, and no other pixel differs
        seen[case] = e32
    # fp32-sized (the largest sum of weights is 18, an ulp there 1.9e-6), and largest where the weights are
    assert all(0 < e < 1e-4 for e in seen.values()), seen
    assert max(seen.values()) == seen['eight']
    # the weights of a case are what the issue says: 1/nview, and 0.5 ... 4 for `eight`
    assert [v[3] for v in R.views('eight')] == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    assert [v[1:3] for v in R.views('three_scales')] == [(0, 0), (2, 1)] * 3 and R.views('down_one')[0][1:] == (0, 1, 1.0)
