"""Host-logic tests (CPU, no GPU) of batched dynamic inference (addk.dynamic.BatchedGate): the live state its sub-plans hand over at
every cut, read off the launch lists' named regions; the launches of a forced scenario; the error paths; the C layout of the two
structs of addk_gather_rows.  Launches are stubbed as in tests/test_gate_plan.py; the arithmetic is checked in
tests/test_gpu_batched_gate.py and tests/test_gpu_rows.py."""
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
SHAPE = (4, 3, 129, 257)


def _add(F=20, arch=ARCH_C2):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(F), arch['low_level_layer']).eval()


def _buf_names(regions):
    return {r[0] for r in regions if r[0][0] == 'buf'}


def test_rows_struct_layouts_match_header():
    structs = {'addk_rows_item': L.RowsItem, 'addk_gather_rows_args': L.GatherRowsArgs}
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
    assert [f for f, _ in L.RowsItem._fields_] == ['src', 'dst', 'row_bytes']
    assert [f for f, _ in L.GatherRowsArgs._fields_] == ['items', 'nitems', 'src_row', 'dst_row', 'nrows']
    assert 'addk_gather_rows' in L.EXPORTED_SYMBOLS
    lib = addk.load()
    assert lib.addk_gather_rows(None, None) != 0                                                      # null struct: refused before any device call
    a = L.GatherRowsArgs()
    assert lib.addk_gather_rows(ctypes.byref(a), None) != 0                                           # null table
    a.items, a.nitems, a.nrows = 1, 0, 1
    assert lib.addk_gather_rows(ctypes.byref(a), None) != 0                                           # nitems < 1
    a.nitems, a.nrows = 1, 0
    assert lib.addk_gather_rows(ctypes.byref(a), None) != 0                                           # nrows < 1


@pytest.mark.parametrize('arch', ['c2', 'c3'])
def test_live_state_at_every_cut(dry, arch):
    """Batch 4, sub-plans 4..1: at every cut the per-image live sets pair up (count, geometry), every paired buffer is written before the
    cut and read behind it, and the replay set holds the input-independent producers (the eval-BN affine launch, the weight-pack launch
    where the plan has one) and no launch that depends on the image."""
    from addk.dynamic import BatchedGate, pair_live
    m = _add(20, ARCH_C2 if arch == 'c2' else ARCH_C3)
    bg = BatchedGate(m, SHAPE, 'entropy')
    assert bg.gates == (1 if arch == 'c2' else 2)
    plans = {n: bg.sub(n) for n in (4, 3, 2, 1)}
    assert all(bg.sub(n) is plans[n] for n in plans) and all(plans[n].batch == n for n in plans)
    assert all(tuple(plans[n]._conf_host.shape) == (2 * n,) for n in plans)                       # 2n gate words per sub-plan
    for k in range(bg.gates):
        counts = set()
        for n, p in plans.items():
            fwd, pos = p.g.fwd, p.head_rng[k][1]
            bufs, replay = p.live(pos)
            counts.add(len(bufs))
            written, read, touched = set(), set(), set()
            for c in fwd[:pos]:
                written |= _buf_names(c.wr)
            for c in fwd[pos:]:
                read |= _buf_names(c.rd)
                touched |= _buf_names(c.wr)          # (a conv names its hoisted weight pack as written, and reads it)
            levels = set()
            for b in bufs:
                assert b.region[0] in written and b.region[0] in read
                N, H, W, ld = b.geom
                assert N == n and b.n == n * H * W * ld
                levels.add((H, W))
            assert len(levels) >= 2                                                                # two resolution levels behind the cut
            assert p.in_name not in {b.region[0] for b in bufs}                                   # the staged image itself is dead by then
            # the replay set: parameters only
            names = [c.name for c in replay]
            before = [c.name for c in fwd[:pos]]
            assert names.count('bn_eval_affine_batch') == 1
            packs = set()                                   # the hoisted packs (one launch) serve the convs on both sides of the cut
            for c in fwd[:pos]:
                if c.name == 'conv_pack_batch':
                    packs |= _buf_names(c.wr)
            assert ('conv_pack_batch' in names) == bool(packs & (read | touched))
            assert 'conv_pack_batch' in before              # (this network has one: stem1's 3x3 convolution)
            assert 'nchw_to_nhwc' not in names
            dep = set(id(c) for c, d in zip(fwd, p.image_dep) if d)
            assert p.image_dep[0] and fwd[0].name == 'nchw_to_nhwc'
            assert not any(id(c) in dep for c in replay)
            assert all(id(c) in set(map(id, fwd[:pos])) for c in replay)
            # ... and it writes every input-independent plan buffer read behind the cut
            per_image = set()
            for c, d in zip(fwd[:pos], p.image_dep):
                if d:
                    per_image |= _buf_names(c.wr)
            rewritten = set()
            for c in replay:
                rewritten |= _buf_names(c.wr)
            assert (written & (read | touched)) - per_image <= rewritten
        assert len(counts) == 1
        for mm in (4, 3, 2):
            for n in range(1, mm):
                pairs = pair_live(plans[mm], plans[n], k)
                assert len(pairs) == counts.copy().pop()
                for x, y, words in pairs:
                    assert x.geom[1:] == y.geom[1:] and words == x.geom[1] * x.geom[2] * x.geom[3]
                    assert x.n == mm * words and y.n == n * words


def test_weight_packs_behind_the_cut_are_replayed(dry):
    """At 193 x 385 and batch >= 2 the decoder's 3x3 convolutions take the halo-patch kernel: their hoisted packs are written by the ONE
    `conv_pack_batch` launch in front of the cut, and the convs behind it name the packs under `wr` only.  A sub-plan entered behind the
    cut has to replay that launch (tests/test_gpu_batched_gate.py::test_weight_packs_behind_the_cut runs this shape)."""
    from addk.dynamic import BatchedGate
    bg = BatchedGate(_add(20, ARCH_C2), (3, 3, 193, 385), 'entropy')
    for n in (3, 2):
        p = bg.sub(n)
        pos = p.head_rng[0][1]
        replay = p.live(pos)[1]
        assert [c.name for c in replay] == ['bn_eval_affine_batch', 'conv_pack_batch']
        packs = _buf_names(replay[1].wr)
        users = [c for c in p.g.fwd[pos:] if _buf_names(c.wr) & packs]
        assert users and all(c.name == 'conv_fwd' for c in users) and not any(_buf_names(c.rd) & packs for c in p.g.fwd[pos:])
        assert not packs & {b.region[0] for b in p.live(pos)[0]}                                  # never copied


def test_pairing_refuses_other_geometry(dry):
    from addk.dynamic import BatchedGate, pair_live
    m = _add(20, ARCH_C2)
    bg = BatchedGate(m, SHAPE, 'entropy')
    p4, p2 = bg.sub(4), bg.sub(2)
    other = BatchedGate(m, (2, 3, 65, 129), 'entropy').sub(2)
    with pytest.raises(addk.AddkError):
        pair_live(p4, other, 0)
    b = p2.live(p2.head_rng[0][1])[0][0]
    saved, b.geom = b.geom, None
    try:
        with pytest.raises(addk.AddkError):
            pair_live(p4, p2, 0)
    finally:
        b.geom = saved
    assert len(pair_live(p4, p2, 0)) > 0


def test_forced_scenario_launches(dry, monkeypatch):
    """Rows 0 and 2 leave at gate 0 (their gate words are preset: the stubbed launches write none): one gather_rows for the state, one per
    label scatter, the tail on the batch-2 sub-plan only."""
    from addk.dynamic import BatchedGate
    monkeypatch.setenv('ADDK_GRAPH_INFER', '0')         # three calls: the third would capture a hipGraph
    m = _add(20, ARCH_C2)
    bg = BatchedGate(m, SHAPE, 'entropy')
    p4 = bg.sub(4)
    p4._conf_host[:] = torch.tensor([0.1, 0.0, 0.9, 0.0, 0.1, 0.0, 0.9, 0.0])
    dry.clear()
    labels, exits, values = bg.run(torch.randn(SHAPE), 0.5)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (4, 129, 257)
    assert exits.dtype == torch.int64 and exits.tolist() == [0, 1, 0, 1]
    assert values.dtype == torch.float32 and tuple(values.shape) == (4, 1)
    assert torch.allclose(values[:, 0], torch.tensor([0.1, 0.9, 0.1, 0.9]))
    assert dry['gather_rows'] == 3 and bg.counts['state'] == 1 and bg.counts['labels'] == 2
    cut, hend = p4.head_rng[0]
    n2 = len(bg.sub(2).g.fwd)
    assert bg.trace == [(4, 0, cut), (2, bg.sub(2).head_rng[0][1], n2)]
    assert bg.moves == [(4, 2, 0, [1, 3])]
    assert sorted(bg.subs) == [2, 4]                                                             # sub-plans 3 and 1 were never built
    assert dry['gate_label_upsample'] == 1 and dry['label_upsample'] == 1
    assert dry['nchw_to_nhwc'] == 1                                                              # the batch-2 plan did not stage an input
    assert dry['bn_eval_affine_batch'] == 2                                                      # ... but recomputed its affine table
    assert bg._idx.host[0].tolist() == [[0, 2, 0, 0], [0, 2, 0, 0], [1, 3, 0, 0]]
    assert bg._idx.host[1][1].tolist()[:2] == [1, 3]
    # nobody leaves: no state moves, one scatter (the final head's)
    p4._conf_host[:] = 0.9
    dry.clear()
    bg.counts.clear()
    _, exits, values = bg.run(torch.randn(SHAPE), 0.5)
    assert exits.tolist() == [1, 1, 1, 1] and dry['gather_rows'] == 1 and bg.counts['state'] == 0
    assert bg.trace == [(4, 0, cut), (4, hend, len(p4.g.fwd))] and bg.moves == []
    # everybody leaves: one scatter, nothing behind the gate
    p4._conf_host[:] = 0.1
    dry.clear()
    _, exits, values = bg.run(torch.randn(SHAPE), 0.5)
    assert exits.tolist() == [0, 0, 0, 0] and dry['gather_rows'] == 1 and bg.trace == [(4, 0, cut)]
    sizes = bg.nbytes
    assert sizes['total'] >= sizes[4] + sizes[2] and sizes[4] > sizes[2] > 0
    bg.close()
    assert not bg.subs and not bg.tables


def test_per_gate_thresholds_c3(dry):
    from addk.dynamic import BatchedGate
    m = _add(20, ARCH_C3)
    bg = BatchedGate(m, (3, 3, 129, 257), 'max')
    bg.sub(3)._conf_host[:] = torch.tensor([0.0, 0.9, 0.0, 0.2, 0.0, 0.3])              # shares: image 0 leaves at gate 0 (0.9 > 0.5)
    bg.sub(2)._conf_host[:] = torch.tensor([0.0, 0.5, 0.0, 0.1])                         # gate 1 at 0.4: the first survivor leaves
    labels, exits, values = bg.run(torch.randn(3, 3, 129, 257), [0.5, 0.4])
    assert exits.tolist() == [0, 1, 2]
    assert bg.moves == [(3, 2, 0, [1, 2]), (2, 1, 1, [1])]
    assert [t[0] for t in bg.trace] == [3, 2, 1]
    v = values.tolist()
    assert v[0][0] == pytest.approx(0.9) and v[0][1] != v[0][1]                          # NaN: gate 1 never saw image 0
    assert v[1] == pytest.approx([0.2, 0.5]) and v[2] == pytest.approx([0.3, 0.1])
    assert bg.counts['state'] == 2 and bg.counts['labels'] == 3
    with pytest.raises(ValueError):
        bg.run(torch.randn(3, 3, 129, 257), [0.5])
    with pytest.raises(ValueError):
        bg.run(torch.randn(3, 3, 129, 257), [0.5, 0.4, 0.3])


def test_errors(dry):
    from addk.dynamic import BatchedGate
    m = _add(4, ARCH_C2)
    x = torch.randn(2, 3, 65, 129)
    with pytest.raises(ValueError):
        BatchedGate(m, (2, 3, 65, 129), 'edm')
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(x, 0.5, confidence='edm')
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(x, 0.5, confidence='pool')
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(x, 0.5, label_lut=torch.zeros(255, dtype=torch.uint8))
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(x, 0.5, label_lut=torch.zeros(256, dtype=torch.int64))
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(torch.randn(0, 3, 65, 129), 0.5)
    with pytest.raises(ValueError):
        BatchedGate(m, (0, 3, 65, 129), 'entropy')
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(x, [0.5, 0.5])                                             # config 2 has one gate
    labels, exits, secs, values = m.dynamic_inference_batch(x, [0.5])
    assert tuple(labels.shape) == (2, 65, 129) and isinstance(secs, float) and tuple(values.shape) == (2, 1)
    key = [k for k in m._plans() if k[0] == 'dynb']
    assert len(key) == 1
    bg = m._plans()[key[0]]
    m.dynamic_inference_batch(x, 0.5)
    assert m._plans()[key[0]] is bg                                                            # cached by shape, kind and lut
    m.dynamic_inference_batch(x, 0.5, label_lut=torch.arange(256, dtype=torch.uint8))
    m.dynamic_inference_batch(x, 0.5, confidence='max')
    assert len([k for k in m._plans() if k[0] == 'dynb']) == 3


def test_single_image_path_still_refuses_a_batch(dry):
    from addk.modeling.ADD import EDM
    m = _add(4, ARCH_C2)
    for kind in ('entropy', 'max', 'edm'):
        for output in ('logits', 'labels'):
            with pytest.raises(RuntimeError):
                m.dynamic_inference(torch.randn(2, 3, 65, 129), 0.5, confidence=kind, edm=EDM().eval(), output=output)
    plan = m._gate_plan(torch.randn(1, 3, 65, 129), 'entropy', 'labels')
    assert tuple(plan._conf_host.shape) == (2,)                                                  # the single-image plans keep their words
