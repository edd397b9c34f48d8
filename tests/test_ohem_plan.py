"""Host-logic tests of hard example mining in the training step (CPU, no GPU): train.TrainStep(ohem=...) is built with the kernel launches
stubbed out (the `dry` pattern of tests/test_plan_dryrun.py) and the launch list is inspected, plus the C ABI of the two entry points.
Arithmetic is tests/test_gpu_ohem.py."""
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


def test_struct_layouts_match_header():
    structs = {'addk_ohem_select_args': L.OhemSelectArgs, 'addk_ce_upsample_ohem_args': L.CeUpsampleOhemArgs}
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
    assert L.CeUpsampleOhemArgs.ce.offset == 0 and ctypes.sizeof(L.CeUpsampleOhemArgs) == ctypes.sizeof(L.CeUpsampleArgs) + 16


def test_host_side_queries():
    lib = addk.load()
    assert lib.addk_ohem_select_supported(2, 17, 33, 65, 129, 19) == 1
    assert lib.addk_ohem_select_supported(2, 17, 33, 65, 129, 7) == 0 and lib.addk_ohem_select_supported(0, 17, 33, 65, 129, 19) == 0
    assert lib.addk_ohem_select_supported(8, 128, 256, 16384, 16384, 19) == 0          # 2^31 pixels: the 32-bit histogram counters
    assert lib.addk_ohem_select_ws_bytes(2, 65, 129) >= 4 * (2048 + 2048 + 1024) and lib.addk_ohem_select_ws_bytes(0, 65, 129) == 0
    # null argument blocks are refused on the host, before any launch
    assert lib.addk_ohem_select(None, None) == -1 and lib.addk_ce_upsample_ohem_fwd_bwd(None, None) == -1


def test_train_step_with_ohem_has_one_select_and_one_mining_head_per_exit(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, ohem=(0.7, 1000), use_graph=False)
    names = collections.Counter(c.name for c in ts.g.bwd)
    allnames = names + collections.Counter(c.name for c in ts.g.fwd)
    assert len(ts.outs) == 2 and names['ohem_select'] == 2 and names['ce_upsample_ohem'] == 2
    assert allnames['ce_upsample'] == 0 and allnames['resize_nchw'] == 0 and allnames['resize_nchw_bwd'] == 0 and allnames['ce_count'] == 0
    assert all(o.y is None and o.head == 'ce' and tuple(o.shape) == (2, 19, 65, 129) for o in ts.outs)
    assert not _has_full_resolution_buffer(ts.g, (2, 19, 65, 129))
    # the parameters reach each exit's argument block: thresh as given, K = min_kept * N; every exit owns its map, tau and sums
    sel = [c.args[0]._obj for c in ts.g.bwd if c.name == 'ohem_select']
    head = [c.args[0]._obj for c in ts.g.bwd if c.name == 'ce_upsample_ohem']
    for s in sel:
        assert abs(s.thresh - 0.7) < 1e-7 and s.min_kept_total == 2000 and (s.N, s.C, s.OH, s.OW) == (2, 19, 65, 129)
    assert len({s.pix_loss for s in sel}) == len({s.tau for s in sel}) == len({s.wsum_kept for s in sel}) == len({s.ws for s in sel}) == 2
    for s in sel:
        h = [b for b in head if b.pix_loss == s.pix_loss]
        assert len(h) == 1 and h[0].tau == s.tau and h[0].ce.wsum == s.wsum_kept and h[0].ce.logits == s.logits and h[0].ce.target == s.target
    # the hazard tracker orders each head after its own select, and only after its own
    order = [c.name for c in ts.g.bwd]
    deps = list(P.deps(ts.g.bwd))
    for i, c in enumerate(ts.g.bwd):
        if c.name == 'ce_upsample_ohem':
            mine = [j for j in deps[i] if ts.g.bwd[j].name == 'ohem_select']
            assert len(mine) == 1 and ts.g.bwd[mine[0]].args[0]._obj.pix_loss == c.args[0]._obj.pix_loss and mine[0] < i
        if c.name == 'ohem_select':
            assert not [j for j in deps[i] if ts.g.bwd[j].name in ('ohem_select', 'ce_upsample_ohem')]
    assert order.index('ohem_select') < order.index('ce_upsample_ohem')
    ts.g.run_parallel(ts.g.bwd, None)
    assert dry['ohem_select'] == 2 and dry['ce_upsample_ohem'] == 2
    assert ts.ohem_stats() == [(0.0, 0, 0), (0.0, 0, 0)]            # nothing ran: the zero-initialised words


def test_without_ohem_the_plan_is_the_parents(dry):
    from addk.train import TrainStep
    ts = TrainStep(_add(4), SHAPE, use_graph=False)
    bwd = collections.Counter(c.name for c in ts.g.bwd)
    fwd = collections.Counter(c.name for c in ts.g.fwd)
    assert bwd['ce_upsample'] == 2 and bwd['ohem_select'] == 0 and bwd['ce_upsample_ohem'] == 0 and fwd['ce_count'] == 1
    assert all('ohem' not in o.binding for o in ts.outs)
    with pytest.raises(ValueError):
        ts.ohem_stats()
    # command for command the names of a step that has the parameter at its default
    ts2 = TrainStep(_add(4), SHAPE, use_graph=False, ohem=None)
    assert [c.name for c in ts2.g.fwd] == [c.name for c in ts.g.fwd] and [c.name for c in ts2.g.bwd] == [c.name for c in ts.g.bwd]
    # and a mining step differs from it in the loss heads and the target count only
    ts3 = TrainStep(_add(4), SHAPE, use_graph=False, ohem=(0.7, 1000))
    strip = lambda lst: sorted(c.name for c in lst if c.name not in ('ce_upsample', 'ohem_select', 'ce_upsample_ohem', 'ce_count'))   # noqa: E731
    assert strip(ts3.g.fwd) == strip(ts.g.fwd) and strip(ts3.g.bwd) == strip(ts.g.bwd)


@pytest.mark.parametrize('ohem', [(0.0, 1000), (1.5, 1000), (-0.1, 1000), (float('nan'), 1000), (0.7, 0), (0.7, -5), (0.7, 10.5), (0.7,), 0.7,
                                  ('a', 'b'), (0.7, 1000, 3)])
def test_bad_parameters_raise_before_a_plan_is_built(dry, ohem, monkeypatch):
    from addk.train import TrainStep
    built = []
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: built.append(1))
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, ohem=ohem, use_graph=False)
    assert not built


def test_unfused_head_or_unsupported_exit_raises(dry, monkeypatch):
    from addk.train import TrainStep
    built = []
    real = P.Graph.finalize
    monkeypatch.setattr(P.Graph, 'finalize', lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    monkeypatch.setenv('ADDK_FUSE_CE', '0')
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, ohem=(0.7, 1000), use_graph=False)
    monkeypatch.setenv('ADDK_FUSE_CE', '1')
    # an exit whose shape the fused head does not take (more than 16 output rows per input row): no materialised fallback
    lib = addk.load()
    monkeypatch.setattr(lib, 'addk_ce_upsample_supported', lambda *a: 0)
    with pytest.raises(ValueError):
        TrainStep(_add(4), SHAPE, ohem=(0.7, 1000), use_graph=False)
    assert not built
    TrainStep(_add(4), SHAPE, use_graph=False)                     # the plain step still takes the three-kernel form there
    assert built
