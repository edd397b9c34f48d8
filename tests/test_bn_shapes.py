"""Shape guard (CPU, no GPU): dry-build config 2's train plan at 2x1024x2048 with the launches stubbed and read every BatchNorm-statistics,
branch-sum and GAP launch off it.  tests/test_gpu_bn_kernels.py runs those kernels at the shapes its NET_* tables list; this test fails as
soon as the plan runs one the tables do not, so the kernel tests cannot drift from the network unnoticed."""
import collections

import torch

import addk
import addk.plan as P
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args
import test_gpu_bn_kernels as K


def network_shapes(monkeypatch):
    """The distinct shapes of config 2's train plan at 2x1024x2048 (F = 20), one launch per BatchNorm (ADDK_LEVEL_BATCH=0)."""
    monkeypatch.setenv('ADDK_LEVEL_BATCH', '0')
    monkeypatch.setattr(P.Graph, 'run', lambda self, cmds, stream: None)
    monkeypatch.setattr(P, 'require_device', lambda x: None)
    monkeypatch.setattr(P, 'current_stream', lambda: 0)
    from addk.modeling.ADD import ADD
    lib = addk._lib.load()
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), ARCH_C2['low_level_layer'])
    m.train()
    m(torch.empty(2, 3, 1024, 2048))
    plan = next(iter(m._plans().values()))
    s = collections.defaultdict(set)
    obj = lambda a: a._obj if hasattr(a, '_obj') else a         # noqa: E731  (C.byref(struct) -> struct)
    for c in list(plan.g.fwd) + list(plan.g.bwd):
        a = c.args
        if c.fn is lib.addk_bn_finalize:
            f = obj(a[0])
            s['bn'].add((f.C, int(f.count)))
            s['fin'].add((f.C, int(f.count), f.rows))
        elif c.fn is lib.addk_bn_bwd:
            b = obj(a[0])
            s['bn'].add((b.C, int(b.count)))
            s['bwd'].add((b.C, int(b.count), tuple(sorted(b.rows[i] for i in range(b.nslab)))))
        elif c.fn is lib.addk_bn_bwd_apply:
            it = obj(a[0])
            s['apply'].add((it.C, int(it.P)))
        elif c.fn is lib.addk_affine_sum_fwd:
            f = obj(a[0])
            s['affine'].add((int(f.P), f.C, f.nterm, f.ldo))
        elif c.fn is lib.addk_affine_sum_bwd:
            f = obj(a[0])
            s['affine_bwd'].add((int(f.P), f.C, f.nterm, f.lddo))
        elif c.fn is lib.addk_gap_fwd:
            src = obj(a[0])
            s['gap'].add((src.C, src.ld, int(a[1]), int(a[2]), int(a[6]), src.relu, bool(src.a)))
        elif c.fn is lib.addk_gap_bwd:
            src = obj(a[0])
            s['gap_bwd'].add((src.C, src.ld, int(a[1]), int(a[2]), src.relu, bool(src.a)))
    return s


def test_gpu_bn_kernel_tables_cover_the_network(monkeypatch):
    s = network_shapes(monkeypatch)
    assert len(s['bn']) > 5 and s['apply'] and s['affine'] and s['gap']       # the plan was read at all
    missing = {
        'BatchNorm (C, count)': s['bn'] - set(K.NET_BN),
        'bn_bwd_apply (C, P)': s['apply'] - set(K.NET_BN),
        'bn_finalize (C, count, rows)': s['fin'] - set(K.NET_FIN),
        'bn_bwd (C, count, slab rows)': s['bwd'] - set((c, n, tuple(sorted(r))) for c, n, r in K.NET_BWD),
        'affine_sum (P, C, nterm, ldo)': s['affine'] - set(K.NET_AFFINE) - set(K.NET_BIAS_ACC),
        'affine_sum_bwd (P, C, nterm, lddo)': s['affine_bwd'] - set(K.NET_AFFINE),
        'gap_fwd (C, ld, N, HW, mean, relu, lazy)': s['gap'] - set(K.NET_GAP),
        'gap_bwd (C, ld, N, HW, relu, lazy)': s['gap_bwd'] - set(g[:4] + g[5:] for g in K.NET_GAP),
    }
    missing = {k: sorted(v) for k, v in missing.items() if v}
    assert not missing, 'shapes of the train plan that tests/test_gpu_bn_kernels.py does not run: %s' % missing
