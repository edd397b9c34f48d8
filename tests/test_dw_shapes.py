"""Shape guard (CPU, no GPU) of tests/test_gpu_dw_kernels.py: dry-build config 2's train plan at 2x1024x2048 with the launches stubbed, read
every addk_dw_fwd / addk_dw_bwd argument struct and every addk_pool3_* call off it, and fail as soon as the plan runs a launch the NET_DW /
NET_POOL tables do not list.  Then what the GPU module's checks rest on and a CPU can verify: the kernel the library chooses for every
shape of its tables (addk_dw_*_config decides on the host), that the bounds of the sum-type outputs lie below one single term with the
seeds the GPU tests use, and the replacement of inputs at the ReLU threshold."""
import pytest
import torch

import addk
import addk.plan as P
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args
import test_gpu_dw_kernels as K


def network_launches(monkeypatch):
    """The distinct depthwise and pooling launches of config 2's train plan at 2x1024x2048 (F = 20), unbatched (ADDK_LEVEL_BATCH=0)."""
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
    fwd, bwd, pool, other = set(), set(), set(), []
    obj = lambda a: a._obj if hasattr(a, '_obj') else a         # noqa: E731  (C.byref(struct) -> struct)
    for c in list(plan.g.fwd) + list(plan.g.bwd):
        a = c.args
        if c.fn is lib.addk_dw_fwd:
            f = obj(a[0])
            if (f.KH, f.pad) != (f.KW, f.dil * (f.KH // 2)):
                other.append('dw_fwd %dx%d pad %d dil %d' % (f.KH, f.KW, f.pad, f.dil))
            fwd.add((f.N, f.H, f.W, f.src.C, f.KH, f.stride, f.dil, f.src.ld, f.ldy, f.src.relu, bool(f.src.a)))
        elif c.fn is lib.addk_dw_bwd:
            b = obj(a[0])
            if (b.KH, b.pad, b.defer_wreduce, b.dw_accumulate) != (b.KW, b.dil * (b.KH // 2), 1, 0):
                other.append('dw_bwd %dx%d pad %d dil %d defer %d dw_accumulate %d' % (b.KH, b.KW, b.pad, b.dil, b.defer_wreduce, b.dw_accumulate))
            bwd.add((b.N, b.H, b.W, b.src.C, b.KH, b.stride, b.dil, b.src.ld, b.lddy, b.ldg, b.src.relu, bool(b.src.a), bool(b.g), b.accumulate,
                     bool(b.dab)))
        elif c.fn is lib.addk_pool3_fwd or c.fn is lib.addk_pool3_bwd:
            s = obj(a[0])
            pool.add((int(a[1]), int(a[2]), int(a[3]), s.C, int(a[6]), int(a[7]), s.ld, int(a[9])))
    return fwd, bwd, pool, other


def test_gpu_dw_kernel_tables_cover_the_network(monkeypatch):
    fwd, bwd, pool, other = network_launches(monkeypatch)
    assert fwd and bwd                                                        # the plan was read at all
    listed_fwd = set(t[:9] + t[10:12] for t in K.NET_DW)
    missing = {
        'dw_fwd (N, H, W, C, k, stride, dil, ld, ldy, relu, lazy)': fwd - listed_fwd,
        'dw_bwd (N, H, W, C, k, stride, dil, ld, lddy, ldg, relu, lazy, g, accumulate, dab)': bwd - set(K.NET_DW),
        'pool3 (N, H, W, C, stride, mode, ld, ldy)': pool - set(K.NET_POOL),
        'geometry or reduction the tables do not describe': set(other),
    }
    missing = {k: sorted(v) for k, v in missing.items() if v}
    assert not missing, 'launches of the train plan that tests/test_gpu_dw_kernels.py does not run: %s' % missing
    stale = set(K.NET_DW) - bwd
    assert not stale, 'NET_DW lists launches the plan no longer runs: %s' % sorted(stale)


SPECS = [(K.net_spec(i), 100 + i) for i in range(len(K.NET_DW))] + [(s, 200 + i) for i, s in enumerate(K.CONTRACT)]


@pytest.mark.parametrize('spec,seed', SPECS, ids=[s.name for s, _ in SPECS])
def test_kernel_choice_and_the_bounds_of_the_sums(spec, seed):
    """The same data as on the GPU (a CPU generator draws them), in host memory: the kernel addk_dw_*_config chooses is the one the
    table expects, no input is left at the ReLU threshold, and the dw / dab bounds — for the chosen kernel and the generic one, the
    wave and the batched reduction — lie below the median non-zero single term."""
    lib = addk._lib.load()
    d = K.Dw(spec, seed, dev='cpu')
    cf, cb, rows = d.configs(lib)
    K._expect(d, cf, cb, rows)
    chains = [d.chain(cb, False), d.chain(cb, True)]
    mask = int(lib.addk_get_fast_paths())
    try:
        lib.addk_set_fast_paths(0)
        gf, gb, _ = d.configs(lib)
    finally:
        lib.addk_set_fast_paths(mask)
    assert gf[0] == 0 and gb[0] == 0 and gb[6] == rows
    chains += [d.chain(gb, False), d.chain(gb, True)]
    d.assert_sums_see_one_term(chains, rows)


def test_contract_table_reaches_every_edge():
    """What the CONTRACT table is there for, read off its expected configurations."""
    e = {s.name: (s, s.expect) for s in K.CONTRACT}
    tiled_b = [s for s, x in e.values() if x['bwd'][0]]
    assert any(x['bwd'][2] < x['bwd'][3] for _, x in e.values() if x['bwd'][0])                         # zero-filled workspace rows
    assert any(s.N * K._cdiv(s.H, s.expect['bwd'][1]) * K._cdiv(s.W, 16) > s.expect['bwd'][2] for s in tiled_b)   # a block walks several tiles
    assert any(s.W % 16 and s.H % s.expect['bwd'][1] for s in tiled_b) and any(s.H == s.expect['bwd'][1] < 15 for s in tiled_b)
    assert {s.C for s in tiled_b} >= {44, 48, 160} and {s.k for s in tiled_b} == {3, 5} and {s.dil for s in tiled_b} == {1, 2}
    assert any(x['fwd'][0] and not x['bwd'][0] and s.stride == 2 for s, x in e.values())
    assert any(s.N * s.H * s.W == 2048 and x['bwd'][0] for s, x in e.values()) and any(s.N * s.H * s.W == 2046 and not x['bwd'][0] for s, x in e.values())


def test_inputs_at_the_relu_threshold_are_replaced():
    """Planted: x with a x + b = 0 to the last bit, and one ulp to either side of it; all are replaced, the rest is left alone."""
    gen = K._rng(7)
    a = (0.5 + K._rand(gen, 8)) * torch.where(K._rand(gen, 8) < 0.5, -1.0, 1.0)
    b = 0.3 * K._randn(gen, 8)
    x = K._randn(gen, 50, 8)
    root = (-b.double() / a.double()).float()
    x[3], x[17], x[40] = root, torch.nextafter(root, torch.full_like(root, 9.0)), torch.nextafter(root, torch.full_like(root, -9.0))
    y, n = K._clear_of_zero(x.clone(), a, b)
    assert n >= 24
    z = a.double() * y.double() + b.double()
    assert bool((z.abs() >= 4 * K.U * ((a.double() * y.double()).abs() + b.double().abs())).all())
    changed = (y != x).any(1)
    assert changed[[3, 17, 40]].all() and int(changed.sum()) == 3
    assert bool(((a * y[[3, 17, 40]] + b) > 0.9).all())
    y2, n2 = K._clear_of_zero(x.clone(), None, None)
    assert n2 == 0 and torch.equal(y2, x)


@pytest.mark.parametrize('rows', K.WREDUCE_ROWS)
def test_wreduce_bound_resolves_one_term(rows):
    for n, acc, ws, old in K.wreduce_data(rows, dev='cpu'):
        assert bool((K.wreduce_bound(rows, ws, old if acc else None) < ws.abs().double().median(0).values).all())


def test_pool_reference_on_the_cpu():
    """The pooling reference builds on the CPU (shapes, routing of ties to the first maximum)."""
    p = K.Pool(1, 1, 3, 1, 1, 0, False, 0, ties=True, seed=450, dev='cpu')
    p.x.copy_(torch.tensor([[1.0], [1.0], [0.0]]))
    p.dy.copy_(torch.tensor([[1.0], [2.0], [4.0]]))
    R = p.reference()
    assert R.g.reshape(-1).tolist() == [3.0, 4.0, 0.0]                     # windows (x0 x1), (x0 x1 x2), (x1 x2): first maximum each
