"""GPU tests of the fused SepConv-half backward (csrc/sepb.hip) after its (row band, channel group) work items were spread
over 8-16 waves per tile: the config-2 shapes at exact size and channel counts with a partial last group against fp64
autograd, and every output bit for bit against the hashes recorded from the parent commit's library
(tests/golden/sepb_parent_bits.json, written by tests/tools/make_sepb_bits.py).  The re-mapping changes which wave runs an
item, never what a lane computes, so the second test allows no difference at all."""
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5              # tests/test_gpu_fast_kernels.py: fp32 products with fp32 accumulation against the fp64 reference's max-abs
FAST_ALL = 31
HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location('make_sepb_bits', os.path.join(HERE, 'tools', 'make_sepb_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

SHAPES = [
    # name,          N,  H,   W,  C, k
    ('c80_k3_l2',    2, 64, 128, 80, 3),      # the level-2 map of config 2 at exact size: 256 tiles of 16 waves, 20 items
    ('c80_k5_l2',    2, 64, 128, 80, 5),
    ('c48_k5_small', 1,  9,  11, 48, 5),      # map smaller than a tile row: row bands 2 and 3 of the last tile row lie beyond the map
    ('c36_k5_tail',  1, 40,  70, 36, 5),      # KG = 3, last group holds 4 of 16 channels (quads 1-3 of its items are beyond C)
    ('c36_k3_tail',  1, 40,  71, 36, 3),      # ... on the 8-wave 3x3
    ('c68_k3_tail',  2, 33,  65, 68, 3),      # KG = 5, last group holds 4 of 16 channels: the second item of waves 0-3
    ('c68_k5_tail',  1, 35,  66, 68, 5),
]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    L.load().addk_set_fast_paths(FAST_ALL)
    yield L
    L.load().addk_set_fast_paths(FAST_ALL)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_sepb_work_items_match_fp64_autograd(lib, shape):
    """addk_sep_bwd against fp64 autograd of y = pw(dw(relu(a*x + b))): gradient wrt x (first touch and accumulate), the
    (dA, dB) sums, the depthwise weight gradient from the workspace rows; bit-identical run to run."""
    L = lib
    lb = L.load()
    name, N, H, W, Cc, k = shape
    dev = torch.device('cuda:0')
    gen = torch.Generator(device='cpu').manual_seed(11 + sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    P = N * H * W
    x, a, b = rnd(P, Cc), rnd(Cc), 0.3 * rnd(Cc)
    wdw, wpw, dy = 0.3 * rnd(Cc, k * k), 0.2 * rnd(Cc, Cc), rnd(P, Cc)
    g0 = rnd(P, Cc)
    xr = x.double().view(N, H, W, Cc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ar_, br_ = a.double().requires_grad_(True), b.double().requires_grad_(True)
    wd = wdw.double().view(Cc, 1, k, k).requires_grad_(True)
    z = F.relu(ar_.view(1, -1, 1, 1) * xr + br_.view(1, -1, 1, 1))
    y = F.conv2d(F.conv2d(z, wd, padding=k // 2, groups=Cc), wpw.double().view(Cc, Cc, 1, 1))
    y.backward(dy.double().view(N, H, W, Cc).permute(0, 3, 1, 2))
    flat = lambda v: v.permute(0, 2, 3, 1).reshape(P, Cc)
    ba = L.SepBwdArgs()
    ba.dy, ba.lddy, ba.N, ba.H, ba.W, ba.K = dy.data_ptr(), Cc, N, H, W, k
    ba.src.x, ba.src.a, ba.src.b, ba.src.ld, ba.src.C, ba.src.relu = x.data_ptr(), a.data_ptr(), b.data_ptr(), Cc, Cc, 1
    ba.Cout, ba.ldw, ba.dw_w, ba.pw_w = Cc, Cc, wdw.data_ptr(), wpw.data_ptr()
    rows = lb.addk_sep_bwd_rows(C.byref(ba))
    assert rows > 0
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for acc in (0, 1, 0):
        g = g0.clone() if acc else torch.full((P, Cc), float('nan'), device=dev)
        dab = torch.full((rows, Cc, 2), float('nan'), device=dev, dtype=torch.float64)
        ws = torch.full((rows, Cc, k * k), float('nan'), device=dev)
        ba.g, ba.ldg, ba.accumulate, ba.dab, ba.ws = g.data_ptr(), Cc, acc, dab.data_ptr(), ws.data_ptr()
        L.check(lb.addk_sep_bwd(C.byref(ba), st), 'sep_bwd')
        torch.cuda.synchronize()
        outs.append((g, dab.sum(0), ws.double().sum(0)))
    assert all(torch.equal(u, v) for u, v in zip(outs[0], outs[2])), 'not reproducible'
    gx = flat(xr.grad)
    errs = {'dx': _rel(outs[0][0], gx), 'dx_acc': _rel(outs[1][0], gx + g0.double()),
            'dab': _rel(outs[0][1], torch.stack([ar_.grad, br_.grad], 1)), 'dw': _rel(outs[0][2], wd.grad.view(Cc, k * k))}
    print(name, ' '.join('%s %.2e' % kv for kv in errs.items()))
    bad = ['%s %.2e' % kv for kv in errs.items() if not kv[1] <= TOL]
    assert not bad, '%s beyond %.0e: %s' % (name, TOL, ', '.join(bad))


def _golden():
    """The fixture's records by case name; it must list exactly the tool's cases, each with its input hash and all four output
    hashes, and between them every (KS, KG, KP, R) config 2 runs and both the 56- and the 72-stride siblings."""
    with open(os.path.join(HERE, 'golden', 'sepb_parent_bits.json')) as f:
        rec = json.load(f)['cases']
    assert [(r['name'], r['shape'], r['seed']) for r in rec] == [(c[0], list(c[1:6]), c[6]) for c in bits.CASES], 'fixture and tool list different cases'
    for r in rec:
        assert all(len(r[key]) == 64 for key in ('inputs',) + bits.OUTPUTS), r['name']
    variants = {tuple(r['variant']) for r in rec}
    assert {(5, 5, 88, 1), (3, 5, 88, 1), (5, 3, 40, 2), (3, 3, 40, 2), (5, 5, 72, 1), (3, 5, 72, 1), (5, 3, 56, 2), (3, 3, 56, 2)} <= variants
    return {r['name']: r for r in rec}


@pytest.mark.parametrize('case', bits.CASES, ids=[c[0] for c in bits.CASES])
def test_sepb_outputs_are_bit_identical_to_the_parent(lib, case):
    """sha256 of g (first touch and accumulate), dab and ws equals what the parent commit's library wrote on the same inputs."""
    rec = _golden()[case[0]]
    arrs, hin = bits.make_inputs(case)
    assert hin == rec['inputs'], '%s: the seeded INPUTS differ from the fixture (numpy RandomState stream or dtype handling changed)' % case[0]
    got, variant = bits.run_case(lib, case, arrs)
    assert variant == rec['variant'], '%s runs variant %s, the fixture was recorded on %s' % (case[0], variant, rec['variant'])
    diff = [o for o in bits.OUTPUTS if got[o] != rec[o]]
    assert not diff, '%s: %s differ from the parent commit bit for bit' % (case[0], ', '.join(diff))
