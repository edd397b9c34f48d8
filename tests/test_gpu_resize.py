"""GPU tests of the bilinear resize kernels (csrc/resize.hip) through the C ABI:

 * the table-driven NHWC backward and the LDS-tiled NCHW backward against fp64 autograd, and against the per-thread kernels they replace;
 * every launch form of addk_resize_fwd / addk_resize_bwd, one small case per code path, bit for bit against the hashes recorded from the
   parent of the commit that gave the file its one kernel choice (tests/golden/resize_parent_bits.json, written by
   tests/tools/make_resize_bits.py): that commit names shared pieces, every floating-point operation stays the same operation in the
   same order, so no difference at all is allowed;
 * addk_resize_bwd_batch_prepare / addk_resize_bwd_batch_run against the single launches they merge."""
import ctypes as C
import functools
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-5
FAST_ALL = 31

_spec = importlib.util.spec_from_file_location('make_resize_bits', os.path.join(HERE, 'tools', 'make_resize_bits.py'))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


def _log(fmt, *a):
    print(fmt % a)          # the measured errors, shown with -s or on failure


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    import addk
    addk.load()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    import addk  # noqa: F401
    from addk import _lib as L
    yield L
    L.load().addk_set_fast_paths(FAST_ALL)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('shape', [(2, 40, 32, 64, 63, 127), (1, 40, 63, 127, 64, 128), (2, 64, 64, 128, 16, 32), (1, 80, 64, 128, 32, 64),
                                   (2, 256, 16, 32, 32, 64), (1, 40, 128, 256, 125, 253), (2, 160, 32, 64, 128, 256), (1, 80, 31, 63, 125, 253), (1, 160, 16, 32, 128, 256), (2, 400, 32, 64, 64, 128)],
                         ids=['up_32_63', 'fit_63_64', 'down4', 'down2', 'up2_c256', 'fit_128_125', 'up4_c160', 'up4_odd', 'up8_c160', 'up2_c400'])
def test_table_driven_resize_backward_matches_fp64_autograd(dev, shape):
    """addk_resize_bwd on the table-driven kernel (csrc/resize.hip: resizes of at most x8 up-sampling: 5 taps per axis up to x2, 9 up to x4, 17 up to x8) through the C ABI against
    fp64 autograd of F.interpolate(relu(a*x + b)): gradient wrt x (first touch and accumulate) and the (dA, dB) sums; and
    bit-identical to the per-thread kernel it replaces (fast path off)."""
    import addk._lib as L
    lb = L.load()
    N, Cc, H, W, OH, OW = shape
    gen = torch.Generator().manual_seed(H * 7 + OW)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    P = N * H * W
    x, a, b, dy, g0 = rnd(P, Cc), rnd(Cc), 0.3 * rnd(Cc), rnd(N * OH * OW, Cc), rnd(P, Cc)
    xr = x.double().view(N, H, W, Cc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ar_, br_ = a.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.interpolate(F.relu(ar_.view(1, -1, 1, 1) * xr + br_.view(1, -1, 1, 1)), size=(OH, OW), mode='bilinear', align_corners=False)
    y.backward(dy.double().view(N, OH, OW, Cc).permute(0, 3, 1, 2))
    gx = xr.grad.permute(0, 2, 3, 1).reshape(P, Cc)
    ba = L.ResizeBwdArgs()
    ba.dy, ba.lddy, ba.nchw_in = dy.data_ptr(), Cc, 0
    ba.src.x, ba.src.a, ba.src.b, ba.src.ld, ba.src.C, ba.src.relu = x.data_ptr(), a.data_ptr(), b.data_ptr(), Cc, Cc, 1
    ba.N, ba.H, ba.W, ba.OH, ba.OW = N, H, W, OH, OW
    rows = lb.addk_ew_rows(P, Cc)
    res = {}
    try:
        for fast in (31, 0):
            lb.addk_set_fast_paths(fast)
            for acc in (0, 1):
                g = g0.clone() if acc else torch.full((P, Cc), float('nan'), device=dev)
                dab = torch.full((rows, Cc, 2), float('nan'), device=dev, dtype=torch.float64)
                ba.g, ba.ldg, ba.accumulate, ba.dab = g.data_ptr(), Cc, acc, dab.data_ptr()
                L.check(lb.addk_resize_bwd(C.byref(ba), torch.cuda.current_stream().cuda_stream), 'resize_bwd')
                torch.cuda.synchronize()
                res[(fast, acc)] = (g, dab.sum(0))
    finally:
        lb.addk_set_fast_paths(31)
    rel = lambda u, v: float((u.double() - v).abs().max() / v.abs().max())
    e = {'dx': rel(res[(31, 0)][0], gx), 'dx_acc': rel(res[(31, 1)][0], gx + g0.double()),
         'dab': rel(res[(31, 0)][1], torch.stack([ar_.grad, br_.grad], 1))}
    _log('resize_bwd table kernel %s: %s', shape, ' '.join('%s %.1e' % kv for kv in e.items()))
    assert all(v <= 5e-5 for v in e.values()), e          # fp32 source coordinates: ~1e-5 at scale 128/125 (the per-thread kernel and ATen alike)
    assert torch.equal(res[(31, 0)][0], res[(0, 0)][0]) and torch.equal(res[(31, 1)][0], res[(0, 1)][0]), 'differs from the per-thread kernel'


@pytest.mark.parametrize('N,H,W,OH,OW,Cc', [(2, 64, 128, 256, 512, 19), (1, 33, 65, 129, 257, 19), (1, 40, 50, 80, 100, 6)])
def test_logits_upsample_backward_tiled_matches_autograd(lib, N, H, W, OH, OW, Cc):
    """NCHW gradient of the up-sampled logits -> NHWC gradient of the low-resolution logits (decoder.py:28)."""
    L = lib
    l = L.load()
    dev = torch.device('cuda:0')
    gen = torch.Generator(device='cpu').manual_seed(N * 1000 + H)
    dy = torch.randn(N, Cc, OH, OW, generator=gen).to(dev)
    a = torch.randn(Cc, generator=gen).to(dev)
    x = torch.zeros(N, Cc, H, W, device=dev, dtype=torch.float64, requires_grad=True)
    y = F.interpolate(x * a.double().view(1, -1, 1, 1), size=(OH, OW), mode='bilinear', align_corners=False)
    y.backward(dy.double() * 0.5)
    ref = x.grad.permute(0, 2, 3, 1).reshape(-1, Cc)
    scale = torch.full((1,), 0.5, device=dev)
    bz = torch.zeros(Cc, device=dev)
    outs = []
    for fast in (FAST_ALL, 0):
        l.addk_set_fast_paths(fast)
        ld = (Cc + 3) // 4 * 4
        g = torch.zeros(N * H * W, ld, device=dev)
        ar = L.ResizeBwdArgs()
        ar.dy, ar.lddy, ar.nchw_in, ar.dy_scale = dy.data_ptr(), 0, 1, scale.data_ptr()
        ar.src.x, ar.src.a, ar.src.b, ar.src.ld, ar.src.C, ar.src.relu = g.data_ptr(), a.data_ptr(), bz.data_ptr(), ld, Cc, 0
        ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
        ar.g, ar.ldg, ar.accumulate = g.data_ptr(), ld, 0
        L.check(l.addk_resize_bwd(C.byref(ar), torch.cuda.current_stream().cuda_stream), 'resize_bwd')
        torch.cuda.synchronize()
        outs.append(g[:, :Cc].clone())
        assert _rel(outs[-1], ref) <= TOL, 'mask %d: %.2e' % (fast, _rel(outs[-1], ref))
    assert torch.equal(outs[0], outs[1]) or _rel(outs[0], outs[1]) <= 1e-6


# ---- every launch form against the parent commit's bits ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _golden():
    """The fixture's records by case name; it must list exactly the tool's cases, each with its input hash and every run."""
    with open(os.path.join(HERE, 'golden', 'resize_parent_bits.json')) as f:
        rec = json.load(f)['cases']
    assert [(k, v['shape']) for k, v in rec.items()] == [(c[0], list(c[1:9])) for c in bits.BWD + bits.FWD], 'fixture and tool list different cases'
    for case in bits.BWD:
        want = sorted('%s/acc%d/fast%d' % (v[0], acc, fast) for v in bits.variants(case) for acc in (0, 1) for fast in bits.FAST)
        assert sorted(rec[case[0]]['runs']) == want, case[0]
    for case in bits.FWD:
        assert sorted(rec[case[0]]['runs']) == ['relu0', 'relu1'], case[0]
    assert all(len(r['inputs']) == 64 and all(len(h) == 64 for bufs in r['runs'].values() for h in bufs.values()) for r in rec.values())
    return rec


def test_bit_cases_take_the_kernels_they_claim(lib):
    bits.check_paths(lib, lib.load())


@pytest.mark.parametrize('case', bits.BWD + bits.FWD, ids=[c[0] for c in bits.BWD + bits.FWD])
def test_resize_launches_are_bit_identical_to_the_parent(lib, case):
    """sha256 of every buffer each launch writes (y; g and the whole (dA, dB) slab) equals what the parent commit's library wrote on the
    same inputs: accumulate 0 / 1, with and without the slab and the ReLU prologue, fast paths on and off."""
    rec = _golden()[case[0]]
    arrs, hin = bits.make_inputs(case)
    assert hin == rec['inputs'], '%s: the seeded INPUTS differ from the fixture (numpy RandomState stream or dtype handling changed)' % case[0]
    got = (bits.run_bwd if case in bits.BWD else bits.run_fwd)(lib, lib.load(), case, arrs)
    want = rec['runs']
    assert sorted(got) == sorted(want)
    diff = ['%s:%s' % (run, b) for run in sorted(want) for b in sorted(want[run]) if got[run].get(b) != want[run][b]]
    assert not diff, '%s: %s differ from the parent commit bit for bit' % (case[0], ', '.join(diff))


# ---- the batched run against the single launches ------------------------------------------------------------------------------------------------

# three items of one key and different shapes (different slab rows), N, C, H, W, OH, OW
BATCHES = {5: [(1, 40, 16, 32, 32, 64), (2, 40, 8, 16, 15, 31), (1, 80, 12, 20, 24, 40)],
           9: [(1, 40, 8, 16, 32, 64), (2, 40, 5, 9, 20, 33), (1, 80, 6, 10, 24, 40)],
           17: [(1, 40, 8, 16, 64, 128), (2, 40, 3, 5, 24, 37), (1, 80, 8, 12, 60, 96)]}


def _prepare(lb, items, blob=None):
    arr = (type(items[0]) * len(items))(*items)
    meta = (C.c_int64 * 8)()
    size = int(lb.addk_resize_bwd_batch_prepare(arr, len(items), blob, len(blob) if blob is not None else 0, meta))
    return size, meta


@pytest.mark.parametrize('key', sorted(BATCHES))
def test_batched_resize_backward_equals_the_single_launches(lib, key):
    """addk_resize_bwd_batch_prepare + addk_resize_bwd_batch_run on three items of one key: g (first touch and accumulate) and the (dA, dB)
    slabs equal three addk_resize_bwd calls on the same inputs bit for bit; a batch of mixed keys is refused."""
    L, lb = lib, lib.load()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    lb.addk_set_fast_paths(FAST_ALL)
    gen = torch.Generator().manual_seed(900 + key)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    items = []
    for N, Cc, H, W, OH, OW in BATCHES[key]:
        P = N * H * W
        t = {'x': rnd(P, Cc), 'a': rnd(Cc), 'b': 0.3 * rnd(Cc), 'dy': rnd(N * OH * OW, Cc), 'g0': rnd(P, Cc), 'rows': int(lb.addk_ew_rows(P, Cc)), 'C': Cc}
        ba = L.ResizeBwdArgs()
        ba.dy, ba.lddy, ba.nchw_in = t['dy'].data_ptr(), Cc, 0
        ba.src.x, ba.src.a, ba.src.b, ba.src.ld, ba.src.C, ba.src.relu = t['x'].data_ptr(), t['a'].data_ptr(), t['b'].data_ptr(), Cc, Cc, 1
        ba.N, ba.H, ba.W, ba.OH, ba.OW, ba.ldg = N, H, W, OH, OW, Cc
        assert int(lb.addk_resize_bwd_batch_key(C.byref(ba))) == -1          # no gradient buffer yet: rejected, no key
        items.append((t, ba))
    assert len({t['rows'] for t, _ in items}) > 1

    def run(acc, batched):
        outs = []
        for t, ba in items:
            g = t['g0'].clone() if acc else torch.full_like(t['g0'], float('nan'))
            slab = torch.full((t['rows'], t['C'], 2), float('nan'), device=dev, dtype=torch.float64)
            ba.g, ba.accumulate, ba.dab = g.data_ptr(), acc, slab.data_ptr()
            assert int(lb.addk_resize_bwd_batch_key(C.byref(ba))) == key
            outs.append((g, slab))
        if batched:
            size, _ = _prepare(lb, [ba for _, ba in items])
            assert size > 0, lb.addk_last_error()
            blob = (C.c_char * size)()
            size2, meta = _prepare(lb, [ba for _, ba in items], blob)
            assert size2 == size and list(meta[:3]) == [key, 3, max(t['rows'] for t, _ in items)], list(meta[:4])
            dblob = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
            L.check(lb.addk_resize_bwd_batch_run(dblob.data_ptr(), meta, st), 'resize_bwd_batch_run')
        else:
            for _, ba in items:
                L.check(lb.addk_resize_bwd(C.byref(ba), st), 'resize_bwd')
        torch.cuda.synchronize()
        return outs
    for acc in (0, 1):
        single, batch = run(acc, False), run(acc, True)
        for i, ((gs, ss), (gb, sb)) in enumerate(zip(single, batch)):
            assert not torch.isnan(gs).any() and not torch.isnan(ss).any(), (key, acc, i)
            assert torch.equal(gs, gb) and torch.equal(ss, sb), 'key %d accumulate %d item %d: the batched run differs from the single launch' % (key, acc, i)
    other = [k for k in BATCHES if k != key][0]
    ba = items[0][1]
    alien = L.ResizeBwdArgs.from_buffer_copy(ba)
    alien.N, alien.H, alien.W = 1, 8, 8                                   # a shape of another key on the same pointers: queried, never launched
    alien.OH = alien.OW = {5: 16, 9: 32, 17: 64}[other]
    assert int(lb.addk_resize_bwd_batch_key(C.byref(alien))) == other
    assert _prepare(lb, [ba, alien])[0] < 0 and b'mixed kernel variants' in lb.addk_last_error()
