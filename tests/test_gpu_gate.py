"""GPU tests of dynamic inference gated by exit entropy / top-probability share: the gate kernel (addk_gate_upsample) through the
C ABI against fp64 CPU references, and ADD.dynamic_inference(confidence='entropy' | 'max') against the model's own forward()."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402

LD = 24
THRESHOLDS = (0.2, 0.35, 0.5, 0.8)
NEAR = 1e-5                  # |pmax - thr| window inside which the fp32 kernel and the fp64 reference may fall on different sides
NEAR_SHARE = 0.002           # ... and how much of the image may lie inside it
CASES = {'x8': (1, (8, 16), (64, 128)), 'odd_ladder': (1, (9, 17), (65, 129)), 'partial_tiles': (1, (5, 7), (33, 49)),
         'band13': (1, (3, 5), (40, 70)), 'x32': (1, (4, 4), (128, 128)), 'n2': (2, (6, 9), (41, 67))}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(case):
    """Inputs and the fp64 CPU reference of one case, computed once and never modified."""
    N, lo, hi = CASES[case]
    x = rand_tensor(43, 'gate_x:' + case, (N,) + lo + (19,)) * 3
    up64 = Fn.interpolate(x.double().permute(0, 3, 1, 2), size=hi, mode='bilinear', align_corners=False)
    lp = torch.log_softmax(up64, dim=1)
    ent64 = -(lp.exp() * lp).sum((1, 2, 3)) / (math.log(19) * hi[0] * hi[1])        # operations.py:161-170, per image
    return dict(x=x, ent64=ent64, pmax64=lp.exp().amax(1))


def _padded(x, dev, seed, ld=LD):
    """the logits in a pixel stride `ld` with finite garbage in the padding channels"""
    xa = (rand_tensor(seed, 'gate_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
    xa[..., :19] = x.to(dev)
    return xa.contiguous()


class _Gate:
    """One set of buffers of the gate launch: threshold word, device and pinned outputs, zero-initialised workspace."""

    def __init__(self, lib, L, shape, dev):
        self.lib, self.L, self.shape = lib, L, shape
        N, _, (OH, OW) = shape
        self.thr = torch.zeros(1, device=dev)
        self.out = torch.full((N, 2), -7.0, device=dev)
        self.host = torch.full((N, 2), -9.0).pin_memory()
        self.ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)

    def __call__(self, xa, ld, thr, C_=19):
        N, (H, W), (OH, OW) = self.shape
        self.thr.fill_(thr)
        self.out.fill_(-7.0)
        self.host.fill_(-9.0)
        a = self.L.GateUpsampleArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, C_, OH, OW
        a.max_thr, a.out, a.out_host, a.ws = self.thr.data_ptr(), self.out.data_ptr(), self.host.data_ptr(), self.ws.data_ptr()
        rc = self.lib.addk_gate_upsample(C.byref(a), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, self.out.cpu().clone(), self.host.clone()


def _unfused_entropy(lib, L, xa, shape, dev):
    """the parent's path, per image: addk_resize_fwd materialises the fp32 full-resolution logits, addk_entropy_sum reads them"""
    N, (H, W), (OH, OW) = shape
    y = torch.empty((N, 19, OH, OW), device=dev)
    ar = L.ResizeArgs()
    ar.src.x, ar.src.ld, ar.src.C = xa.data_ptr(), LD, 19
    ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.addk_resize_fwd(C.byref(ar), st), 'resize_fwd')
    out, ws = torch.zeros(N, device=dev), torch.zeros(1024, device=dev)
    for n in range(N):
        L.check(lib.addk_entropy_sum(y[n].data_ptr(), 1, 19, OH * OW, out[n:].data_ptr(), ws.data_ptr(), st), 'entropy_sum')
    torch.cuda.synchronize()
    return out.double().cpu() / (math.log(19) * OH * OW)


@pytest.mark.parametrize('case', list(CASES))
def test_gate_upsample_matches_fp64(dev, case):
    """addk_gate_upsample against F.interpolate(bilinear, align_corners=False) + log_softmax in fp64, per image: normalised entropy
    at the bound of the scoring kernel (4x the error of the materialised path, or 2e-6 relative), the share of pixels with
    pmax > thr within the pixels that sit inside 1e-5 of the threshold; device and pinned outputs, determinism, padding channels,
    dense stride, the threshold word."""
    import addk._lib as L
    lib = L.load()
    N, (H, W), (OH, OW) = shape = CASES[case]
    ref = _reference(case)
    npix = OH * OW
    assert lib.addk_gate_upsample_supported(N, H, W, OH, OW, 19) == 1
    xa = _padded(ref['x'], dev, 1)
    gate = _Gate(lib, L, shape, dev)
    rc, out, host = gate(xa, LD, 0.5)
    assert rc == 0
    assert torch.equal(out, host)                                            # device and pinned words: the same bits
    assert int(gate.ws[:4].view(torch.int32).item()) == 0                    # the ticket is back at zero
    e_unf = _unfused_entropy(lib, L, xa, shape, dev)
    for n in range(N):
        e64 = float(ref['ent64'][n])
        err_f, err_u = abs(float(out[n, 0].double()) - e64), abs(float(e_unf[n]) - e64)
        print('%s[%d] entropy fused %.9g unfused %.9g ref64 %.9g: rel err fused %.3g unfused %.3g' % (
            case, n, float(out[n, 0]), float(e_unf[n]), e64, err_f / e64, err_u / e64))
        assert err_f <= max(4 * err_u, 2e-6 * abs(e64))
    if N > 1:
        assert float(out[0, 0]) != float(out[1, 0]) and float(out[0, 1]) != float(out[1, 1])
    shares = {}
    for thr in THRESHOLDS:
        rc, o, h = gate(xa, LD, thr)
        assert rc == 0 and torch.equal(o, h)
        assert torch.equal(o[:, 0], out[:, 0])                               # only the word behind max_thr changed: the entropy stays
        shares[thr] = o[:, 1].clone()
        for n in range(N):
            pm = ref['pmax64'][n]
            count64 = int((pm > thr).sum())
            near = int(((pm - thr).abs() < NEAR).sum())
            count = float(o[n, 1].double()) * npix
            print('%s[%d] thr %.2f count %.3f ref64 %d near %d of %d' % (case, n, thr, count, count64, near, npix))
            assert abs(count - round(count)) < 1e-2                          # share = count / npix, rounded to fp32 once
            assert near <= NEAR_SHARE * npix
            assert abs(round(count) - count64) <= near
            assert 0 < count64 < npix                                        # both sides of the threshold are populated
    assert not torch.equal(shares[0.2], shares[0.8])                         # ... and the threshold word moves the share
    # run to run
    for _ in range(2):
        rc, o, h = gate(xa, LD, 0.5)
        assert rc == 0 and torch.equal(o, out) and torch.equal(h, out)
    # other garbage in the padding channels: nothing moves
    rc, o, h = gate(_padded(ref['x'], dev, 2), LD, 0.5)
    assert rc == 0 and torch.equal(o, out) and torch.equal(h, out)
    # dense pixel stride (19: the scalar-load kernel) computes the same bits as the 16-byte-load kernel
    rc, o, h = gate(ref['x'].to(dev).contiguous(), 19, 0.5)
    assert rc == 0 and torch.equal(o, out) and torch.equal(h, out)
    # no pinned words: the device result alone
    a = L.GateUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), LD, N, H, W, 19, OH, OW
    gate.thr.fill_(0.5)
    gate.out.fill_(-7.0)
    a.max_thr, a.out, a.out_host, a.ws = gate.thr.data_ptr(), gate.out.data_ptr(), None, gate.ws.data_ptr()
    L.check(lib.addk_gate_upsample(C.byref(a), torch.cuda.current_stream().cuda_stream), 'gate_upsample')
    torch.cuda.synchronize()
    assert torch.equal(gate.out.cpu(), out)


def test_gate_upsample_refuses_what_it_does_not_take(dev):
    import addk
    import addk._lib as L
    lib = L.load()
    shape = (1, (8, 16), (64, 128))
    assert lib.addk_gate_upsample_supported(1, 8, 16, 64, 128, 21) == 0
    gate = _Gate(lib, L, shape, dev)
    xa = torch.zeros((1, 8, 16, 24), device=dev)
    rc, out, host = gate(xa, 24, 0.5, C_=21)
    assert rc != 0                                                           # an error code ...
    assert torch.equal(out, torch.full((1, 2), -7.0)) and torch.equal(host, torch.full((1, 2), -9.0))      # ... and no launch
    with pytest.raises(addk.AddkError):
        L.check(rc, 'gate_upsample')
    assert lib.addk_gate_upsample(C.byref(L.GateUpsampleArgs()), None) != 0  # null pointers


# ------------------------------------------------------------------------------------------------------------------------
# public path
# ------------------------------------------------------------------------------------------------------------------------
def _model(arch, dev):
    from addk.modeling.ADD import ADD
    m = ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(20), arch['low_level_layer'])
    fill_params(m, 12)
    return m.to(dev).eval()


@functools.lru_cache(maxsize=None)
def _c2(dev):
    """the config 2 model, its input and its own forward() logits (cloned: forward()'s outputs are plan buffers), shared by both kinds"""
    m = _model(ARCH_C2, dev)
    x = rand_tensor(9, 'dynx', (1, 3, 129, 257)).to(dev)
    with torch.no_grad():
        ys = [y.clone() for y in m(x)]
    return m, x, ys


@pytest.mark.parametrize('kind', ['entropy', 'max'])
def test_dynamic_inference_by_exit_prediction(dev, kind):
    """F = 20, config 2: at a threshold that forces the exit y is addk's own m(x)[0], at one that forbids it m(x)[-1] (bit for bit: the
    gated plan runs forward()'s launches); the gate value is a float, the same for eager calls and hipGraph replays, and equals the
    stand-alone helpers of addk.modeling.operations on m(x)[0]; the decision flips at value +- 0.05."""
    from addk.modeling.operations import confidence_max, normalized_shannon_entropy
    m, x, ys = _c2(dev)
    max_thr = 0.5
    # 'entropy' leaves when value < threshold; 'max' when share(threshold) > threshold: the share is 1 at a threshold <= 0 and 0 at one >= 1
    force, forbid = (float('inf'), float('-inf')) if kind == 'entropy' else (-0.5, 1.5)
    vals = []
    with torch.no_grad():
        for call in range(5):                                                # calls 3+ replay captured graphs
            thr = force if call % 2 == 0 else forbid
            y, early, secs, val = m.dynamic_inference(x, threshold=thr, confidence=kind)
            assert isinstance(val, float) and isinstance(secs, float) and tuple(y.shape) == (1, 19, 129, 257)
            assert early == (1 if call % 2 == 0 else 0)
            assert torch.equal(y, ys[0] if early else ys[-1]), (call, float((y - (ys[0] if early else ys[-1])).abs().max()))
            if kind == 'entropy':
                vals.append(val)
        if kind == 'max':
            for call in range(5):
                vals.append(m.dynamic_inference(x, threshold=max_thr, confidence=kind)[3])
        plan = m._gate_plan(x, kind)
        assert plan.heads[0].gate_fused and plan.calls >= 5 and len(plan.graphs) >= 2
        assert len(set(vals)) == 1, vals
        v = vals[0]
        if kind == 'entropy':
            want = normalized_shannon_entropy(ys[0])
            print('entropy gate %.9g, normalized_shannon_entropy(m(x)[0]) %.9g' % (v, want))
            assert abs(v - want) <= 1e-5
            assert m.dynamic_inference(x, threshold=v + 0.05, confidence=kind)[1] == 1
            assert m.dynamic_inference(x, threshold=v - 0.05, confidence=kind)[1] == 0
        else:
            npix = 129 * 257
            want = confidence_max(ys[0], max_thr)
            pm = torch.softmax(ys[0].double(), dim=1).amax(1)
            near = int(((pm - max_thr).abs() < NEAR).sum())
            print('max gate %.9g (count %.2f), confidence_max(m(x)[0], %.2f) %.9g, near %d of %d' % (v, v * npix, max_thr, want, near, npix))
            assert near <= NEAR_SHARE * npix
            assert abs(v * npix - want * npix) <= near + 1e-2
            # the same number is threshold of pmax and of the share (ADD.py:476,481): share(t) falls with t, the exit flips where they cross
            lo_t, hi_t = 0.05, 0.95
            y, early, _, s = m.dynamic_inference(x, threshold=lo_t, confidence=kind)
            assert early == int(s > lo_t) and abs(s * npix - confidence_max(ys[0], lo_t) * npix) <= NEAR_SHARE * npix
            y, early, _, s = m.dynamic_inference(x, threshold=hi_t, confidence=kind)
            assert early == int(s > hi_t) and abs(s * npix - confidence_max(ys[0], hi_t) * npix) <= NEAR_SHARE * npix


def test_dynamic_inference_three_exits(dev):
    """config 3 (two gates): entropy thresholds +inf / between the two exits' values / -inf return exit 0, exit 1 and the final head."""
    m = _model(ARCH_C3, dev)
    x = rand_tensor(9, 'dynx', (1, 3, 129, 257)).to(dev)
    with torch.no_grad():
        ys = [y.clone() for y in m(x)]
        assert len(ys) == 3
        y, early, _, v0 = m.dynamic_inference(x, threshold=float('inf'), confidence='entropy')
        assert early == 1 and torch.equal(y, ys[0])
        y, early, _, v1 = m.dynamic_inference(x, threshold=float('-inf'), confidence='entropy')
        assert early == 0 and torch.equal(y, ys[2])                          # v1: the LAST gate evaluated, exit 1's
        print('config 3 exit entropies %.6f %.6f' % (v0, v1))
        assert v0 != v1
        if v1 < v0:                                                          # exit 0 stays, exit 1 leaves
            y, early, _, v = m.dynamic_inference(x, threshold=0.5 * (v0 + v1), confidence='entropy')
            assert early == 1 and v == v1 and torch.equal(y, ys[1])
        else:                                                                # no threshold passes exit 0 and stops at exit 1 ...
            y, early, _, v = m.dynamic_inference(x, threshold=0.5 * (v0 + v1), confidence='entropy')
            assert early == 1 and v == v0 and torch.equal(y, ys[0])
            # ... so exit 1 is reached through the 'max' gate instead: share(t) of exit 0 <= t < share(t) of exit 1 is not guaranteed either;
            # check the second head's logits through the plan's own segments
            plan = m._gate_plan(x, 'entropy')
            plan.x_static.copy_(x)
            plan._seg(0, plan.head_rng[0][0])
            plan._seg(plan.head_rng[0][1], plan.head_rng[1][0])
            plan._seg(*plan.head_rng[1])
            torch.cuda.synchronize()
            assert torch.equal(plan.heads[1].y, ys[1])
