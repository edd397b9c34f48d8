"""GPU tests of the calibration head (addk_calib_upsample) and of the tempered gate and profile launches (addk_gate_upsample_t,
addk_profile_upsample_t) through the C ABI: the calibration statistics against the fp64 reference of tests/_calib_ref.py, the tempered
launches bit for bit against the untempered ones at the word 1.0 and against fp64 at other temperatures."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _calib_ref as R                                                                              # noqa: E402
from _util import rand_tensor                                                                       # noqa: E402
from test_gpu_exit_profile import CASES, LD, THRESHOLDS, _gate, _padded, _Profile, _targets        # noqa: E402
from test_gpu_gate import NEAR, NEAR_SHARE                                                          # noqa: E402

INPUTS = ('plain', 'correlated')
NT = len(R.TEMPERATURES)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _inputs(case, kind):
    """logits [N,H,W,19], targets [N,OH,OW], the fp64 up-sample and the reference at the default grid: computed once, never modified"""
    N, lo, hi = CASES[case]
    x = rand_tensor(43, 'gate_x:' + case, (N,) + lo + (19,)) * 3
    if kind == 'plain':
        t = _targets(N, hi, 17)
    else:
        x, t = R.correlated_input(x, hi, 17)
    z64 = R.upsample64(x, hi)
    return dict(x=x, t=t, z64=z64, ref=R.reference(z64, t, R.inverse_words(R.TEMPERATURES)))


class _Calib:
    """One set of buffers of the calibration launch: inverse temperatures, accumulators, zero-initialised workspace."""

    def __init__(self, lib, L, shape, dev, temperatures=R.TEMPERATURES, fill=0):
        self.lib, self.L, self.shape = lib, L, shape
        N, _, (OH, OW) = shape
        self.inv = R.inverse_words(temperatures).to(dev)
        self.bins = torch.full((len(temperatures), R.BINS, 3), fill, dtype=torch.int64, device=dev)
        self.nll = torch.full((len(temperatures),), float(fill), dtype=torch.float64, device=dev)
        self.ws = torch.zeros(int(lib.addk_calib_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)

    def args(self, xa, ld, ta, nt=None, C_=19):
        N, (H, W), (OH, OW) = self.shape
        a = self.L.CalibUpsampleArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, C_, OH, OW
        a.target, a.inv_temp, a.nt = ta.data_ptr(), self.inv.data_ptr(), self.inv.numel() if nt is None else nt
        a.bins, a.nll, a.ws = self.bins.data_ptr(), self.nll.data_ptr(), self.ws.data_ptr()
        return a

    def __call__(self, xa, ld, ta, zero=True, **kw):
        if zero:
            self.bins.zero_()
            self.nll.zero_()
        rc = self.lib.addk_calib_upsample(C.byref(self.args(xa, ld, ta, **kw)), _stream())
        torch.cuda.synchronize()
        return rc, self.bins.cpu(), self.nll.cpu()

    def ticket(self):
        """the ticket word, which a launch leaves at zero — as it leaves the replicas of the bins behind the NLL partials"""
        assert int(self.ws[-32 * 8 * R.BINS * 3 * 8:].view(torch.int64).abs().sum()) == 0
        return int(self.ws[:4].view(torch.int32).item())


def _resize(lib, L, xa, ld, shape):
    """addk_resize_fwd: the materialised fp32 full-resolution logits [N,19,OH,OW]"""
    N, (H, W), (OH, OW) = shape
    y = torch.empty((N, 19, OH, OW), device=xa.device)
    ar = L.ResizeArgs()
    ar.src.x, ar.src.ld, ar.src.C = xa.data_ptr(), ld, 19
    ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    L.check(lib.addk_resize_fwd(C.byref(ar), _stream()), 'resize_fwd')
    return y


def _unfused_nll(y, ta, inv):
    """the materialised fp32 form on the same device: cross_entropy(y * inv_T, t, 'sum') over the valid pixels, per temperature"""
    t = torch.where((ta >= 0) & (ta < 19), ta, torch.full_like(ta, -100))
    return torch.stack([torch.nn.functional.cross_entropy(y * w, t, ignore_index=-100, reduction='sum') for w in inv]).double().cpu()


@pytest.mark.parametrize('kind', INPUTS)
@pytest.mark.parametrize('case', list(CASES))
def test_calib_upsample_matches_fp64(dev, case, kind):
    """addk_calib_upsample at the default grid against F.interpolate(bilinear, align_corners=False) in fp64 and the definitions of
    include/addk.h in fp64: every pixel counted once, counts within the pixels that sit inside 1e-5 of a bin edge, hits within those and the
    near-ties, confidence sums per bin, the NLL sums at 4x the error of the materialised fp32 form (or 2e-6 relative); reruns bit-equal, a
    second launch doubles every sum exactly, the ticket returns to zero, padding channels and the dense stride change nothing, and one
    temperature alone carries the bits of its column."""
    import addk._lib as L
    lib = L.load()
    N, (H, W), (OH, OW) = shape = CASES[case]
    inp = _inputs(case, kind)
    ref = inp['ref']
    assert lib.addk_calib_upsample_supported(N, H, W, OH, OW, 19, NT) == 1
    xa, ta = _padded(inp['x'], dev, 1), inp['t'].to(dev)
    cal = _Calib(lib, L, shape, dev)
    rc, bins, nll = cal(xa, LD, ta)
    assert rc == 0 and cal.ticket() == 0
    tag = '%s/%s' % (case, kind)
    if kind == 'correlated':
        means = (ref['nll'] / ref['valid']).tolist()
        print('%s: fp64 mean NLL per temperature %s' % (tag, ['%.4f' % v for v in means]))
        assert abs(ref['accuracy'] - 0.81) < 0.02
        assert means.index(min(means)) == R.TEMPERATURES.index(1.5)                      # an interior minimum
    assert 0 < ref['valid'] < inp['t'].numel()                                           # some targets are skipped
    R.check_bins(tag, bins, ref)
    R.check_nll(tag, nll, ref, _unfused_nll(_resize(lib, L, xa, LD, shape), ta, cal.inv))
    assert not torch.equal(bins[0], bins[-1])                                            # the temperatures differ
    # run to run
    for _ in range(2):
        rc, b2, n2 = cal(xa, LD, ta)
        assert rc == 0 and torch.equal(b2, bins) and torch.equal(n2.view(torch.int64), nll.view(torch.int64))
    # a second launch without zeroing: every integer counter and every fp64 sum doubles exactly
    rc, b3, n3 = cal(xa, LD, ta, zero=False)
    assert rc == 0 and torch.equal(b3, 2 * bins) and torch.equal(n3.view(torch.int64), (2 * nll).view(torch.int64))
    assert cal.ticket() == 0
    # other garbage in the padding channels, and the dense pixel stride (19: the scalar-load kernel): the same bits
    rc, b4, n4 = cal(_padded(inp['x'], dev, 2), LD, ta)
    assert rc == 0 and torch.equal(b4, bins) and torch.equal(n4.view(torch.int64), nll.view(torch.int64))
    rc, b5, n5 = cal(inp['x'].to(dev).contiguous(), 19, ta)
    assert rc == 0 and torch.equal(b5, bins) and torch.equal(n5.view(torch.int64), nll.view(torch.int64))
    # one temperature alone
    j = R.TEMPERATURES.index(1.0)
    one = _Calib(lib, L, shape, dev, (1.0,))
    rc, b6, n6 = one(xa, LD, ta)
    assert rc == 0 and one.ticket() == 0
    assert torch.equal(b6[0], bins[j]) and torch.equal(n6.view(torch.int64), nll[j:j + 1].view(torch.int64))


def test_calib_upsample_refuses_what_it_does_not_take(dev):
    import addk
    import addk._lib as L
    lib = L.load()
    shape = (1, (8, 16), (64, 128))
    cal = _Calib(lib, L, shape, dev, fill=5)
    xa, ta = torch.zeros((1, 8, 16, 24), device=dev), torch.zeros((1, 64, 128), dtype=torch.int64, device=dev)

    def untouched(rc):
        torch.cuda.synchronize()
        assert rc != 0                                                                   # an error code and no launch
        assert torch.equal(cal.bins.cpu(), torch.full((NT, R.BINS, 3), 5)) and torch.equal(cal.nll.cpu(), torch.full((NT,), 5.0, dtype=torch.float64))
        assert cal.ticket() == 0
        with pytest.raises(addk.AddkError):
            L.check(rc, 'calib_upsample')
    sup = lib.addk_calib_upsample_supported
    assert sup(1, 8, 16, 64, 128, 19, 1) == 1 and sup(1, 8, 16, 64, 128, 19, 8) == 1
    assert sup(1, 8, 16, 64, 128, 19, 0) == 0 and sup(1, 8, 16, 64, 128, 19, 9) == 0 and sup(1, 8, 16, 64, 128, 21, 8) == 0
    untouched(cal(xa, 24, ta, zero=False, nt=0)[0])
    untouched(cal(xa, 24, ta, zero=False, nt=9)[0])
    untouched(cal(xa, 24, ta, zero=False, C_=21)[0])
    untouched(cal(xa, 16, ta, zero=False)[0])                                            # a stride shorter than the channels
    for field in ('logits', 'target', 'inv_temp', 'bins', 'nll', 'ws'):
        a = cal.args(xa, 24, ta)
        setattr(a, field, None)
        untouched(lib.addk_calib_upsample(C.byref(a), _stream()))
    assert lib.addk_calib_upsample(C.byref(L.CalibUpsampleArgs()), None) != 0
    assert lib.addk_calib_upsample(None, None) != 0


# ------------------------------------------------------------------------------------------------------------------------
# tempered gate and profile
# ------------------------------------------------------------------------------------------------------------------------
class _GateT:
    """One set of buffers of the tempered gate launch, with and without the label map."""

    def __init__(self, lib, L, shape, dev):
        self.lib, self.L, self.shape = lib, L, shape
        N, _, (OH, OW) = shape
        self.thr, self.inv = torch.zeros(1, device=dev), torch.ones(1, device=dev)
        self.out = torch.full((N, 2), -7.0, device=dev)
        self.lab = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=dev)
        self.ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)

    def args(self, xa, ld, labels, lut=None):
        N, (H, W), (OH, OW) = self.shape
        a = self.L.GateUpsampleTArgs()
        g = a.gate
        g.logits, g.ld, g.N, g.H, g.W, g.C, g.OH, g.OW = xa.data_ptr(), ld, N, H, W, 19, OH, OW
        g.max_thr, g.out, g.out_host, g.ws = self.thr.data_ptr(), self.out.data_ptr(), None, self.ws.data_ptr()
        a.inv_temp = self.inv.data_ptr()
        a.lut256, a.labels = lut.data_ptr() if lut is not None else None, self.lab.data_ptr() if labels else None
        return a

    def __call__(self, xa, ld, thr, inv, labels=False, lut=None):
        self.thr.fill_(thr)
        self.inv.fill_(inv)
        self.out.fill_(-7.0)
        self.lab.fill_(77)
        rc = self.lib.addk_gate_upsample_t(C.byref(self.args(xa, ld, labels, lut)), _stream())
        torch.cuda.synchronize()
        return rc, self.out.cpu(), self.lab.cpu()


def _gate_label(lib, L, xa, ld, shape, thr, lut=None):
    """addk_gate_label_upsample -> ([N,2], map)"""
    N, (H, W), (OH, OW) = shape
    dev = xa.device
    word, out = torch.full((1,), thr, device=dev), torch.full((N, 2), -7.0, device=dev)
    lab = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)
    a = L.GateLabelUpsampleArgs()
    g = a.gate
    g.logits, g.ld, g.N, g.H, g.W, g.C, g.OH, g.OW = xa.data_ptr(), ld, N, H, W, 19, OH, OW
    g.max_thr, g.out, g.out_host, g.ws = word.data_ptr(), out.data_ptr(), None, ws.data_ptr()
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, lab.data_ptr()
    L.check(lib.addk_gate_label_upsample(C.byref(a), _stream()), 'gate_label_upsample')
    torch.cuda.synchronize()
    return out.cpu(), lab.cpu()


def _profile_t(prof, xa, ld, ta, inv):
    """addk_profile_upsample_t on the buffers of a _Profile"""
    b = prof.L.ProfileUpsampleTArgs()
    b.profile, b.inv_temp = prof.args(xa, ld, ta), inv.data_ptr()
    prof.cm.zero_()
    prof.ent.fill_(-7.0)
    prof.share.fill_(-7.0)
    prof.pred.fill_(77)
    rc = prof.lib.addk_profile_upsample_t(C.byref(b), _stream())
    torch.cuda.synchronize()
    return rc, prof.ent.cpu(), prof.share.cpu(), prof.cm.cpu(), prof.pred.cpu()


def _bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('case', list(CASES))
def test_tempered_launches_at_one_carry_the_untempered_bits(dev, case):
    """The word 1.0: entropy and the share at four thresholds are addk_gate_upsample's words, with the map addk_gate_label_upsample's words
    and bytes (with and without a table); the tempered profile is addk_profile_upsample's entropy, shares, matrix and map.  Both pixel
    strides."""
    import addk._lib as L
    lib = L.load()
    N, lo, hi = shape = CASES[case]
    inp = _inputs(case, 'plain')
    ta = inp['t'].to(dev)
    lut = torch.arange(255, -1, -1, dtype=torch.uint8, device=dev)
    one = torch.ones(1, device=dev)
    for ld, xa in ((LD, _padded(inp['x'], dev, 1)), (19, inp['x'].to(dev).contiguous())):
        gt = _GateT(lib, L, shape, dev)
        for thr in THRESHOLDS:
            want = _gate(lib, L, xa, ld, shape, thr)
            rc, out, lab = gt(xa, ld, thr, 1.0)
            assert rc == 0 and _bits(out, want) and torch.equal(lab, torch.full_like(lab, 77))      # the gate alone writes no map
            for table in (None, lut):
                want_l, want_map = _gate_label(lib, L, xa, ld, shape, thr, table)
                rc, out, lab = gt(xa, ld, thr, 1.0, labels=True, lut=table)
                assert rc == 0 and _bits(out, want_l) and _bits(out, want) and torch.equal(lab, want_map)
        assert int(gt.ws[:4].view(torch.int32).item()) == 0
        p0, p1 = _Profile(lib, L, shape, dev), _Profile(lib, L, shape, dev)
        rc0, ent0, share0, cm0, pred0 = p0(xa, ld, ta)
        rc1, ent1, share1, cm1, pred1 = _profile_t(p1, xa, ld, ta, one)
        assert rc0 == 0 and rc1 == 0
        assert _bits(ent1, ent0) and _bits(share1, share0) and torch.equal(cm1, cm0) and torch.equal(pred1, pred0)
        assert int(p1.ws[:4].view(torch.int32).item()) == 0


def _unfused_entropy_t(lib, L, y, inv, shape):
    """the materialised fp32 form: addk_entropy_sum over y * inv_T, per image"""
    N, _, (OH, OW) = shape
    ys = (y * inv).contiguous()
    out, ws = torch.zeros(N, device=y.device), torch.zeros(1024, device=y.device)
    for n in range(N):
        L.check(lib.addk_entropy_sum(ys[n].data_ptr(), 1, 19, OH * OW, out[n:].data_ptr(), ws.data_ptr(), _stream()), 'entropy_sum')
    torch.cuda.synchronize()
    return out.double().cpu() / (math.log(19) * OH * OW)


@pytest.mark.parametrize('T', [2.0, 0.5])
@pytest.mark.parametrize('case', list(CASES))
def test_tempered_gate_and_profile_match_fp64(dev, case, T):
    """softmax(z / T) in fp64 by the rules of tests/test_gpu_gate.py: the entropy at 4x the error of the materialised fp32 form (or 2e-6
    relative), the share at each threshold within the pixels inside 1e-5 of it (capped at NEAR_SHARE).  The tempered profile carries the
    tempered gate's words; map and matrix do not move with the temperature; a new word is honoured by the next launch."""
    import addk._lib as L
    lib = L.load()
    N, lo, (OH, OW) = shape = CASES[case]
    npix = OH * OW
    inp = _inputs(case, 'plain')
    xa, ta = _padded(inp['x'], dev, 1), inp['t'].to(dev)
    ent64, pmax64 = R.tempered_gate_reference(inp['z64'], T)
    inv = 1.0 / T                                                                        # exact in fp32 for both temperatures
    e_unf = _unfused_entropy_t(lib, L, _resize(lib, L, xa, LD, shape), inv, shape)
    gt = _GateT(lib, L, shape, dev)
    want_map = _gate_label(lib, L, xa, LD, shape, 0.5)[1]
    plain = _gate(lib, L, xa, LD, shape, 0.5)
    shares = []
    for thr in THRESHOLDS:
        rc, out, lab = gt(xa, LD, thr, inv, labels=True)
        assert rc == 0 and torch.equal(lab, want_map)                                    # the same bytes at any temperature
        rc, alone, _ = gt(xa, LD, thr, inv)
        assert rc == 0 and _bits(alone, out)
        shares.append(out[:, 1].clone())
        for n in range(N):
            e64 = float(ent64[n])
            err_f, err_u = abs(float(out[n, 0].double()) - e64), abs(float(e_unf[n]) - e64)
            count64 = int((pmax64[n] > thr).sum())
            near = int(((pmax64[n] - thr).abs() < NEAR).sum())
            count = float(out[n, 1].double()) * npix
            print('%s[%d] T %.1f thr %.2f: entropy %.9g ref64 %.9g rel err fused %.3g unfused %.3g; count %.3f ref64 %d near %d of %d' % (
                case, n, T, thr, float(out[n, 0]), e64, err_f / e64, err_u / e64, count, count64, near, npix))
            assert err_f <= max(4 * err_u, 2e-6 * abs(e64))
            assert abs(count - round(count)) < 1e-2
            assert near <= NEAR_SHARE * npix
            assert abs(round(count) - count64) <= near
    assert not _bits(out[:, 0], plain[:, 0])                                             # the temperature moves the entropy
    prof = _Profile(lib, L, shape, dev)
    rc, ent, share, cm, pred = _profile_t(prof, xa, LD, ta, torch.full((1,), inv, device=dev))
    assert rc == 0 and _bits(ent, out[:, 0]) and _bits(share, torch.stack(shares, dim=1))
    rc, _, _, cm1, pred1 = _Profile(lib, L, shape, dev)(xa, LD, ta)
    assert rc == 0 and torch.equal(cm, cm1) and torch.equal(pred, pred1) and torch.equal(pred, want_map)
    # the word alone changes: the next launch honours it
    rc, back, _ = gt(xa, LD, 0.5, 1.0)
    assert rc == 0 and _bits(back, plain)


def test_tempered_launches_refuse_what_they_do_not_take(dev):
    import addk._lib as L
    lib = L.load()
    shape = (1, (8, 16), (64, 128))
    xa, ta = torch.zeros((1, 8, 16, 24), device=dev), torch.zeros((1, 64, 128), dtype=torch.int64, device=dev)
    gt = _GateT(lib, L, shape, dev)
    for field, where in (('inv_temp', None), ('logits', 'gate'), ('ws', 'gate'), ('out', 'gate'), ('max_thr', 'gate')):
        a = gt.args(xa, 24, True)
        setattr(getattr(a, where) if where else a, field, None)
        assert lib.addk_gate_upsample_t(C.byref(a), _stream()) != 0
    a = gt.args(xa, 24, True)
    a.gate.C = 21
    assert lib.addk_gate_upsample_t(C.byref(a), _stream()) != 0
    a = gt.args(xa, 16, False)
    assert lib.addk_gate_upsample_t(C.byref(a), _stream()) != 0
    assert lib.addk_gate_upsample_t(None, None) != 0
    prof = _Profile(lib, L, shape, dev)
    prof.cm.fill_(5)
    b = L.ProfileUpsampleTArgs()
    b.profile, b.inv_temp = prof.args(xa, 24, ta), None
    assert lib.addk_profile_upsample_t(C.byref(b), _stream()) != 0
    b.profile, b.inv_temp = prof.args(xa, 24, ta, nthr=17), gt.inv.data_ptr()
    assert lib.addk_profile_upsample_t(C.byref(b), _stream()) != 0
    assert lib.addk_profile_upsample_t(None, None) != 0
    torch.cuda.synchronize()
    assert torch.equal(gt.out.cpu(), torch.full((1, 2), -7.0)) and torch.equal(gt.lab.cpu(), torch.full((1, 64, 128), 77, dtype=torch.uint8))
    assert torch.equal(prof.cm.cpu(), torch.full((1, 19, 19), 5)) and torch.equal(prof.ent.cpu(), torch.full((1,), -7.0))
