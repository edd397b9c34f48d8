"""GPU tests of label-map inference: the label head (addk_label_upsample) and the gate launch that leaves the map
(addk_gate_label_upsample) through the C ABI, byte for byte against the two paths that exist without them — the prediction map
of addk_score_upsample and addk_argmax_nchw on addk_resize_fwd's materialised logits — and ADD.dynamic_inference(output='labels')
and addk.segment.Segmenter against the arg-max of the logits the same model returns.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402

LD = 24
GUARD = 64
# widths that are no multiple of 64, heights that are no multiple of 32, non-integer ratios (odd_ladder, partial_tiles, band13), row
# pairs that change inside a wave's 8 rows (every case but x32_n1, whose 32 rows per input row keep a pair for whole waves), several
# workgroups per image in both directions (x8, odd_ladder, x32_n1), and one down-sampling shape
CASES = {'x8': (2, (8, 16), (64, 128)), 'odd_ladder': (2, (9, 17), (65, 129)), 'partial_tiles': (2, (5, 7), (33, 49)),
         'band13': (2, (3, 5), (40, 70)), 'x32_n1': (1, (4, 4), (128, 128)), 'down': (2, (9, 9), (5, 5))}
GATE_CASES = ('odd_ladder', 'partial_tiles', 'x32_n1')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    import addk._lib as L
    return L.load(), L


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _logits(case):
    N, lo, hi = CASES[case]
    return rand_tensor(47, 'label_x:' + case, (N,) + lo + (19,)) * 3


def _padded(x, dev, seed=1, ld=LD):
    """the logits in a pixel stride `ld` with finite garbage in the padding channels"""
    xa = (rand_tensor(seed, 'label_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
    xa[..., :19] = x.to(dev)
    return xa.contiguous()


class _Map:
    """A label buffer between two guards of 64 bytes of 0xAB."""

    def __init__(self, shape, dev):
        N, _, (OH, OW) = shape
        self.n, self.dims = N * OH * OW, (N, OH, OW)
        self.raw = torch.full((self.n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def read(self):
        """the map on the host; the guards must be untouched"""
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == 0xAB).all()) and bool((raw[GUARD + self.n:] == 0xAB).all()), 'a guard byte was written'
        return raw[GUARD:GUARD + self.n].view(self.dims).clone()

    def untouched(self):
        return bool((self.raw.cpu() == 0xAB).all())


def _label(xa, ld, shape, lut=None, C_=19, into=None):
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape
    m = into if into is not None else _Map(shape, xa.device)
    a = L.LabelUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, C_, OH, OW
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, m.ptr
    rc = lib.addk_label_upsample(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, m


def _score_pred(xa, ld, shape):
    """pred_out of addk_score_upsample on the same logits (the target plays no part in it)"""
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape
    dev = xa.device
    tgt = torch.zeros((N, OH, OW), dtype=torch.int64, device=dev)
    wsum, loss, ent = torch.ones(1, device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    cm = torch.zeros((19, 19), dtype=torch.int64, device=dev)
    pred = torch.full((N, OH, OW), 77, dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(lib.addk_score_upsample_ws_floats(N, OH, OW)), device=dev)
    a = L.ScoreUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, 19, OH, OW
    a.target, a.class_w, a.ignore_index = tgt.data_ptr(), None, 255
    a.wsum, a.scale, a.loss_out, a.ent_out = wsum.data_ptr(), 1.0, loss.data_ptr(), ent.data_ptr()
    a.cm, a.pred_out, a.ws = cm.data_ptr(), pred.data_ptr(), ws.data_ptr()
    L.check(lib.addk_score_upsample(C.byref(a), _stream()), 'score_upsample')
    torch.cuda.synchronize()
    return pred.cpu()


def _argmax(y):
    """addk_argmax_nchw of NCHW logits, as the uint8 map a label head writes"""
    lib, L = _lib()
    N, Cc, OH, OW = y.shape
    y = y.contiguous()
    am = torch.empty((N, OH, OW), dtype=torch.int64, device=y.device)
    L.check(lib.addk_argmax_nchw(y.data_ptr(), N, Cc, OH * OW, am.data_ptr(), _stream()), 'argmax_nchw')
    torch.cuda.synchronize()
    return am.to(torch.uint8).cpu()


def _materialised(xa, ld, shape):
    """addk_argmax_nchw of addk_resize_fwd's NCHW output"""
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape
    y = torch.empty((N, 19, OH, OW), device=xa.device)
    ar = L.ResizeArgs()
    ar.src.x, ar.src.ld, ar.src.C = xa.data_ptr(), ld, 19
    ar.N, ar.H, ar.W, ar.OH, ar.OW = N, H, W, OH, OW
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    L.check(lib.addk_resize_fwd(C.byref(ar), _stream()), 'resize_fwd')
    return _argmax(y)


@functools.lru_cache(maxsize=None)
def _reference(case, dev):
    """The two existing paths on the stride-24 logits of one case, computed once and never modified."""
    shape = CASES[case]
    xa = _padded(_logits(case), dev)
    return _score_pred(xa, LD, shape), _materialised(xa, LD, shape)


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [LD, 19], ids=['stride24', 'dense19'])
@pytest.mark.parametrize('case', list(CASES))
def test_label_upsample_equals_the_existing_paths(dev, case, ld):
    lib, L = _lib()
    N, (H, W), (OH, OW) = shape = CASES[case]
    assert lib.addk_label_upsample_supported(N, H, W, OH, OW, 19) == 1
    scored, materialised = _reference(case, dev)
    xa = _padded(_logits(case), dev) if ld == LD else _logits(case).to(dev).contiguous()
    rc, m = _label(xa, ld, shape)
    assert rc == 0
    got = m.read()
    assert len(got.unique()) > 4                                             # a real map, not a constant
    assert torch.equal(got, scored)
    assert torch.equal(got, materialised)
    if ld == 19:                                                             # the references of the scalar loader itself
        assert torch.equal(got, _score_pred(xa, 19, shape)) and torch.equal(got, _materialised(xa, 19, shape))
    else:                                                                    # other garbage in the padding channels: nothing moves
        assert torch.equal(_label(_padded(_logits(case), dev, seed=2), ld, shape)[1].read(), got)
    # a second launch into the same buffer gives the same bytes
    rc, m = _label(xa, ld, shape, into=m)
    assert rc == 0 and torch.equal(m.read(), got)


@pytest.mark.parametrize('case', ['odd_ladder', 'down'])
def test_label_upsample_lut(dev, case):
    shape = CASES[case]
    xa = _padded(_logits(case), dev)
    lut = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 256).astype(np.uint8))
    plain = _label(xa, LD, shape)[1].read()
    rc, m = _label(xa, LD, shape, lut=lut.to(dev))
    assert rc == 0 and torch.equal(m.read(), lut[plain.long()])
    from addk.data import VALID_CLASSES, decode_segmap_lut
    ids = _label(xa, LD, shape, lut=torch.from_numpy(decode_segmap_lut()).to(dev))[1].read()
    assert torch.equal(ids, torch.tensor(VALID_CLASSES, dtype=torch.uint8)[plain.long()])


@pytest.mark.parametrize('ld', [LD, 19], ids=['stride24', 'dense19'])
def test_label_upsample_ties_go_to_the_lowest_channel(dev, ld):
    shape = CASES['odd_ladder']
    x = _logits('odd_ladder').clone()
    top = x.amax(-1) + 1.0
    x[..., 3] = top
    x[..., 11] = top                                                         # two identical planes above every other channel
    xa = _padded(x, dev) if ld == LD else x.to(dev).contiguous()
    rc, m = _label(xa, ld, shape)
    assert rc == 0 and bool((m.read() == 3).all())
    assert bool((_materialised(xa, ld, shape) == 3).all())


class _Gate:
    """One set of buffers of the gate launches: threshold word, device and pinned outputs, workspace zeroed ONCE."""

    def __init__(self, shape, dev):
        lib, L = _lib()
        N, _, (OH, OW) = self.shape = shape
        self.thr = torch.zeros(1, device=dev)
        self.out = torch.full((N, 2), -7.0, device=dev)
        self.host = torch.full((N, 2), -9.0).pin_memory()
        self.ws = torch.zeros(int(lib.addk_gate_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=dev)

    def args(self, xa, ld, C_=19):
        _, L = _lib()
        N, (H, W), (OH, OW) = self.shape
        a = L.GateUpsampleArgs()
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xa.data_ptr(), ld, N, H, W, C_, OH, OW
        a.max_thr, a.out, a.out_host, a.ws = self.thr.data_ptr(), self.out.data_ptr(), self.host.data_ptr(), self.ws.data_ptr()
        return a

    def reset(self, thr):
        self.thr.fill_(thr)
        self.out.fill_(-7.0)
        self.host.fill_(-9.0)

    def result(self):
        torch.cuda.synchronize()
        return self.out.cpu().clone(), self.host.clone()

    def ticket(self):
        return int(self.ws[:4].view(torch.int32).item())


def _gate_label_args(gate, xa, ld, m, lut=None, C_=19):
    _, L = _lib()
    b = L.GateLabelUpsampleArgs()
    b.gate = gate.args(xa, ld, C_)
    b.lut256, b.labels = lut.data_ptr() if lut is not None else None, m.ptr
    return b


@pytest.mark.parametrize('ld', [LD, 19], ids=['stride24', 'dense19'])
@pytest.mark.parametrize('case', GATE_CASES)
def test_gate_label_upsample_is_the_gate_and_the_label_head(dev, case, ld):
    lib, L = _lib()
    shape = CASES[case]
    thr = 0.5
    xa = _padded(_logits(case), dev) if ld == LD else _logits(case).to(dev).contiguous()
    plain = _Gate(shape, dev)
    plain.reset(thr)
    L.check(lib.addk_gate_upsample(C.byref(plain.args(xa, ld)), _stream()), 'gate_upsample')
    want_out, want_host = plain.result()
    assert torch.equal(want_out, want_host)
    assert bool((want_out[:, 1] > 0).all()) and bool((want_out[:, 1] < 1).all())      # the threshold lies inside the top probabilities
    want_map = _label(xa, ld, shape)[1].read()
    gate, m = _Gate(shape, dev), _Map(shape, dev)
    for launch in range(2):                                                  # the workspace was zeroed once
        gate.reset(thr)
        L.check(lib.addk_gate_label_upsample(C.byref(_gate_label_args(gate, xa, ld, m)), _stream()), 'gate_label_upsample')
        out, host = gate.result()
        assert torch.equal(out, want_out) and torch.equal(host, want_out)
        assert torch.equal(m.read(), want_map)
        assert gate.ticket() == 0
    lut = torch.from_numpy(np.random.default_rng(6).integers(0, 256, 256).astype(np.uint8))
    gate.reset(thr)
    L.check(lib.addk_gate_label_upsample(C.byref(_gate_label_args(gate, xa, ld, m, lut=lut.to(dev))), _stream()), 'gate_label_upsample')
    out, host = gate.result()
    assert torch.equal(out, want_out) and torch.equal(host, want_out) and torch.equal(m.read(), lut[want_map.long()])


def test_gate_label_upsample_replays_from_a_graph(dev):
    lib, L = _lib()
    case = 'odd_ladder'
    shape = CASES[case]
    xa = _padded(_logits(case), dev)
    gate, m = _Gate(shape, dev), _Map(shape, dev)
    b = _gate_label_args(gate, xa, LD, m)
    gate.reset(0.5)
    L.check(lib.addk_gate_label_upsample(C.byref(b), _stream()), 'gate_label_upsample')
    want_out, want_host = gate.result()
    want_map = m.read()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(lib.addk_gate_label_upsample(C.byref(b), _stream()), 'gate_label_upsample')
    for replay in range(2):
        gate.reset(0.5)
        m.raw.fill_(0xAB)
        graph.replay()
        out, host = gate.result()
        assert torch.equal(out, want_out) and torch.equal(host, want_host) and torch.equal(m.read(), want_map)
        assert gate.ticket() == 0


def test_label_heads_refuse_what_they_do_not_take(dev):
    import addk
    lib, L = _lib()
    shape = (2, (8, 16), (64, 128))
    assert lib.addk_label_upsample_supported(2, 8, 16, 64, 128, 7) == 0
    assert lib.addk_gate_upsample_supported(2, 8, 16, 64, 128, 7) == 0
    xa = torch.zeros((2, 8, 16, 8), device=dev)
    rc, m = _label(xa, 8, shape, C_=7)
    assert rc == -1 and m.untouched()                                        # ADDK_ERR_INVALID, and no launch
    with pytest.raises(addk.AddkError):
        L.check(rc, 'label_upsample')
    gate = _Gate(shape, dev)
    gate.reset(0.5)
    rc = lib.addk_gate_label_upsample(C.byref(_gate_label_args(gate, xa, 8, m, C_=7)), _stream())
    out, host = gate.result()
    assert rc == -1 and m.untouched()
    assert torch.equal(out, torch.full((2, 2), -7.0)) and torch.equal(host, torch.full((2, 2), -9.0)) and gate.ticket() == 0
    assert lib.addk_label_upsample(C.byref(L.LabelUpsampleArgs()), None) == -1           # null pointers
    assert lib.addk_gate_label_upsample(C.byref(L.GateLabelUpsampleArgs()), None) == -1


# ------------------------------------------------------------------------------------------------------------------------
# public path
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(dev):
    """F = 4, config 2.  Synthetic weights drive the last exit's logits to |z| ~ 1e5 (every softmax one-hot): the classifier is scaled
    down as in tests/test_gpu_validate.py, which leaves every arg-max where it was."""
    from addk.modeling.ADD import ADD, EDM
    from addk.module import conv2d
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), 0)
    fill_params(m, 600)
    with torch.no_grad():
        m.decoder._conv[7].weight.mul_(4e-5)
        m.decoder._conv[7].bias.mul_(4e-5)
    edm = EDM()
    edm.conv = conv2d(4 * 5 * 4, 128, 3, stride=2, padding=1, bias=False)    # the gated feature of F = 4 has 80 channels, not 400
    fill_params(edm, 701)
    return m.to(dev).eval(), edm.to(dev).eval()


# (forces the early exit, forbids it): 'entropy' leaves below the threshold; 'max' when share(t) > t, and the share is 1 at t <= 0 and 0
# at t >= 1; 'edm' goes on when the confidence is above the threshold
THRESHOLDS = {'entropy': (float('inf'), float('-inf')), 'max': (-0.5, 1.5), 'edm': (1e30, -1e30)}


@pytest.mark.parametrize('hw', [(65, 129), (64, 128)], ids=['65x129', '64x128'])
@pytest.mark.parametrize('kind', list(THRESHOLDS))
def test_dynamic_inference_labels_are_the_argmax_of_its_logits(dev, kind, hw):
    m, edm = _model(dev)
    x = rand_tensor(9, 'label_dynx', (1, 3) + hw).to(dev)
    maps = {}
    with torch.no_grad():
        for want_early, thr in zip((1, 0), THRESHOLDS[kind]):
            for call in range(5):                                            # calls 3+ replay captured graphs
                y, early, secs, val = m.dynamic_inference(x, threshold=thr, confidence=kind, edm=edm)
                assert early == want_early and tuple(y.shape) == (1, 19) + hw
                want, val = _argmax(y), (val.clone() if torch.is_tensor(val) else val)
                lab, early_l, secs_l, val_l = m.dynamic_inference(x, threshold=thr, confidence=kind, edm=edm, output='labels')
                assert lab.dtype == torch.uint8 and tuple(lab.shape) == (1,) + hw and isinstance(secs_l, float)
                assert early_l == early
                assert torch.equal(val_l, val) if torch.is_tensor(val) else (isinstance(val_l, float) and val_l == val)
                assert torch.equal(lab.cpu(), want), (kind, thr, call, int((lab.cpu() != want).sum()))
            maps[want_early] = want
    assert len(maps[0].unique()) > 1 and not torch.equal(maps[0], maps[1])    # two different, non-constant maps
    lab_plan = m._dynamic_plan(x, edm, 'labels') if kind == 'edm' else m._gate_plan(x, kind, 'labels')
    names = [c.name for c in lab_plan.g.fwd]
    assert 'resize_nchw' not in names and lab_plan.calls >= 10 and len(lab_plan.graphs) >= 2
    if kind != 'edm':
        assert lab_plan.heads[0].gate_fused and names.count('gate_label_upsample') == 1


@pytest.mark.parametrize('exit', [0, 1])
def test_segmenter_equals_the_argmax_of_forward(dev, exit):
    from addk.data import VALID_CLASSES, decode_segmap_lut
    from addk.segment import Segmenter
    m, _ = _model(dev)
    shape = (2, 3, 65, 129)
    xs = [rand_tensor(21 + i, 'label_segx', shape).to(dev) for i in range(2)]
    try:
        with torch.no_grad():
            wants = [_argmax(m.eval()(x)[exit]) for x in xs]
        assert not torch.equal(wants[0], wants[1])
        m.train()                                                            # the Segmenter must not care, and must not touch it
        before = {k: v.clone() for k, v in m.state_dict().items()}
        seg = Segmenter(m, shape, exit=exit)
        ids = Segmenter(m, shape, exit=exit - 2, label_lut=decode_segmap_lut())     # the same exit, counted from the end
        assert ids.exit == seg.exit == exit
        table = torch.tensor(VALID_CLASSES, dtype=torch.uint8)
        for call in range(4):                                                # two eager calls, the capture, a replay
            y = seg.step(xs[call % 2])
            assert y.dtype == torch.uint8 and tuple(y.shape) == (2, 65, 129)
            assert torch.equal(y.cpu(), wants[call % 2]), (call, int((y.cpu() != wants[call % 2]).sum()))
            assert torch.equal(ids.step(xs[call % 2]).cpu(), table[wants[call % 2].long()])
        assert seg.graph is not None and ids.graph is not None
        assert 'resize_nchw' not in [c.name for c in seg.g.fwd]
        assert m.training
        after = m.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        seg.close(), ids.close()
    finally:
        m.eval()
