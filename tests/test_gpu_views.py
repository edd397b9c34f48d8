"""GPU tests of multi-scale + flip label maps: the multi-view label head (addk_label_views_upsample) through the C ABI against the fp64
arg-max of the formula it implements, and segment.MultiViewSegmenter against the same formula on the logits the model itself returns.

The rule of every comparison with fp64 is tests/_views_ref.py's: e32 = max |fp32 - fp64| of the torch formula on the CPU for these very
inputs, tau = 64 * e32; a pixel whose fp64 top-2 gap is below tau is excused, at most 0.2 % of the pixels may be, every other pixel must
carry the fp64 arg-max.  For the kernel cases: tau = 6.0e-6 (three_scales), 4.0e-5 (odd), 3.4e-5 (down_one), 1.1e-3 (eight)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402
import _views_ref as R                                                                     # noqa: E402

LD = 24
GUARD = 64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    import addk._lib as L
    return L.load(), L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Map:
    """A label buffer between two guards of 64 bytes of 0xAB."""

    def __init__(self, N, size, dev):
        self.n, self.dims = N * size[0] * size[1], (N,) + tuple(size)
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


def _device_logits(x, ld, dev, seed=1):
    """x [B,h,w,19] on the device -> (tensor that owns the memory, address of pixel 0).  ld == 24: finite garbage in the padding channels,
    16-byte aligned (the vector loader); ld == 19: dense, from a base offset by one float (the scalar loader)."""
    if ld == LD:
        xa = (rand_tensor(seed, 'views_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
        xa[..., :19] = x.to(dev)
        xa = xa.contiguous()
        assert xa.data_ptr() % 16 == 0
        return xa, xa.data_ptr()
    flat = torch.full((x.numel() + 1,), 1e30, device=dev)
    flat[1:] = x.to(dev).reshape(-1)
    assert (flat.data_ptr() + 4) % 16 != 0
    return flat, flat.data_ptr() + 4


def _launch(vs, N, size, ld, dev, lut=None, C_=19, nview=None, into=None, edit=None):
    """addk_label_views_upsample on the views `vs` ([(x [B,h,w,19], n0, mirror, weight)]) -> (rc, _Map)"""
    lib, L = _lib()
    m = into if into is not None else _Map(N, size, dev)
    a, keep = L.LabelViewsArgs(), {}
    for i, (x, n0, mirror, weight) in enumerate(vs):
        if id(x) not in keep:                                                # the plain and the mirrored view share one batch-2N tensor
            keep[id(x)] = _device_logits(x, ld, dev)
        v = a.view[i]
        v.logits, v.ld, v.n0, v.H, v.W, v.mirror, v.weight = keep[id(x)][1], ld, n0, x.shape[1], x.shape[2], mirror, weight
    a.nview, a.N, a.C, a.OH, a.OW = (len(vs) if nview is None else nview), N, C_, size[0], size[1]
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, m.ptr
    if edit is not None:
        edit(a)
    rc = lib.addk_label_views_upsample(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, m


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [LD, 19], ids=['stride24', 'dense19'])
@pytest.mark.parametrize('case', list(R.CASES))
def test_label_views_upsample_is_the_fp64_argmax(dev, case, ld):
    lib, L = _lib()
    N, _, size = R.CASES[case]
    vs = R.views(case)
    assert lib.addk_label_views_upsample_supported(len(vs), N, size[0], size[1], 19) == 1
    _, want, excused, e32, tau = R.reference(case)
    rc, m = _launch(vs, N, size, ld, dev)
    assert rc == 0
    got = m.read()                                                           # the guards are checked here
    print('%s/%d: e32 = %.2e, tau = %.2e' % (case, ld, e32, tau))
    R.check_map(got, want, excused, '%s/%d' % (case, ld))
    assert len(got.unique()) > 4                                             # a real map, not a constant
    # a second launch into the same buffer gives the same bytes
    rc, m = _launch(vs, N, size, ld, dev, into=m)
    assert rc == 0 and torch.equal(m.read(), got)


@pytest.mark.parametrize('case', ['odd', 'down_one'])
def test_two_half_weight_views_are_the_one_view_map(dev, case):
    N, sizes, size = R.CASES[case]
    x = R.views(case)[0][0]
    one = _launch([(x, 0, 0, 1.0)], N, size, LD, dev)[1].read()
    rc, m = _launch([(x, 0, 0, 0.5), (x, 0, 0, 0.5)], N, size, LD, dev)
    assert rc == 0 and torch.equal(m.read(), one)
    # ... and one view's map is the label head's: soft-max keeps the arg-max of the logits
    lib, L = _lib()
    xa, ptr = _device_logits(x, LD, dev)
    lab = _Map(N, size, dev)
    a = L.LabelUpsampleArgs()
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = ptr, LD, N, x.shape[1], x.shape[2], 19, size[0], size[1]
    a.lut256, a.labels = None, lab.ptr
    L.check(lib.addk_label_upsample(C.byref(a), _stream()), 'label_upsample')
    torch.cuda.synchronize()
    differ = lab.read() != one                                               # only where exp rounds two near-equal logits to one value
    assert float(differ.float().mean()) <= R.CAP


@pytest.mark.parametrize('case', ['odd', 'eight'])
def test_label_views_upsample_lut(dev, case):
    N, _, size = R.CASES[case]
    vs = R.views(case)
    lut = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 256).astype(np.uint8))
    plain = _launch(vs, N, size, LD, dev)[1].read()
    rc, m = _launch(vs, N, size, LD, dev, lut=lut.to(dev))
    assert rc == 0 and torch.equal(m.read(), lut[plain.long()])


def test_label_views_upsample_refuses_what_it_does_not_take(dev):
    import addk
    lib, L = _lib()
    N, _, size = R.CASES['three_scales']
    vs = R.views('three_scales')
    m = _Map(N, size, dev)

    def setter(**kw):
        def edit(a):
            for k, v in kw.items():
                if k.startswith('view1_'):
                    setattr(a.view[1], k[6:], v)
                else:
                    setattr(a, k, v)
        return edit
    bad = [dict(nview=0), dict(nview=9), dict(nview=-1), dict(C=21), dict(C=7), dict(labels=None), dict(view1_logits=None),
           dict(view1_weight=0.0), dict(view1_weight=-0.5), dict(view1_weight=float('inf')), dict(view1_weight=float('nan')),
           dict(N=0), dict(N=65536), dict(OH=0), dict(OW=-3), dict(OH=65536 * 16 + 1), dict(view1_H=0), dict(view1_W=-1), dict(view1_ld=18),
           dict(view1_n0=-1)]
    for kw in bad:
        rc, _ = _launch(vs, N, size, LD, dev, into=m, edit=setter(**kw))
        assert rc == -1 and m.untouched(), kw                                # ADDK_ERR_INVALID, and no launch
    with pytest.raises(addk.AddkError):
        L.check(rc, 'label_views_upsample')
    assert lib.addk_label_views_upsample(C.byref(L.LabelViewsArgs()), None) == -1
    rc, _ = _launch(vs, N, size, LD, dev, into=m)                            # the same arguments, unedited, are taken
    assert rc == 0 and not m.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# public path
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(dev):
    """F = 4, config 2; the recipe of tests/test_gpu_labels.py::_model.  Synthetic weights drive the last exit's logits to |z| ~ 1e5 (every
    softmax one-hot): the classifier is scaled down, which leaves every arg-max where it was."""
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), 0)
    fill_params(m, 600)
    with torch.no_grad():
        m.decoder._conv[7].weight.mul_(4e-5)
        m.decoder._conv[7].bias.mul_(4e-5)
    return m.to(dev).eval()


def _judge(vs, N, size, what):
    """the rule of tests/_views_ref.py on views given as NHWC tensors: (fp64 arg-max, excused pixels)"""
    a64 = R.formula(vs, N, size, torch.float64)
    e32 = float((R.formula(vs, N, size, torch.float32).double() - a64).abs().max())
    print('%s: e32 = %.2e, tau = %.2e' % (what, e32, R.FACTOR * e32))
    return R.judge(a64, R.FACTOR * e32)[1:]


# The amplitude of the images decides how many pixels the fp64 formula ITSELF leaves within tau of a tie (the excused share is a property
# of the reference, whatever computes the map).  This model's first exit answers unit-variance images with logits of ~1e-3: its
# probabilities are flat to 1e-4 and 0.27 % of the pixels are excused (46 of 16770; the cap allows 33); at amplitude 4, 0.08 - 0.11 %.
# The last exit is nearly one-hot already at amplitude 1 (0.006 - 0.024 % excused); at amplitude 4 the two views saturate on different
# classes and 1 % of the pixels are exact 0.5 / 0.5 ties.  So each exit gets the amplitude at which its prediction is neither.
@pytest.mark.parametrize('exit,amplitude', [(0, 4.0), (1, 1.0)], ids=['exit0', 'exit1'])
def test_flip_averaging_equals_the_formula_on_forward(dev, exit, amplitude):
    from addk.segment import MultiViewSegmenter
    m = _model(dev)
    N, size = 2, (65, 129)
    shape = (N, 3) + size
    xs = [(rand_tensor(31 + i, 'views_segx', shape) * amplitude).to(dev) for i in range(2)]
    try:
        wants = []
        with torch.no_grad():
            for x in xs:                                                     # 0.5 softmax(model(x)[k]) + 0.5 softmax(model(flip x)[k]) flipped back
                ya, yb = m(x)[exit], m(x.flip(3))[exit]
                vs = [(ya.permute(0, 2, 3, 1).cpu(), 0, 0, 0.5), (yb.permute(0, 2, 3, 1).cpu(), 0, 1, 0.5)]
                wants.append(_judge(vs, N, size, 'flip/exit%d' % exit))
        assert not torch.equal(wants[0][0], wants[1][0]) and len(wants[0][0].unique()) > 1
        m.train()                                                            # the step must not care, and must not touch it
        before = {k: v.clone() for k, v in m.state_dict().items()}
        seg = MultiViewSegmenter(m, shape, scales=(1.0,), flip=True, exit=exit)
        assert seg.exit == exit and [(s, mir, hw) for s, mir, hw, _ in seg.views] == [(1.0, False, size), (1.0, True, size)]
        for call in range(4):                                                # two eager calls, the capture, a replay
            y = seg.step(xs[call % 2])
            assert y.dtype == torch.uint8 and tuple(y.shape) == (N,) + size
            R.check_map(y.cpu(), *wants[call % 2], 'flip/exit%d/call%d' % (exit, call))
        assert seg.graph is not None
        names = [c.name for c in seg.g.fwd]
        assert names.count('label_views_upsample') == 1 and 'resize_nchw' not in names
        assert m.training
        after = m.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        seg.close()
    finally:
        m.eval()


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def test_three_scales_with_flip(dev):
    from addk.segment import MultiViewSegmenter
    m = _model(dev)
    N, size, exit = 2, (64, 128), 1
    shape = (N, 3) + size
    x = rand_tensor(33, 'views_msx', shape).to(dev)
    seg = MultiViewSegmenter(m, shape, scales=(0.75, 1.0, 1.25), flip=True)
    assert seg.exit == exit and [hw for _, _, hw, _ in seg.views] == [(48, 96)] * 2 + [(64, 128)] * 2 + [(80, 160)] * 2
    for call in range(4):
        y = seg.step(x).cpu()
        logits = [t.cpu() for t in seg.view_logits()]
        vs = [(t, 0, int(mir), 1.0 / 6) for t, (_, mir, _, _) in zip(logits, seg.views)]
        want, excused = _judge(vs, N, size, 'three_scales/call%d' % call)
        R.check_map(y, want, excused, 'three_scales/call%d' % call)
        assert len(y.unique()) > 1
    assert seg.graph is not None
    # every view is the model on that view of the images: its logits, up-sampled to the view's size, against model(x_v)[k]
    with torch.no_grad():
        for t, (s, mir, hw, low) in zip(logits, seg.views):
            assert tuple(t.shape) == (N,) + low + (19,)
            xv = F.interpolate(x.flip(3) if mir else x, hw, mode='bilinear', align_corners=False) if hw != size else (x.flip(3) if mir else x)
            ref = m(xv.contiguous())[exit]
            up = F.interpolate(t.permute(0, 3, 1, 2).to(dev), hw, mode='bilinear', align_corners=False)
            err = _rel_l2(up, ref)
            print('view scale %g mirror %d: rel L2 %.2e' % (s, mir, err))
            assert err < 1e-3, (s, mir, err)
    seg.close()
