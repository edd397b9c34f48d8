"""GPU tests of sliding-window label maps: the tiled label head (addk_label_tiles_upsample) through the C ABI against the fp64 arg-max of
the formula it implements, addk_gather_tiles against torch's crop-and-pad, and segment.TiledSegmenter against the same formula on the
logits it stored and against the model on every window.

The rule of every comparison with fp64 is tests/_views_ref.py's, through tests/_tiles_ref.py: e32 = max |fp32 - fp64| of the torch formula on
the CPU for these very inputs, tau = 64 * e32; a pixel whose fp64 top-2 gap is below tau is excused, at most 0.2 % of the pixels may be,
every other pixel must carry the fp64 arg-max."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402
import _tiles_ref as R                                                                     # noqa: E402

LD = 24
GUARD = 64
T0 = {'pad': 3, 'grid': 2}            # cases whose tiles sit behind others in the store (t0 > 0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    import addk._lib as L
    return L.load(), L


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """`n` bytes between two guards of 64 bytes of 0xAB; the bytes themselves start as 0xAB too."""

    def __init__(self, n, dev):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def read(self):
        """the bytes on the host; the guards must be untouched"""
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == 0xAB).all()) and bool((raw[GUARD + self.n:] == 0xAB).all()), 'a guard byte was written'
        return raw[GUARD:GUARD + self.n].clone()

    def untouched(self):
        return bool((self.raw.cpu() == 0xAB).all())


def _map(N, size, dev):
    m = _Guarded(N * size[0] * size[1], dev)
    m.dims = (N,) + tuple(size)
    return m


def _device_tiles(x, ld, t0, dev):
    """x [T,h,w,C] -> (tensor that owns the memory, address of tile 0 of the store); the case's tiles are tiles t0.. of the store, the ones
    in front of them hold other values.  ld == 24: finite garbage in the padding channels, 16-byte aligned (the vector loader); ld == C:
    dense, from a base offset by one float (the scalar loader)."""
    T, h, w, Cc = x.shape
    if t0:
        x = torch.cat([rand_tensor(3, 'tiles_front', (t0, h, w, Cc)) * 7, x])
    if ld == LD:
        xa = (rand_tensor(1, 'tiles_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
        xa[..., :Cc] = x.to(dev)
        xa = xa.contiguous()
        assert xa.data_ptr() % 16 == 0
        return xa, xa.data_ptr()
    assert ld == Cc
    flat = torch.full((x.numel() + 1,), 1e30, device=dev)
    flat[1:] = x.to(dev).reshape(-1)
    assert (flat.data_ptr() + 4) % 16 != 0
    return flat, flat.data_ptr() + 4


def _launch(case, Cc, ld, dev, lut=None, into=None, edit=None):
    """addk_label_tiles_upsample on a case -> (rc, guarded map)"""
    lib, L = _lib()
    N, size, tile, _, (h, w) = R.CASES[case]
    ys, xs = R.origins(case)
    t0 = T0.get(case, 0)
    m = into if into is not None else _map(N, size, dev)
    keep, ptr = _device_tiles(R.logits(case, Cc), ld, t0, dev)
    a = L.LabelTilesArgs()
    a.logits, a.ld, a.h, a.w, a.th, a.tw = ptr, ld, h, w, tile[0], tile[1]
    a.N, a.C, a.OH, a.OW, a.t0, a.ny, a.nx = N, Cc, size[0], size[1], t0, len(ys), len(xs)
    a.y0[:len(ys)], a.x0[:len(xs)] = ys, xs
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, m.ptr
    if edit is not None:
        edit(a)
    rc = lib.addk_label_tiles_upsample(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, m


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [LD, 0], ids=['stride24', 'dense'])
@pytest.mark.parametrize('Cc', R.CLASSES)
@pytest.mark.parametrize('case', list(R.CASES))
def test_label_tiles_upsample_is_the_fp64_argmax(dev, case, Cc, ld):
    lib, L = _lib()
    ld = ld or Cc
    N, size, _, _, _ = R.CASES[case]
    ys, xs = R.origins(case)
    assert lib.addk_label_tiles_upsample_supported(N, size[0], size[1], len(ys), len(xs), Cc) == 1
    _, want, excused, e32, tau = R.reference(case, Cc)
    rc, m = _launch(case, Cc, ld, dev)
    assert rc == 0
    got = m.read().view(m.dims)                                              # the guards are checked here
    print('%s/C%d/%d: e32 = %.2e, tau = %.2e, t0 = %d' % (case, Cc, ld, e32, tau, T0.get(case, 0)))
    R.check_map(got, want, excused, '%s/C%d/%d' % (case, Cc, ld))
    assert len(got.unique()) > 4                                             # a real map, not a constant
    # a second launch into the same buffer gives the same bytes
    rc, m = _launch(case, Cc, ld, dev, into=m)
    assert rc == 0 and torch.equal(m.read().view(m.dims), got)


@pytest.mark.parametrize('ld', [LD, 19], ids=['stride24', 'dense19'])
def test_one_window_is_one_view_bit_for_bit(dev, ld):
    lib, L = _lib()
    N, size, tile, _, (h, w) = R.CASES['exact']
    assert N == 1 and size == tile and R.origins('exact') == ([0], [0])
    rc, m = _launch('exact', 19, ld, dev)
    assert rc == 0
    keep, ptr = _device_tiles(R.logits('exact', 19), ld, 0, dev)
    lab = _map(N, size, dev)
    a = L.LabelViewsArgs()
    v = a.view[0]
    v.logits, v.ld, v.n0, v.H, v.W, v.mirror, v.weight = ptr, ld, 0, h, w, 0, 1.0
    a.nview, a.N, a.C, a.OH, a.OW, a.lut256, a.labels = 1, N, 19, size[0], size[1], None, lab.ptr
    L.check(lib.addk_label_views_upsample(C.byref(a), _stream()), 'label_views_upsample')
    torch.cuda.synchronize()
    assert torch.equal(m.read(), lab.read())


@pytest.mark.parametrize('case,Cc', [('grid', 21), ('odd', 19)])
def test_label_tiles_upsample_lut(dev, case, Cc):
    lut = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 256).astype(np.uint8))
    plain = _launch(case, Cc, LD, dev)[1].read()
    rc, m = _launch(case, Cc, LD, dev, lut=lut.to(dev))
    assert rc == 0 and torch.equal(m.read(), lut[plain.long()])


def test_label_tiles_upsample_refuses_what_it_does_not_take(dev):
    import addk
    lib, L = _lib()
    N, size = R.CASES['grid'][:2]
    m = _map(N, size, dev)
    for edit in R.REFUSALS:
        rc, _ = _launch('grid', 19, LD, dev, into=m, edit=edit)
        assert rc == -1 and m.untouched(), edit.what                         # ADDK_ERR_INVALID, and no launch
    with pytest.raises(addk.AddkError):
        L.check(rc, 'label_tiles_upsample')
    assert lib.addk_label_tiles_upsample(C.byref(L.LabelTilesArgs()), None) == -1
    rc, _ = _launch('grid', 19, LD, dev, into=m)                             # the same arguments, unedited, are taken
    assert rc == 0 and not m.untouched()
    m.read()


# ------------------------------------------------------------------------------------------------------------------------
# addk_gather_tiles
# ------------------------------------------------------------------------------------------------------------------------
def _crop_pad(img, y0, x0, th, tw):
    """torch's form: pad the image with zeros on the right and at the bottom, then crop"""
    return F.pad(img, (0, tw, 0, th))[:, y0:y0 + th, x0:x0 + tw]


# (sizes of the two images, tile, B, windows as (image, y0, x0)): inside the image, over its right edge, over its bottom edge, over both, a
# window larger than its image, and one that starts inside the small image; ntiles < B.  The first has more output rows than the launch has
# workgroup rows, the second more columns than a workgroup
@pytest.mark.parametrize('sizes,tile,B,wins', [
    (((150, 70), (60, 30)), (100, 40), 8, [(0, 5, 7), (0, 10, 50), (0, 90, 3), (0, 90, 50), (1, 0, 0), (1, 30, 15)]),
    (((40, 700), (3, 9)), (5, 300), 5, [(0, 0, 0), (0, 35, 400), (0, 10, 650), (1, 0, 0)])], ids=['rows', 'columns'])
def test_gather_tiles_is_crop_and_pad(dev, sizes, tile, B, wins):
    lib, L = _lib()
    Cin, (th, tw) = 3, tile
    imgs = [rand_tensor(9, 'tiles_img:%d' % i, (Cin,) + s).to(dev).contiguous() for i, s in enumerate(sizes)]
    arr = (L.TileDesc * len(wins))()
    for d, (k, y0, x0) in zip(arr, wins):
        d.image, d.H, d.W, d.y0, d.x0 = imgs[k].data_ptr(), sizes[k][0], sizes[k][1], y0, x0
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    x = _Guarded(B * Cin * th * tw * 4, dev)
    assert len(wins) < B
    rc = lib.addk_gather_tiles(table.data_ptr(), len(wins), Cin, th, tw, x.ptr, B, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = x.read().view(torch.float32).view(B, Cin, th, tw)
    want = torch.zeros((B, Cin, th, tw))
    for b, (k, y0, x0) in enumerate(wins):
        want[b] = _crop_pad(imgs[k].cpu(), y0, x0, th, tw)
    assert torch.equal(got, want)                                            # exactly; the slots behind the windows are zero
    assert float(want[:len(wins)].abs().sum()) > 0 and bool((want[len(wins) - 1] == 0).any())
    # refused without a launch
    y = _Guarded(64, dev)
    for bad in ((None, 1, Cin, th, tw, y.ptr, B), (table.data_ptr(), 1, Cin, th, tw, None, B), (table.data_ptr(), B + 1, Cin, th, tw, y.ptr, B),
                (table.data_ptr(), -1, Cin, th, tw, y.ptr, B), (table.data_ptr(), 1, 0, th, tw, y.ptr, B), (table.data_ptr(), 1, Cin, 0, tw, y.ptr, B),
                (table.data_ptr(), 1, Cin, th, -1, y.ptr, B), (table.data_ptr(), 0, Cin, th, tw, y.ptr, 0)):
        assert lib.addk_gather_tiles(*bad, _stream()) == -1, bad
    torch.cuda.synchronize()
    assert y.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# public path
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(dev):
    """F = 4, config 2; the recipe of tests/test_gpu_views.py::_model (same classifier scaling, which leaves every arg-max where it was)."""
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), 0)
    fill_params(m, 600)
    with torch.no_grad():
        m.decoder._conv[7].weight.mul_(4e-5)
        m.decoder._conv[7].bias.mul_(4e-5)
    return m.to(dev).eval()


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


TILE, STRIDE = (3, 3, 65, 129), (32, 71)


# The amplitude of the images decides how many pixels the fp64 formula ITSELF leaves within tau of a tie (tests/test_gpu_views.py says why:
# the excused share is a property of the reference, whatever computes the map).  This model's first exit answers unit-variance images
# with logits of ~1e-2: its probabilities are flat, and the reference excuses 0.2 - 0.5 % of these images' pixels at amplitude 1 and still
# 0.3 % of the 40 x 100 image at amplitude 4, the amplitude of that file (a zero-padded window and a sum over up to four windows are new
# here); at amplitude 32 (logits up to ~2) it excuses 0.01 - 0.05 %, and no more than 0.15 % with four times the tau.  The last exit is
# nearly one-hot at amplitude 1 (at most 0.005 % excused) and saturates at 4 (up to 1.1 %: exact ties between windows).  The shares were
# evaluated on the CPU with the oracle model on the zero-padded crops; the test prints what it finds.
@pytest.mark.parametrize('exit,amplitude', [(0, 32.0), (1, 1.0)], ids=['exit0', 'exit1'])
def test_tiled_segmenter_equals_the_formula_and_the_model_on_every_window(dev, exit, amplitude):
    from addk.segment import Segmenter, TiledSegmenter, tile_starts
    m = _model(dev)
    B, Cin, th, tw = TILE
    batch = (rand_tensor(41, 'tiles_segx', (2, 3, 97, 200)) * amplitude).to(dev)
    several = [(rand_tensor(42 + i, 'tiles_segl', (3,) + s) * amplitude).to(dev) for i, s in enumerate(((65, 129), (40, 100), (97, 200)))]
    inputs = [batch, several]
    try:
        m.train()                                                            # the step must not care, and must not touch it
        before = {k: v.clone() for k, v in m.state_dict().items()}
        seg = TiledSegmenter(m, TILE, STRIDE, exit=exit)
        assert seg.exit == exit
        kept = {}
        for call in range(4):                                                # chunks run eagerly twice, then the capture, then replays
            images = inputs[call % 2]
            maps = seg.segment(images)
            logits = seg.tile_logits().cpu()
            imgs = list(images.unbind(0)) if isinstance(images, torch.Tensor) else images
            assert len(maps) == len(imgs) and logits.shape[0] == len(seg.tiles)
            t0 = 0
            for k, (im, y) in enumerate(zip(imgs, maps)):
                size = tuple(im.shape[1:])
                ys, xs = tile_starts(size[0], th, STRIDE[0]), tile_starts(size[1], tw, STRIDE[1])
                assert seg.tiles[t0:t0 + len(ys) * len(xs)] == [(k, y0, x0) for y0 in ys for x0 in xs]
                assert y.dtype == torch.uint8 and tuple(y.shape) == size
                _, want, excused, e32, tau = R.judge_tiles(logits, 1, size, (th, tw), ys, xs, t0)
                what = 'exit%d/call%d/image%d' % (exit, call, k)
                print('%s: e32 = %.2e, tau = %.2e' % (what, e32, tau))
                R.check_map(y.cpu()[None], want, excused, what)
                t0 += len(ys) * len(xs)
            assert t0 == len(seg.tiles)
            kept[call % 2] = (logits, list(seg.tiles), [y.cpu().clone() for y in maps])
        assert seg.graph is not None
        names = [c.name for c in seg.g.fwd]
        assert not {'resize_nchw', 'label_upsample', 'label_views_upsample'} & set(names)
        assert m.training
        after = m.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        m.eval()
        # every stored window is the model on that window of its image: its logits, up-sampled to the tile size, against model(crop)[exit]
        with torch.no_grad():
            for which, images in enumerate(inputs):
                logits, tiles, maps = kept[which]
                imgs = list(images.unbind(0)) if isinstance(images, torch.Tensor) else images
                crops = torch.stack([_crop_pad(imgs[k], y0, x0, th, tw) for k, y0, x0 in tiles]).contiguous()
                ref = m(crops)[exit]
                up = F.interpolate(logits.permute(0, 3, 1, 2).to(dev), (th, tw), mode='bilinear', align_corners=False)
                for t in range(len(tiles)):
                    err = _rel_l2(up[t], ref[t])
                    print('exit%d input %d window %s: rel L2 %.2e' % (exit, which, tiles[t], err))
                    assert err < 1e-3, (tiles[t], err)
        # the image that is exactly one window: Segmenter's map
        one = Segmenter(m, (1, 3, th, tw), exit=exit)
        y1 = one.step(several[0][None]).cpu()[0]
        differ = float((y1 != kept[1][2][0]).float().mean())
        print('exit%d: the one-window image differs from Segmenter on %.4f %% of the pixels' % (exit, 100 * differ))
        assert differ <= R.CAP
        assert len(kept[0][2][0].unique()) > 1
        one.close()
        seg.close()
    finally:
        m.eval()
