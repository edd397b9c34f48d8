"""GPU tests of multi-scale + flip sliding windows: the tiled multi-view label head (addk_label_tile_views_upsample) through the C ABI against
the fp64 arg-max of the formula it implements, addk_gather_tile_views against addk_resize_fwd + torch's flip, crop and pad, and
segment.TiledSegmenter with views against the same formula on the logits it stored and against the model on every window.

The rule of every comparison with fp64 is tests/_views_ref.py's, through tests/_tile_views_ref.py: e32 = max |fp32 - fp64| of the torch formula
on the CPU for these very inputs, tau = 64 * e32; a pixel whose fp64 top-2 gap is below tau is excused, at most 0.2 % of the pixels may be,
every other pixel must carry the fp64 arg-max."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402
import _tile_views_ref as R                                                                # noqa: E402

LD = 24
GUARD = 64
T0 = 3                                # every case's tiles sit behind three others in the store


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
    dense, from a base offset by one float (the scalar loader).  The store ends with its last tile: a read behind it leaves the allocation."""
    T, h, w, Cc = x.shape
    if t0:
        x = torch.cat([rand_tensor(3, 'tile_views_front', (t0, h, w, Cc)) * 7, x])
    if ld == LD:
        xa = (rand_tensor(1, 'tile_views_pad', tuple(x.shape[:3]) + (ld,)) * 50).to(dev)
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
    """addk_label_tile_views_upsample on a case -> (rc, guarded map)"""
    lib, L = _lib()
    N, size = R.CASES[case][:2]
    m = into if into is not None else _map(N, size, dev)
    keep, ptr = _device_tiles(R.logits(case, Cc), ld, T0, dev)
    a = R.fill_args(L.LabelTileViewsArgs(), case, Cc, T0)
    a.logits, a.ld = ptr, ld
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, m.ptr
    if edit is not None:
        edit(a)
    rc = lib.addk_label_tile_views_upsample(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, m


# ------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [LD, 0], ids=['stride24', 'dense'])
@pytest.mark.parametrize('Cc', R.CLASSES)
@pytest.mark.parametrize('case', list(R.CASES))
def test_label_tile_views_upsample_is_the_fp64_argmax(dev, case, Cc, ld):
    lib, L = _lib()
    ld = ld or Cc
    N, size = R.CASES[case][:2]
    assert lib.addk_label_tile_views_upsample_supported(len(R.CASES[case][5]), N, size[0], size[1], Cc) == 1
    _, want, excused, e32, tau = R.reference(case, Cc)
    rc, m = _launch(case, Cc, ld, dev)
    assert rc == 0
    got = m.read().view(m.dims)                                              # the guards are checked here
    print('%s/C%d/%d: e32 = %.2e, tau = %.2e, t0 = %d' % (case, Cc, ld, e32, tau, T0))
    R.check_map(got, want, excused, '%s/C%d/%d' % (case, Cc, ld))
    assert len(got.unique()) > 4                                             # a real map, not a constant
    # a second launch into the same buffer gives the same bytes
    rc, m = _launch(case, Cc, ld, dev, into=m)
    assert rc == 0 and torch.equal(m.read().view(m.dims), got)


@pytest.mark.parametrize('Cc,ld', [(19, LD), (21, 21)], ids=['C19-stride24', 'C21-dense'])
def test_one_plain_view_without_overlap_is_the_tiled_head_bit_for_bit(dev, Cc, ld):
    """image (66, 130), window and stride (33, 65): 2 x 2 windows that touch; every pixel has one cover, so weight 1 over cover 1 is the
    single-view head's 1.0f / sum e, and at scale 1 the coordinates are its own"""
    lib, L = _lib()
    N, size, tile, low = 2, (66, 130), (33, 65), (9, 17)
    ys, xs = [0, 33], [0, 65]
    x = rand_tensor(R.SEED, 'tile_views_flat:%d' % Cc, (N * 4,) + low + (Cc,)) * 3
    keep, ptr = _device_tiles(x, ld, T0, dev)
    a = L.LabelTilesArgs()
    a.logits, a.ld, a.h, a.w, a.th, a.tw = ptr, ld, low[0], low[1], tile[0], tile[1]
    a.N, a.C, a.OH, a.OW, a.t0, a.ny, a.nx = N, Cc, size[0], size[1], T0, 2, 2
    a.y0[:2], a.x0[:2] = ys, xs
    one = _map(N, size, dev)
    a.lut256, a.labels = None, one.ptr
    L.check(lib.addk_label_tiles_upsample(C.byref(a), _stream()), 'label_tiles_upsample')
    b = L.LabelTileViewsArgs()
    b.nview, b.logits, b.ld, b.h, b.w, b.th, b.tw = 1, ptr, ld, low[0], low[1], tile[0], tile[1]
    b.N, b.C, b.OH, b.OW = N, Cc, size[0], size[1]
    v = b.view[0]
    v.Hv, v.Wv, v.t0, v.ny, v.nx, v.mirror, v.weight = size[0], size[1], T0, 2, 2, 0, 1.0
    v.y0[:2], v.x0[:2] = ys, xs
    many = _map(N, size, dev)
    b.lut256, b.labels = None, many.ptr
    L.check(lib.addk_label_tile_views_upsample(C.byref(b), _stream()), 'label_tile_views_upsample')
    torch.cuda.synchronize()
    got = many.read()
    assert torch.equal(got, one.read()) and len(got.unique()) > 4


@pytest.mark.parametrize('case,Cc', [('three', 21), ('odd', 19)])
def test_label_tile_views_upsample_lut(dev, case, Cc):
    lut = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 256).astype(np.uint8))
    plain = _launch(case, Cc, LD, dev)[1].read()
    rc, m = _launch(case, Cc, LD, dev, lut=lut.to(dev))
    assert rc == 0 and torch.equal(m.read(), lut[plain.long()])


def test_label_tile_views_upsample_refuses_what_it_does_not_take(dev):
    import addk
    lib, L = _lib()
    N, size = R.CASES['three'][:2]
    m = _map(N, size, dev)
    for edit in R.REFUSALS:
        rc, _ = _launch('three', 19, LD, dev, into=m, edit=edit)
        assert rc == -1 and m.untouched(), edit.what                         # ADDK_ERR_INVALID, and no launch
    with pytest.raises(addk.AddkError):
        L.check(rc, 'label_tile_views_upsample')
    assert lib.addk_label_tile_views_upsample(C.byref(L.LabelTileViewsArgs()), None) == -1
    rc, _ = _launch('three', 19, LD, dev, into=m)                            # the same arguments, unedited, are taken
    assert rc == 0 and not m.untouched()
    m.read()


# ------------------------------------------------------------------------------------------------------------------------
# addk_gather_tile_views
# ------------------------------------------------------------------------------------------------------------------------
def _crop_pad(img, y0, x0, th, tw):
    """torch's form: pad the image with zeros on the right and at the bottom, then crop"""
    return F.pad(img, (0, tw, 0, th))[:, y0:y0 + th, x0:x0 + tw]


def _resize_fwd(img, Hv, Wv):
    """addk_resize_fwd on the planes of one image [Cin,H,W] (each plane a one-channel NHWC image) -> [Cin,Hv,Wv] on the device"""
    lib, L = _lib()
    Cin, H, W = img.shape
    y = torch.zeros((Cin, Hv, Wv), dtype=torch.float32, device=img.device)
    a = L.ResizeArgs()
    a.src.x, a.src.a, a.src.b, a.src.ld, a.src.C, a.src.relu, a.src.rs_hw = img.data_ptr(), None, None, 1, 1, 0, 0
    a.N, a.H, a.W, a.OH, a.OW, a.y, a.ldy, a.nchw_out = Cin, H, W, Hv, Wv, y.data_ptr(), 1, 1
    L.check(lib.addk_resize_fwd(C.byref(a), _stream()), 'resize_fwd')
    return y


def test_gather_tile_views_is_resize_flip_crop_and_pad(dev):
    """two images of different sizes share the chunks: the scales of `odd` and mirrored views, windows inside, over the edges and larger than
    the scaled image, a partly filled last chunk.  Exactly addk_resize_fwd's image, flipped, cropped and zero-padded by torch; at scale 1,
    unmirrored, addk_gather_tiles' bytes."""
    from addk.segment import view_size
    lib, L = _lib()
    Cin, (th, tw), B = 3, (32, 64), 4
    sizes = ((37, 61), (50, 90))
    imgs = [rand_tensor(9, 'tile_views_img:%d' % i, (Cin,) + s).to(dev).contiguous() for i, s in enumerate(sizes)]
    # (image, scale, mirror, y0, x0)
    wins = [(0, 0.5, 0, 0, 0), (0, 1.5, 1, 0, 0), (0, 1.5, 1, 24, 28), (1, 1.75, 0, 60, 100), (1, 1.75, 1, 30, 94), (0, 1.75, 0, 33, 43),
            (1, 1.0, 1, 18, 26), (1, 1.0, 0, 18, 26), (0, 1.0, 0, 5, 0), (1, 0.5, 1, 0, 0)]
    arr, plain = (L.TileViewDesc * len(wins))(), (L.TileDesc * len(wins))()
    want = torch.zeros((len(wins), Cin, th, tw))
    for i, (k, s, mirror, y0, x0) in enumerate(wins):
        H, W = sizes[k]
        Hv, Wv = view_size(H, W, s)
        d = arr[i]
        d.image, d.H, d.W, d.Hv, d.Wv, d.y0, d.x0, d.mirror = imgs[k].data_ptr(), H, W, Hv, Wv, y0, x0, mirror
        p = plain[i]
        p.image, p.H, p.W, p.y0, p.x0 = imgs[k].data_ptr(), H, W, y0, x0
        S = _resize_fwd(imgs[k], Hv, Wv)
        torch.cuda.synchronize()
        if mirror:
            S = S.flip(2)
        want[i] = _crop_pad(S.cpu(), y0, x0, th, tw)
        assert y0 < Hv and x0 < Wv
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    sz = C.sizeof(L.TileViewDesc)
    for t in range(0, len(wins), B):
        nb = min(B, len(wins) - t)
        x = _Guarded(B * Cin * th * tw * 4, dev)
        rc = lib.addk_gather_tile_views(table.data_ptr() + t * sz, nb, Cin, th, tw, x.ptr, B, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        got = x.read().view(torch.float32).view(B, Cin, th, tw)
        assert torch.equal(got[:nb], want[t:t + nb]), t                       # exactly
        assert nb == B or (nb == 2 and bool((got[nb:] == 0).all()))           # the slots behind the windows are zero
    assert all(float(w.abs().sum()) > 0 for w in want) and bool((want[0] == 0).any()) and bool((want[3] == 0).any())
    # scale 1, unmirrored: the single-view gather's bytes
    same = [i for i, wdw in enumerate(wins) if wdw[1] == 1.0 and not wdw[2]]
    assert len(same) == 2
    tv = torch.frombuffer(bytearray(b''.join(bytes(arr[i]) for i in same)), dtype=torch.uint8).to(dev)
    tp = torch.frombuffer(bytearray(b''.join(bytes(plain[i]) for i in same)), dtype=torch.uint8).to(dev)
    xa, xb = _Guarded(B * Cin * th * tw * 4, dev), _Guarded(B * Cin * th * tw * 4, dev)
    assert lib.addk_gather_tile_views(tv.data_ptr(), 2, Cin, th, tw, xa.ptr, B, _stream()) == 0
    assert lib.addk_gather_tiles(tp.data_ptr(), 2, Cin, th, tw, xb.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(xa.read(), xb.read())
    # a descriptor whose scaled size is not positive leaves zeros
    bad = (L.TileViewDesc * 1)()
    bad[0].image, bad[0].H, bad[0].W, bad[0].Hv, bad[0].Wv = imgs[0].data_ptr(), 37, 61, 0, -3
    tb = torch.frombuffer(bytearray(bytes(bad)), dtype=torch.uint8).to(dev)
    xc = _Guarded(Cin * th * tw * 4, dev)
    assert lib.addk_gather_tile_views(tb.data_ptr(), 1, Cin, th, tw, xc.ptr, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((xc.read() == 0).all())
    # refused without a launch
    y = _Guarded(64, dev)
    for r in ((None, 1, Cin, th, tw, y.ptr, B), (table.data_ptr(), 1, Cin, th, tw, None, B), (table.data_ptr(), B + 1, Cin, th, tw, y.ptr, B),
              (table.data_ptr(), -1, Cin, th, tw, y.ptr, B), (table.data_ptr(), 1, 0, th, tw, y.ptr, B), (table.data_ptr(), 1, Cin, 0, tw, y.ptr, B),
              (table.data_ptr(), 1, Cin, th, -1, y.ptr, B), (table.data_ptr(), 0, Cin, th, tw, y.ptr, 0)):
        assert lib.addk_gather_tile_views(*r, _stream()) == -1, r
    torch.cuda.synchronize()
    assert y.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# public path
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(dev):
    """F = 4, config 2; the recipe of tests/test_gpu_tiles.py::_model"""
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
SCALES = (0.75, 1.0, 1.5)


def _torch_window(im, scale, mirror, y0, x0, th, tw):
    """the window as torch builds it: interpolate, flip, crop, pad"""
    from addk.segment import view_size
    Hv, Wv = view_size(im.shape[1], im.shape[2], scale)
    S = F.interpolate(im[None], (Hv, Wv), mode='bilinear', align_corners=False)[0]
    if mirror:
        S = S.flip(2)
    return _crop_pad(S, y0, x0, th, tw)


def _check_maps(seg, imgs, maps, logits, what):
    """every map of a call against the formula on the stored logits, under the rule"""
    _, _, th, tw = TILE
    t0 = 0
    for k, (im, y) in enumerate(zip(imgs, maps)):
        size = tuple(im.shape[1:])
        gr = R.grids_of(1, size, (th, tw), STRIDE, seg.views, t0)
        want_tiles = [(k, v, y0, x0) for v, g in enumerate(gr) for y0 in g[2] for x0 in g[3]]
        assert seg.tiles[t0:t0 + len(want_tiles)] == want_tiles
        assert y.dtype == torch.uint8 and tuple(y.shape) == size
        _, want, excused, e32, tau = R.judge_views(logits, 1, size, (th, tw), seg.low, seg.views, gr)
        print('%s/image%d: e32 = %.2e, tau = %.2e' % (what, k, e32, tau))
        R.check_map(y.cpu()[None], want, excused, '%s/image%d' % (what, k))
        t0 += len(want_tiles)
    assert t0 == len(seg.tiles)


# The last exit at amplitude 1: tests/test_gpu_tiles.py says why (nearly one-hot probabilities; the excused share is a property of the
# reference).  (65, 129) is smaller than the window at scale 0.75, (40, 100) at 0.75 and 1.0.
def test_tiled_segmenter_with_views_equals_the_formula_and_the_model_on_every_window(dev):
    from addk.segment import TiledSegmenter
    m = _model(dev)
    B, Cin, th, tw = TILE
    batch = rand_tensor(41, 'tile_views_segx', (2, 3, 97, 200)).to(dev)
    several = [rand_tensor(42 + i, 'tile_views_segl', (3,) + s).to(dev) for i, s in enumerate(((65, 129), (40, 100), (97, 200)))]
    inputs = [batch, several]
    seg = TiledSegmenter(m, TILE, STRIDE, exit=1, scales=SCALES, flip=True)
    assert seg.views == [(s, mir, 1 / 6) for s in SCALES for mir in (False, True)]
    kept = {}
    for call in range(4):                                                    # chunks run eagerly twice, then the capture, then replays
        images = inputs[call % 2]
        maps = seg.segment(images)
        imgs = list(images.unbind(0)) if isinstance(images, torch.Tensor) else images
        assert len(maps) == len(imgs)
        if call < 2:
            logits = seg.tile_logits().cpu()
            assert logits.shape[0] == len(seg.tiles)
            _check_maps(seg, imgs, maps, logits, 'call%d' % call)
            kept[call] = (logits, list(seg.tiles), [y.cpu().clone() for y in maps])
        else:                                                                # two calls write the same bytes
            assert seg.tiles == kept[call % 2][1] and torch.equal(seg.tile_logits().cpu(), kept[call % 2][0])
            assert all(torch.equal(y.cpu(), z) for y, z in zip(maps, kept[call % 2][2]))
    assert seg.graph is not None
    names = [c.name for c in seg.g.fwd]
    assert not {'resize_nchw', 'label_upsample', 'label_views_upsample'} & set(names)
    assert len(kept[0][2][0].unique()) > 1
    # every stored window is the model on that window of its resized, mirrored image
    with torch.no_grad():
        for which, images in enumerate(inputs):
            logits, tiles, _ = kept[which]
            imgs = list(images.unbind(0)) if isinstance(images, torch.Tensor) else images
            crops = torch.stack([_torch_window(imgs[k], seg.views[v][0], seg.views[v][1], y0, x0, th, tw) for k, v, y0, x0 in tiles]).contiguous()
            worst = 0.0
            for c0 in range(0, len(tiles), 24):
                ref = m(crops[c0:c0 + 24])[1]
                up = F.interpolate(logits[c0:c0 + 24].permute(0, 3, 1, 2).to(dev), (th, tw), mode='bilinear', align_corners=False)
                for t in range(up.shape[0]):
                    err = _rel_l2(up[t], ref[t])
                    worst = max(worst, err)
                    assert err < 1e-3, (tiles[c0 + t], err)
            print('input %d: %d windows, worst rel L2 %.2e' % (which, len(tiles), worst))
    seg.close()
    # one plain view of weight 1 against the plain call: the same stored logits, and both maps carry the fp64 arg-max
    one = TiledSegmenter(m, TILE, STRIDE, exit=1, scales=(1.0,), flip=False, weights=(1.0,))
    plain = TiledSegmenter(m, TILE, STRIDE, exit=1)
    ya, yb = one.segment(several), plain.segment(several)
    la, lb = one.tile_logits().cpu(), plain.tile_logits().cpu()
    assert [(k, y0, x0) for k, _, y0, x0 in one.tiles] == plain.tiles and torch.equal(la, lb)
    _check_maps(one, several, ya, la, 'one view')
    _check_maps(one, several, yb, la, 'plain')
    one.close()
    plain.close()
