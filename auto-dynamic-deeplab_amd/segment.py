"""Static label-map inference (reference eval.py:218-221: `pred = argmax(output, 1)`): one exit of the path in inference form,
ending in the label head — ONE `addk_label_upsample` launch writes the uint8 [N,H,W] arg-max map straight from the decoder's
low-resolution logits (plan.Graph.head 'labels': heads._label_head), so the [N,C,H,W] logits are never written and no such buffer exists.  The plan holds
the trunk only up to the chosen exit's cell: an early exit costs its share of the network.  Emitted once over a resident input
buffer and replayed as a single hipGraph launch.

    seg = Segmenter(model, (N, 3, H, W), exit=-1, label_lut=decode_segmap_lut())
    for images in loader:
        labels = seg.step(images)            # uint8 [N,H,W], plan-owned: overwritten by the next step; no host synchronisation

Multi-scale + flip inference (what a DeepLab-family submission is scored on): the arg-max of the weighted mean of the class
probabilities over several input scales and each scale's horizontal mirror.  ONE plan holds every view — the staged input, resized per
scale (Graph.resize), runs through the model once per scale at batch 2N, the mirrored images riding along — and ends in ONE
`addk_label_views_upsample` launch (plan.Graph.head 'views': heads._views_head) that reads every view's low-resolution logits and writes the map: each view
is interpolated once, from the decoder's grid straight to (H, W), and no [N,C,·,·] tensor exists for any of them.
The label head takes the class counts of `_lib.head_classes()` (19: Cityscapes, 21: Pascal VOC) and Segmenter uses the stand-alone kernels
at any other; the multi-view head takes `_lib.gate_head_classes()` (19) and MultiViewSegmenter raises at any other.

    seg = MultiViewSegmenter(model, (N, 3, H, W), scales=(0.75, 1.0, 1.25), flip=True, label_lut=decode_segmap_lut())
    labels = seg.step(images)                # uint8 [N,H,W], plan-owned; no host synchronisation

Sliding-window (tiled) inference: ONE plan of a fixed window size serves images of any size, a list of differently sized images
included.  The windows of a call (tile_starts: the last window of an axis is clamped to the image edge, an image smaller than the
window is one zero-padded window) are cut by `addk_gather_tiles`, one launch per chunk of B windows, run through the tile plan, and their
low-resolution logits are kept in a store; ONE `addk_label_tiles_upsample` launch per image (plan.Graph.head 'tiles': heads._tiles_head)
then writes the arg-max of the summed class probabilities of every window that covers a pixel.  No [T,C,th,tw] tensor and no
full-resolution probability buffer exists.  The head takes `_lib.head_classes()` (19, 21) and TiledSegmenter raises at any other.

    seg = TiledSegmenter(model, (B, 3, 769, 769), stride=(513, 513))
    maps = seg.segment(images)               # [n,3,H,W] or a list of [3,H_i,W_i] -> list of uint8 [H_i,W_i], owned by `seg`

Both at once (how VOC and crop-trained Cityscapes models are scored): with `scales` / `flip` every view of an image — the image resized
to view_size(H, W, scale), mirrored or not — is evaluated under the sliding window.  `addk_gather_tile_views` cuts the windows straight
out of the resized, mirrored image without writing that image, and ONE `addk_label_tile_views_upsample` launch per image writes the arg-max
of the weighted mean over views of the mean class probabilities of the view's windows that cover a pixel.  Still one tile plan, no
[C,H,W] map of any view and no resized or flipped image.

    seg = TiledSegmenter(model, (B, 3, 769, 769), stride=(513, 513), scales=(0.75, 1.0, 1.25), flip=True)
    maps = seg.segment(images)
"""
import ctypes as C
import math

import torch

from . import _lib as L
from . import plan as _plan
from .heads import label_lut as _label_lut
from .resident import InferenceStep
from .sched import Cmd


class Segmenter(InferenceStep):
    head = 'labels'

    def __init__(self, model, batch_shape, exit=-1, label_lut=None, use_graph=None, nstreams=None):
        from .modeling.ADD import ADD
        if not isinstance(model, ADD):
            raise TypeError('Segmenter takes an ADD model (got %s)' % type(model).__name__)
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.lut = _label_lut(label_lut, next(model.parameters()).device)
        super().__init__(model, batch_shape, use_graph, nstreams, target=False)
        self._build()

    def _emit(self, g, a):
        N, _, H, W = self.batch_shape
        self.out = self.model._emit_exit(g, a, self.exit)
        assert self.out.head == 'labels' and tuple(self.out.y.shape) == (N, H, W), 'the model did not end in Graph.resize_to_nchw'

    def step(self, images=None):
        """-> the uint8 [N,H,W] label map of the resident batch (or of `images` if given).  The tensor belongs to the plan and is
        overwritten by the next step.  No host synchronisation, except once when the third call captures the hipGraph."""
        if images is not None:
            self.load_batch(images)
        with torch.no_grad():
            self._replay()
        return self.out.y


def view_size(H, W, scale):
    """(H_v, W_v) of an input scale: round half up"""
    return int(math.floor(H * scale + 0.5)), int(math.floor(W * scale + 0.5))


class MultiViewSegmenter(InferenceStep):
    """Label map of one exit averaged over views.  `views`: [(scale, mirror, (H_v, W_v), (h_v, w_v)), ...] in kernel order — per scale the
    plain view, then (with `flip`) the mirrored one; (H_v, W_v) is the view's input size, (h_v, w_v) its low-resolution logits grid.
    `weights`: one positive number per view in that order (default 1/len(views)).  With `flip` the resident input `x` is [2N,3,H,W]:
    load_batch writes the images and their flip(3), and view (s, mirrored) is images N..2N-1 of scale s's logits."""
    head = 'views'

    def __init__(self, model, batch_shape, scales=(0.75, 1.0, 1.25), flip=True, exit=-1, weights=None, label_lut=None, use_graph=None,
                 nstreams=None):
        from .modeling.ADD import ADD
        if not isinstance(model, ADD):
            raise TypeError('MultiViewSegmenter takes an ADD model (got %s)' % type(model).__name__)
        N, Cin, H, W = (int(v) for v in batch_shape)
        scales = tuple(float(s) for s in scales)
        self.flip = bool(flip)
        per = 2 if self.flip else 1
        if not scales:
            raise ValueError('scales is empty')
        if any(not (s > 0 and math.isfinite(s)) for s in scales):
            raise ValueError('scales must be positive (got %r)' % (scales,))
        if len(scales) * per > L.MAX_VIEWS:
            raise ValueError('at most %d views (got %d scales%s)' % (L.MAX_VIEWS, len(scales), ' with flip' if self.flip else ''))
        self.sizes = [view_size(H, W, s) for s in scales]
        for s, (hv, wv) in zip(scales, self.sizes):
            # below one pixel nothing is left to run; at 2^15 rows / 2^16 columns the plan's resized sources no longer describe their map
            if not (1 <= hv < (1 << 15) and 1 <= wv < (1 << 16)):
                raise ValueError('the plan cannot build the view of scale %g: %dx%d -> %dx%d' % (s, H, W, hv, wv))
        nview = len(scales) * per
        weights = [1.0 / nview] * nview if weights is None else [float(w) for w in weights]
        if len(weights) != nview:
            raise ValueError('one weight per view: %d views, %d weights' % (nview, len(weights)))
        if any(not (w > 0 and math.isfinite(w)) for w in weights):
            raise ValueError('weights must be positive and finite (got %r)' % (weights,))
        self.scales, self.weights = scales, weights
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.lut = _label_lut(label_lut, next(model.parameters()).device)
        self.image_shape = (N, Cin, H, W)
        super().__init__(model, (per * N, Cin, H, W), use_graph, nstreams, target=False)
        self._build()

    def _emit(self, g, a):
        N, _, H, W = self.image_shape
        per = 2 if self.flip else 1
        self.outs, self.views = [], []
        for i, (s, (hv, wv)) in enumerate(zip(self.scales, self.sizes)):
            av = a if (hv, wv) == (H, W) else g.resize(a, hv, wv)
            out = self.model._emit_exit(g, av, self.exit)
            assert out.head == 'views' and out.shape[1] in L.gate_head_classes() and (out.shape[0],) + tuple(out.shape[2:]) == (per * N, hv, wv), \
                'the model did not end in Graph.resize_to_nchw'
            out.binding = {'N': N, 'size': (H, W),
                           'views': [(m * N, m, self.weights[i * per + m]) for m in range(per)]}
            self.outs.append(out)
            self.views += [(s, bool(m), (hv, wv), (out.src.H, out.src.W)) for m in range(per)]

    def load_batch(self, images):
        N = self.image_shape[0]
        self.x[:N].copy_(images, non_blocking=True)
        if self.flip:
            self.x[N:].copy_(self.x[:N].flip(3))

    def step(self, images=None):
        """-> the uint8 [N,H,W] label map of the resident batch (or of `images` if given).  The tensor belongs to the plan and is
        overwritten by the next step.  No host synchronisation, except once when the third call captures the hipGraph."""
        if images is not None:
            self.load_batch(images)
        with torch.no_grad():
            self._replay()
        return self.g.view_labels

    def view_logits(self):
        """Copies of every view's low-resolution NHWC logits [N,h_v,w_v,C], in the order of `views` (inspection and tests)."""
        N = self.image_shape[0]
        return [o.src.raw.view()[n0:n0 + N].clone() for o in self.outs for n0, _, _ in o.binding['views']]


def tile_starts(L_, t, s):
    """Window origins along one axis of L_ pixels, window t, stride s: [0] if L_ <= t (one window, the image padded to it), else
    ceil((L_ - t) / s) + 1 origins min(i * s, L_ - t) — the last window is clamped to the image edge, not padded.  Needs 1 <= s <= t, so
    that consecutive windows touch or overlap; the origins strictly increase (both checked).  More than MAX_TILES_AXIS windows is a
    ValueError.  Clamping lets three windows overlap: tile_starts(70, 33, 17) == [0, 17, 34, 37]."""
    L_, t, s = int(L_), int(t), int(s)
    if L_ < 1 or t < 1:
        raise ValueError('an axis of %d pixels and a window of %d: both must be positive' % (L_, t))
    if not 1 <= s <= t:
        raise ValueError('the stride must be within 1..window (got stride %d, window %d)' % (s, t))
    if L_ <= t:
        return [0]
    n = -((t - L_) // s) + 1
    if n > L.MAX_TILES_AXIS:
        raise ValueError('%d windows of %d at stride %d along %d pixels: at most %d per axis' % (n, t, s, L_, L.MAX_TILES_AXIS))
    starts = [min(i * s, L_ - t) for i in range(n)]
    assert starts[0] == 0 and starts[-1] + t == L_ and all(a < b <= a + t for a, b in zip(starts, starts[1:])), starts
    return starts


class TiledSegmenter(InferenceStep):
    """Label maps of images of any size from one tile plan at batch B (see the module text).  `tiles`: the last call's windows as
    (image, y0, x0), in store order — image-major, then window row, then window column.  `maps`: the last call's label maps.
    With `scales`, `flip` or `weights` the windows run over views: `views` lists (scale, mirror, weight) in kernel order — per scale the plain
    view, then (with `flip`) the mirrored one; `weights` is one positive number per view in that order (default 1/len(views)); `tiles` then
    holds (image, view, y0, x0), origins in the view's scaled image, in store order — image-major, then view, window row, window column.
    Without the three arguments `views` is None and the call is the single-view one above."""
    head = 'tiles'

    def __init__(self, model, tile_shape, stride, exit=-1, label_lut=None, use_graph=None, nstreams=None, scales=None, flip=False, weights=None):
        from .modeling.ADD import ADD
        if not isinstance(model, ADD):
            raise TypeError('TiledSegmenter takes an ADD model (got %s)' % type(model).__name__)
        B, Cin, th, tw = (int(v) for v in tile_shape)
        sy, sx = (int(v) for v in stride)
        if B < 1 or Cin < 1 or th < 1 or tw < 1:
            raise ValueError('tile_shape must be positive (got %r)' % (tuple(tile_shape),))
        if not (1 <= sy <= th and 1 <= sx <= tw):
            raise ValueError('the stride must be within 1..tile (got stride %r, tile %dx%d)' % ((sy, sx), th, tw))
        self.stride = (sy, sx)
        self.views = None
        if scales is not None or flip or weights is not None:
            scales = (1.0,) if scales is None else tuple(float(s) for s in scales)
            per = 2 if flip else 1
            if not scales:
                raise ValueError('scales is empty')
            if any(not (s > 0 and math.isfinite(s)) for s in scales):
                raise ValueError('scales must be positive (got %r)' % (scales,))
            if len(scales) * per > L.MAX_VIEWS:
                raise ValueError('at most %d views (got %d scales%s)' % (L.MAX_VIEWS, len(scales), ' with flip' if flip else ''))
            nview = len(scales) * per
            weights = [1.0 / nview] * nview if weights is None else [float(w) for w in weights]
            if len(weights) != nview:
                raise ValueError('one weight per view: %d views, %d weights' % (nview, len(weights)))
            if any(not (w > 0 and math.isfinite(w)) for w in weights):
                raise ValueError('weights must be positive and finite (got %r)' % (weights,))
            self.views = [(s, bool(m), weights[i * per + m]) for i, s in enumerate(scales) for m in range(per)]
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.lut = _label_lut(label_lut, next(model.parameters()).device)
        self.tiles, self.maps, self._images = [], [], []
        self._store = None                                     # [Tcap,h,w,ld]: the low-resolution logits of a call's windows
        self._desc_host = self._desc_dev = self._desc_evt = None
        self._label_buf = None
        super().__init__(model, (B, Cin, th, tw), use_graph, nstreams, target=False)
        self._build()

    def _emit(self, g, a):
        B, _, th, tw = self.batch_shape
        self.out = self.model._emit_exit(g, a, self.exit)
        assert self.out.head == 'tiles' and (self.out.shape[0],) + tuple(self.out.shape[2:]) == (B, th, tw), \
            'the model did not end in Graph.resize_to_nchw'
        src = self.out.src.raw
        self.ncls, self.low = src.C, (src.H, src.W)
        self.ld = (src.C + 3) // 4 * 4                         # the store's pixel stride: what the head's 16-byte loader asks for

    # ---------------- per call ----------------
    def _launch(self, name, fn, *args):
        """one launch on the current stream, through the plan's launch loop"""
        self.g.run([Cmd(name, fn, args)], _plan.current_stream())

    def _windows(self, images):
        """-> ([(image tensor [Cin,H,W], H, W, y origins, x origins, first tile)], [(image, y0, x0)]) of a call"""
        Cin, th, tw = self.batch_shape[1:]
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise ValueError('images: a tensor [n,%d,H,W] or a list of [%d,H,W] tensors (got %s)' % (Cin, Cin, tuple(images.shape)))
            images = list(images.unbind(0))
        images = list(images)
        if not images:
            raise ValueError('no image')
        per, tiles = [], []
        for k, im in enumerate(images):
            if im.dim() != 3 or im.shape[0] != Cin or im.shape[1] < 1 or im.shape[2] < 1:
                raise ValueError('image %d: expected [%d,H,W] (got %s)' % (k, Cin, tuple(im.shape)))
            if im.dtype != torch.float32:
                raise ValueError('image %d: expected normalised float32 (got %s)' % (k, im.dtype))
            _plan.require_device(im)
            H, W = int(im.shape[1]), int(im.shape[2])
            if self.views is not None:
                grids = []                                     # per view: (Hv, Wv, y origins, x origins, first tile), on the scaled image
                for v, (s, _, _) in enumerate(self.views):
                    Hv, Wv = view_size(H, W, s)
                    ys, xs = tile_starts(Hv, th, self.stride[0]), tile_starts(Wv, tw, self.stride[1])
                    grids.append((Hv, Wv, ys, xs, len(tiles)))
                    tiles += [(k, v, y, x) for y in ys for x in xs]
                per.append((im.contiguous(), H, W, grids))
                continue
            ys, xs = tile_starts(H, th, self.stride[0]), tile_starts(W, tw, self.stride[1])
            per.append((im.contiguous(), H, W, ys, xs, len(tiles)))
            tiles += [(k, y, x) for y in ys for x in xs]
        return per, tiles

    def _descriptors(self, per, cap):
        """the call's window descriptors in store order, as a ctypes array of `cap` entries (the ones behind the windows stay zero)"""
        if self.views is None:
            arr = (L.TileDesc * cap)()
            i = 0
            for im, H, W, ys, xs, _ in per:
                for y in ys:
                    for x in xs:
                        d = arr[i]
                        d.image, d.H, d.W, d.y0, d.x0 = im.data_ptr(), H, W, y, x
                        i += 1
            return arr
        arr = (L.TileViewDesc * cap)()
        i = 0
        for im, H, W, grids in per:
            for (_, mirror, _), (Hv, Wv, ys, xs, _) in zip(self.views, grids):
                for y in ys:
                    for x in xs:
                        d = arr[i]
                        d.image, d.H, d.W, d.Hv, d.Wv, d.y0, d.x0, d.mirror = im.data_ptr(), H, W, Hv, Wv, y, x, int(mirror)
                        i += 1
        return arr

    def _upload(self, per, T):
        """The call's descriptor table on the device: written into pinned host words, copied without blocking; an event guards the words'
        reuse by the next call (it waits for that one copy, not for the device)."""
        B = self.batch_shape[0]
        cap = -(-T // B) * B
        arr = self._descriptors(per, cap)
        nb = C.sizeof(arr)
        if self._desc_host is None or self._desc_host.numel() < nb:
            self._desc_host = torch.zeros(nb, dtype=torch.uint8)
            self._desc_dev = torch.zeros(nb, dtype=torch.uint8, device=self.dev)
            if self.dev.type == 'cuda':
                self._desc_host = self._desc_host.pin_memory()
            self._desc_evt = None
        if self._desc_evt is not None:
            self._desc_evt.synchronize()
        self._desc_host[:nb].copy_(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))
        self._desc_dev[:nb].copy_(self._desc_host[:nb], non_blocking=True)
        if self.dev.type == 'cuda':
            if self._desc_evt is None:
                self._desc_evt = torch.cuda.Event()
            self._desc_evt.record()
        return self._desc_dev.data_ptr()

    def segment(self, images):
        """-> the uint8 [H_i,W_i] label map of every image: `images` is a tensor [n,Cin,H,W] or a list of [Cin,H_i,W_i] tensors of any sizes,
        normalised float32 on the plan's device.  The maps belong to this object and are overwritten by the next call.  No host
        synchronisation, except once when the third replay captures the hipGraph."""
        lib = self.lib
        B, Cin, th, tw = self.batch_shape
        h, w = self.low
        per, tiles = self._windows(images)
        T = len(tiles)
        if self._storage() != self._ptrs:          # the parameters moved: the plan (and with it the class count and grid) is rebuilt first
            self._build()
            h, w = self.low
        if self._store is None or self._store.shape[0] < T or tuple(self._store.shape[1:]) != (h, w, self.ld):
            self._store = torch.zeros((T, h, w, self.ld), dtype=torch.float32, device=self.dev)      # outside the graph: it may grow
        table = self._upload(per, T)
        logits = self.out.src.raw.view()
        if self.views is None:
            gather = ('gather_tiles', lib.addk_gather_tiles, C.sizeof(L.TileDesc))
        else:
            gather = ('gather_tile_views', lib.addk_gather_tile_views, C.sizeof(L.TileViewDesc))
        with torch.no_grad():
            for t in range(0, T, B):
                nb = min(B, T - t)
                self._launch(gather[0], gather[1], table + t * gather[2], nb, Cin, th, tw, self.x.data_ptr(), B)
                self._replay()
                self._store[t:t + nb, :, :, :self.ncls].copy_(logits[:nb])
            npix = sum(p[1] * p[2] for p in per)
            if self._label_buf is None or self._label_buf.numel() < npix:
                self._label_buf = torch.zeros(npix, dtype=torch.uint8, device=self.dev)
            maps, off = [], 0
            for p in per:
                H, W = p[1], p[2]
                lab = self._label_buf[off:off + H * W].view(H, W)
                off += H * W
                if self.views is not None:
                    a = L.LabelTileViewsArgs()
                    a.nview, a.logits, a.ld, a.h, a.w, a.th, a.tw = len(self.views), self._store.data_ptr(), self.ld, h, w, th, tw
                    a.N, a.C, a.OH, a.OW = 1, self.ncls, H, W
                    for v, (_, mirror, weight), (Hv, Wv, ys, xs, t0) in zip(a.view, self.views, p[3]):
                        v.Hv, v.Wv, v.t0, v.ny, v.nx, v.mirror, v.weight = Hv, Wv, t0, len(ys), len(xs), int(mirror), weight
                        v.y0[:len(ys)], v.x0[:len(xs)] = ys, xs
                    a.lut256, a.labels = self.lut.data_ptr() if self.lut is not None else None, lab.data_ptr()
                    self._launch('label_tile_views_upsample', lib.addk_label_tile_views_upsample, C.byref(a))
                    maps.append(lab)
                    continue
                ys, xs, t0 = p[3:]
                a = L.LabelTilesArgs()
                a.logits, a.ld, a.h, a.w, a.th, a.tw = self._store.data_ptr(), self.ld, h, w, th, tw
                a.N, a.C, a.OH, a.OW, a.t0, a.ny, a.nx = 1, self.ncls, H, W, t0, len(ys), len(xs)
                a.y0[:len(ys)], a.x0[:len(xs)] = ys, xs
                a.lut256, a.labels = self.lut.data_ptr() if self.lut is not None else None, lab.data_ptr()
                self._launch('label_tiles_upsample', lib.addk_label_tiles_upsample, C.byref(a))
                maps.append(lab)
        self.tiles, self.maps, self._images = tiles, maps, [p[0] for p in per]      # the images stay alive while the device may read them
        return maps

    def tile_logits(self):
        """Copies of the stored low-resolution NHWC logits [T,h,w,C] of the last call's windows, in the order of `tiles` (inspection and tests)."""
        return self._store[:len(self.tiles), :, :, :self.ncls].clone()
