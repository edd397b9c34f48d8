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

Per-window early exits: with `threshold` the tile plan is a gate plan at batch B, cut into stages at the gates (TileGatePlan).  Every early
exit ends in ONE `addk_gate_tiles_upsample` launch that judges each window over the part of it that lies on its image; a window that is
sure leaves — ONE `addk_scatter_tile_logits` launch puts the leavers' logits into the store — and the survivors' live state is parked in a
pool (`addk_gather_rows`) until the survivors of several chunks fill a batch again (TileGateSchedule).  The batch size never changes, so a
window's stored logits are the static plan's at the exit it left at; the stitching heads are used as they are, views included.

    seg = TiledSegmenter(model, (B, 3, 769, 769), stride=(513, 513), threshold=0.35, confidence='entropy')
    maps = seg.segment(images)               # seg.exits: the exit of every window of seg.tiles; seg.values: its gate values
"""
import collections
import ctypes as C
import math

import torch

from . import _lib as L
from . import dynamic as _dynamic
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


class TileGateSchedule:
    """The order of work of a gated sliding-window call, as a pure host object: `run(T, execute)` walks T windows through a plan of B rows
    that is cut into gates + 1 stages, hands every operation to `execute(op)` in the order the device has to see it, and takes the
    decisions from it.  The operations:

        ('gather', t0, n)            windows t0 .. t0+n-1 -> plan rows 0 .. n-1
        ('run', k, ids)              stage k over rows 0 .. len(ids)-1, which hold the windows `ids`; for k < gates `execute` returns one
                                     bool per row: True = the window leaves at exit k
        ('scatter', k, rows, ids)    exit k's logits of plan rows `rows` -> the store's tiles `ids`
        ('park', k, rows, slots)     the live state behind gate k of plan rows `rows` -> ring slots `slots` of pool k
        ('unpark', k, slots)         ring slots `slots` of pool k -> plan rows 0 .. len(slots)-1; stage k+1 runs next

    Per chunk of up to B windows: gather, stage 0, the leavers scatter, the survivors park in pool 0.  Whenever a pool holds B rows, B of
    them are unparked and the next stage runs at a full batch, its leavers scatter, its survivors park one pool further — deepest pool
    first, so nothing waits behind a full pool.  After the last chunk the pools are flushed in order 0, 1, ...: each partial batch runs its
    stage once.  A batch none of whose rows leaves is not parked where going straight on costs no extra run (`stage` in `run`): with
    thresholds no window passes, no state is moved at all.  Stage k therefore runs ceil(n_k / B) times for the n_k windows that reach it, a pool of 2B ring slots never holds more than
    2B - 1 rows, every window is scattered once, and plan rows are parked before anything is unparked over them (`pending` says which
    rows still wait; `run` asserts all of it).  `ops`: the operations of the last run; `peak`: the most rows each pool held."""

    def __init__(self, B, gates):
        self.B, self.gates = int(B), int(gates)
        if self.B < 1 or self.gates < 1:
            raise ValueError('a tile gate schedule needs B >= 1 rows and at least one gate (got B = %d, %d gates)' % (self.B, self.gates))
        self.ops, self.peak = [], [0] * self.gates

    def run(self, T, execute):
        B, G = self.B, self.gates
        self.ops, self.peak = [], [0] * G
        self.pending = []                                      # plan rows whose state still has to be parked
        pools = [[] for _ in range(G)]                         # per gate: (window, ring slot) in arrival order
        head = [0] * G                                         # the ring slot the next parked row takes

        def do(*op):
            self.ops.append(op)
            return execute(op)

        def stage(k, ids, last):
            """Run stage k on plan rows 0 .. len(ids)-1, then move every row out of the plan.  `last`: no later chunk will come.  Rows that
            ALL stay go straight on to the next stage, without a pool, when that costs no extra run of it: a full batch always; a partial
            one when nothing else can still reach that stage (the last chunk is in, the pools in front of it are empty)."""
            assert not self.pending and 1 <= len(ids) <= B
            while k < G:
                leave = [bool(v) for v in do('run', k, list(ids))]
                assert len(leave) == len(ids), 'one decision per row'
                out = [r for r in range(len(ids)) if leave[r]]
                stay = [r for r in range(len(ids)) if not leave[r]]
                if out:
                    self.pending = list(stay)
                    do('scatter', k, out, [ids[r] for r in out])
                elif len(ids) == B or (last and not any(pools[:k + 1])):
                    k += 1
                    continue
                if stay:
                    self.pending = list(stay)
                    slots = [(head[k] + i) % (2 * B) for i in range(len(stay))]
                    head[k] = (head[k] + len(stay)) % (2 * B)
                    pools[k] += [(ids[r], s) for r, s in zip(stay, slots)]
                    assert len(pools[k]) <= 2 * B - 1
                    self.peak[k] = max(self.peak[k], len(pools[k]))
                    do('park', k, stay, slots)
                self.pending = []
                return
            do('run', k, list(ids))
            do('scatter', k, list(range(len(ids))), list(ids))

        def drain(flush):
            """unpark and run while a pool holds a full batch (deepest first); flushing, also the partial batches, shallowest first"""
            while True:
                k = next((k for k in reversed(range(G)) if len(pools[k]) >= B), None)
                if k is None and flush:
                    k = next((k for k in range(G) if pools[k]), None)
                if k is None:
                    return
                take, pools[k] = pools[k][:B], pools[k][B:]
                assert not self.pending
                do('unpark', k, [s for _, s in take])
                stage(k + 1, [t for t, _ in take], flush)

        for t0 in range(0, T, B):
            n = min(B, T - t0)
            do('gather', t0, n)
            stage(0, list(range(t0, t0 + n)), t0 + n == T)
            drain(False)
        drain(True)
        assert not any(pools)


class TileGatePlan(_dynamic.GatePlan):
    """The gated tile plan: GatePlan's launch list at batch B with the 'tile_gate' head (heads._tile_gate_head) — every early exit ends in
    its low-resolution logits and ONE `gate_tiles_upsample` launch — cut into stages at the gates and replayed stage by stage through
    DynamicPlan._seg.  `ext`: the int32 [B,2] device words of the valid extent of the window in every row, which the gate launches read.
    Per gate k a pool: a copy of the per-window live buffers behind the gate (GatePlan.live) with 2B rows, and of `ext`; `park[k]` /
    `unpark[k]` are the addk_gather_rows item tables between the plan and that pool.  The pools hold state only: the plan is the same
    one at every stage, so its input-independent tables stay valid."""

    def __init__(self, model, x, kind, temperature=None):
        B = int(x.shape[0])
        self.ext = torch.zeros((B, 2), dtype=torch.int32, device=x.device)
        super().__init__(model, x, kind, 'logits', None, batched=True, temperature=temperature, head='tile_gate', gate_extra={'ext': self.ext})
        self.batch, self.use_graph = B, True
        self.inref.bind(x)                                    # the windows are gathered straight into the caller's resident input
        self.x_static = x
        self.outs = self.heads + [self.final]
        self.cuts = [h.gate_cut for h in self.heads]
        self.runs = collections.Counter()
        low = {(o.src.raw.H, o.src.raw.W, o.src.raw.C) for o in self.outs}
        if len(low) != 1:
            raise ValueError('gated windows need exits whose low-resolution logits share one (h, w, C): one store row must fit every '
                             'exit (got %s)' % sorted(low))
        self.pools, self.park, self.unpark, self.pool_bytes = [], [], [], 0
        for k, cut in enumerate(self.cuts):
            bufs = self.live(cut)[0]
            for b in bufs:
                if b.geom is None or b.geom[0] != B or b.n != B * b.geom[1] * b.geom[2] * b.geom[3]:
                    raise L.AddkError('gate %d: live buffer %r is not one whole NHWC tensor of the plan\'s batch' % (k, b.region[0]))
            words = [b.n // B for b in bufs]
            pool = [torch.zeros(2 * B * w, dtype=torch.float32, device=x.device) for w in words]
            pext = torch.zeros((2 * B, 2), dtype=torch.int32, device=x.device)
            self.pool_bytes += sum(4 * p.numel() for p in pool) + 4 * pext.numel()
            there = [(b.ptr, p.data_ptr(), 4 * w) for b, p, w in zip(bufs, pool, words)] + [(self.ext.data_ptr(), pext.data_ptr(), 8)]
            self.pools.append((bufs, pool, pext))
            self.park.append(self._items(there))
            self.unpark.append(self._items([(d, s, n) for s, d, n in there]))

    def _items(self, triples):
        arr = (L.RowsItem * len(triples))()
        for it, (src, dst, nbytes) in zip(arr, triples):
            it.src, it.dst, it.row_bytes = src, dst, nbytes
        return self.g._table(bytes(arr)), len(triples)

    def stage(self, k):
        """the launch-list range [begin, end) of stage k; end -1: to the end of the list"""
        return (self.cuts[k - 1] if k else 0), (self.cuts[k] if k < len(self.cuts) else -1)

    def _seg(self, i0, i1):
        # DynamicPlan._seg runs a segment eagerly twice and captures it on its third run; a stage may first run in a late call, so the
        # count it looks at is this segment's own
        key = (i0, len(self.g.fwd) if i1 < 0 else i1)
        self.runs[key] += 1
        self.calls = self.runs[key] if self.use_graph else 0
        super()._seg(i0, i1)


class TiledSegmenter(InferenceStep):
    """Label maps of images of any size from one tile plan at batch B (see the module text).  `tiles`: the last call's windows as
    (image, y0, x0), in store order — image-major, then window row, then window column.  `maps`: the last call's label maps.
    With `scales`, `flip` or `weights` the windows run over views: `views` lists (scale, mirror, weight) in kernel order — per scale the plain
    view, then (with `flip`) the mirrored one; `weights` is one positive number per view in that order (default 1/len(views)); `tiles` then
    holds (image, view, y0, x0), origins in the view's scaled image, in store order — image-major, then view, window row, window column.
    Without the three arguments `views` is None and the call is the single-view one above.
    `threshold` (None: the static plan above, launch for launch; else a number or one per gate) makes the plan a TileGatePlan up to the
    last exit: every window leaves at the first exit whose gate passes (`segment`), `confidence` 'entropy' or 'max', `temperature` as
    dynamic.check_temperature takes it.  ValueError: `exit` other than the last exit, 'edm', a model with one exit, exits whose
    low-resolution logits differ in (h, w, C)."""
    head = 'tiles'

    def __init__(self, model, tile_shape, stride, exit=-1, label_lut=None, use_graph=None, nstreams=None, scales=None, flip=False, weights=None,
                 threshold=None, confidence='entropy', temperature=None):
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
        self.threshold = threshold
        if threshold is not None:
            self._init_gated(model, B, confidence, temperature)
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

    # ---------------- gated mode: per-window early exits ----------------
    def _init_gated(self, model, B, confidence, temperature):
        """The checks of `threshold=`: every error comes before any plan is built, except the one that needs the plan (exits whose
        low-resolution logits differ: TileGatePlan)."""
        if confidence == 'edm':
            raise ValueError("windows are gated by 'entropy' or 'max': the 'edm' gate stays with the single-image path")
        if confidence not in _dynamic.KINDS:
            raise ValueError('confidence must be one of %s (got %r)' % (_dynamic.KINDS, confidence))
        nex = model.num_exits()
        if nex < 2:
            raise ValueError('gated windows need a model with an early exit (this one has %d exit)' % nex)
        if self.exit != nex - 1:
            raise ValueError('gated windows run up to the last exit: exit=%d with a threshold is a contradiction' % self.exit)
        self.kind, self.gates = confidence, nex - 1
        self.temperature = _dynamic.check_temperature(temperature, nex)
        self._thresholds(self.threshold)
        self.exits = self.values = None
        self.counts, self.trace = collections.Counter(), []
        self.schedule = TileGateSchedule(B, self.gates)

    def _thresholds(self, threshold):
        """a number, or one number per gate (BatchedGate._thresholds' rule) -> one float per gate"""
        try:
            return [float(threshold)] * self.gates
        except TypeError:
            pass
        thr = [float(v) for v in threshold]
        if len(thr) != self.gates:
            raise ValueError('one threshold per gate: %d gates, %d thresholds' % (self.gates, len(thr)))
        return thr

    def set_temperature(self, temperature):
        """Other temperatures for the calls that follow (a tempered gated segmenter only): device words, no rebuild."""
        if self.threshold is None:
            raise ValueError('this TiledSegmenter was built without a threshold: it has no gates to temper')
        self.plan.set_temperature(temperature)
        self.temperature = self.plan.temperature

    def _build(self):
        if self.threshold is None:
            return super()._build()
        B = self.batch_shape[0]
        plan = self.plan = TileGatePlan(self.model, self.x, self.kind, self.temperature)
        g = self.g = plan.g
        g.nstreams, plan.use_graph = self.nstreams, self.use_graph
        assert not g.bwd and not g.nbt and len(plan.heads) == self.gates
        src = plan.final.src.raw
        self.ncls, self.low = src.C, (src.H, src.W)
        self.ld = (src.C + 3) // 4 * 4
        self._ptrs = self._storage()
        self.nbytes = g.nbytes + plan.pool_bytes
        self.graph, self.calls = None, 0
        # index words of the scatter / park / unpark launches: written on the host, copied to the device words the launches read; a ring of
        # slots, one event per slot guards the reuse of its pinned words
        self._idx_host = torch.zeros((4, 2, B), dtype=torch.int32)
        self._idx_dev = torch.zeros((4, 2, B), dtype=torch.int32, device=self.dev)
        if self.dev.type == 'cuda':
            self._idx_host = self._idx_host.pin_memory()
        self._idx_evt, self._idx_next = [None] * 4, 0

    def _idx(self, *rows):
        slot = self._idx_next
        self._idx_next = (slot + 1) % len(self._idx_evt)
        if self._idx_evt[slot] is not None:
            self._idx_evt[slot].synchronize()                  # the previous copy out of these pinned words has been made
        for r, vals in enumerate(rows):
            self._idx_host[slot, r, :len(vals)] = torch.tensor(vals, dtype=torch.int32)
        self._idx_dev[slot].copy_(self._idx_host[slot], non_blocking=True)
        if self.dev.type == 'cuda':
            if self._idx_evt[slot] is None:
                self._idx_evt[slot] = torch.cuda.Event()
            self._idx_evt[slot].record()
        return self._idx_dev[slot]

    def _extents(self, per, cap):
        """the valid extent (vh, vw) of every window in store order, as the bytes of int32 [cap][2]: the part of the window that lies on
        its (view's scaled) image; the rest of it is zero padding, which the gate must not judge"""
        th, tw = self.batch_shape[2:]
        ext = []
        for p in per:
            grids = [(p[1], p[2], p[3], p[4])] if self.views is None else [g[:4] for g in p[3]]
            for Hv, Wv, ys, xs in grids:
                ext += [(min(th, Hv - y), min(tw, Wv - x)) for y in ys for x in xs]
        arr = torch.zeros((cap, 2), dtype=torch.int32)
        arr[:len(ext)] = torch.tensor(ext, dtype=torch.int32)
        return arr.numpy().tobytes()

    def _rows(self, table, src_row, dst_row, nrows):
        a = L.GatherRowsArgs()
        a.items, a.nitems, a.nrows = table[0].data_ptr(), table[1], nrows
        a.src_row, a.dst_row = src_row.data_ptr(), None if dst_row is None else dst_row.data_ptr()
        self._launch('gather_rows', self.lib.addk_gather_rows, C.byref(a))

    def _run_gated(self, table, gather, T, thr):
        """The windows of a call through the gated plan, in TileGateSchedule's order: every window's logits reach the store from the exit
        it left at, through `addk_scatter_tile_logits`."""
        plan, (B, Cin, th, tw), G = self.plan, self.batch_shape, self.gates
        h, w = self.low
        entropy = plan.kind == 'entropy'
        col = 0 if entropy else 1
        self.exits = torch.full((T,), G, dtype=torch.int64)
        self.values = torch.full((T, G), float('nan'), dtype=torch.float32)
        self.trace = []
        cap = -(-T // B) * B
        ext = self._desc_dev[self._ext_off:self._ext_off + 8 * cap].view(torch.int32).view(cap, 2)
        word = [None]                                          # what the threshold word holds

        def execute(op):
            what = op[0]
            if what == 'gather':
                _, t0, n = op
                self._launch(gather[0], gather[1], table + t0 * gather[2], n, Cin, th, tw, self.x.data_ptr(), B)
                plan.ext[:n].copy_(ext[t0:t0 + n], non_blocking=True)
            elif what == 'run':
                _, k, ids = op
                n = len(ids)
                if k < G:
                    # a finite word for the kernel: every top probability lies in (0, 1], so clamping an infinite threshold changes no comparison
                    v = min(max(thr[k], -1.0), 2.0)
                    if v != word[0]:
                        plan._thr.fill_(v)
                        word[0] = v
                plan._seg(*plan.stage(k))
                self.counts[('seg', k)] += 1
                self.trace.append((k, n))
                if k == G:
                    return None
                if plan._conf_evt is not None:
                    plan._conf_evt.record()
                    plan._conf_evt.synchronize()               # the host waits for these 2n words only
                words = plan._conf_host[:2 * n].tolist()
                vals = [words[2 * i + col] for i in range(n)]
                self.values[ids, k] = torch.tensor(vals, dtype=torch.float32)
                return [(v < thr[k]) if entropy else (v > thr[k]) for v in vals]
            elif what == 'scatter':
                _, k, rows, ids = op
                d = self._idx(rows, ids)
                src = plan.outs[k].src.raw
                a = L.ScatterTileLogitsArgs()
                a.src, a.lds, a.B, a.store, a.ld, a.T = src.ptr, src.ld, B, self._store.data_ptr(), self.ld, self._store.shape[0]
                a.h, a.w, a.C, a.src_row, a.dst_tile, a.n = h, w, self.ncls, d[0].data_ptr(), d[1].data_ptr(), len(rows)
                self._launch('scatter_tile_logits', self.lib.addk_scatter_tile_logits, C.byref(a))
                self.counts['scatter'] += 1
                self.exits[ids] = k
            elif what == 'park':
                _, k, rows, slots = op
                d = self._idx(rows, slots)
                self._rows(plan.park[k], d[0], d[1], len(rows))
                self.counts['park'] += 1
            else:
                _, k, slots = op
                d = self._idx(slots)
                self._rows(plan.unpark[k], d[0], None, len(slots))
                self.counts['unpark'] += 1
        self.schedule.run(T, execute)

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

    def _upload(self, per, T, gated=False):
        """The call's descriptor table on the device: written into pinned host words, copied without blocking; an event guards the words'
        reuse by the next call (it waits for that one copy, not for the device).  `gated`: the windows' valid extents (_extents) travel
        behind the table, from byte `_ext_off` on."""
        B = self.batch_shape[0]
        cap = -(-T // B) * B
        arr = self._descriptors(per, cap)
        if gated:
            self._ext_off = (C.sizeof(arr) + 15) // 16 * 16
            arr = bytes(arr).ljust(self._ext_off, b'\0') + self._extents(per, cap)
        nb = len(bytes(arr))
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

    def segment(self, images, threshold=None):
        """-> the uint8 [H_i,W_i] label map of every image: `images` is a tensor [n,Cin,H,W] or a list of [Cin,H_i,W_i] tensors of any sizes,
        normalised float32 on the plan's device.  The maps belong to this object and are overwritten by the next call.  No host
        synchronisation, except once when the third replay captures the hipGraph.
        Built with `threshold` (gated mode) every window leaves at the first exit whose gate passes — `confidence` 'entropy': the
        normalised entropy of the window's prediction over the part of it that lies on its image is below the threshold; 'max': the
        share of those pixels whose top probability exceeds the threshold is above it (GatePlan.run's rule; with `temperature` the gates
        judge softmax(z_k / T_k)) — and the survivors of several chunks are pooled until they fill a batch again (TileGateSchedule).  The
        host reads every stage's gate words, so each stage synchronises once.  `threshold` here: other thresholds for this call (a
        number or one per gate).  Afterwards `exits` is int64 [T] on the host, the exit each window of `tiles` left at; `values` float32
        [T, gates] on the host, NaN where a gate was not evaluated for that window; `counts` ('seg', k) -> how often stage k ran, and the
        'park' / 'unpark' / 'scatter' launches, over all calls; `trace` the last call's (stage, rows) in run order."""
        lib = self.lib
        B, Cin, th, tw = self.batch_shape
        h, w = self.low
        per, tiles = self._windows(images)
        T = len(tiles)
        gated = self.threshold is not None
        if gated:
            thr = self._thresholds(self.threshold if threshold is None else threshold)
        elif threshold is not None:
            raise ValueError('this TiledSegmenter was built without a threshold: its plan has no gates')
        if self._storage() != self._ptrs:          # the parameters moved: the plan (and with it the class count and grid) is rebuilt first
            self._build()
            h, w = self.low
        if self._store is None or self._store.shape[0] < T or tuple(self._store.shape[1:]) != (h, w, self.ld):
            self._store = torch.zeros((T, h, w, self.ld), dtype=torch.float32, device=self.dev)      # outside the graph: it may grow
        if self.views is None:
            gather = ('gather_tiles', lib.addk_gather_tiles, C.sizeof(L.TileDesc))
        else:
            gather = ('gather_tile_views', lib.addk_gather_tile_views, C.sizeof(L.TileViewDesc))
        with torch.no_grad():
            if gated:
                self.calls += 1
                self._run_gated(self._upload(per, T, gated=True), gather, T, thr)
            else:
                table = self._upload(per, T)
                logits = self.out.src.raw.view()
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

    def close(self):
        super().close()
        if self.threshold is not None:
            self.plan.graphs.clear()
            self.plan.segs.clear()

    def tile_logits(self):
        """Copies of the stored low-resolution NHWC logits [T,h,w,C] of the last call's windows, in the order of `tiles` (inspection and tests)."""
        return self._store[:len(self.tiles), :, :, :self.ncls].clone()
