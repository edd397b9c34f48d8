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

The view arguments of both multi-view front ends are checked by view_spec.  Inside TiledSegmenter every image is (im, H, W, grids), one grid
per view — the single-view call is one view under its own kernels, chosen once in __init__ —, and a call is _windows (bookkeeping),
_run_static / _run_gated (the chunks) and _stitch.  The gate reader, the thresholds, the pinned index words and the `addk_gather_rows`
tables and launches are dynamic.py's (GatePlan.gate_values / leaves, gate_thresholds, PinnedWords, rows_table, gather_rows).
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


def _require_add(who, model):
    from .modeling.ADD import ADD
    if not isinstance(model, ADD):
        raise TypeError('%s takes an ADD model (got %s)' % (type(who).__name__, type(model).__name__))


class _LabelStep(InferenceStep):
    """What the resident segmenters share: the step.  `_labels()`: the plan-owned map the head of the CURRENT plan writes."""

    def step(self, images=None):
        """-> the uint8 [N,H,W] label map of the resident batch (or of `images` if given).  The tensor belongs to the plan and is
        overwritten by the next step.  No host synchronisation, except once when the third call captures the hipGraph."""
        if images is not None:
            self.load_batch(images)
        with torch.no_grad():
            self._replay()
        return self._labels()


class Segmenter(_LabelStep):
    head = 'labels'

    def __init__(self, model, batch_shape, exit=-1, label_lut=None, use_graph=None, nstreams=None):
        _require_add(self, model)
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.lut = _label_lut(label_lut, next(model.parameters()).device)
        super().__init__(model, batch_shape, use_graph, nstreams, target=False)
        self._build()

    def _emit(self, g, a):
        N, _, H, W = self.batch_shape
        self.out = self.model._emit_exit(g, a, self.exit)
        assert self.out.head == 'labels' and tuple(self.out.y.shape) == (N, H, W), 'the model did not end in Graph.resize_to_nchw'

    def _labels(self):
        return self.out.y


def view_size(H, W, scale):
    """(H_v, W_v) of an input scale: round half up"""
    return int(math.floor(H * scale + 0.5)), int(math.floor(W * scale + 0.5))


def view_spec(scales, flip, weights, size=None):
    """The view list of `scales` / `flip` / `weights`, checked -> (the scales as floats, views per scale: the plain one and with `flip`
    the mirrored one, one positive weight per view in kernel order — default 1 / views).  `size`: the (H, W) a resident plan builds
    every view of."""
    scales = tuple(float(s) for s in scales)
    per = 2 if flip else 1
    if not scales:
        raise ValueError('scales is empty')
    if any(not (s > 0 and math.isfinite(s)) for s in scales):
        raise ValueError('scales must be positive (got %r)' % (scales,))
    if len(scales) * per > L.MAX_VIEWS:
        raise ValueError('at most %d views (got %d scales%s)' % (L.MAX_VIEWS, len(scales), ' with flip' if flip else ''))
    for s in scales if size is not None else ():
        hv, wv = view_size(*size, s)
        # below one pixel nothing is left to run; at 2^15 rows / 2^16 columns the plan's resized sources no longer describe their map
        if not (1 <= hv < (1 << 15) and 1 <= wv < (1 << 16)):
            raise ValueError('the plan cannot build the view of scale %g: %dx%d -> %dx%d' % ((s,) + tuple(size) + (hv, wv)))
    nview = len(scales) * per
    weights = [1.0 / nview] * nview if weights is None else [float(w) for w in weights]
    if len(weights) != nview:
        raise ValueError('one weight per view: %d views, %d weights' % (nview, len(weights)))
    if any(not (w > 0 and math.isfinite(w)) for w in weights):
        raise ValueError('weights must be positive and finite (got %r)' % (weights,))
    return scales, per, weights


class MultiViewSegmenter(_LabelStep):
    """Label map of one exit averaged over views.  `views`: [(scale, mirror, (H_v, W_v), (h_v, w_v)), ...] in kernel order — per scale the
    plain view, then (with `flip`) the mirrored one; (H_v, W_v) is the view's input size, (h_v, w_v) its low-resolution logits grid.
    `weights`: one positive number per view in that order (default 1/len(views)).  With `flip` the resident input `x` is [2N,3,H,W]:
    load_batch writes the images and their flip(3), and view (s, mirrored) is images N..2N-1 of scale s's logits."""
    head = 'views'

    def __init__(self, model, batch_shape, scales=(0.75, 1.0, 1.25), flip=True, exit=-1, weights=None, label_lut=None, use_graph=None,
                 nstreams=None):
        _require_add(self, model)
        N, Cin, H, W = (int(v) for v in batch_shape)
        self.flip = bool(flip)
        self.scales, per, self.weights = view_spec(scales, self.flip, weights, (H, W))
        self.sizes = [view_size(H, W, s) for s in self.scales]
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

    def _labels(self):
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
                if not _dynamic.whole_rows(b, B):
                    raise L.AddkError('gate %d: live buffer %r is not one whole NHWC tensor of the plan\'s batch' % (k, b.region[0]))
            words = [b.n // B for b in bufs]
            pool = [torch.zeros(2 * B * w, dtype=torch.float32, device=x.device) for w in words]
            pext = torch.zeros((2 * B, 2), dtype=torch.int32, device=x.device)
            self.pool_bytes += sum(4 * p.numel() for p in pool) + 4 * pext.numel()
            there = [(b.ptr, p.data_ptr(), 4 * w) for b, p, w in zip(bufs, pool, words)] + [(self.ext.data_ptr(), pext.data_ptr(), 8)]
            self.pools.append((bufs, pool, pext))
            self.park.append(_dynamic.rows_table(self.g, there))
            self.unpark.append(_dynamic.rows_table(self.g, [(d, s, n) for s, d, n in there]))

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


def _fill(block, **vals):
    """Set those of `vals` that the ctypes block declares (an array field: its first len(value) entries).  The single-view blocks
    declare no Hv / Wv / mirror / weight / nview: their one view is the image itself."""
    for f, t in block._fields_:
        if f in vals:
            if issubclass(t, C.Array):
                getattr(block, f)[:len(vals[f])] = vals[f]
            else:
                setattr(block, f, vals[f])


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
        _require_add(self, model)
        B, Cin, th, tw = (int(v) for v in tile_shape)
        sy, sx = (int(v) for v in stride)
        if B < 1 or Cin < 1 or th < 1 or tw < 1:
            raise ValueError('tile_shape must be positive (got %r)' % (tuple(tile_shape),))
        if not (1 <= sy <= th and 1 <= sx <= tw):
            raise ValueError('the stride must be within 1..tile (got stride %r, tile %dx%d)' % ((sy, sx), th, tw))
        self.stride = (sy, sx)
        # The ONE place that tells the two forms of a call apart.  Inside, every image is (im, H, W, grids) with one grid per view; the
        # single-view form is the view (1.0, not mirrored) under its own kernels: window descriptor, gather launch, stitching head, the
        # head's argument block, where in that block a view's grid goes, and what `tiles` shows of a window
        if scales is None and not flip and weights is None:
            self.views, self._views = None, [(1.0, False, 1.0)]
            self._desc_type, self._gather, self._tile_id = L.TileDesc, 'gather_tiles', lambda k, v, y, x: (k, y, x)
            self._head = ('label_tiles_upsample', L.LabelTilesArgs, lambda a: [a])
        else:
            scales, per, weights = view_spec((1.0,) if scales is None else scales, flip, weights)
            self.views = self._views = [(s, bool(m), weights[i * per + m]) for i, s in enumerate(scales) for m in range(per)]
            self._desc_type, self._gather, self._tile_id = L.TileViewDesc, 'gather_tile_views', lambda k, v, y, x: (k, v, y, x)
            self._head = ('label_tile_views_upsample', L.LabelTileViewsArgs, lambda a: a.view)
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.threshold = threshold
        if threshold is not None:
            self._init_gated(model, B, confidence, temperature)
        self.lut = _label_lut(label_lut, next(model.parameters()).device)
        self.tiles, self.maps, self._images = [], [], []
        self._store = None                                     # [Tcap,h,w,ld]: the low-resolution logits of a call's windows
        self._desc = None                                      # the call's descriptor table (and extents): dynamic.PinnedWords, one slot
        self._label_buf = None
        super().__init__(model, (B, Cin, th, tw), use_graph, nstreams, target=False)
        self._build()

    def _emit(self, g, a):
        B, _, th, tw = self.batch_shape
        self.out = self.model._emit_exit(g, a, self.exit)
        assert self.out.head == 'tiles' and (self.out.shape[0],) + tuple(self.out.shape[2:]) == (B, th, tw), \
            'the model did not end in Graph.resize_to_nchw'
        self._logits_grid(self.out.src.raw)

    def _logits_grid(self, src):
        """what the store and the heads take from the plan's low-resolution logits `src`: class count, grid, the store's pixel stride"""
        self.ncls, self.low = src.C, (src.H, src.W)
        self.ld = (src.C + 3) // 4 * 4                         # what the head's 16-byte loader asks for

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
        _dynamic.gate_thresholds(self.threshold, self.gates)
        self.exits = self.values = None
        self.counts, self.trace = collections.Counter(), []
        self.schedule = TileGateSchedule(B, self.gates)

    def set_temperature(self, temperature):
        """Other temperatures for the calls that follow (a tempered gated segmenter only): device words, no rebuild."""
        if self.threshold is None:
            raise ValueError('this TiledSegmenter was built without a threshold: it has no gates to temper')
        self.plan.set_temperature(temperature)
        self.temperature = self.plan.temperature

    def _build(self):
        if self.threshold is None:
            return super()._build()
        plan = self.plan = TileGatePlan(self.model, self.x, self.kind, self.temperature)
        g = self.g = plan.g
        g.nstreams, plan.use_graph = self.nstreams, self.use_graph
        assert not g.bwd and not g.nbt and len(plan.heads) == self.gates
        self._logits_grid(plan.final.src.raw)
        self._ptrs = self._storage()
        self.nbytes = g.nbytes + plan.pool_bytes
        self.graph, self.calls = None, 0
        # index words of the scatter / park / unpark launches: a ring of slots, taken in turn (_index)
        self._idx, self._idx_next = _dynamic.PinnedWords((4, 2, self.batch_shape[0]), torch.int32, self.dev), 0

    def _index(self, *rows):
        slot, self._idx_next = self._idx_next, (self._idx_next + 1) % 4
        return self._idx.put(slot, *rows)

    def _extents(self, per, cap):
        """the valid extent (vh, vw) of every window in store order, as the bytes of int32 [cap][2]: the part of the window that lies on
        its (view's scaled) image; the rest of it is zero padding, which the gate must not judge"""
        th, tw = self.batch_shape[2:]
        ext = [(min(th, Hv - y), min(tw, Wv - x)) for _, _, _, grids in per for Hv, Wv, ys, xs, _ in grids for y in ys for x in xs]
        arr = torch.zeros((cap, 2), dtype=torch.int32)
        arr[:len(ext)] = torch.tensor(ext, dtype=torch.int32)
        return arr.numpy().tobytes()

    def _run_gated(self, table, T, thr):
        """The windows of a call through the gated plan, in TileGateSchedule's order: every window's logits reach the store from the exit
        it left at, through `addk_scatter_tile_logits`."""
        plan, B, G = self.plan, self.batch_shape[0], self.gates
        h, w = self.low
        self.exits = torch.full((T,), G, dtype=torch.int64)
        self.values = torch.full((T, G), float('nan'), dtype=torch.float32)
        self.trace = []
        cap = -(-T // B) * B
        ext = self._desc.dev.view(-1)[self._ext_off:self._ext_off + 8 * cap].view(torch.int32).view(cap, 2)

        def execute(op):
            what = op[0]
            if what == 'gather':
                _, t0, n = op
                self._cut(table, t0, n)
                plan.ext[:n].copy_(ext[t0:t0 + n], non_blocking=True)
            elif what == 'run':
                _, k, ids = op
                if k < G:
                    plan.set_threshold(thr[k])
                plan._seg(*plan.stage(k))
                self.counts[('seg', k)] += 1
                self.trace.append((k, len(ids)))
                if k == G:
                    return None
                vals = plan.gate_values(k, len(ids))           # the host waits for these words only
                self.values[ids, k] = torch.tensor(vals, dtype=torch.float32)
                return [plan.leaves(v, thr[k]) for v in vals]
            elif what == 'scatter':
                _, k, rows, ids = op
                d = self._index(rows, ids)
                src = plan.outs[k].src.raw
                a = L.ScatterTileLogitsArgs()
                a.src, a.lds, a.B, a.store, a.ld, a.T = src.ptr, src.ld, B, self._store.data_ptr(), self.ld, self._store.shape[0]
                a.h, a.w, a.C, a.src_row, a.dst_tile, a.n = h, w, self.ncls, d[0].data_ptr(), d[1].data_ptr(), len(rows)
                self._launch('scatter_tile_logits', C.byref(a))
                self.counts['scatter'] += 1
                self.exits[ids] = k
            elif what == 'park':
                _, k, rows, slots = op
                d = self._index(rows, slots)
                _dynamic.gather_rows(self.g, plan.park[k], d[0], d[1], len(rows))
                self.counts['park'] += 1
            else:
                _, k, slots = op
                _dynamic.gather_rows(self.g, plan.unpark[k], self._index(slots)[0], None, len(slots))
                self.counts['unpark'] += 1
        self.schedule.run(T, execute)

    # ---------------- per call ----------------
    def _launch(self, name, *args):
        """one launch of the library's addk_<name> on the current stream, through the plan's launch loop"""
        self.g.run([Cmd(name, getattr(self.lib, 'addk_' + name), args)], _plan.current_stream())

    def _windows(self, images):
        """The window bookkeeping of a call -> ([(image tensor [Cin,H,W], H, W, grids)], `tiles`); grids: per view (Hv, Wv, y origins,
        x origins, first tile) on the view's scaled image"""
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
            grids = []
            for v, (s, _, _) in enumerate(self._views):
                Hv, Wv = view_size(H, W, s)                    # (H, W) at scale 1
                ys, xs = tile_starts(Hv, th, self.stride[0]), tile_starts(Wv, tw, self.stride[1])
                grids.append((Hv, Wv, ys, xs, len(tiles)))
                tiles += [self._tile_id(k, v, y, x) for y in ys for x in xs]
            per.append((im.contiguous(), H, W, grids))
        return per, tiles

    def _descriptors(self, per, cap):
        """the call's window descriptors in store order, as a ctypes array of `cap` entries (the ones behind the windows stay zero)"""
        arr = (self._desc_type * cap)()
        i = 0
        for im, H, W, grids in per:
            for (_, mirror, _), (Hv, Wv, ys, xs, _) in zip(self._views, grids):
                for y in ys:
                    for x in xs:
                        _fill(arr[i], image=im.data_ptr(), H=H, W=W, Hv=Hv, Wv=Wv, y0=y, x0=x, mirror=int(mirror))
                        i += 1
        return arr

    def _upload(self, per, T):
        """The call's descriptor table on the device -> its address.  It travels through pinned host words (dynamic.PinnedWords, made
        again when the table grows): the next call waits for this one copy, not for the device.  Gated: the windows' valid extents
        (_extents) travel behind the table, from byte `_ext_off` on."""
        B = self.batch_shape[0]
        cap = -(-T // B) * B
        data = bytes(self._descriptors(per, cap))
        if self.threshold is not None:
            self._ext_off = (len(data) + 15) // 16 * 16
            data = data.ljust(self._ext_off, b'\0') + self._extents(per, cap)
        if self._desc is None or self._desc.host.numel() < len(data):
            self._desc = _dynamic.PinnedWords((1, 1, len(data)), torch.uint8, self.dev)
        return self._desc.put(0, torch.frombuffer(bytearray(data), dtype=torch.uint8)).data_ptr()

    def _cut(self, table, t0, n):
        """one gather launch: windows t0 .. t0+n-1 of the descriptor table -> rows 0 .. n-1 of the resident input"""
        B, Cin, th, tw = self.batch_shape
        self._launch(self._gather, table + t0 * C.sizeof(self._desc_type), n, Cin, th, tw, self.x.data_ptr(), B)

    def _run_static(self, table, T):
        """chunk by chunk through the static plan: gather, replay, the chunk's logits into the store"""
        B = self.batch_shape[0]
        logits = self.out.src.raw.view()
        for t in range(0, T, B):
            nb = min(B, T - t)
            self._cut(table, t, nb)
            self._replay()
            self._store[t:t + nb, :, :, :self.ncls].copy_(logits[:nb])

    def _stitch(self, per):
        """one stitching-head launch per image: the store's windows -> the image's label map, a slice of the call's label bytes"""
        (th, tw), (h, w) = self.batch_shape[2:], self.low
        name, block, views_of = self._head
        npix = sum(H * W for _, H, W, _ in per)
        if self._label_buf is None or self._label_buf.numel() < npix:
            self._label_buf = torch.zeros(npix, dtype=torch.uint8, device=self.dev)
        maps, off = [], 0
        for _, H, W, grids in per:
            lab = self._label_buf[off:off + H * W].view(H, W)
            off += H * W
            a = block()
            _fill(a, nview=len(grids), logits=self._store.data_ptr(), ld=self.ld, h=h, w=w, th=th, tw=tw, N=1, C=self.ncls, OH=H, OW=W,
                  lut256=self.lut.data_ptr() if self.lut is not None else None, labels=lab.data_ptr())
            for v, (_, mirror, weight), (Hv, Wv, ys, xs, t0) in zip(views_of(a), self._views, grids):
                _fill(v, Hv=Hv, Wv=Wv, t0=t0, ny=len(ys), nx=len(xs), mirror=int(mirror), weight=weight, y0=ys, x0=xs)
            self._launch(name, C.byref(a))
            maps.append(lab)
        return maps

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
        per, tiles = self._windows(images)
        T = len(tiles)
        if self.threshold is not None:
            thr = _dynamic.gate_thresholds(self.threshold if threshold is None else threshold, self.gates)
        elif threshold is not None:
            raise ValueError('this TiledSegmenter was built without a threshold: its plan has no gates')
        if self._storage() != self._ptrs:          # the parameters moved: the plan (and with it the class count and grid) is rebuilt first
            self._build()
        row = self.low + (self.ld,)
        if self._store is None or self._store.shape[0] < T or tuple(self._store.shape[1:]) != row:
            self._store = torch.zeros((T,) + row, dtype=torch.float32, device=self.dev)      # outside the graph: it may grow
        with torch.no_grad():
            table = self._upload(per, T)
            if self.threshold is None:
                self._run_static(table, T)
            else:
                self.calls += 1
                self._run_gated(table, T, thr)
            maps = self._stitch(per)
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
