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
"""
import math

import torch

from . import _lib as L
from .heads import label_lut as _label_lut
from .resident import InferenceStep


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
