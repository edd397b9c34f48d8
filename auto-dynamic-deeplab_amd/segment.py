"""Static label-map inference (reference eval.py:218-221: `pred = argmax(output, 1)`): one exit of the path in inference form,
ending in the label head — ONE `addk_label_upsample` launch writes the uint8 [N,H,W] arg-max map straight from the decoder's
low-resolution logits (plan.Graph.head 'labels'), so the [N,19,H,W] logits are never written and no such buffer exists.  The plan holds
the trunk only up to the chosen exit's cell: an early exit costs its share of the network.  Emitted once over a resident input
buffer and replayed as a single hipGraph launch.

    seg = Segmenter(model, (N, 3, H, W), exit=-1, label_lut=decode_segmap_lut())
    for images in loader:
        labels = seg.step(images)            # uint8 [N,H,W], plan-owned: overwritten by the next step; no host synchronisation
"""
import torch

from . import plan as _plan
from .resident import InferenceStep


class Segmenter(InferenceStep):
    head = 'labels'

    def __init__(self, model, batch_shape, exit=-1, label_lut=None, use_graph=None, nstreams=None):
        from .modeling.ADD import ADD
        if not isinstance(model, ADD):
            raise TypeError('Segmenter takes an ADD model (got %s)' % type(model).__name__)
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.lut = _plan.label_lut(label_lut, next(model.parameters()).device)
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
