"""Static label-map inference (reference eval.py:218-221: `pred = argmax(output, 1)`): one exit of the path in inference form,
ending in the label head — ONE `addk_label_upsample` launch writes the uint8 [N,H,W] arg-max map straight from the decoder's
low-resolution logits (plan.Graph.labels), so the [N,19,H,W] logits are never written and no such buffer exists.  The plan holds
the trunk only up to the chosen exit's cell: an early exit costs its share of the network.  Emitted once over a resident input
buffer and replayed as a single hipGraph launch.

    seg = Segmenter(model, (N, 3, H, W), exit=-1, label_lut=decode_segmap_lut())
    for images in loader:
        labels = seg.step(images)            # uint8 [N,H,W], plan-owned: overwritten by the next step; no host synchronisation
"""
import os

import torch

from . import _lib as L
from . import plan as _plan
from .module import ensure_layout
from .plan import Graph


class Segmenter:
    def __init__(self, model, batch_shape, exit=-1, label_lut=None, use_graph=None, nstreams=None):
        from .modeling.ADD import ADD
        if not isinstance(model, ADD):
            raise TypeError('Segmenter takes an ADD model (got %s)' % type(model).__name__)
        self.exit = range(model.num_exits())[exit]             # forward()'s output list; IndexError out of range
        self.lib = L.load()
        p0 = next(model.parameters())
        _plan.require_device(p0)
        self.model, self.dev = model, p0.device
        self.batch_shape = tuple(int(v) for v in batch_shape)
        self.lut = _plan.label_lut(label_lut, self.dev)
        self.x = torch.zeros(self.batch_shape, dtype=torch.float32, device=self.dev)
        if nstreams is None:
            nstreams = int(os.environ.get('ADDK_STREAMS', '2'))
        self.nstreams = nstreams
        if use_graph is None:
            use_graph = self.dev.type == 'cuda' and os.environ.get('ADDK_GRAPH_INFER', '1') == '1'
        self.use_graph = use_graph
        self._build()

    # ---------------- plan ----------------
    def _build(self):
        """Emit the plan for the model's CURRENT parameter storage (the launch list holds raw pointers; step() builds again when
        they move, as validate.ValidationStep does)."""
        model = self.model
        N, _, H, W = self.batch_shape
        for p in model.parameters():
            ensure_layout(p)
        # an inference plan whatever model.training says (Graph.training decides, not the modules): the model's mode, parameters,
        # running statistics and num_batches_tracked are left alone
        g = self.g = Graph(self.dev, False, False, None)
        g.labels = {'lut': self.lut}
        g.reorder = True
        a, self.inref = g.input_nchw(self.x)
        self.inref.bind(self.x)
        self.out = model._emit_exit(g, a, self.exit)
        assert self.out.labels and tuple(self.out.y.shape) == (N, H, W), 'the model did not end in Graph.resize_to_nchw'
        g.finalize(self.nstreams)
        assert not g.bwd and not g.nbt
        self._ptrs = self._storage()
        self.nbytes = g.nbytes
        self.graph, self.calls = None, 0

    def _storage(self):
        """addresses the launch list was built on: the parameters the plan touches and the BatchNorm running statistics"""
        bufs = [b for n, b in self.model.named_buffers() if not n.endswith('num_batches_tracked')]
        return [t.data_ptr() for t in list(self.g.params) + bufs]

    # ---------------- replay ----------------
    def _run(self):
        main = torch.cuda.current_stream() if self.dev.type == 'cuda' else None
        self.g.run_parallel(self.g.fwd, main)

    def step(self, images=None):
        """-> the uint8 [N,H,W] label map of the resident batch (or of `images` if given).  The tensor belongs to the plan and is
        overwritten by the next step.  No host synchronisation, except once when the third call captures the hipGraph."""
        if self._storage() != self._ptrs:
            self._build()
        if images is not None:
            self.x.copy_(images, non_blocking=True)
        self.calls += 1
        with torch.no_grad():
            if self.use_graph and self.calls >= 3:
                if self.graph is None:             # the list has run eagerly twice; the capture itself executes nothing
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                        self._run()
                    self.graph = graph
                self.graph.replay()
            else:
                self._run()
        return self.out.y

    def close(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        self.graph = None
