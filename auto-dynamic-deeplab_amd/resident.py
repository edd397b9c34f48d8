"""The resident inference plan: the path in inference form, emitted ONCE over resident input (and target) buffers into a static
plan.Graph and replayed as a single hipGraph launch.  validate.ValidationStep, exit_profile.ExitProfile and segment.Segmenter are
this plan with another logits head (plan.Graph.head, emitted by heads.py) and another result; each supplies `head`, `_emit` and its own `step`
(segment.Segmenter and MultiViewSegmenter share theirs: segment._LabelStep)."""
import torch

from . import _lib as L
from . import plan as _plan
from .module import ensure_layout
from .plan import Graph


class InferenceStep:
    head = None          # plan.Graph.head, a key of heads.HEADS: who consumes the decoder's low-resolution logits
    lut = None           # plan.Graph.lut of a 'labels' head
    nex = 0              # exits, fixed together with `ncls` by the first build

    def __init__(self, model, batch_shape, use_graph, nstreams, target=True):
        """The resident buffers and the replay defaults; the subclass calls _build() once its own tensors exist."""
        self.lib = L.load()
        p0 = next(model.parameters())
        _plan.require_device(p0)
        self.model, self.dev = model, p0.device
        self.batch_shape = tuple(int(v) for v in batch_shape)
        N, _, H, W = self.batch_shape
        self.x = torch.zeros(self.batch_shape, dtype=torch.float32, device=self.dev)
        self.target = torch.zeros((N, H, W), dtype=torch.int64, device=self.dev) if target else None
        self.nstreams = _plan.env_streams() if nstreams is None else nstreams
        self.use_graph = self.dev.type == 'cuda' and _plan.env_graph_infer() if use_graph is None else use_graph

    # ---------------- plan ----------------
    def _build(self):
        """Emit the plan for the model's CURRENT parameter storage.  The launch list holds raw pointers: a TrainStep built on the
        same model later re-points the parameters into its flat buffer, `.to()` re-allocates them — _replay() then builds again,
        which drops the captured graph; whatever a step has accumulated stays."""
        for p in self.model.parameters():
            ensure_layout(p)
        # an inference plan whatever model.training says (Graph.training decides, not the modules): the model's mode, parameters,
        # running statistics and num_batches_tracked are left alone
        g = self.g = Graph(self.dev, False, False, None)
        g.head, g.lut = self.head, self.lut
        g.reorder = True
        a, self.inref = g.input_nchw(self.x)
        self.inref.bind(self.x)
        self._emit(g, a)
        g.finalize(self.nstreams)
        assert not g.bwd and not g.nbt
        self._ptrs = self._storage()
        self.nbytes = g.nbytes
        self.graph, self.calls = None, 0

    def _emit(self, g, a):
        """Emit the model from the input activation `a`, keep its OutRefs and bind what this step's heads write; on the first build
        allocate those tensors."""
        raise NotImplementedError

    def _emit_exits(self, g, a):
        """model.emit: every exit, each ending in this step's head -> (OutRefs, whether this is the first build, which fixes nex / ncls)."""
        N, _, H, W = self.batch_shape
        outs = self.model.emit(g, a)
        outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
        assert all(getattr(o, 'head', None) == self.head for o in outs), 'the model did not end in Graph.resize_to_nchw'
        ncls = outs[0].shape[1]
        assert all(tuple(o.shape) == (N, ncls, H, W) for o in outs)
        first = self.nex == 0
        if first:
            self.nex, self.ncls = len(outs), ncls
        assert (len(outs), ncls) == (self.nex, self.ncls)
        return outs, first

    def _storage(self):
        """addresses the launch list was built on: the parameters the plan touches and the BatchNorm running statistics"""
        bufs = [b for n, b in self.model.named_buffers() if not n.endswith('num_batches_tracked')]
        return [t.data_ptr() for t in list(self.g.params) + bufs]

    # ---------------- replay ----------------
    def _run(self):
        """One pass of the list; what _replay() captures."""
        main = torch.cuda.current_stream() if self.dev.type == 'cuda' else None
        self.g.run_parallel(self.g.fwd, main)

    def load_batch(self, images, targets=None):
        self.x.copy_(images, non_blocking=True)
        if self.target is not None:
            self.target.copy_(targets, non_blocking=True)

    def _replay(self):
        """Run the plan on the resident batch.  No host synchronisation, except once when the third call captures the hipGraph."""
        if self._storage() != self._ptrs:
            self._build()
        self.calls += 1
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

    def close(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        self.graph = None
