"""Validation pass of the path (reference train.py:250-322, eval.py:165-193): forward of all exits in inference form and, per
exit, the criterion, the evaluator's confusion matrix and the entropy meter — emitted as ONE static plan over resident
input / target buffers and replayed as a single hipGraph launch.  The full-resolution logits are never written: every exit
ends in one `addk_score_upsample` launch that scores the decoder's low-resolution logits (plan.Graph.fuse_score).

    val = ValidationStep(model, (N, 3, H, W), class_weight=w)
    for images, targets in loader:
        val.step(images, targets)            # no host synchronisation
    r = val.result()                         # the one sync: r['exits'][i]['mIoU'], r['test_loss'], r['new_pred'], ...
"""
import math
import os

import torch

from . import _lib as L
from . import plan as _plan
from .metrics import mean_iou
from .module import ensure_layout
from .plan import Graph


class ValidationStep:
    def __init__(self, model, batch_shape, class_weight=None, ignore_index=255, keep_predictions=False, use_graph=None,
                 nstreams=None):
        self.lib = L.load()
        p0 = next(model.parameters())
        _plan.require_device(p0)
        self.model, self.dev = model, p0.device
        self.batch_shape = tuple(int(v) for v in batch_shape)
        N, _, H, W = self.batch_shape
        self.ignore_index = int(ignore_index)
        self.keep_predictions = bool(keep_predictions)
        self.x = torch.zeros(self.batch_shape, dtype=torch.float32, device=self.dev)
        self.target = torch.zeros((N, H, W), dtype=torch.int64, device=self.dev)
        self.cw = class_weight.to(self.dev).float().contiguous() if class_weight is not None else None
        self.wsum = torch.zeros(1, dtype=torch.float32, device=self.dev)
        if nstreams is None:
            nstreams = int(os.environ.get('ADDK_STREAMS', '2'))
        self.nstreams = nstreams
        if use_graph is None:
            use_graph = self.dev.type == 'cuda' and os.environ.get('ADDK_GRAPH_INFER', '1') == '1'
        self.use_graph = use_graph
        self.nex = 0
        self._build()
        self.batches = 0

    # ---------------- plan ----------------
    def _build(self):
        """Emit the plan for the model's CURRENT parameter storage.  The launch list holds raw pointers: a TrainStep built on the
        same model later re-points the parameters into its flat buffer, `.to()` re-allocates them — step() then builds again."""
        lib, dev, model = self.lib, self.dev, self.model
        N, _, H, W = self.batch_shape
        for p in model.parameters():
            ensure_layout(p)
        # an inference plan whatever model.training says (Graph.training decides, not the modules): the model's mode, parameters,
        # running statistics and num_batches_tracked are left alone
        g = self.g = Graph(dev, False, False, None)
        g.fuse_score = True
        g.reorder = True
        a, self.inref = g.input_nchw(self.x)
        self.inref.bind(self.x)
        outs = model.emit(g, a)
        outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
        assert all(getattr(o, 'fused_score', False) for o in outs), 'the model did not end in Graph.resize_to_nchw'
        nex, ncls = len(outs), outs[0].shape[1]
        assert all(tuple(o.shape) == (N, ncls, H, W) for o in outs)
        if self.cw is not None and self.cw.numel() != ncls:
            raise ValueError('ValidationStep: class_weight has %d entries for %d classes' % (self.cw.numel(), ncls))
        if self.nex == 0:
            self.nex, self.ncls = nex, ncls
            self.scal = torch.zeros(2 * nex, dtype=torch.float32, device=dev)     # this batch: [loss per exit | entropy sum per exit]
            self.acc = torch.zeros(2 * nex, dtype=torch.float64, device=dev)      # running sums of `scal` over the batches
            self.cm = torch.zeros((nex, ncls, ncls), dtype=torch.int64, device=dev)
            self.pred = torch.zeros((nex, N, H, W), dtype=torch.uint8, device=dev) if self.keep_predictions else None
        assert (nex, ncls) == (self.nex, self.ncls)
        ws = torch.zeros(int(lib.addk_ce_ws_floats(N, H * W)), dtype=torch.float32, device=dev)
        self._keep = [ws]
        cwp = self.cw.data_ptr() if self.cw is not None else None
        g._add(g.fwd, 'score_zero', lib.addk_fill, self.scal.data_ptr(), 2 * nex, 0.0, wr=[self.scal])
        g._add(g.fwd, 'ce_count', lib.addk_ce_count, self.target.data_ptr(), N * H * W, cwp, self.ignore_index, ncls,
               self.wsum.data_ptr(), ws.data_ptr(), rd=[self.target], wr=[self.wsum, ws])      # one count for every exit
        for i, o in enumerate(outs):
            o.score = dict(target=self.target, class_w=cwp, ignore_index=self.ignore_index, wsum=self.wsum, scale=1.0,
                           loss=self.scal[i:i + 1], entropy=self.scal[nex + i:nex + i + 1], confusion=self.cm[i],
                           pred=self.pred[i] if self.pred is not None else None)
        self.outs = outs
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
        self.acc.add_(self.scal)               # fp64 += fp32, on the stream the list joined; inside the captured region too

    def load_batch(self, images, targets):
        self.x.copy_(images, non_blocking=True)
        self.target.copy_(targets, non_blocking=True)

    def step(self, images=None, targets=None):
        """Scores the resident batch (or `images` / `targets` if given) and adds it to the running figures on the device.  No
        host synchronisation, except once when the third call captures the hipGraph."""
        if self._storage() != self._ptrs:
            self._build()
        if images is not None:
            self.load_batch(images, targets)
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
        self.batches += 1

    # ---------------- results ----------------
    def reset(self):
        self.acc.zero_()
        self.cm.zero_()
        self.batches = 0

    def result(self):
        """The single synchronisation of a pass.  Per exit: `confusion` (int64 device tensor), `mIoU` (Evaluator's formula),
        `confidence` (mean over batches of the normalised Shannon entropy, the reference's AverageMeter) and `loss` (mean over
        batches); `test_loss` = sum over batches of the mean over exits (train.py:272-273), `new_pred` = mean mIoU (train.py:313)."""
        nex = self.nex
        _, _, H, W = self.batch_shape
        miou = torch.stack([mean_iou(self.cm[i]) for i in range(nex)]).double()
        host = torch.cat([self.acc, miou]).cpu()
        nb = max(self.batches, 1)
        norm = math.log(self.ncls) * H * W     # operations.py:161-170: per pixel and per log C, not per image
        exits = []
        for i in range(nex):
            exits.append(dict(confusion=self.cm[i].clone(), mIoU=float(host[2 * nex + i]),
                              confidence=float(host[nex + i]) / norm / nb, loss=float(host[i]) / nb))
        return dict(exits=exits, test_loss=float(host[:nex].sum()) / nex, new_pred=sum(e['mIoU'] for e in exits) / nex,
                    batches=self.batches)

    def predictions(self):
        """uint8 [N,H,W] arg-max maps of the last batch, one per exit (keep_predictions=True)."""
        if not self.keep_predictions:
            raise L.AddkError('ValidationStep was built without keep_predictions=True')
        out = []
        for i, o in enumerate(self.outs):
            wide = o.score.get('pred_i64')      # exits scored by the stand-alone kernels keep an int64 map
            out.append(wide.to(torch.uint8) if wide is not None else self.pred[i].clone())
        return out

    def close(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        self.graph = None
