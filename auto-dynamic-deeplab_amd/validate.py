"""Validation pass of the path (reference train.py:250-322, eval.py:165-193): forward of all exits in inference form and, per
exit, the criterion, the evaluator's confusion matrix and the entropy meter — emitted as ONE static plan over resident
input / target buffers and replayed as a single hipGraph launch.  The full-resolution logits are never written: every exit
ends in one `addk_score_upsample` launch that scores the decoder's low-resolution logits (plan.Graph.head 'score': heads._score_head).

    val = ValidationStep(model, (N, 3, H, W), class_weight=w)
    for images, targets in loader:
        val.step(images, targets)            # no host synchronisation
    r = val.result()                         # the one sync: r['exits'][i]['mIoU'], r['test_loss'], r['new_pred'], ...
"""
import math

import torch

from . import _lib as L
from . import trimap as _trimap
from .metrics import mean_iou
from .resident import InferenceStep


class ValidationStep(InferenceStep):
    head = 'score'

    def __init__(self, model, batch_shape, class_weight=None, ignore_index=255, keep_predictions=False, use_graph=None,
                 nstreams=None, trimap=None):
        super().__init__(model, batch_shape, use_graph, nstreams)
        # boundary-band mIoU (trimap.py): None, or the ladder of widths in pixels
        self.trimap = _trimap.check_widths(trimap) if trimap is not None else None
        self.ignore_index = int(ignore_index)
        self.keep_predictions = bool(keep_predictions)
        self.cw = class_weight.to(self.dev).float().contiguous() if class_weight is not None else None
        self.wsum = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self._build()
        self.batches = 0

    # ---------------- plan ----------------
    def _emit(self, g, a):
        lib, dev = self.lib, self.dev
        N, _, H, W = self.batch_shape
        outs, first = self._emit_exits(g, a)
        nex, ncls = self.nex, self.ncls
        if self.cw is not None and self.cw.numel() != ncls:
            raise ValueError('ValidationStep: class_weight has %d entries for %d classes' % (self.cw.numel(), ncls))
        if first:
            self.scal = torch.zeros(2 * nex, dtype=torch.float32, device=dev)     # this batch: [loss per exit | entropy sum per exit]
            self.acc = torch.zeros(2 * nex, dtype=torch.float64, device=dev)      # running sums of `scal` over the batches
            self.cm = torch.zeros((nex, ncls, ncls), dtype=torch.int64, device=dev)
            # the band launches read the uint8 maps: with a trimap they exist whether or not predictions() hands them out
            want_pred = self.keep_predictions or self.trimap is not None
            self.pred = torch.zeros((nex, N, H, W), dtype=torch.uint8, device=dev) if want_pred else None
            if self.trimap is not None:
                self.rings = torch.zeros((nex, len(self.trimap), ncls, ncls), dtype=torch.int64, device=dev)   # accumulate like `cm`
                self.dist = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
        ws =torch.zeros(int(lib.addk_ce_ws_floats(N, H * W)), dtype=torch.float32, device=dev)
        self._keep = [ws]
        cwp = self.cw.data_ptr() if self.cw is not None else None
        g._add(g.fwd, 'score_zero', lib.addk_fill, self.scal.data_ptr(), 2 * nex, 0.0, wr=[self.scal])
        g._add(g.fwd, 'ce_count', lib.addk_ce_count, self.target.data_ptr(), N * H * W, cwp, self.ignore_index, ncls,
               self.wsum.data_ptr(), ws.data_ptr(), rd=[self.target], wr=[self.wsum, ws])      # one count for every exit
        if self.trimap is not None:
            _trimap.emit_boundary_dist(g, self.target, self.dist, ncls, self.trimap)          # one distance map for every exit
        for i, o in enumerate(outs):
            o.binding = dict(target=self.target, class_w=cwp, ignore_index=self.ignore_index, wsum=self.wsum, scale=1.0,
                             loss=self.scal[i:i + 1], entropy=self.scal[nex + i:nex + i + 1], confusion=self.cm[i],
                             pred=self.pred[i] if self.pred is not None else None)
            if self.trimap is not None:
                o.binding['trimap'] = dict(rings=self.rings[i], widths=self.trimap, dist=self.dist)
        self.outs = outs

    # ---------------- replay ----------------
    def _run(self):
        super()._run()
        self.acc.add_(self.scal)               # fp64 += fp32, on the stream the list joined; inside the captured region too

    def step(self, images=None, targets=None):
        """Scores the resident batch (or `images` / `targets` if given) and adds it to the running figures on the device.  No
        host synchronisation, except once when the third call captures the hipGraph."""
        if images is not None:
            self.load_batch(images, targets)
        self._replay()
        self.batches += 1

    # ---------------- results ----------------
    def reset(self):
        self.acc.zero_()
        self.cm.zero_()
        if self.trimap is not None:
            self.rings.zero_()
        self.batches = 0

    def result(self):
        """The single synchronisation of a pass.  Per exit: `confusion` (int64 device tensor), `mIoU` (Evaluator's formula),
        `confidence` (mean over batches of the normalised Shannon entropy, the reference's AverageMeter) and `loss` (mean over
        batches); `test_loss` = sum over batches of the mean over exits (train.py:272-273), `new_pred` = mean mIoU (train.py:313).
        Built with `trimap=widths`: also `trimap_widths` and, per exit, `trimap`: one dict per width with `width`, `confusion` (int64 [C,C]
        over the pixels within `width` of a ground-truth class boundary, include/addk.h), its `mIoU` and `pixels`."""
        nex = self.nex
        _, _, H, W = self.batch_shape
        miou = torch.stack([mean_iou(self.cm[i]) for i in range(nex)]).double()
        parts = [self.acc, miou]
        if self.trimap is not None:
            cum = self.rings.cumsum(1)             # the rings are disjoint: "within w[j]" is their prefix sum
            parts.append(_trimap.band_figures(cum))
        host = torch.cat(parts).cpu()
        nb = max(self.batches, 1)
        norm = math.log(self.ncls) * H * W     # operations.py:161-170: per pixel and per log C, not per image
        exits = []
        for i in range(nex):
            exits.append(dict(confusion=self.cm[i].clone(), mIoU=float(host[2 * nex + i]),
                              confidence=float(host[nex + i]) / norm / nb, loss=float(host[i]) / nb))
        r = dict(exits=exits, test_loss=float(host[:nex].sum()) / nex, new_pred=sum(e['mIoU'] for e in exits) / nex,
                 batches=self.batches)
        if self.trimap is not None:
            fig = host[3 * nex:].reshape(2, nex, len(self.trimap))
            for i, e in enumerate(exits):
                e['trimap'] = _trimap.band_entries(self.trimap, cum[i], (fig[0, i], fig[1, i]))
            r['trimap_widths'] = self.trimap
        return r

    def predictions(self):
        """uint8 [N,H,W] arg-max maps of the last batch, one per exit (keep_predictions=True)."""
        if not self.keep_predictions:
            raise L.AddkError('ValidationStep was built without keep_predictions=True')
        out = []
        for i, o in enumerate(self.outs):
            wide = o.binding.get('pred_i64')      # exits scored by the stand-alone kernels keep an int64 map
            out.append(wide.to(torch.uint8) if wide is not None else self.pred[i].clone())
        return out
