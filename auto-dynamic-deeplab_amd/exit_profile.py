"""Early-exit operating curve from ONE validation pass (reference eval.py:195-230, `Evaluation.dynamic_inference`).

The reference runs every validation image through the gated network at one threshold and prints mIoU, the share of early exits and
the average confidence; a sweep repeats the whole set per threshold.  For the 'entropy' and 'max' gates (dynamic.GatePlan) none of
what the gate reads depends on the threshold of the DECISION: exit k's prediction is forward()'s `model(x)[k]`, its entropy is one
number per image, and its top-probability share is one number per image and per top-probability threshold.  ExitProfile therefore runs
the static, batched inference plan of resident.InferenceStep and ends every exit in one `addk_profile_upsample` launch
(plan.Graph.head 'profile', heads.py; csrc/score_up.hip profile_up_kernel) that leaves, PER IMAGE, the entropy, the share at each of `max_thresholds` and the
confusion matrix.  Every point of the curve follows on the host (exit_curve) by GatePlan.run's own decision rule.

    prof = ExitProfile(model, (N, 3, H, W), max_thresholds=(0.5, 0.9, 0.99))
    for images, targets in loader:
        prof.step(images, targets)           # no host synchronisation
    rec = prof.records()                     # the one sync
    pts = prof.curve('entropy', thresholds=[0.1, 0.2, 0.3])
    pts = prof.curve('max')                  # at max_thresholds

The 'edm' gate is out of reach of this pass: its early head is not forward()'s.

`temperature` (None, a scalar or one per exit, e.g. calibrate.ExitCalibration.fit()): entropy and shares are those of
softmax(z_k / T_k), what dynamic_inference(..., temperature=) judges — the curve of the tempered gates.  Matrices and maps do not move."""
import torch

from . import _lib as L
from . import trimap as _trimap
from .dynamic import KINDS, check_temperature, finite_threshold, inverse_words
from .metrics import mean_iou
from .resident import InferenceStep

MAX_THRESHOLDS = 16


def _check_thresholds(ts):
    ts = [float(t) for t in ts]
    if len(ts) > MAX_THRESHOLDS:
        raise ValueError('at most %d max_thresholds (got %d)' % (MAX_THRESHOLDS, len(ts)))
    if any(not b > a for a, b in zip(ts, ts[1:])) or any(t != t for t in ts):
        raise ValueError('max_thresholds must be strictly ascending (got %r)' % (ts,))
    return tuple(ts)


def exit_curve(entropy, share, confusion, kind, thresholds, max_thresholds=None, exit_ms=None, band_confusion=None, widths=None):
    """Operating points of the early-exit network from per-image records, on CPU tensors:
    entropy [nex, M] fp32, share [nex, M, NT] fp32 (NT = len(max_thresholds)), confusion [nex, M, C, C] int64.

    Decision per image, exactly dynamic.GatePlan.run's: the early exits k = 0 .. nex-2 in order, the recorded fp32 value promoted to a
    Python float and compared with the Python-float threshold — 'entropy': the image leaves at the first k with entropy[k, i] < thr;
    'max': at the first k with share[k, i, j] > thr, where thr == max_thresholds[j] (one number in both roles, ADD.py:476,481; any other
    threshold is a ValueError) — otherwise it takes the final exit.  Its confidence is the last gate value evaluated.

    One dict per threshold with the figures of eval.py:223-230: `threshold`, `mIoU` and `confusion` (sum of the chosen exits' matrices),
    `exit_of_image` (int64 [M]; nex-1 is the final exit), `exit_counts` (images per exit), `num_earlier_exit` (percent of M),
    `avg_confidence` (mean over the M images; `confidence_of_image` holds the M values, fp64).  With `exit_ms` (one latency per exit,
    measured by the caller) also `expected_ms` = sum_k exit_counts[k] * exit_ms[k] / M and `fps` = 1000 / expected_ms: a PROJECTION from the supplied latencies
    (`projected_from_exit_ms` is True), nothing here is timed.

    With `band_confusion` [nex, M, nw, C, C] int64 (per image, cumulative over `widths`: ExitProfile.records()) every point also has
    `trimap`: one dict per width with `width`, `confusion` (the chosen exits' band matrices summed), `mIoU` and `pixels`."""
    if kind not in KINDS:
        raise ValueError('kind must be one of %s (got %r)' % (KINDS, kind))
    nex, M = int(entropy.shape[0]), int(entropy.shape[1])
    if tuple(confusion.shape[:2]) != (nex, M):
        raise ValueError('confusion is %s for entropy %s' % (tuple(confusion.shape), tuple(entropy.shape)))
    if band_confusion is not None:
        widths = tuple(int(w) for w in (widths if widths is not None else ()))
        if band_confusion.dim() != 5 or tuple(band_confusion.shape[:3]) != (nex, M, len(widths)):
            raise ValueError('band_confusion is %s for %d exits, %d images and %d widths' % (tuple(band_confusion.shape), nex, M, len(widths)))
    if exit_ms is not None:
        exit_ms = [float(v) for v in exit_ms]
        if len(exit_ms) != nex:
            raise ValueError('exit_ms needs one latency per exit (%d), got %d' % (nex, len(exit_ms)))
    if kind == 'max':
        mt = [float(t) for t in (max_thresholds if max_thresholds is not None else ())]
        if tuple(share.shape) != (nex, M, len(mt)):
            raise ValueError('share is %s for %d exits, %d images and %d max_thresholds' % (tuple(share.shape), nex, M, len(mt)))
    points = []
    for thr in thresholds:
        thr = float(thr)
        if kind == 'entropy':
            g = entropy
        else:
            if thr not in mt:
                raise ValueError("the 'max' gate was recorded at max_thresholds %r only (got %r)" % (tuple(mt), thr))
            g = share[:, :, mt.index(thr)]
        g = g[:nex - 1].double()                                   # fp32 -> fp64 is the promotion of float(tensor)
        leave = (g < thr) if kind == 'entropy' else (g > thr)      # [nex-1, M]
        if nex > 1:
            left = leave.any(0)
            first = leave.int().argmax(0)                          # the first exit that lets the image go
            exit_of = torch.where(left, first, torch.full_like(first, nex - 1))
            conf = g.gather(0, torch.where(left, first, torch.full_like(first, nex - 2))[None])[0]
        else:
            exit_of, conf = torch.zeros(M, dtype=torch.int64), torch.full((M,), float('nan'), dtype=torch.float64)
        cm = confusion[exit_of, torch.arange(M)].sum(0) if M else confusion.new_zeros(confusion.shape[2:])
        counts = [int(v) for v in torch.bincount(exit_of, minlength=nex)]
        pt = dict(threshold=thr, mIoU=float(mean_iou(cm)), confusion=cm, exit_of_image=exit_of, exit_counts=counts,
                  num_earlier_exit=100.0 * (M - counts[nex - 1]) / M if M else 0.0,
                  avg_confidence=float(conf.sum()) / M if M else float('nan'), confidence_of_image=conf)
        if exit_ms is not None and M:
            pt['expected_ms'] = sum(c * ms for c, ms in zip(counts, exit_ms)) / M
            pt['fps'] = 1000.0 / pt['expected_ms']
            pt['projected_from_exit_ms'] = True
        if band_confusion is not None:
            bands = band_confusion[exit_of, torch.arange(M)].sum(0) if M else band_confusion.new_zeros(band_confusion.shape[2:])
            fig = _trimap.band_figures(bands).reshape(2, len(widths))
            pt['trimap'] = _trimap.band_entries(widths, bands, (fig[0], fig[1]))
        points.append(pt)
    return points


class ExitProfile(InferenceStep):
    head = 'profile'

    def __init__(self, model, batch_shape, max_thresholds=(0.5, 0.9, 0.99), ignore_index=255, keep_predictions=False,
                 use_graph=None, nstreams=None, temperature=None, trimap=None):
        self.max_thresholds = _check_thresholds(max_thresholds)
        # boundary-band mIoU (trimap.py): None, or the ladder of widths in pixels
        self.trimap = _trimap.check_widths(trimap) if trimap is not None else None
        self.temperature = check_temperature(temperature, model.num_exits())
        super().__init__(model, batch_shape, use_graph, nstreams)
        # 1 / T of every exit: the words the tempered launches read (None: the untempered plan)
        self.temp = None if self.temperature is None else inverse_words(self.temperature).to(self.dev)
        # the evaluator counts every label in [0, classes) (utils/metrics.py:34-43); ignore_index is what the loader paints elsewhere
        self.ignore_index = int(ignore_index)
        self.keep_predictions = bool(keep_predictions)
        self.thr = torch.zeros(max(len(self.max_thresholds), 1), dtype=torch.float32, device=self.dev)
        self._write_thresholds()
        self._build()
        self.reset()

    def _write_thresholds(self):
        # the words GatePlan.set_threshold hands its kernel
        if self.max_thresholds:
            self.thr.copy_(torch.tensor([finite_threshold(t) for t in self.max_thresholds], dtype=torch.float32))

    def set_max_thresholds(self, max_thresholds):
        """Other top-probability thresholds for the steps that follow.  The same number of them: the words live in a device buffer the
        plan reads when it runs, so nothing is rebuilt or captured again.  The logs are emptied: their shares belong to the old set."""
        ts = _check_thresholds(max_thresholds)
        if len(ts) != len(self.max_thresholds):
            raise ValueError('set_max_thresholds takes %d thresholds, as the plan was built (got %d)' % (len(self.max_thresholds), len(ts)))
        self.max_thresholds = ts
        self._write_thresholds()
        self.reset()

    def set_temperature(self, temperature):
        """Other temperatures for the steps that follow (a tempered profile only): device words, so nothing is rebuilt or captured again.
        The logs are emptied when the values change: their entropies and shares belong to the old ones."""
        if self.temperature is None or temperature is None:
            raise ValueError('this ExitProfile was built %s a temperature: the other kind is another plan' % ('without' if self.temperature is None else 'with'))
        ts = check_temperature(temperature, len(self.temperature))
        if ts != self.temperature:
            self.temperature = ts
            self.temp.copy_(inverse_words(ts))
            self.reset()

    # ---------------- plan ----------------
    def _emit(self, g, a):
        dev = self.dev
        N, _, H, W = self.batch_shape
        NT = len(self.max_thresholds)
        outs, first = self._emit_exits(g, a)
        nex, ncls = self.nex, self.ncls
        if 0 <= self.ignore_index < ncls:
            raise ValueError('ExitProfile: ignore_index %d is one of the %d classes the evaluator counts' % (self.ignore_index, ncls))
        if first:
            self.ent = torch.zeros((nex, N), dtype=torch.float32, device=dev)             # this batch, per exit and image
            self.share = torch.zeros((nex, N, NT), dtype=torch.float32, device=dev)
            self.cm = torch.zeros((nex, N, ncls, ncls), dtype=torch.int64, device=dev)
            # the band launches read the uint8 maps: with a trimap they exist whether or not predictions() hands them out
            want_pred = self.keep_predictions or self.trimap is not None
            self.pred = torch.zeros((nex, N, H, W), dtype=torch.uint8, device=dev) if want_pred else None
            if self.trimap is not None:
                self.rings = torch.zeros((nex, N, len(self.trimap), ncls, ncls), dtype=torch.int64, device=dev)   # this batch, per image
                self.dist = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
        # the launch adds into the matrices: zero bits of int64 written as twice as many fp32 zeros
        g._add(g.fwd, 'profile_zero', self.lib.addk_fill, self.cm.data_ptr(), 2 * self.cm.numel(), 0.0, wr=[self.cm])
        if self.trimap is not None:
            g._add(g.fwd, 'trimap_zero', self.lib.addk_fill, self.rings.data_ptr(), 2 * self.rings.numel(), 0.0, wr=[self.rings])
            _trimap.emit_boundary_dist(g, self.target, self.dist, ncls, self.trimap)          # one distance map for every exit
        for i, o in enumerate(outs):
            o.binding = dict(target=self.target, thr=self.thr, nthr=NT, entropy=self.ent[i], share=self.share[i], confusion=self.cm[i],
                             pred=self.pred[i] if self.pred is not None else None)
            if self.trimap is not None:
                o.binding['trimap'] = dict(rings=self.rings[i], widths=self.trimap, dist=self.dist,
                                           image_stride=len(self.trimap) * ncls * ncls)
            if self.temp is not None:
                o.binding['temp'] = self.temp[i:i + 1]
        self.outs = outs

    # ---------------- replay ----------------
    def step(self, images=None, targets=None, count=None):
        """Profiles the resident batch (or `images` / `targets` if given) and appends the rows of its first `count` images (default: all N;
        a short last batch passes fewer and the rest is dropped) to the device-side logs.  No host synchronisation, except once when the
        third call captures the hipGraph."""
        N = self.batch_shape[0]
        count = N if count is None else int(count)
        if not 0 <= count <= N:
            raise ValueError('count must lie in [0, %d] (got %d)' % (N, count))
        if images is not None:
            self.load_batch(images, targets)
        self._replay()
        # outside the captured region, ordered behind it on the same stream: copies of the batch's rows
        row = (self.ent[:, :count].clone(), self.share[:, :count].clone(), self.cm[:, :count].clone())
        self._log.append(row + (self.rings[:, :count].clone(),) if self.trimap is not None else row)
        self.batches += 1

    # ---------------- results ----------------
    def reset(self):
        self._log, self._rec, self.batches = [], None, 0

    def records(self):
        """The single synchronisation of a pass: `entropy` [nex, M] fp32, `share` [nex, M, NT] fp32 and `confusion` [nex, M, C, C] int64
        of the M images logged since reset(), on the CPU, and `static`: per exit the summed `confusion` and its `mIoU` by
        metrics.mean_iou — the figures ValidationStep.result() reports for the same images.  Built with `trimap=widths`: also
        `trimap_widths`, `band_confusion` [nex, M, nw, C, C] int64 (per image, cumulative over the widths: the pixels within widths[j] of a
        ground-truth class boundary, include/addk.h) and, in every `static[i]`, `trimap` as in ValidationStep.result()."""
        if self._rec is not None and self._rec[0] == len(self._log):
            return self._rec[1]
        nex, NT, C_ = self.nex, len(self.max_thresholds), self.ncls
        if self._log:
            ent, share, cm, *rings = (torch.cat(ts, dim=1) for ts in zip(*self._log))
        else:
            ent, share = self.ent.new_zeros((nex, 0)), self.share.new_zeros((nex, 0, NT))
            cm = self.cm.new_zeros((nex, 0, C_, C_))
            rings = [self.rings.new_zeros((nex, 0) + tuple(self.rings.shape[2:]))] if self.trimap is not None else []
        total = cm.sum(1)
        miou = torch.stack([mean_iou(total[i]) for i in range(nex)]).cpu()
        rec = dict(entropy=ent.cpu(), share=share.cpu(), confusion=cm.cpu(), max_thresholds=self.max_thresholds,
                   static=[dict(confusion=c, mIoU=float(m)) for c, m in zip(total.cpu(), miou)])
        if self.trimap is not None:
            bands = rings[0].cumsum(2)             # the rings are disjoint: "within w[j]" is their prefix sum
            cum = bands.sum(1)
            fig = _trimap.band_figures(cum).cpu().reshape(2, nex, len(self.trimap))
            cum = cum.cpu()
            for i, s in enumerate(rec['static']):
                s['trimap'] = _trimap.band_entries(self.trimap, cum[i], (fig[0, i], fig[1, i]))
            rec['band_confusion'], rec['trimap_widths'] = bands.cpu(), self.trimap
        self._rec = (len(self._log), rec)
        return rec

    def curve(self, kind, thresholds=None, exit_ms=None):
        """exit_curve on the records: 'entropy' at `thresholds`; 'max' at `thresholds` out of max_thresholds (default: all of them)."""
        if thresholds is None:
            if kind != 'max':
                raise ValueError("curve(%r) needs thresholds; only 'max' has recorded ones" % (kind,))
            thresholds = self.max_thresholds
        r = self.records()
        return exit_curve(r['entropy'], r['share'], r['confusion'], kind, thresholds, self.max_thresholds, exit_ms,
                          band_confusion=r.get('band_confusion'), widths=r.get('trimap_widths'))

    def predictions(self):
        """uint8 [N,H,W] arg-max maps of the last batch, one per exit (keep_predictions=True)."""
        if not self.keep_predictions:
            raise L.AddkError('ExitProfile was built without keep_predictions=True')
        return [self.pred[i].clone() for i in range(self.nex)]
