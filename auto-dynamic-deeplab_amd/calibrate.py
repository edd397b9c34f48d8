"""Per-exit temperature scaling (Guo et al. 2017) from ONE validation pass.

ADD has one Decoder, so one 1x1 classifier serves every exit: the same weights on features of different depth, and an early exit is
not as confident as the final one for the same accuracy.  The 'entropy' and 'max' gates (dynamic.GatePlan) compare that confidence with
one threshold for all exits.  Temperature scaling fits one scalar T per exit by minimising the NLL of softmax(z / T) on the validation
set; the arg-max does not move, so label maps and mIoU are untouched, and the gates then judge softmax(z_k / T_k).

ExitCalibration runs the static, batched inference plan of resident.InferenceStep and ends every exit in one `addk_calib_upsample`
launch (plan.Graph.head 'calib': heads._calib_head, csrc/calib_up.hip) that adds, for up to 8 temperatures at once, the reliability bins (16 equal-width
bins of the top probability: count, hits, confidence sum) and the NLL sum of the exit's up-sampled prediction to device accumulators.

    cal = ExitCalibration(model, (N, 3, H, W))
    for images, targets in loader:
        cal.step(images, targets)            # no host synchronisation
    res = cal.result()                       # the one sync: per exit nll / ece / mce / bins per temperature
    T = cal.fit()                            # one temperature per exit
    ExitProfile(model, shape, temperature=T) / model.dynamic_inference(x, thr, 'entropy', temperature=T)

The fit is a grid search refined by a parabola in log T (fit_temperature); when the minimum sits at an end of the grid, widen it with
set_temperatures and run the pass again."""
import math

import torch

from . import _lib as L
from .resident import InferenceStep

TEMPERATURES = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0)
CONF_UNIT = 2.0 ** -24          # the kernel sums confidences as integers in this unit


def _check_temperatures(ts):
    ts = [float(t) for t in ts]
    if not 1 <= len(ts) <= L.CALIB_MAX_T:
        raise ValueError('1..%d temperatures (got %d)' % (L.CALIB_MAX_T, len(ts)))
    if any(not (0.0 < t < float('inf')) for t in ts) or any(not b > a for a, b in zip(ts, ts[1:])):
        raise ValueError('temperatures must be positive, finite and strictly ascending (got %r)' % (ts,))
    return tuple(ts)


def reliability(bins, conf_sum):
    """Reliability diagram of one exit at one temperature from its bins: `bins` [B, 2] (count, hits) and `conf_sum` [B] (sum of the top
    probability per bin) -> dict with `ece` = sum_b |hits_b - conf_b| / valid (the count-weighted mean gap between accuracy and
    confidence), `mce` = the largest gap of a non-empty bin, and per bin `accuracy` and `confidence` (NaN for an empty bin), fp64."""
    bins = torch.as_tensor(bins).double()
    conf_sum = torch.as_tensor(conf_sum).double()
    count, hits = bins[:, 0], bins[:, 1]
    valid = float(count.sum())
    some = count > 0
    safe = torch.where(some, count, torch.ones_like(count))
    nan = torch.full_like(count, float('nan'))
    acc, conf = torch.where(some, hits / safe, nan), torch.where(some, conf_sum / safe, nan)
    gap = torch.where(some, (hits - conf_sum).abs() / safe, torch.zeros_like(count))
    return dict(ece=float((hits - conf_sum).abs().sum()) / valid if valid else float('nan'),
                mce=float(gap.max()) if valid else float('nan'), accuracy=acc, confidence=conf)


def fit_temperature(temperatures, nll):
    """-> (T, at_edge): the temperature that minimises `nll` sampled on the ascending grid `temperatures`.  The grid arg-min (the first
    one on a tie); when it is interior, the vertex of the parabola through it and its two neighbours in log T, clamped to their
    interval; when it is an end of the grid, that grid value with at_edge True — the minimum may lie outside: widen the grid."""
    ts = [float(t) for t in temperatures]
    ys = [float(v) for v in nll]
    if len(ts) != len(ys) or not ts:
        raise ValueError('one NLL per temperature (got %d and %d)' % (len(ts), len(ys)))
    i = min(range(len(ys)), key=ys.__getitem__)
    if i == 0 or i == len(ts) - 1:
        return ts[i], True
    x0, x1, x2 = (math.log(t) for t in ts[i - 1:i + 2])
    y0, y1, y2 = ys[i - 1:i + 2]
    # Newton form y = y0 + d01 (x - x0) + a (x - x0)(x - x1); a > 0 at a strict interior minimum; y' = 0 at (x0 + x1) / 2 - d01 / 2a
    d01, d12 = (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1)
    a = (d12 - d01) / (x2 - x0)
    if not a > 0.0:
        return ts[i], False
    x = 0.5 * (x0 + x1) - 0.5 * d01 / a
    return math.exp(min(max(x, x0), x2)), False


class ExitCalibration(InferenceStep):
    head = 'calib'

    def __init__(self, model, batch_shape, temperatures=TEMPERATURES, ignore_index=255, use_graph=None, nstreams=None):
        self.temperatures = _check_temperatures(temperatures)
        super().__init__(model, batch_shape, use_graph, nstreams)
        # the evaluator counts every label in [0, classes) (utils/metrics.py:34-43); ignore_index is what the loader paints elsewhere
        # and what step() paints over the images a short batch does not have
        self.ignore_index = int(ignore_index)
        self.inv_temp = torch.zeros(len(self.temperatures), dtype=torch.float32, device=self.dev)
        self._write_temperatures()
        self._build()
        self.reset()

    def _write_temperatures(self):
        self.inv_temp.copy_(torch.tensor([1.0 / t for t in self.temperatures], dtype=torch.float32))

    def set_temperatures(self, temperatures):
        """Another grid for the steps that follow.  The same number of temperatures: the words live in a device buffer the plan reads
        when it runs, so nothing is rebuilt or captured again.  The accumulators are emptied: they belong to the old grid."""
        ts = _check_temperatures(temperatures)
        if len(ts) != len(self.temperatures):
            raise ValueError('set_temperatures takes %d temperatures, as the plan was built (got %d)' % (len(self.temperatures), len(ts)))
        self.temperatures = ts
        self._write_temperatures()
        self.reset()

    # ---------------- plan ----------------
    def _emit(self, g, a):
        nt = len(self.temperatures)
        outs, first = self._emit_exits(g, a)
        if 0 <= self.ignore_index < self.ncls:
            raise ValueError('ExitCalibration: ignore_index %d is one of the %d classes the evaluator counts' % (self.ignore_index, self.ncls))
        if first:      # what the launches add to, per exit: [nt, 16, 3] (count, hits, confidence sum / 2^-24) and the NLL sums
            self.bins = torch.zeros((self.nex, nt, L.CALIB_BINS, 3), dtype=torch.int64, device=self.dev)
            self.nll = torch.zeros((self.nex, nt), dtype=torch.float64, device=self.dev)
        for i, o in enumerate(outs):
            o.binding = dict(target=self.target, inv_temp=self.inv_temp, nt=nt, bins=self.bins[i], nll=self.nll[i])
        self.outs = outs

    # ---------------- replay ----------------
    def step(self, images=None, targets=None, count=None):
        """Adds the resident batch (or `images` / `targets` if given) to the accumulators: its first `count` images (default: all N; for a
        short last batch the targets of the others are painted with ignore_index on the device, so they add nothing).  No host
        synchronisation, except once when the third call captures the hipGraph."""
        N = self.batch_shape[0]
        count = N if count is None else int(count)
        if not 0 <= count <= N:
            raise ValueError('count must lie in [0, %d] (got %d)' % (N, count))
        if images is not None:
            self.load_batch(images, targets)
        if count < N:
            self.target[count:].fill_(self.ignore_index)
        self._replay()
        self.batches += 1
        self.images += count

    # ---------------- results ----------------
    def reset(self):
        self.bins.zero_()
        self.nll.zero_()
        self.batches, self.images = 0, 0

    def result(self):
        """The single synchronisation of a pass -> one dict per exit, on the CPU: `temperatures`, `valid` (pixels with a label in
        [0, classes)), `accuracy` (of the arg-max: the same at every temperature), and per temperature `nll` (mean per valid pixel, fp64
        [nt]), `ece` and `mce` ([nt], as reliability()), `bins` (int64 [nt, 16, 2]: count, hits) and `conf_sum` (fp64 [nt, 16])."""
        bins, nll = self.bins.cpu(), self.nll.cpu()
        out = []
        for k in range(self.nex):
            b2, cs = bins[k, :, :, :2].contiguous(), bins[k, :, :, 2].double() * CONF_UNIT
            valid = int(b2[0, :, 0].sum())
            rel = [reliability(b2[j], cs[j]) for j in range(len(self.temperatures))]
            out.append(dict(temperatures=self.temperatures, valid=valid,
                            accuracy=float(b2[0, :, 1].sum()) / valid if valid else float('nan'),
                            nll=nll[k] / valid if valid else torch.full_like(nll[k], float('nan')),
                            ece=torch.tensor([r['ece'] for r in rel], dtype=torch.float64),
                            mce=torch.tensor([r['mce'] for r in rel], dtype=torch.float64), bins=b2, conf_sum=cs))
        return out

    def fit(self, with_edges=False):
        """One temperature per exit of forward() (fit_temperature on result()'s NLL): what the `temperature=` of ExitProfile,
        dynamic_inference and dynamic_inference_batch takes.  with_edges: -> (temperatures, [at_edge per exit])."""
        fits = [fit_temperature(r['temperatures'], r['nll'].tolist()) for r in self.result()]
        ts = [t for t, _ in fits]
        return (ts, [e for _, e in fits]) if with_edges else ts
