"""Gated dynamic inference (reference ADD.dynamic_inference, ADD.py:379-488; eval.py:195-230 `--confidence {edm,entropy,max}`).

The gate stays on the host and only selects which exit's kernels fire (north_star): the trunk is emitted
once into a single launch list that is cut into segments.  All segments share one buffer set.

DynamicPlan ('edm', ADD.py:379-438): [stems+cells up to gate k + EDM] and, per gate, [early head k]; the last segment is
[remaining cells + final head].

GatePlan ('entropy' / 'max', operations.py:161-180; the reference's own branch ADD.py:440-488 is broken, SURVEY Q6, so the
semantics are this project's): the gate judges exit k's PREDICTION, so head k runs before the decision —
[trunk up to exit k] [head k down to the decoder's low-resolution logits + the gate launch] [resize of head k to NCHW] ...
[remaining cells + final head + its resize].  The gate launch (csrc/label_up.hip gate_up_kernel) takes the entropy / top-probability
share of the x8 up-sampled prediction straight from the low-resolution logits and writes them to pinned host words; the full-size
logits are written only for the image that leaves.  Exit k's logits are forward()'s (`model(x)[k]`): aspp_size from 2^-(last+2)
and conv_aspp[k] when the level differs; no EDM runs, so its in-place ReLU (Q3) does not happen.  The 2^-last size (Q5) is a
quirk of the working 'edm' path and stays only there: the heads training optimises are forward()'s.

output='labels' (both plans): every exit ends in a label head instead (plan.Graph.head 'labels', heads.py) and returns the plan-owned uint8 [1,H,W]
arg-max map of its logits; no [N,C,H,W] buffer exists.  'edm': [early head k] and the final head end in one `label_upsample` launch.
'entropy' / 'max': the gate launch leaves the map as well (`gate_label_upsample`), so nothing is left to replay for the image that
leaves — [trunk up to exit k] [head k + the gate-and-labels launch] ... [remaining cells + final head + its `label_upsample`].

What every gated front end shares lives here (BatchedGate below, segment.TiledSegmenter): the gate is read by GatePlan.set_threshold /
gate_values / leaves and by nothing else; gate_thresholds maps a threshold argument to one float per gate; PinnedWords carries a call's
index words and tables to the device; rows_table / gather_rows build and issue an `addk_gather_rows` launch; whole_rows says what it can move."""
import collections
import ctypes as C
import os

import torch

from . import _lib as L
from . import plan as _plan
from .module import ensure_layout
from .heads import label_lut as _label_lut
from .plan import Act, Cmd, Graph, OutRef, env_graph_infer, env_streams

OUTPUTS = ('logits', 'labels')


class DynamicPlan:
    def __init__(self, model, edm, x, output='logits', label_lut=None):
        from .modeling.ADD import _aspp_size
        # the gate scalar travels through pinned host memory: the fused EDM head (csrc/edm.hip) writes it there itself; on the generic path an
        # asynchronous 4-byte copy does.  Either way the host waits on ONE event, not on the whole device (ADD.py:421 does
        # `if confidence_value > threshold`, a blocking read)
        a = self._begin((model, edm), x, output, label_lut, 1)
        g = self.g
        self.conf_fused = []
        size = (a.H, a.W)
        aspp_size = _aspp_size(size, model.network_arch[-1])          # 2^-last
        self.trunk_end, self.head_rng, self.conf, self.heads = [], [], [], []
        gen = model._trunk(g, a)
        send, it = None, 0
        self.final = None
        while True:
            try:
                i, y, low = gen.send(send)
            except StopIteration:
                break
            send = None
            if i in model.C_index or i == model.num_net - 1:
                if i != model.num_net - 1:
                    g.edm_fused = False
                    ca = edm.emit(g, y, host_out=self._conf_host if x.is_cuda else None)
                    self.conf_fused.append(bool(g.edm_fused))
                    if g.edm_fused:                                   # the head wrote [N,1,1,1] itself (and the pinned word): no layout launch
                        conf = OutRef(ca.raw.view().permute(0, 3, 1, 2))
                    else:
                        conf = g.output_nchw(ca)                      # EDM applies ReLU to y in place (Q3) ...
                    y = Act(y.raw, y.bn, True, False, rs=y.rs)              # ... so everything downstream sees relu(y)
                    send = y
                    self.trunk_end.append(len(g.fwd))
                    self.conf.append(conf)
                    h0 = len(g.fwd)
                    self.heads.append(model._head(g, y, low, size, aspp_size, it, model.network_arch[i]))
                    self.head_rng.append((h0, len(g.fwd)))
                    it += 1                                           # ADD.py:422 increments on every passed gate
                else:
                    self.final = model._head(g, y, low, size, aspp_size, it, model.network_arch[i], resize=False, adapt=False)
        self._finish(x)

    def _begin(self, modules, x, output, label_lut, words, batched=False):
        """What both plans start with: the checks, the inference Graph with its label mode, `words` pinned host words the gate value
        travels through and the event the host waits on, and the input -> its activation.  `batched`: a sub-plan of BatchedGate, the
        one caller that decides per image; `words` then covers every image of the batch."""
        if output not in OUTPUTS:
            raise ValueError('output must be one of %s (got %r)' % (OUTPUTS, output))
        lut = _label_lut(label_lut, x.device)
        for m in modules:
            for p in m.parameters():
                ensure_layout(p)
        if x.shape[0] != 1 and not batched:
            # ADD.py:421 `if confidence_value > threshold` on a [bs, 1] tensor raises for bs > 1 ("Boolean value of Tensor with more
            # than one value is ambiguous"): the gate is a per-image decision (eval.py:195-230 runs bs = 1); same error class here
            raise RuntimeError('dynamic_inference gates one image at a time (got batch size %d): the reference\'s '
                               '`if confidence_value > threshold` is ambiguous for more than one value' % x.shape[0])
        self.g = g = Graph(x.device, False, False, None)
        if output == 'labels':
            g.head, g.lut = 'labels', lut
        self._conf_host = host_words(words, torch.float32, x.device)
        # (dry-run planning on CPU in tests/test_plan_dryrun.py builds plans without a device)
        self._conf_evt = torch.cuda.Event() if x.is_cuda else None
        a, self.inref = g.input_nchw(x)
        self.in_name = a.raw.buf.region[0]             # the input staging buffer: what depends on the image is reachable from it
        return a

    def _finish(self, x):
        g = self.g
        g.finalize()
        self.params = list(g.params)
        self.ptrs = [p.data_ptr() for p in self.params]
        self.x_static = torch.empty_like(x, dtype=torch.float32, memory_format=torch.contiguous_format)
        self.inref.bind(self.x_static)
        self.graphs = {}          # (begin, end) -> hipGraph of that launch-list segment
        self.segs = {}            # (begin, end) -> that segment's launch list, level-ordered / batched / scheduled on two streams
        g.nstreams = env_streams()
        self.calls = 0

    def check_params(self):
        return all(p.data_ptr() == q for p, q in zip(self.params, self.ptrs))

    def _seg(self, i0, i1):
        """Run launch-list segment [i0, i1): eagerly the first two calls, then as a captured hipGraph (each segment —
        trunk up to a gate, an exit head, the remainder — is its own graph; the host gate picks which ones replay)."""
        g = self.g
        if i1 < 0:
            i1 = len(g.fwd)
        cmds = self.segs.get((i0, i1))
        if cmds is None:          # every command belongs to exactly one segment: re-order and schedule the slice on its own
            cmds = list(g.fwd[i0:i1])
            if os.environ.get('ADDK_LEVEL_BATCH', '1') == '1':
                g.level_batch(cmds)
            g.place(cmds)
            self.segs[(i0, i1)] = cmds
        if self.calls < 3 or not env_graph_infer():
            g.run_parallel(cmds, None)
            return
        gr = self.graphs.get((i0, i1))
        if gr is None:
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                g.run_parallel(cmds, None)
            self.graphs[(i0, i1)] = gr
        gr.replay()

    def run(self, x, threshold):
        self.calls += 1
        self.x_static.copy_(x)
        pos, conf = 0, None
        with torch.no_grad():
            for k, end in enumerate(self.trunk_end):
                self._seg(pos, end)
                conf = self.conf[k].y.reshape(x.shape[0], -1)
                assert conf.numel() == 1
                h0, h1 = self.head_rng[k]
                if not self.conf_fused[k]:
                    self._conf_host[:1].copy_(conf.reshape(-1), non_blocking=True)
                if self._conf_evt is not None:
                    self._conf_evt.record()
                    self._conf_evt.synchronize()                      # the host waits for this one scalar only
                if bool(self._conf_host[0] > threshold):              # the gate (ADD.py:421); bs = 1 as in eval.py:195-230
                    pos = h1
                    continue
                self._seg(h0, h1)
                return self.heads[k].y, 1, conf
            self._seg(pos, -1)
        return self.final.y, 0, conf


KINDS = ('entropy', 'max')


def host_words(shape, dtype, device):
    """zeroed host words that `device` copies from or writes to: pinned when it is a GPU, plain memory in a dry run"""
    t = torch.zeros(shape, dtype=dtype)
    return t.pin_memory() if device.type == 'cuda' else t


class PinnedWords:
    """Host words [slots, ...] (host_words), their device copy and one event per slot: what a call's index words and tables travel
    through.  put(slot, *rows) waits for the slot's previous copy — that one copy, not the device —, writes the rows, copies the slot
    without blocking and records.  Which slot to take is the caller's business; on the CPU there is nothing to pin or to wait for."""

    def __init__(self, shape, dtype, device):
        self.host = host_words(shape, dtype, device)
        self.dev = torch.zeros(shape, dtype=dtype, device=device)
        self.evt = [torch.cuda.Event() for _ in range(shape[0])] if device.type == 'cuda' else None

    def put(self, slot, *rows):
        """row r of the slot begins with rows[r] (a list or a tensor; what lies behind it stays) -> the slot's device words"""
        if self.evt:
            self.evt[slot].synchronize()               # the previous copy out of these pinned words has been made
        for r, vals in enumerate(rows):
            if len(vals):
                self.host[slot, r, :len(vals)] = torch.as_tensor(vals, dtype=self.host.dtype)
        self.dev[slot].copy_(self.host[slot], non_blocking=True)
        if self.evt:
            self.evt[slot].record()
        return self.dev[slot]


def rows_table(g, triples):
    """(src, dst, bytes per row) of every buffer an `addk_gather_rows` launch moves -> (its item table on the device of plan `g`, kept
    alive with the plan; the number of items)"""
    arr = (L.RowsItem * len(triples))()
    for it, (src, dst, nbytes) in zip(arr, triples):
        it.src, it.dst, it.row_bytes = src, dst, nbytes
    return g._table(bytes(arr)), len(triples)


def gather_rows(g, table, src_row, dst_row, nrows):
    """one addk_gather_rows launch on the current stream, through the plan's launch loop: row src_row[i] of every item's source -> row
    dst_row[i] of its destination (device int32 words; None: row i)"""
    a = L.GatherRowsArgs()
    a.items, a.nitems, a.nrows = table[0].data_ptr(), table[1], nrows
    a.src_row = None if src_row is None else src_row.data_ptr()
    a.dst_row = None if dst_row is None else dst_row.data_ptr()
    g.run([Cmd('gather_rows', g.lib.addk_gather_rows, (C.byref(a),))], _plan.current_stream())


def whole_rows(buf, batch):
    """is plan buffer `buf` one whole NHWC tensor of `batch` images — what gather_rows can move image by image"""
    return buf.geom is not None and buf.geom[0] == batch and buf.n == batch * buf.geom[1] * buf.geom[2] * buf.geom[3]


def finite_threshold(thr):
    """a finite word for the kernel: every top probability lies in (0, 1], so clamping an infinite threshold changes no comparison"""
    return min(max(thr, -1.0), 2.0)


def gate_thresholds(threshold, gates):
    """a number, or one number per gate -> one float per gate"""
    try:
        return [float(threshold)] * gates
    except TypeError:
        pass
    thr = [float(v) for v in threshold]
    if len(thr) != gates:
        raise ValueError('one threshold per gate: %d gates, %d thresholds' % (gates, len(thr)))
    return thr


def check_temperature(temperature, nex):
    """`temperature` of a tempered gate or profile -> None, or one positive finite float per exit of forward() (`nex` of them: what
    calibrate.ExitCalibration.fit() returns).  A scalar serves every exit; anything else is a ValueError."""
    if temperature is None:
        return None
    try:
        ts = [float(temperature)] * nex
    except TypeError:
        ts = [float(t) for t in temperature]
        if len(ts) != nex:
            raise ValueError('temperature takes a scalar or one number per exit: %d exits, %d temperatures' % (nex, len(ts)))
    if any(not (0.0 < t < float('inf')) for t in ts):
        raise ValueError('a temperature must be positive and finite (got %r)' % (ts,))
    return tuple(ts)


def inverse_words(ts):
    """the fp32 words 1 / T the tempered launches read"""
    return torch.tensor([1.0 / t for t in ts], dtype=torch.float32)


class GatePlan(DynamicPlan):
    """Dynamic inference gated by the entropy ('entropy') or the top-probability share ('max') of each early exit's prediction.
    `temperature` (None, a scalar or one per exit of forward(): check_temperature): the gates judge softmax(z_k / T_k) — the tempered
    plan, whose gate launches read 1 / T_k from device words (set_temperature: no rebuild, no recapture); exit k's logits and label
    map are what they are without it."""

    def __init__(self, model, x, kind, output='logits', label_lut=None, batched=False, temperature=None, head=None, gate_extra=None):
        """`head` / `gate_extra` (segment.TileGatePlan): another logits head than `output` names (a key of heads.HEADS) and further
        entries of the gate's dict, for a head that emits its own gate launch."""
        from .modeling.ADD import _aspp_size
        if kind not in KINDS:
            raise ValueError('confidence must be one of %s (got %r)' % (('edm',) + KINDS, kind))
        self.kind = kind
        self.image_dep, self._live = None, {}
        # (entropy, share) of the gated exit travel through pinned host memory: the gate launch writes them there itself; on the
        # stand-alone path an asynchronous 8-byte copy does.  Either way the host waits on ONE event, not on the whole device
        # (`batched`, a sub-plan of BatchedGate: the pair of every image of the batch)
        a = self._begin((model,), x, output, label_lut, 2 * x.shape[0] if batched else 2, batched)
        g = self.g
        if head is not None:
            g.head = head
        self._thr = torch.zeros(1, dtype=torch.float32, device=x.device)      # the word the 'max' gate compares against
        self._thr_word = 0.0                                                  # ... and what it holds
        self.nex = model.num_exits()
        self.temperature, self._temp = None, None
        if temperature is not None:
            check_temperature(temperature, self.nex)
            self._temp = torch.ones(max(self.nex - 1, 1), dtype=torch.float32, device=x.device)      # 1 / T of every gate
        size = (a.H, a.W)
        aspp_size = _aspp_size(size, model.network_arch[-1] + 2)       # forward()'s (ADD.emit)
        self.trunk_end, self.head_rng, self.heads, self.final = [], [], [], None
        for i, y, low, it, lvl in model._exits(g, a):
            if i == model.num_net - 1:
                self.final = model._head(g, y, low, size, aspp_size, it, lvl)
            else:
                self.trunk_end.append(len(g.fwd))
                g.gate = dict(gate_extra or {}, kind=kind, host=self._conf_host if x.is_cuda else None, thr=self._thr)
                if self._temp is not None:
                    g.gate['temp'] = self._temp[len(self.heads):len(self.heads) + 1]
                h = model._head(g, y, low, size, aspp_size, it, lvl)
                g.gate = None
                self.heads.append(h)
                self.head_rng.append((h.gate_cut, len(g.fwd)))          # [trunk_end, gate_cut): head + gate; [gate_cut, end): resize (labels: empty)
        self._finish(x)
        if temperature is not None:
            self.set_temperature(temperature)

    def set_temperature(self, temperature):
        """Other temperatures for the calls that follow (a tempered plan only).  The gates use the first num_exits() - 1 values; the words
        are written only when the values change."""
        if self._temp is None or temperature is None:
            raise ValueError('this plan was built %s a temperature: the other kind is another plan' % ('without' if self._temp is None else 'with'))
        ts = check_temperature(temperature, self.nex)
        if ts != self.temperature:
            if self.nex > 1:
                self._temp.copy_(inverse_words(ts[:self.nex - 1]))
            self.temperature = ts

    def set_threshold(self, thr):
        """The threshold of the gate launches that follow, as the finite word they read; written only when it changes."""
        word = finite_threshold(thr)
        if word != self._thr_word:
            self._thr.fill_(word)
            self._thr_word = word

    def gate_values(self, k, n=1):
        """The gate values of exit k for rows 0 .. n-1 as Python floats, once the launches issued so far have run: the host waits on
        ONE event for the 2n pinned words (entropy, share) per row — the gate launch wrote them itself, or an asynchronous copy of
        `gate_out` does.  The words are fp32 widened exactly to double, and the fused heads leave gate_scale == 1.0, so a value is bit for
        bit the word the device wrote; only the stand-alone entropy kernel leaves a sum for the host to scale."""
        h = self.heads[k]
        if not h.gate_fused:
            self._conf_host[:2 * n].copy_(h.gate_out.reshape(-1)[:2 * n], non_blocking=True)
        if self._conf_evt is not None:
            self._conf_evt.record()
            self._conf_evt.synchronize()
        words = self._conf_host[:2 * n].tolist()
        return [w * h.gate_scale for w in words[0::2]] if self.kind == 'entropy' else words[1::2]

    def leaves(self, value, thr):
        """the rule: entropy BELOW the threshold, or the share of pixels with top probability above the threshold ABOVE it"""
        return value < thr if self.kind == 'entropy' else value > thr

    def taint(self):
        """`image_dep`: which launches depend on the image — those that (transitively, in list order) read something written from the
        staging buffer.  Nothing here is a hand-kept list of activations: everything is read off the launch list's named regions
        (sched.Cmd.rd / wr)."""
        tainted, self.image_dep = set(), []
        for c in self.g.fwd:
            dep = self.in_name in _names(c.wr) or bool(_names(c.rd) & tainted)
            if dep:
                tainted |= _names(c.wr)
            self.image_dep.append(dep)

    def live(self, pos):
        """The state a run that continues at launch `pos` needs from fwd[:pos] -> (per-image plan buffers in order of first write,
        the input-independent launches of fwd[:pos] to replay, in list order).  Live = plan buffers written by fwd[:pos] and read by
        fwd[pos:].  Per-image = written by a launch that depends on the image; the rest (the eval-BN affine table, the hoisted weight
        packs, anything computed from parameters only) is recomputed by replaying its producers, never copied.  On that side a buffer
        that fwd[pos:] names as WRITTEN counts as read as well: a conv lists its hoisted weight pack under `wr` (without the hoist it
        packs the weights itself) and reads what `conv_pack_batch` left there."""
        got = self._live.get(pos)
        if got is not None:
            return got
        if self.image_dep is None:
            self.taint()
        fwd = self.g.fwd
        later, touched = set(), set()
        for c in fwd[pos:]:
            later |= _names(c.rd)
            touched |= _names(c.wr)
        first, per_image = {}, set()
        for i, c in enumerate(fwd[:pos]):
            for j, r in enumerate(c.wr):
                if r[0][0] == 'buf':
                    first.setdefault(r[0], (i, j))
                    if self.image_dep[i]:
                        per_image.add(r[0])
        bufs = [self.g._bufs[n[1]] for n in sorted(first, key=first.get) if n in later and n in per_image]
        needed, replay = (later | touched) - per_image, []
        for i in range(pos - 1, -1, -1):
            c = fwd[i]
            if not self.image_dep[i] and _names(c.wr) & needed:
                replay.append(c)
                needed |= _names(c.rd)
        replay.reverse()
        self._live[pos] = bufs, replay
        return bufs, replay

    def run(self, x, threshold):
        """-> (logits or label map, earlier_exit, gate value).  The image leaves at the first exit whose entropy is BELOW the threshold
        ('entropy'), or whose share of pixels with top probability above the threshold is ABOVE it ('max': the same number plays
        both roles, ADD.py:476,481)."""
        self.calls += 1
        self.x_static.copy_(x)
        thr = float(threshold)
        self.set_threshold(thr)
        pos, value = 0, None
        with torch.no_grad():
            for k, (cut, hend) in enumerate(self.head_rng):
                self._seg(pos, cut)
                value = self.gate_values(k)[0]
                if self.leaves(value, thr):
                    if hend > cut:
                        self._seg(cut, hend)
                    return self.heads[k].y, 1, value
                pos = hend
            self._seg(pos, -1)
        return self.final.y, 0, value


# ------------------------------------------------------------------------------------------------------------------------
# batched gating: per-image exits with batch compaction
# ------------------------------------------------------------------------------------------------------------------------
def _names(regions, kind=None):
    return {r[0] for r in regions if kind is None or r[0][0] == kind}


class _SubPlan(GatePlan):
    """The gate plan (label heads) at one live batch size of a BatchedGate; what it hands over at a cut is GatePlan.live."""

    def __init__(self, model, x, kind, label_lut, temperature=None):
        super().__init__(model, x, kind, 'labels', label_lut, batched=True, temperature=temperature)
        self.batch = int(x.shape[0])
        self.taint()


def pair_live(pm, pn, k):
    """The per-image live buffers of sub-plans `pm` and `pn` behind gate k, paired in order of first write -> [(Buf of pm, Buf of pn,
    words per image)].  Refuses what it cannot move row by row: a buffer that is not one whole NHWC tensor of its plan's batch, another
    count, another per-image geometry (H, W, ld)."""
    a, b = pm.live(pm.head_rng[k][1])[0], pn.live(pn.head_rng[k][1])[0]
    if len(a) != len(b):
        raise L.AddkError('gate %d: the plans of batch %d and %d keep %d and %d per-image buffers alive' % (k, pm.batch, pn.batch, len(a), len(b)))
    pairs = []
    for x, y in zip(a, b):
        for p, buf in ((pm, x), (pn, y)):
            if not whole_rows(buf, p.batch):
                raise L.AddkError('gate %d: live buffer %r of the batch-%d plan is not one whole NHWC tensor of its batch' % (k, buf.region[0], p.batch))
        if x.geom[1:] != y.geom[1:]:
            raise L.AddkError('gate %d: live buffers %r / %r differ per image: (H, W, ld) %r and %r' % (k, x.region[0], y.region[0], x.geom[1:], y.geom[1:]))
        pairs.append((x, y, x.geom[1] * x.geom[2] * x.geom[3]))
    return pairs


class BatchedGate:
    """Gated dynamic inference of a batch: every image takes GatePlan's decision on its own, and the images that left stop costing
    anything.

        bg = BatchedGate(model, (N, 3, H, W), confidence='entropy' | 'max', label_lut=None)
        labels, exits, values = bg.run(images, threshold)

    One sub-plan per live batch size n in 1..N — a gate plan with label heads emitted at batch n, built on first use and kept — replayed
    segment by segment through DynamicPlan._seg.  Plan N runs up to the first gate; the host reads the 2n pinned words, one
    `addk_gather_rows` launch scatters the leavers' rows of that exit's label map to their original indices, and when 0 < n' < n images
    stay, ONE more moves the per-image live state (_SubPlan.live, pair_live) into plan n', which continues behind the same gate; its
    input-independent tables are recomputed there by replaying their launches.  With n' = n the same plan goes on and nothing is copied.

    `threshold`: a number, or one number per gate.  -> labels: uint8 [N,H,W], owned by this object and overwritten by the next call
    (the class index, or label_lut[class]); exits: int64 [N] on the host, the index into forward()'s outputs each image left at;
    values: float32 [N, gates] on the host, NaN where a gate was not evaluated for that image.  Surviving images keep their order.
    `temperature`: GatePlan's, for every sub-plan; set_temperature changes the values of a tempered BatchedGate."""

    def __init__(self, model, batch_shape, confidence='entropy', label_lut=None, temperature=None):
        if confidence == 'edm':
            raise ValueError("BatchedGate gates by 'entropy' or 'max': the 'edm' gate stays with the single-image path")
        if confidence not in KINDS:
            raise ValueError('confidence must be one of %s (got %r)' % (KINDS, confidence))
        shape = tuple(int(v) for v in batch_shape)
        if len(shape) != 4 or shape[0] < 1:
            raise ValueError('batch_shape must be (N >= 1, 3, H, W) (got %r)' % (batch_shape,))
        self.model, self.kind, self.shape, self.N = model, confidence, shape, shape[0]
        self.device = next(model.parameters()).device
        self.lut = _label_lut(label_lut, self.device)
        self.gates = model.num_exits() - 1
        self.temperature = check_temperature(temperature, self.gates + 1)
        self.subs = {}                 # live batch size -> _SubPlan
        self.tables = {}               # ('state', m, n, k) / ('labels', n, k) -> (device item table, items, pairs)
        self.labels = torch.zeros((self.N,) + shape[2:], dtype=torch.uint8, device=self.device)
        # index words: per gate (and once more for the final head) a slot of three rows — the leavers' rows in the plan, their original
        # indices, the stayers' rows in the plan; a row that is not given keeps what it held
        self._idx = PinnedWords((self.gates + 1, 3, self.N), torch.int32, self.device)
        self.counts = collections.Counter()    # 'state' / 'labels' gather_rows launches, ('seg', n) segments run per sub-plan; all calls
        self.trace = []                # last call: (live batch, begin, end) of every segment run
        self.moves = []                # last call: (batch before, batch after, gate, rows that stayed)
        self.calls = 0

    # ---- sub-plans -------------------------------------------------------------------------------------------------------
    def sub(self, n):
        p = self.subs.get(n)
        if p is None:
            x = torch.empty((n,) + self.shape[1:], dtype=torch.float32, device=self.device)
            p = self.subs[n] = _SubPlan(self.model, x, self.kind, self.lut, self.temperature)
            assert len(p.trunk_end) == self.gates
        return p

    def set_temperature(self, temperature):
        if self.temperature is None or temperature is None:
            raise ValueError('this BatchedGate was built %s a temperature: the other kind is another plan' % ('without' if self.temperature is None else 'with'))
        ts = check_temperature(temperature, self.gates + 1)
        self.temperature = ts
        for p in self.subs.values():
            p.set_temperature(ts)

    def check_params(self):
        return all(p.check_params() for p in self.subs.values())

    @property
    def nbytes(self):
        """device bytes: {live batch size: its sub-plan's} and 'total' (the sub-plans built so far, the output map, the index words)"""
        per = {n: int(p.g.nbytes) for n, p in sorted(self.subs.items())}
        per['total'] = sum(per.values()) + self.labels.numel() + 4 * self._idx.dev.numel()
        return per

    def close(self):
        """Wait for the device, then drop every captured graph and every sub-plan."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize()
        for p in self.subs.values():
            p.graphs.clear()
            p.segs.clear()
        self.subs.clear()
        self.tables.clear()

    # ---- launches --------------------------------------------------------------------------------------------------------
    def _seg(self, plan, i0, i1):
        self.trace.append((plan.batch, i0, len(plan.g.fwd) if i1 < 0 else i1))
        self.counts[('seg', plan.batch)] += 1
        plan._seg(i0, i1)

    def _gather(self, what, plan, table, src_row, dst_row, nrows):
        self.counts[what] += 1
        gather_rows(plan.g, table, src_row, dst_row, nrows)

    def _scatter(self, plan, k, y, src_row, dst_row, nrows):
        """rows of exit k's label map of `plan` -> the output map, at the images' original indices"""
        H, W = self.shape[2:]
        key = ('labels', plan.batch, k)
        if key not in self.tables:
            self.tables[key] = rows_table(plan.g, [(y.data_ptr(), self.labels.data_ptr(), H * W)])
        self._gather('labels', plan, self.tables[key], src_row, dst_row, nrows)

    def _move(self, pm, pn, k, stay, src_row):
        """the live state behind gate k: rows `stay` of plan pm -> rows 0.. of plan pn"""
        key = ('state', pm.batch, pn.batch, k)
        if key not in self.tables:
            pairs = pair_live(pm, pn, k)
            self.tables[key] = rows_table(pn.g, [(x.ptr, y.ptr, 4 * words) for x, y, words in pairs]) + (pairs,)
        replay = pn.live(pn.head_rng[k][1])[1]
        if replay:
            pn.g.run(replay, _plan.current_stream())
        self._gather('state', pn, self.tables[key], src_row, None, len(stay))
        self.moves.append((pm.batch, pn.batch, k, list(stay)))

    def transition_pairs(self):
        """For tests: per live buffer of every transition of the last call, (the rows taken from the larger plan, the rows of the
        smaller plan) as [n', words] views of the plan buffers."""
        out = []
        for m, n, k, stay in self.moves:
            for x, y, words in self.tables[('state', m, n, k)][2]:
                out.append((x.t[:m * words].view(m, words)[stay], y.t[:n * words].view(n, words)))
        return out

    # ---- one call --------------------------------------------------------------------------------------------------------
    def run(self, images, threshold):
        thr = gate_thresholds(threshold, self.gates)
        if tuple(images.shape) != self.shape:
            raise ValueError('this BatchedGate was built for %r (got %r)' % (self.shape, tuple(images.shape)))
        N, G = self.N, self.gates
        exits = torch.full((N,), G, dtype=torch.int64)
        values = torch.full((N, G), float('nan'), dtype=torch.float32)
        self.calls += 1
        self.trace, self.moves = [], []
        plan = self.sub(N)
        plan.calls += 1
        plan.x_static.copy_(images)
        idx, pos = list(range(N)), 0            # original index of every live row; where the live plan continues
        with torch.no_grad():
            for k in range(G):
                cut, hend = plan.head_rng[k]
                plan.set_threshold(thr[k])
                self._seg(plan, pos, cut)
                n = len(idx)
                vals = plan.gate_values(k, n)
                leave = [i for i in range(n) if plan.leaves(vals[i], thr[k])]
                stay = [i for i in range(n) if i not in leave]
                for i in range(n):
                    values[idx[i], k] = vals[i]
                if leave:
                    if hend > cut:
                        self._seg(plan, cut, hend)
                    d = self._idx.put(k, leave, [idx[i] for i in leave], stay)
                    self._scatter(plan, k, plan.heads[k].y, d[0], d[1], len(leave))
                    for i in leave:
                        exits[idx[i]] = k
                    if not stay:
                        return self.labels, exits, values
                    nxt = self.sub(len(stay))
                    nxt.calls += 1
                    self._move(plan, nxt, k, stay, d[2])
                    plan = nxt
                    idx = [idx[i] for i in stay]
                pos = plan.head_rng[k][1]
            self._seg(plan, pos, -1)
            d = self._idx.put(G, [], idx, [])
            self._scatter(plan, G, plan.final.y, None, d[1], len(idx))
        return self.labels, exits, values
