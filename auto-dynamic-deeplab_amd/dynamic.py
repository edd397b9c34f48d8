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

output='labels' (both plans): every exit ends in a label head instead (plan.Graph.head 'labels') and returns the plan-owned uint8 [1,H,W]
arg-max map of its logits; no [N,C,H,W] buffer exists.  'edm': [early head k] and the final head end in one `label_upsample` launch.
'entropy' / 'max': the gate launch leaves the map as well (`gate_label_upsample`), so nothing is left to replay for the image that
leaves — [trunk up to exit k] [head k + the gate-and-labels launch] ... [remaining cells + final head + its `label_upsample`]."""
import os

import torch

from .module import ensure_layout
from .plan import Act, Graph, OutRef, env_graph_infer, env_streams, label_lut as _label_lut

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

    def _begin(self, modules, x, output, label_lut, words):
        """What both plans start with: the checks, the inference Graph with its label mode, `words` pinned host words the gate value
        travels through and the event the host waits on, and the input -> its activation."""
        if output not in OUTPUTS:
            raise ValueError('output must be one of %s (got %r)' % (OUTPUTS, output))
        lut = _label_lut(label_lut, x.device)
        for m in modules:
            for p in m.parameters():
                ensure_layout(p)
        if x.shape[0] != 1:
            # ADD.py:421 `if confidence_value > threshold` on a [bs, 1] tensor raises for bs > 1 ("Boolean value of Tensor with more
            # than one value is ambiguous"): the gate is a per-image decision (eval.py:195-230 runs bs = 1); same error class here
            raise RuntimeError('dynamic_inference gates one image at a time (got batch size %d): the reference\'s '
                               '`if confidence_value > threshold` is ambiguous for more than one value' % x.shape[0])
        self.g = g = Graph(x.device, False, False, None)
        if output == 'labels':
            g.head, g.lut = 'labels', lut
        self._conf_host = torch.zeros(words, dtype=torch.float32)
        self._conf_evt = None
        if x.is_cuda:                                   # (dry-run planning on CPU in tests/test_plan_dryrun.py builds plans without a device)
            self._conf_host = self._conf_host.pin_memory()
            self._conf_evt = torch.cuda.Event()
        a, self.inref = g.input_nchw(x)
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


class GatePlan(DynamicPlan):
    """Dynamic inference gated by the entropy ('entropy') or the top-probability share ('max') of each early exit's prediction."""

    def __init__(self, model, x, kind, output='logits', label_lut=None):
        from .modeling.ADD import _aspp_size
        if kind not in KINDS:
            raise ValueError('confidence must be one of %s (got %r)' % (('edm',) + KINDS, kind))
        self.kind = kind
        # (entropy, share) of the gated exit travel through pinned host memory: the gate launch writes them there itself; on the
        # stand-alone path an asynchronous 8-byte copy does.  Either way the host waits on ONE event, not on the whole device
        a = self._begin((model,), x, output, label_lut, 2)
        g = self.g
        self._thr = torch.zeros(1, dtype=torch.float32, device=x.device)      # the word the 'max' gate compares against
        size = (a.H, a.W)
        aspp_size = _aspp_size(size, model.network_arch[-1] + 2)       # forward()'s (ADD.emit)
        self.trunk_end, self.head_rng, self.heads, self.final = [], [], [], None
        for i, y, low, it, lvl in model._exits(g, a):
            if i == model.num_net - 1:
                self.final = model._head(g, y, low, size, aspp_size, it, lvl)
            else:
                self.trunk_end.append(len(g.fwd))
                g.gate = {'kind': kind, 'host': self._conf_host if x.is_cuda else None, 'thr': self._thr}
                h = model._head(g, y, low, size, aspp_size, it, lvl)
                g.gate = None
                self.heads.append(h)
                self.head_rng.append((h.gate_cut, len(g.fwd)))          # [trunk_end, gate_cut): head + gate; [gate_cut, end): resize (labels: empty)
        self._finish(x)

    def run(self, x, threshold):
        """-> (logits or label map, earlier_exit, gate value).  The image leaves at the first exit whose entropy is BELOW the threshold
        ('entropy'), or whose share of pixels with top probability above the threshold is ABOVE it ('max': the same number plays
        both roles, ADD.py:476,481)."""
        self.calls += 1
        self.x_static.copy_(x)
        thr = float(threshold)
        # a finite word for the kernel: every top probability lies in (0, 1], so clamping an infinite threshold changes no comparison
        self._thr.fill_(min(max(thr, -1.0), 2.0))
        pos, value = 0, None
        col = 0 if self.kind == 'entropy' else 1
        with torch.no_grad():
            for k, end in enumerate(self.trunk_end):
                h = self.heads[k]
                cut, hend = self.head_rng[k]
                self._seg(pos, cut)
                if not h.gate_fused:
                    self._conf_host.copy_(h.gate_out.reshape(-1)[:2], non_blocking=True)
                if self._conf_evt is not None:
                    self._conf_evt.record()
                    self._conf_evt.synchronize()                      # the host waits for these two words only
                value = float(self._conf_host[col]) * (h.gate_scale if col == 0 else 1.0)
                if (value < thr) if self.kind == 'entropy' else (value > thr):
                    if hend > cut:
                        self._seg(cut, hend)
                    return h.y, 1, value
                pos = hend
            self._seg(pos, -1)
        return self.final.y, 0, value
