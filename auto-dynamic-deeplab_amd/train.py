"""Fused training step of the path (reference train.py:216-242): forward of all exits, CrossEntropyLoss per exit
averaged over exits, backward, SGD(momentum, weight_decay, nesterov) — emitted as ONE static plan over flat
parameter/gradient buffers and replayed as a single hipGraph launch (eager launch list when RCCL collectives
sit inside the step)."""
import ctypes as C
import math
import os

import torch

from . import _lib as L
from . import module as _module
from . import plan as _plan
from .module import ensure_layout
from .plan import Graph, NbtCounter


def _flat_views(params, device):
    """Re-point every parameter into one flat fp32 buffer (16-byte aligned slots, strides preserved) and build
    matching views into a flat gradient buffer."""
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 3) // 4 * 4
    flat_p = torch.zeros(total, dtype=torch.float32, device=device)
    flat_g = torch.zeros(total, dtype=torch.float32, device=device)
    gviews = {}
    for p, o in zip(params, offs):
        pv = torch.as_strided(flat_p, p.shape, p.stride(), o)
        with torch.no_grad():
            pv.copy_(p.data)
        p.data = pv
        gviews[p] = torch.as_strided(flat_g, p.shape, p.stride(), o)
    return flat_p, flat_g, gviews


def _check_ohem(ohem, N):
    """(thresh, min_kept per image) -> (thresh, min_kept * N), or None; ValueError for what the library would refuse."""
    if ohem is None:
        return None
    if os.environ.get('ADDK_FUSE_CE', '1') != '1':
        raise ValueError('ohem needs the fused loss head (ADDK_FUSE_CE=1): there is no form over full-resolution logits')
    try:
        thresh, min_kept = ohem
        thresh, min_kept = float(thresh), int(min_kept)
    except (TypeError, ValueError):
        raise ValueError('ohem must be (thresh, min_kept), got %r' % (ohem,))
    if not (0.0 < thresh <= 1.0) or min_kept < 1 or min_kept != ohem[1]:
        raise ValueError('ohem: thresh must lie in (0, 1] and min_kept must be a positive integer, got %r' % (ohem,))
    return thresh, min_kept * N


def _check_distill(distill):
    """(alpha, temperature) -> two positive finite floats, or None; ValueError for what the library would refuse."""
    if distill is None:
        return None
    if os.environ.get('ADDK_FUSE_CE', '1') != '1':
        raise ValueError('distill needs the fused loss head (ADDK_FUSE_CE=1): there is no form over full-resolution logits')
    try:
        alpha, temp = distill
        alpha, temp = float(alpha), float(temp)
    except (TypeError, ValueError):
        raise ValueError('distill must be (alpha, temperature), got %r' % (distill,))
    a32, t32 = C.c_float(alpha).value, C.c_float(temp).value          # the words the library receives
    if not (math.isfinite(a32) and math.isfinite(t32) and a32 > 0.0 and t32 > 0.0):
        raise ValueError('distill: alpha and temperature must be positive and finite, got %r' % (distill,))
    return alpha, temp


def _check_dice(dice):
    """(weight, smooth) -> a positive and a non-negative finite float, or None; ValueError for what the library would refuse."""
    if dice is None:
        return None
    if os.environ.get('ADDK_FUSE_CE', '1') != '1':
        raise ValueError('dice needs the fused loss head (ADDK_FUSE_CE=1): there is no form over full-resolution logits')
    try:
        weight, smooth = dice
        weight, smooth = float(weight), float(smooth)
    except (TypeError, ValueError):
        raise ValueError('dice must be (weight, smooth), got %r' % (dice,))
    w32, s32 = C.c_float(weight).value, C.c_float(smooth).value       # the words the library receives
    if not (math.isfinite(w32) and math.isfinite(s32) and w32 > 0.0 and s32 >= 0.0):
        raise ValueError('dice: weight must be positive, smooth non-negative, both finite, got %r' % (dice,))
    return weight, smooth


def _check_shape(focal, label_smoothing, distill):
    """(gamma, eps), at most one of them not None: a finite gamma >= 1 or an eps in (0, 1); ValueError for what the library would refuse."""
    if focal is None and label_smoothing is None:
        return None, None
    name = 'focal' if focal is not None else 'label_smoothing'
    if focal is not None and label_smoothing is not None:
        raise ValueError('focal and label_smoothing are two shapes of the same per-pixel loss: give one of them')
    if distill is not None:
        raise ValueError('%s: the fused loss head has no focal or label-smoothed form with distill (smoothed targets are known to hurt '
                         'distillation, and the distillation head has no registers left for a shape)' % name)
    if os.environ.get('ADDK_FUSE_CE', '1') != '1':
        raise ValueError('%s needs the fused loss head (ADDK_FUSE_CE=1): there is no form over full-resolution logits' % name)
    try:
        v = float(focal if focal is not None else label_smoothing)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number, got %r' % (name, focal if focal is not None else label_smoothing))
    v32 = C.c_float(v).value                                           # the word the library receives
    if focal is not None:
        if not (math.isfinite(v32) and v32 >= 1.0):
            raise ValueError('focal: gamma must be finite and at least 1, got %r' % (focal,))
        return v, None
    if not (0.0 < v32 < 1.0):
        raise ValueError('label_smoothing: eps must lie in (0, 1), got %r' % (label_smoothing,))
    return None, v


class TrainStep:
    def __init__(self, model, batch_shape, lr=0.05, momentum=0.9, weight_decay=4e-5, nesterov=True, class_weight=None,
                 ignore_index=255, use_graph=None, sync_comm=None, nstreams=None, ohem=None, distill=None, dice=None,
                 focal=None, label_smoothing=None):
        """ohem = (thresh, min_kept): online hard example mining in every exit's loss head (include/addk.h, addk_ohem_select) — per exit
        and per process, a pixel counts when its target-class probability is below `thresh`, and never fewer than `min_kept` pixels per
        image (min_kept * N of the batch) count.  Only the fused loss head has this form: ValueError otherwise.
        distill = (alpha, temperature): self-distillation from the final exit (include/addk.h, addk_ce_upsample_kd_fwd_bwd) — every exit but
        the last adds scale * alpha * T^2 * mean over valid pixels of KL(softmax(z_last / T) || softmax(z_exit / T)) to its loss; the last
        exit's logits are read detached.  Needs the fused head on every exit, more than one exit and exits on one low-resolution grid.
        dice = (weight, smooth): a soft-Dice region term in every exit's loss head (include/addk.h, addk_dice_stats) — per exit and per
        process, scale * weight * (1 - mean over the classes present in the batch of (2 I_c + smooth) / (P_c + Y_c + smooth)) over the valid
        pixels; class_weight does not weigh it and ohem does not filter it.  Only the fused loss head has this form: ValueError otherwise.
        focal = gamma (finite, >= 1) or label_smoothing = eps (0 < eps < 1), never both: the shape of every exit's per-pixel loss
        (include/addk.h, addk_ce_upsample_shaped_fwd_bwd) — w_t (1 - p_t)^gamma (-log p_t) in the place of w_t (-log p_t), or
        torch.nn.functional.cross_entropy(label_smoothing=eps); the normaliser stays the head's.  Both compose with class_weight, ohem (the
        kept set is still chosen on the plain per-pixel cross-entropy) and dice; neither has a form with distill or over full-resolution
        logits: ValueError.  ValidationStep keeps reporting the plain cross-entropy."""
        lib = self.lib = L.load()
        self.ohem = _check_ohem(ohem, batch_shape[0])
        self.distill = _check_distill(distill)
        self.dice = _check_dice(dice)
        self.focal, self.label_smoothing = _check_shape(focal, label_smoothing, distill)
        dev = next(model.parameters()).device
        _plan.require_device(next(model.parameters()))
        self.model, self.dev = model, dev
        model.train()
        for p in model.parameters():
            ensure_layout(p)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.flat_p, self.flat_g, gviews = _flat_views(self.params, dev)
        self.mom_buf = torch.zeros_like(self.flat_p)
        self.lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
        self.hyper = (momentum, weight_decay, int(nesterov))
        N, Cin, H, W = batch_shape
        self.x = torch.zeros(batch_shape, dtype=torch.float32, device=dev)
        self.target = torch.zeros((N, H, W), dtype=torch.int64, device=dev)
        # data-parallel world: from torch.distributed itself, NOT from the SyncBN communicator — the reference's DDP
        # averages gradients with or without --sync-bn (train.py:173-175)
        import torch.distributed as dist
        self.group = sync_comm.group if sync_comm is not None else None
        self.world = dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1
        self.comm = sync_comm
        g = self.g = Graph(dev, True, True, sync_comm)
        g.pgrad_views = gviews
        # the step never hands out full-resolution logits: up-sampling + loss + their backward run as one launch per exit
        g.head = 'ce' if os.environ.get('ADDK_FUSE_CE', '1') == '1' else None
        a, self.inref = g.input_nchw(self.x)
        self.inref.bind(self.x)
        outs = model.emit(g, a)
        self.outs = outs
        nex = len(outs)
        if self.ohem is not None and any(o.head != 'ce' for o in outs):
            raise ValueError('ohem: an exit of this model has no fused loss head at this shape (addk_ce_upsample_supported == 0: the head takes '
                             '%s and at most 16 output rows per input row)' % L.head_classes_text())
        if self.dice is not None and any(o.head != 'ce' for o in outs):
            raise ValueError('dice: an exit of this model has no fused loss head at this shape (addk_ce_upsample_supported == 0: the head takes '
                             '%s and at most 16 output rows per input row)' % L.head_classes_text())
        for name, v in (('focal', self.focal), ('label_smoothing', self.label_smoothing)):
            if v is not None and any(o.head != 'ce' for o in outs):
                raise ValueError('%s: an exit of this model has no fused loss head at this shape (addk_ce_upsample_supported == 0: the head '
                                 'takes %s and at most 16 output rows per input row)' % (name, L.head_classes_text()))
        if self.distill is not None:
            if nex < 2:
                raise ValueError('distill: this model has a single exit, nobody to teach')
            if any(o.head != 'ce' for o in outs):
                raise ValueError('distill: an exit of this model has no fused loss head at this shape (addk_ce_upsample_supported == 0: the head takes '
                                 '%s and at most 16 output rows per input row)' % L.head_classes_text())
            if len({(o.src.N, o.src.H, o.src.W, o.src.C) for o in outs}) != 1:
                raise ValueError('distill: the exits\' low-resolution logits differ in shape: %r'
                                 % ([(o.src.N, o.src.H, o.src.W, o.src.C) for o in outs],))
        ncls = outs[0].shape[1] if outs[0].head == 'ce' else outs[0].y.shape[1]
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.wsum = torch.zeros(1, dtype=torch.float32, device=dev)
        ws = torch.zeros(int(lib.addk_ce_ws_floats(N, H * W)), dtype=torch.float32, device=dev)
        cw = class_weight.to(dev).float().contiguous() if class_weight is not None else None
        self._keep = [ws, cw]
        cwp = cw.data_ptr() if cw is not None else None
        g._add(g.fwd, 'loss_zero', lib.addk_fill, self.loss.data_ptr(), 1, 0.0, wr=[self.loss])
        if self.ohem is None:             # a mining head normalises by its own kept weight sum
            g._add(g.fwd, 'ce_count', lib.addk_ce_count, self.target.data_ptr(), N * H * W, cwp, ignore_index, ncls,
                   self.wsum.data_ptr(), ws.data_ptr(), rd=[self.target], wr=[self.wsum, ws])
        nvalid = None
        if self.distill is not None:
            # n of the distillation term: the unweighted count of valid pixels.  The plain step's wsum is that count; a step with class
            # weights or mining counts once more, ONE launch for all exits
            nvalid = self.wsum
            if cw is not None or self.ohem is not None:
                nvalid = self.nvalid = torch.zeros(1, dtype=torch.float32, device=dev)
                nws = torch.zeros_like(ws)
                self._keep.append(nws)
                g._add(g.fwd, 'ce_count_valid', lib.addk_ce_count, self.target.data_ptr(), N * H * W, None, ignore_index, ncls,
                       nvalid.data_ptr(), nws.data_ptr(), rd=[self.target], wr=[nvalid, nws])
        self.dlogits = []
        for o in outs:
            if o.head == 'ce':
                o.binding = dict(target=self.target, class_w=cwp, ignore_index=ignore_index, wsum=self.wsum, scale=1.0 / nex, loss=self.loss)
                if self.ohem is not None:
                    o.binding['ohem'] = self.ohem
                if self.distill is not None and o is not outs[-1]:
                    o.binding['distill'] = self.distill + (outs[-1],)
                    o.binding['nvalid'] = nvalid
                if self.dice is not None:
                    o.binding['dice'] = self.dice
                if self.focal is not None:
                    o.binding['focal'] = self.focal
                if self.label_smoothing is not None:
                    o.binding['smooth'] = self.label_smoothing
                self.dlogits.append(None)
                continue
            d = torch.empty_like(o.y)
            self.dlogits.append(d)
            g._add(g.fwd, 'ce_fwd_bwd', lib.addk_ce_fwd_bwd, o.y.data_ptr(), self.target.data_ptr(), N, ncls, H * W, cwp,
                   ignore_index, self.wsum.data_ptr(), 1.0 / nex, self.loss.data_ptr(), d.data_ptr(), ws.data_ptr(),
                   rd=[o.y, self.target, self.wsum], wr=[self.loss, d, ws])
            o.dy_ptr, o.dynamic = d.data_ptr(), False
        has_coll = self.world > 1 or (sync_comm is not None and sync_comm.force)
        self.gsync = None
        if has_coll:
            from .parallel import GradSync
            self.gsync = g.grad_sync = GradSync(self.flat_g, gviews, self.group, int(os.environ.get('ADDK_GRAD_BUCKETS', '4')),
                                                log=getattr(sync_comm, 'log', None))
        if nstreams is None:
            # two HIP streams: independent branches of the cell DAG overlap (-4 ms of 82 at config 2, eager or captured);
            # 3, 4 and 6 streams measure the same or slightly worse (68.5 / 68.7 / 69.8 / 69.7 ms).  The SyncBN path
            # keeps its collectives on one stream.
            nstreams = _plan.env_streams()
        g.finalize(nstreams)
        self.nbt = NbtCounter(g.nbt)
        self.nbt.bump(); self.nbt.flat.sub_(self.nbt.inc)      # flatten now (pointers must be fixed before graph capture)
        self.n_active = self.flat_p.numel()
        self.nbytes = g.nbytes
        if use_graph is None:
            # A step WITHOUT collectives is captured whole.  A step with RCCL collectives: whole when the world is this one
            # process (the forced-exchange rehearsal, tests/test_gpu_train.py) or ADDK_GRAPH_DDP=1 asks for it; with world > 1 the
            # default is the eager launch list until a multi-rank capture has been seen on hardware (no multi-GPU box was available
            # to the builder: DESIGN.md §7; bench.py times the eager list first and then TRIES the capture under a watchdog).
            # (Round 3's third form — hipGraph segments between eager collectives — measured slower than the eager list twice
            # and was removed in round 4.)
            ddp = os.environ.get('ADDK_GRAPH_DDP')
            if ddp is None:
                ddp = '1' if self.world == 1 else '0'
            graphs_on = os.environ.get('ADDK_GRAPH', '1') == '1'
            use_graph = graphs_on and (not has_coll or ddp == '1')
        self.has_coll = has_coll
        self.graph = None
        self.use_graph = use_graph
        self.steps = 0

    # one eager pass of the whole step on the current stream
    def _run(self):
        main = torch.cuda.current_stream()
        st = main.cuda_stream
        g = self.g
        g.run_parallel(g.fwd, main)
        g.run_parallel(g.bwd, main)          # the bucketed gradient all-reduces are commands of this list (parallel.GradSync)
        if self.gsync is not None:
            self.gsync.wait()
        self._sgd(st)
        self.nbt.flat.add_(self.nbt.inc)

    def _sgd(self, st):
        mom, wd, nest = self.hyper
        L.check(self.lib.addk_sgd_step(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.mom_buf.data_ptr(), self.n_active,
                                       self.lr_dev.data_ptr(), mom, wd, nest, 0, 1.0 / self.world, st), 'sgd_step')

    def forward_backward_only(self):
        """Forward + loss + backward without the optimizer update (parity tests)."""
        main = torch.cuda.current_stream()
        self.g.run_parallel(self.g.fwd, main)
        self.g.run_parallel(self.g.bwd, main)
        if self.gsync is not None:
            self.gsync.wait()

    def _capture(self):
        """Capture one step into a hipGraph.  Returns the graph, or None when the step has collectives and ANY rank's runtime
        refused the capture (then every rank stays on the eager launch list: the decision is made collectively, so no rank
        replays a graph while another issues eager collectives).  Nothing is executed here: the caller's eager step stands."""
        graph, err = torch.cuda.CUDAGraph(), None
        try:
            # A step with RCCL exchanges is captured in THREAD-LOCAL error mode: ProcessGroupNCCL's watchdog thread keeps
            # querying the events of the eager step's collectives, and in the default global mode such a query from another
            # thread while this one captures is an illegal call.
            with torch.cuda.graph(graph, capture_error_mode='thread_local' if self.has_coll else 'global'):
                self._run()
        except Exception as e:
            if not self.has_coll:
                raise
            err = e
        if self.has_coll:
            ok = torch.tensor([0.0 if err is not None else 1.0], device=self.dev)
            import torch.distributed as dist
            if self.world > 1 and dist.is_available() and dist.is_initialized():
                dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)
            if float(ok.item()) < 1.0:
                import sys
                why = str(err).splitlines()[0] if err is not None else 'another rank failed'
                sys.stderr.write('[addk] hipGraph capture of the data-parallel step failed (%s): eager replay on every rank\n' % why)
                if self.gsync is not None:
                    del self.gsync.works[:]
                torch.cuda.synchronize()
                return None
        return graph

    def enable_capture(self):
        """Switch a step that runs on the eager list to whole-step capture; the next step() runs eagerly once more and captures
        (a refused capture keeps every rank on the eager list).  Used by bench.py at world > 1 after the eager timing."""
        self.use_graph, self.graph = True, None

    def load_batch(self, images, targets):
        self.x.copy_(images, non_blocking=True)
        self.target.copy_(targets, non_blocking=True)

    def set_lr(self, lr):
        self.lr_dev.fill_(float(lr))

    def step(self, images=None, targets=None, lr=None):
        """Runs one optimisation step on the resident batch (or on `images`/`targets` if given) and returns the
        loss as a device tensor (no host sync; the reference's per-step loss.item() is the caller's choice)."""
        if images is not None:
            self.load_batch(images, targets)
        if lr is not None:
            self.set_lr(lr)
        if self.use_graph:
            if self.graph is None:
                # this call's step runs eagerly (it also warms RCCL); the capture that follows executes nothing
                self._run()
                torch.cuda.synchronize()
                if self.has_coll:
                    # ProcessGroupNCCL's watchdog thread polls the events of the eager step's collectives (every 100 ms) until it has seen them
                    # complete; a query from that thread while this one captures is the one cross-thread HIP call left in the process.  Give
                    # it time to retire them first.  Inference, not a shown cause: an abort inside the capture of a step with collectives was
                    # seen in rounds 2 and 5 (once each, not reproducible) — tests/conftest.py now leaves the native stack
                    import time
                    time.sleep(0.3)
                self.graph = self._capture()
                if self.graph is None:
                    self.use_graph = False
            else:
                self.graph.replay()
        else:
            self._run()
        self.steps += 1
        return self.loss

    def close(self):
        """Release everything that refers to the process group BEFORE `dist.destroy_process_group()`: the captured hipGraph (its
        nodes are RCCL kernels of that communicator), the outstanding Work handles of the gradient buckets and the side streams'
        pending launches.  Callers that own a process group call this, then `torch.cuda.synchronize()`, then destroy the group
        (train.py:49-53 is the lifecycle the drop-in has to survive: a communicator torn down under a live graph or a polling
        watchdog was the one ordering fault found in bench.py's and the tests' teardown paths)."""
        if self.gsync is not None:
            try:
                self.gsync.wait()
            except Exception:
                del self.gsync.works[:]
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        self.graph = None
        self.use_graph = False

    def ohem_stats(self):
        """Per exit (tau, kept, valid) of the last step: the loss threshold, the pixels that counted and the valid pixels of the batch.
        Synchronises the device; not part of the step."""
        if self.ohem is None:
            raise ValueError('this step was built without ohem')
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        res = []
        for o in self.outs:
            st = o.binding['ohem_state']
            valid, kept = (int(v) for v in st['counts'].tolist())
            res.append((float(st['tau'].item()), kept, valid))
        return res

    def distill_stats(self):
        """Per student exit (every exit but the last, in order) the distillation term `kd` of the last step, as it entered the loss.
        Synchronises the device; not part of the step."""
        if self.distill is None:
            raise ValueError('this step was built without distill')
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        return [float(o.binding['distill_state']['kd'].item()) for o in self.outs[:-1]]

    def dice_stats(self):
        """Per exit (dice, [D_c, or None for a class absent from the batch]) of the last step: the term as it entered the loss and the
        per-class soft-Dice scores.  Synchronises the device; not part of the step."""
        if self.dice is None:
            raise ValueError('this step was built without dice')
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        res = []
        for o in self.outs:
            v = o.binding['dice_state']['dice'].tolist()
            res.append((v[0], [None if d < 0 else d for d in v[1:]]))
        return res

    def grads(self):
        return {p: self.g.pgrad.get(p) for p in self.params}
