"""Static execution plans for the ADD hot path.

A module tree (modeling/*.py) is *emitted* once per (input shape, mode) into a `Graph`:
a flat list of C-ABI kernel launches over pre-allocated NHWC buffers plus the matching
backward list (built in reverse with first-touch/accumulate flags decided at build
time, so no memsets and no separate add kernels).  Replaying a plan is a tight loop of
ctypes calls on one HIP stream — or a single hipGraph launch once captured.

Activations are *lazy*: `Act = (raw, bn, relu)` means relu?(a*raw+b) with (a,b) owned by
the producing BatchNorm; consumers apply it while staging their tiles, so BatchNorm/ReLU
never cost a pass over HBM.
"""
import collections
import itertools
import os
import ctypes as C

import torch

from . import _lib as L
from .sched import WHOLE, Cmd, _overlap, _region, deps, level_order, levels, schedule      # noqa: F401  (the launch-list core)


TRACE_BN = None        # diagnostics (tests/tools): a list that receives (BatchNorm module, raw TRef) of every Graph.bn call


def _on(name, default='1'):
    """An ADDK_* switch, read when a plan is emitted (tests change the environment between two plan builds)."""
    return os.environ.get(name, default) == '1'


def _env_int(name, default):
    return int(os.environ.get(name, default))


def env_streams():
    """ADDK_STREAMS: the HIP streams a plan is scheduled on where its caller names no number."""
    return _env_int('ADDK_STREAMS', '2')


def env_graph_infer():
    """ADDK_GRAPH_INFER: inference plans are replayed as hipGraphs (0 = the eager launch loop)."""
    return _on('ADDK_GRAPH_INFER')


def _ptr(x):
    return None if x is None else x.ptr


class Buf:
    """Flat fp32 device buffer; `ordinal` is its place among the buffers of its plan (Graph.buf) and names it as a region."""
    __slots__ = ('t', 'ptr', 'n', 'gbuf', 'ginit', 'region', 'geom')

    def __init__(self, n, device, zero=False, ordinal=0):
        self.n = int(n)
        self.geom = None       # (N, H, W, ld) where the whole buffer is one NHWC tensor (Graph.tensor)
        self.region = (('buf', ordinal),) + WHOLE
        self.t = (torch.zeros if zero else torch.empty)(max(self.n, 4), dtype=torch.float32, device=device)
        self.ptr = self.t.data_ptr()
        self.gbuf = None       # gradient twin
        self.ginit = []        # initialised channel intervals of this (gradient) buffer


class TRef:
    """NHWC view (n,h,w,c) -> buf[off + ((n*H+h)*W+w)*ld + c]."""
    __slots__ = ('buf', 'off', 'N', 'H', 'W', 'C', 'ld')

    def __init__(self, buf, off, N, H, W, C, ld):
        self.buf, self.off, self.N, self.H, self.W, self.C, self.ld = buf, off, N, H, W, C, ld

    @property
    def ptr(self):
        return self.buf.ptr + 4 * self.off

    @property
    def P(self):
        return self.N * self.H * self.W

    @property
    def cols(self):
        """channel interval [c0, c1) of this view inside the pixel row"""
        c0 = self.off % self.ld if self.ld else 0
        return c0, c0 + self.C

    @property
    def region(self):
        return self.buf.region[:1] + self.cols

    def chan(self, c0, C):
        assert 0 <= c0 and c0 + C <= self.C
        return TRef(self.buf, self.off + c0, self.N, self.H, self.W, C, self.ld)

    def view(self):
        """torch view [N,H,W,C] (strided)."""
        return self.buf.t.as_strided((self.N, self.H, self.W, self.C),
                                     (self.H * self.W * self.ld, self.W * self.ld, self.ld, 1), self.off)


class Vec:
    __slots__ = ('buf', 'off', 'n')

    def __init__(self, buf, off, n):
        self.buf, self.off, self.n = buf, off, n

    @property
    def ptr(self):
        return self.buf.ptr + 4 * self.off

    @property
    def region(self):
        return self.buf.region

    def view(self):
        return self.buf.t[self.off:self.off + self.n]


class LateVec:
    """A small device vector whose storage is assigned only after the launch list has been ordered (Graph._bind_late):
    the statistics vectors exchanged by the SyncBN all-reduces of ONE dependency level are laid out back to back in one
    arena, so a level costs a single plain `all_reduce` on a contiguous tensor.  `n` counts 4-byte slots; `f64` marks
    fp64 pairs (forward statistics).  Dependency tracking names it by a serial number, before and after it is bound."""
    __slots__ = ('n', 'f64', 'buf', 'off', 'binders', 'region')
    _serial = itertools.count()

    def __init__(self, n, f64=False):
        self.n, self.f64, self.buf, self.off, self.binders = int(n), f64, None, 0, []
        self.region = (('late', next(LateVec._serial)),) + WHOLE

    @property
    def ptr(self):
        if self.buf is None:
            raise RuntimeError('LateVec used before Graph.finalize() bound it')
        return self.buf.ptr + 4 * self.off

    def bind(self, buf, off):
        self.buf, self.off = buf, off
        for b in self.binders:
            b(self.ptr)

    def view(self):
        t = self.buf.t[self.off:self.off + self.n]
        return t.view(torch.float64) if self.f64 else t


class BNState:
    """Per-call state of one BatchNorm application: lazy affine + saved statistics + the
    partial (dA,dB) slabs its consumers produce in backward."""

    def __init__(self, mod, C, a, b, training, count):
        self.mod, self.C, self.a, self.b = mod, C, a, b
        self.training, self.count = training, count
        self.mean = self.invstd = None
        self.slabs = []          # [(ptr, rows)]
        self.c1 = self.c2 = None


class Act:
    """Lazy activation: value = relu?(a*raw+b).  `rs` (a Resample, shared by every Act derived from one Graph.resize call): `raw` is
    the bilinear interpolation of another map and has NOT been written yet — a 1x1 convolution that consumes it samples the source
    map itself (addk_src.rs_hw); any other consumer makes Graph.src / Graph.lz emit the stand-alone resize launch first."""
    __slots__ = ('raw', 'bn', 'relu', 'needs_grad', 'zero', 'rs')

    def __init__(self, raw, bn=None, relu=False, needs_grad=False, zero=False, rs=None):
        self.raw, self.bn, self.relu, self.needs_grad, self.zero, self.rs = raw, bn, relu, needs_grad, zero, rs

    N = property(lambda s: s.raw.N)
    H = property(lambda s: s.raw.H)
    W = property(lambda s: s.raw.W)
    C = property(lambda s: s.raw.C)


class Resample:
    """Deferred bilinear resize (Graph.resize): `src` is the TRef of the map to sample, `emit()` appends the stand-alone launch that
    writes the resized tensor, `done` says that some launch writes it (that launch, or a folding consumer's copy-out in training)."""
    __slots__ = ('src', 'emit', 'done')

    def __init__(self, src, emit):
        self.src, self.emit, self.done = src, emit, False


def _covered(intervals, c0, c1):
    """how much of [c0, c1) a list of disjoint intervals covers"""
    return sum(max(0, min(c1, b) - max(c0, a)) for a, b in intervals)


def _first_touch(intervals, c0, c1, what):
    """0 the first time [c0, c1) is written in backward order (the interval is recorded), 1 once it has been written whole."""
    covered = _covered(intervals, c0, c1)
    if covered == 0:
        intervals.append((c0, c1))
        return 0
    if covered == c1 - c0:
        return 1
    raise NotImplementedError('partially initialised %s [%d,%d) vs %s' % (what, c0, c1, intervals))


def _out_hw(H, W, k, stride, pad, dil):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _chunks(items, least):
    """`items` cut into ADDK_WGRAD_CHUNKS (3) runs of equal length, in emission (= backward) order, if a run then holds at least `least`"""
    k = _env_int('ADDK_WGRAD_CHUNKS', 3)
    per = max(1, -(-len(items) // (k if len(items) >= least * k else 1)))
    return [items[i:i + per] for i in range(0, len(items), per)]


def _set_geom(x, geom):
    """conv geometry onto an argument struct (ConvArgs, ConvDgradArgs, ConvWgradArgs, DwArgs, DwBwdArgs)"""
    x.N, x.H, x.W, x.OH, x.OW, x.KH, x.KW, x.stride, x.pad, x.dil = geom


# How Graph.level_batch turns the same-kind, same-key launches of one dependency level into ONE launch.  `per_level`: the members of
# a level are merged whatever their network segment, and a lone member is replaced too.
class _Table(collections.namedtuple('_Table', 'fn size')):
    """a table of the members' argument structs -> fn(table, count, largest `size` field)"""
    per_level = False

    def build(self, g, name, cs):
        arr = (type(cs[0].payload) * len(cs))(*[c.payload for c in cs])
        m = Cmd(name + '_batch', getattr(g.lib, self.fn), (g._table(bytes(arr)).data_ptr(), len(cs), max(int(getattr(c.payload, self.size)) for c in cs)))
        m.table = arr
        return m


class _Prepared(collections.namedtuple('_Prepared', 'prepare run')):
    """the library turns the members' argument structs into kernel descriptors: prepare -> blob + meta -> run(blob, meta)"""
    per_level = False

    def build(self, g, name, cs):
        arr = (type(cs[0].payload) * len(cs))(*[c.payload for c in cs])
        blob, meta = g._prepare(getattr(g.lib, self.prepare), arr, len(cs), self.prepare)
        m = Cmd(name + '_batch', getattr(g.lib, self.run), (g._table(blob).data_ptr(), meta))
        m.table = arr
        return m


class _Arena(collections.namedtuple('_Arena', '')):
    """SyncBN exchanges: the vectors of a level are contiguous in one arena (Graph._bind_late) -> ONE plain all-reduce of it"""
    per_level = True

    def build(self, g, name, cs):
        arena, total, f64 = cs[0].arena
        assert all(c.arena[0] is arena for c in cs)
        t = arena.t[:total]
        m = Cmd('allreduce_packed', g.world._allreduce, (t.view(torch.float64) if f64 else t,), pin=True)
        m.members = len(cs)
        return m


BATCHED = {'bn_finalize': _Table('addk_bn_finalize_batch', 'C'), 'bn_bwd': _Table('addk_bn_bwd_batch', 'C'),
           'bn_bwd_apply': _Table('addk_bn_bwd_apply_batch', 'P'),
           'slab_reduce': _Table('addk_slab_reduce_batch', 'C'), 'bn_bwd_coeffs': _Table('addk_bn_bwd_coeffs_batch', 'C'),
           'conv_fwd': _Prepared('addk_conv_fwd_batch_prepare', 'addk_conv_batch_run'),
           'conv_dgrad': _Prepared('addk_conv_dgrad_batch_prepare', 'addk_conv_batch_run'),
           'dw_fwd': _Prepared('addk_dw_fwd_batch_prepare', 'addk_dw_batch_run'), 'dw_bwd': _Prepared('addk_dw_bwd_batch_prepare', 'addk_dw_batch_run'),
           'sep_fwd': _Prepared('addk_sep_fwd_batch_prepare', 'addk_sep_batch_run'),
           'sep_bwd': _Prepared('addk_sep_bwd_batch_prepare', 'addk_sep_bwd_batch_run'),
           'resize_bwd': _Prepared('addk_resize_bwd_batch_prepare', 'addk_resize_bwd_batch_run'),
           'allreduce': _Arena()}


class Graph:
    def __init__(self, device, training, want_grad, world=None):
        self.lib = L.load()
        self.device = device
        self.training = training
        self.want_grad = want_grad
        self.world = world            # SyncBN communicator (parallel.SyncBNComm) or None
        self.fwd, self.bwd = [], []   # [(name, fn, args)]
        self._bwd_emitters = []       # closures emitting backward commands, run in reverse
        self.keep = []                # keep ctypes structs / tensors alive
        self.pgrad = {}               # param -> grad tensor
        self.pgrad_views = None       # param -> view of a flat gradient buffer to use as its gradient (train.TrainStep)
        self.reorder = False          # level-order and batch the lists although this is not a training plan (set before finalize)
        # who consumes the decoder's low-resolution logits (resize_to_nchw; a key of heads.HEADS): None = nobody, the resize writes
        # [N,C,OH,OW]; 'ce' = the fused up-sampling + cross-entropy launch (train.TrainStep); 'score' = the scoring launch
        # (validate.ValidationStep); 'profile' = the per-image exit-profile launch (exit_profile.ExitProfile); 'labels' = the label head
        # (dynamic plans, segment.Segmenter); 'views' = the multi-view label head: every logits output of the plan is one or more views of
        # ONE label map (segment.MultiViewSegmenter); 'calib' = the calibration launch (calibrate.ExitCalibration)
        self.head = None
        self.lut = None               # 'labels' / 'views': the uint8 [256] device table the class indices go through, or None
        self.view_labels = None       # 'views': the plan-owned uint8 [N,OH,OW] map, allocated by finalize() (heads._emit_views)
        self.gate = None              # logits outputs of an inference plan are gated exits (dynamic.GatePlan): {'kind', 'host', 'thr'}; with head None or 'labels'
        #                               optional 'temp': the device word 1 / temperature of a tempered gate (heads.gate_head)
        self._fwd_late = []           # callables emitting forward commands whose bindings arrive after the module tree was emitted (heads.py)
        self.pginit = set()
        self._pcols = {}
        self.params = []              # ordered unique params touched
        self.nbt = {}                 # BatchNorm module -> num_batches_tracked increments per forward
        self._wgrads = []             # wgrad arg structs sharing one scratch buffer (launches are stream-ordered)
        self.nbytes = 0
        self._bufs = []               # owns every device buffer: kernels only see raw pointers
        self.nstreams = 1             # set by finalize(nstreams=k)
        self._streams = None          # side streams of run_parallel, created on first use
        self.tag = ''                 # segment label stamped on emitted commands (stem / cell / low / aspp / decoder)
        self._evalbn, self._evalbn_cmd = [], None
        self._dwreds = []             # deferred depthwise weight-gradient reductions (item, workspace, grad tensor)
        self._packs, self._pack_cmd = [], None   # hoisted weight packs of the halo-patch conv launches (descriptor bytes)
        self.meta = []                # per-launch algorithmic work of the dense convs (bench / roofline)
        self.grad_sync = None         # parallel.GradSync of a data-parallel train step (set before finalize)
        # the arithmetic mode the packed weights and kernel choices of this plan were built for: replaying the launch list under
        # another mode would hand bf16-plane packs to the fp32 kernel — run() / run_parallel() refuse it
        self.precision = int(self.lib.addk_get_conv_precision())

    # ---------------- memory ----------------
    def buf(self, n, zero=False):
        b = Buf(n, self.device, zero, len(self._bufs))
        self._bufs.append(b)
        self.nbytes += 4 * b.n
        return b

    def tensor(self, N, H, W, Cc, ld=None):
        ld = ld or (Cc + 3) // 4 * 4
        b = self.buf(N * H * W * ld, zero=(ld != Cc))
        b.geom = (N, H, W, ld)
        return TRef(b, 0, N, H, W, Cc, ld)

    def vec(self, n, zero=False):
        return Vec(self.buf(n, zero), 0, n)

    def grad(self, tref):
        """Gradient twin of a TRef (same geometry in the twin buffer)."""
        b = tref.buf
        if b.gbuf is None:
            b.gbuf = self.buf(b.n)
        return TRef(b.gbuf, tref.off, tref.N, tref.H, tref.W, tref.C, tref.ld)

    def acc_flag(self, gref):
        """0 the first time a channel interval of a gradient buffer is written in backward order, 1 afterwards."""
        return _first_touch(gref.buf.ginit, *gref.cols, 'gradient interval')

    def grad_ready(self, tref):
        b = tref.buf.gbuf
        return b is not None and _covered(b.ginit, *tref.cols) == tref.C

    def param(self, p):
        if p not in self.pgrad:          # Tensor hashes by identity
            self.pgrad[p] = None
            self.params.append(p)
        return p.data_ptr()

    def param_grad(self, p, cols=None):
        """(ptr, accumulate) of the plan-owned gradient of parameter p.  `cols` = (c0, c1) is the input-channel
        interval a launch writes (virtual-concat sources and the ASPP image-pool fold write disjoint column
        ranges of one weight): first touch of an interval overwrites, later touches accumulate."""
        self.param(p)
        if self.pgrad[p] is None:
            views = self.pgrad_views
            self.pgrad[p] = views[p] if views is not None and p in views else torch.empty_like(p)
            self._pcols[p] = []
        acc = _first_touch(self._pcols[p], *(cols or WHOLE), 'weight-gradient columns')      # no `cols`: the whole tensor
        self.pginit.add(p)
        return self.pgrad[p].data_ptr(), acc

    def finalize(self, nstreams=1):
        """Emit the backward list (reverse op order), schedule both lists on `nstreams` streams and allocate one wgrad
        scratch per stream (launches of one stream are ordered, so they can share it)."""
        for em in self._fwd_late:
            em()
        self._fwd_late = []
        for em in reversed(self._bwd_emitters):
            em()
        self._bwd_emitters = []
        self.nstreams = max(1, int(nstreams))
        if self._evalbn:
            n = len(self._evalbn)
            self._evalbn_cmd.table = (L.BnEvalItem * n)(*self._evalbn)
            self._evalbn_cmd.args[0], self._evalbn_cmd.args[1] = self._table(bytes(self._evalbn_cmd.table)).data_ptr(), n
        self._emit_batched_dw_reductions()
        self._emit_batched_wgrads()
        if self._packs:
            tab = self._table(b''.join(self._packs))
            self._pack_cmd.args[0], self._pack_cmd.args[1] = tab.data_ptr(), len(self._packs)
        batch = ((self.training and self.want_grad) or self.reorder) and _on('ADDK_LEVEL_BATCH')
        for lst in (self.fwd, self.bwd):
            self._bind_late(lst, by_level=batch)          # storage of the exchanged statistics vectors: one arena per level
            if batch:
                self.level_batch(lst)
        if self.grad_sync is not None:
            self.grad_sync.insert(self, self.bwd)          # bucketed gradient all-reduces, each right after its last producer
        for lst in (self.fwd, self.bwd):
            self.place(lst)

    def place(self, lst):
        """Schedule a launch list on this plan's streams and create the events its cross-stream waits need."""
        schedule(lst, self.nstreams)
        for c in lst:
            if c.event:
                c.event = torch.cuda.Event()

    def _table(self, data):
        """A table of host bytes on the plan's device (a CPU copy in dry runs), kept alive with the plan."""
        host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        tab = host.to(self.device) if self.device.type == 'cuda' else host.clone()
        self.keep.append(tab)
        return tab

    def _prepare(self, prep, arr, n, what):
        """A library `*_batch_prepare` call made twice: for the blob's size, then to fill it.  Returns the blob's bytes and the
        meta array (kept alive with the plan: the batched launch reads it)."""
        meta = (C.c_int64 * 8)()
        size = prep(arr, n, None, 0, meta)
        if size < 0:
            L.check(int(size), what)
        blob = (C.c_uint8 * size)()
        rc = prep(arr, n, blob, size, meta)
        if rc < 0:
            L.check(int(rc), what)
        self.keep.append(meta)
        return bytes(blob), meta

    @staticmethod
    def _config(query, args):
        """cfg[8] of a library `*_config` query: the kernel decision of the launch these arguments describe"""
        cfg = (C.c_int32 * 8)()
        L.check(query(C.byref(args), cfg), query.__name__)
        return cfg

    @staticmethod
    def _batchable(cmd, key_fn, args):
        """Let _level_batch merge `cmd` with the same-key commands of its level, if the library gives its arguments a batch key."""
        bk = int(key_fn(C.byref(args)))
        if bk >= 0:
            cmd.payload, cmd.bkey = args, bk

    def _bind_late(self, lst, by_level):
        """Give every exchanged statistics vector (LateVec payload of an 'allreduce' command) its storage.  With level
        batching the vectors of one dependency level share one arena, in list order, and `level_batch` replaces their
        commands by ONE all-reduce of the arena; otherwise each gets its own buffer.  Runs before any table-driven batch is
        built, because the producers (slab_reduce / bn_bwd) and consumers (bn_finalize / bn_bwd_coeffs) of a vector sit on
        other levels and carry its address in their argument structs."""
        ars = [(i, c) for i, c in enumerate(lst) if c.name == 'allreduce' and isinstance(c.payload, LateVec)]
        if not ars:
            return
        level = levels(lst) if by_level else list(range(len(lst)))
        groups = collections.defaultdict(list)
        for i, c in ars:
            groups[(level[i], c.payload.f64)].append(c)
        for (_, f64), cs in sorted(groups.items()):
            unit = 4                                   # slots of 16 bytes: every vector starts 16-byte aligned
            total = sum((c.payload.n + unit - 1) // unit * unit for c in cs)
            arena = self.buf(total, zero=True)
            off = 0
            for c in cs:
                c.payload.bind(arena, off)
                off += (c.payload.n + unit - 1) // unit * unit
            for c in cs:
                c.arena = (arena, total, f64)

    def _unmerged_kinds(self):
        """[r4] Kinds level_batch leaves as single launches.  In the TRAINING step the fused SepConv halves run better one by one (33.6-33.7 vs
        33.95-34.0 ms per step, ABAB on one box): a merged launch waits for its latest input and holds every consumer back, and these launches
        are long enough (15-70 us) for the two streams to overlap them; every other kind measured slower or equal un-merged (bn_bwd +1.3 ms,
        bn_bwd_apply +0.9, conv_dgrad +0.4), and inference (exit latency, forward segment) is equal or better with the halves merged.
        ADDK_NO_BATCH=kind,... overrides."""
        env = os.environ.get('ADDK_NO_BATCH')
        if env is not None:
            return set(filter(None, env.split(',')))
        return {'sep_fwd', 'sep_bwd'} if self.training and self.want_grad else set()

    def level_batch(self, lst):
        """Reorder a launch list by dependency LEVEL (level_order) and merge the mutually independent same-kind launches of one level
        into one table-driven launch each (BATCHED).  The cell DAG offers ~10 independent branches per level, so the 312 finalize /
        312 backward / 312 apply launches of a step — each a ~10 us latency chain on the critical path — shrink to one launch per level."""
        single = self._unmerged_kinds()

        def merge(cmds):
            out, groups = [], collections.defaultdict(list)
            for c in cmds:
                how = BATCHED.get(c.name)
                if how is None or c.payload is None or c.name in single:
                    out.append(c)
                else:
                    # the segment tag is part of the key: a merged launch never mixes network segments (stem / cell / low / aspp / decoder), so the
                    # per-segment figures bench.segment_roofline reports time exactly that segment's work; all-reduces stay per level
                    groups[(c.name, c.bkey, '' if how.per_level else c.tag)].append(c)
            for (name, _, _), cs in groups.items():
                how = BATCHED[name]
                if len(cs) == 1 and not how.per_level:
                    out.append(cs[0])
                    continue
                m = how.build(self, name, cs)
                m.rd = [r for c in cs for r in c.rd]
                m.wr = [r for c in cs for r in c.wr]
                m.tag = cs[0].tag
                m.tags = {c.tag for c in cs}           # the segments of the members (bench.segment_roofline checks)
                out.append(m)
            return out
        level_order(lst, merge)

    _level_batch = level_batch      # the name this method had while it was private: code outside this tree still looks it up

    def _hoist_pack(self, desc_fn, args, weight, wpk, create):
        """Move the weight pack of a halo-patch conv launch out of the launch: all packs of the plan (forward and data
        gradient: the weights only change in the optimizer) run as ONE launch placed before the first such conv."""
        if self._pack_cmd is None:
            if not create:
                return
            self._pack_cmd = self._add(self.fwd, 'conv_pack_batch', self.lib.addk_conv_pack_batch, None, 0)
            self._pack_cmd.table = []
        nb = int(self.lib.addk_conv_pack_desc_bytes())
        buf = (C.c_uint8 * nb)()
        L.check(desc_fn(C.byref(args), buf), 'conv_pack_desc')
        self._packs.append(bytes(buf))
        args.wpack_ready = 1
        self._pack_cmd.table.append(args)
        self._pack_cmd.rd.append(_region(weight))
        self._pack_cmd.wr.append(_region(wpk))

    def _emit_batched_dw_reductions(self):
        """One launch reduces the weight-gradient partials of every depthwise conv of the backward pass; two items that
        write the same weight (a module used twice) go to consecutive launches, in emission order."""
        waves = []
        for it, ws, grad in self._dwreds:
            if not waves or it.dw in waves[-1][1]:
                waves.append(([], set()))
            waves[-1][0].append((it, ws, grad))
            waves[-1][1].add(it.dw)
        for items in [part for items, _ in waves for part in _chunks(items, 8)]:
            n = len(items)
            arr = (L.DwWreduceItem * n)(*[it for it, _, _ in items])
            self._add(self.bwd, 'dw_wreduce_batch', self.lib.addk_dw_wreduce_batch, self._table(bytes(arr)).data_ptr(), n,
                      rd=[ws for _, ws, _ in items], wr=[g for _, _, g in items]).table = arr

    def _emit_batched_wgrads(self):
        """All weight gradients of the backward pass are deferred to its end and launched in a few batches: one launch
        per tile configuration covers every conv that uses it (their dy / activation buffers are never reused, so
        deferral is safe).  Two gradients that accumulate into the same weight columns (the ASPP/decoder head is
        shared by the exits) must not sit in the same batch: the second goes to a later wave."""
        if not self._wgrads:
            return
        lib = self.lib
        waves = []          # [ {cfg: [(wa, rd, grad)]} , set(regions) ]
        for wa, rd, grad, region in self._wgrads:
            cfg = (C.c_int32 * 4)()
            L.check(lib.addk_conv_wgrad_config(C.byref(wa), cfg), 'conv_wgrad_config')
            key = (cfg[0], cfg[1], cfg[2])
            for groups, used in waves:
                if not any(_overlap(r, region) for r in used):
                    break
            else:
                groups, used = {}, []
                waves.append((groups, used))
            used.append(region)
            groups.setdefault(key, []).append((wa, rd, grad))
        for groups, _ in waves:
            # big groups (the cells' 1x1 / dilated convs: ~100-300 ops) are cut into batches (_chunks): the early batches only need the gradients
            # of the late cells, so the level pass can place them in the middle of the backward pass where they overlap with it on the second stream
            for key, items in [(key, part) for key, items in groups.items() for part in _chunks(items, 32)]:
                n = len(items)
                arr = (L.ConvWgradArgs * n)()
                for i, (wa, _, _) in enumerate(items):
                    ws = self.buf(wa.ws_floats)
                    wa.ws = ws.ptr
                    arr[i] = wa
                host, meta = self._prepare(lib.addk_conv_wgrad_batch_prepare, arr, n, 'conv_wgrad_batch_prepare')
                blob = self._table(host)
                self.nbytes += len(host)
                if _on('ADDK_DEBUG_WGRAD', '0'):      # algorithmic work of this batch (tuning aid)
                    fl = sum(2.0 * w.N * w.OH * w.OW * w.Cout * w.KH * w.KW * w.src.C for w, _, _ in items)
                    by = sum(4.0 * (w.N * w.OH * w.OW * w.Cout + w.N * w.H * w.W * w.src.C) for w, _, _ in items)
                    shapes = collections.Counter((w.OH, w.OW, w.Cout, w.src.C, w.KH, w.stride) for w, _, _ in items)
                    print('wgrad batch kind/cty/ctz=%s n=%d blocks=%d  %.1f GF  %.1f MB min traffic  %s' % (
                        key, n, meta[5], fl / 1e9, by / 1e6, dict(shapes)), flush=True)
                self._add(self.bwd, 'conv_wgrad_batch', lib.addk_conv_wgrad_batch_run, blob.data_ptr(), meta,
                          rd=[r for _, rd, _ in items for r in rd], wr=[g for _, _, g in items]).table = arr

    # ---------------- command helpers ----------------
    def _add(self, lst, name, fn, *args, rd=(), wr=(), pin=False):
        c = Cmd(name, fn, args, rd, wr, pin)
        c.tag = self.tag
        lst.append(c)
        return c

    def _check_mode(self):
        if int(self.lib.addk_get_conv_precision()) != self.precision:
            raise L.AddkError('this plan was built under arithmetic mode %d and cannot be replayed under mode %d: its packed weights and '
                              'kernel choices belong to the mode it was built in (rebuild the plan after addk.set_precision)'
                              % (self.precision, int(self.lib.addk_get_conv_precision())))

    def run(self, cmds, stream):
        """Sequential replay on one stream."""
        self._check_mode()
        for name, fn, args in cmds:
            rc = fn(*args, stream)
            if rc:
                L.check(rc, name)

    def run_parallel(self, cmds, main):
        """Replay a scheduled list on `nstreams` HIP streams (stream 0 = `main`, a torch.cuda.Stream): independent
        branches of the cell DAG overlap, which is what fills 256 CUs when single launches are small.  Works eagerly
        and under hipGraph capture (fork/join through events)."""
        ns = self.nstreams
        if self.device.type != 'cuda':          # dry-run planning on CPU (tests): launches are stubbed
            return self.run(cmds, current_stream())
        self._check_mode()
        if main is None:
            main = torch.cuda.current_stream()
        if ns == 1:
            return self.run(cmds, main.cuda_stream)
        streams = [main] + self._side_streams()
        fork = torch.cuda.Event()
        fork.record(main)
        for s in streams[1:]:
            s.wait_event(fork)
        ptrs = [s.cuda_stream for s in streams]
        for c in cmds:
            s = streams[c.stream]
            for j in c.waits:
                s.wait_event(cmds[j].event)
            rc = c.fn(*c.args, ptrs[c.stream])
            if rc:
                L.check(rc, c.name)
            if c.event is not None:
                c.event.record(s)
        for s in streams[1:]:
            e = torch.cuda.Event()
            e.record(s)
            main.wait_event(e)

    def _side_streams(self):
        if self._streams is None:
            self._streams = [torch.cuda.Stream(device=self.device) for _ in range(self.nstreams - 1)]
        return self._streams

    def _pending(self, act):
        return act.rs is not None and not act.rs.done

    def _map(self, act, fold):
        """The map a consumer of lazy activation `act` reads.  fold=True (a consumer that samples a deferred resize itself): the map to
        interpolate; otherwise act.raw, a still-deferred resize being emitted as its own launch now."""
        if self._pending(act):
            if fold:
                return act.rs.src
            act.rs.emit()
        return act.raw

    def src(self, act, relu_in=False, fold=False):
        """Source descriptor of a lazy activation (`fold`: see _map)."""
        s = L.Src()
        r = self._map(act, fold)
        s.x, s.ld = r.ptr, r.ld
        if r is not act.raw:
            s.rs_hw = (r.H << 16) | r.W
        if act.bn is not None:
            s.a, s.b = act.bn.a.ptr, act.bn.b.ptr
        s.C, s.relu = act.raw.C, int(bool(act.relu or relu_in))
        return s

    def lz(self, act, fold=False):
        """Memory regions a consumer of lazy activation `act` reads."""
        return [self._map(act, fold)] + ([act.bn.a, act.bn.b] if act.bn is not None else [])

    def _backward(self, out, emit):
        """Register the backward emitter of the op that wrote `out`: finalize() calls `emit(dy)` in reverse op order, if a consumer
        has written the gradient `dy` of `out` by then."""
        def em():
            if self.grad_ready(out):
                emit(self.grad(out))
        self._bwd_emitters.append(em)

    def _grad_into(self, src, rows=None):
        """The gradient edge into lazy source `src`: (gradient twin of src.raw, 0 = first touch / 1 = accumulate, slab).  `rows`: the
        workgroup rows of the launch that also produces the (dA,dB) partials of src's BatchNorm; when that BatchNorm is in training
        mode the fp64 [rows][C][2] slab is allocated here and handed to it.  rows=None: the launch produces none."""
        gs = self.grad(src.raw)
        acc = self.acc_flag(gs)
        slab = None
        if rows is not None and src.bn is not None and src.bn.training and self.want_grad:
            slab = self.buf(rows * src.C * 4)
            src.bn.slabs.append((slab, rows))
        return gs, acc, slab

    def _defer_wgrad(self, dy, s, relu_in, weight, geom, ldw, cin_total, choff):
        """Record the gradient of columns [choff, choff + s.C) of `weight` (source `s`, output gradient `dy`) for the batched launches
        at the end of the backward pass (_emit_batched_wgrads).  What it writes is named by the weight's region (the parameters of a
        train step are views of ONE flat buffer: the byte interval tells them apart) and the column interval inside the weight."""
        wa = L.ConvWgradArgs()
        wa.dy, wa.lddy, wa.Cout = dy.ptr, dy.ld, dy.C
        _set_geom(wa, geom)
        wa.src = self.src(s, relu_in)
        cols = (choff, choff + s.C)
        gp, acc = self.param_grad(weight, cols)
        wa.dw, wa.ldw, wa.cin_total, wa.w_choff, wa.accumulate = gp, ldw, cin_total, choff, acc
        wa.ws_floats = self.lib.addk_conv_wgrad_ws(dy.P, dy.C, s.C, geom[5] * geom[6])
        self._wgrads.append((wa, [dy] + self.lz(s), self.pgrad[weight], (_region(weight),) + cols))

    def _defer_dw_wreduce(self, weight, rows, n):
        """Workspace of a depthwise weight gradient: its [rows][n] partials are reduced at the end of the backward pass, all convs in one
        launch (_emit_batched_dw_reductions).  Returns (workspace, gradient pointer, accumulate)."""
        gp, acc = self.param_grad(weight)
        ws = self.buf(rows * n)
        it = L.DwWreduceItem()
        it.ws, it.dw, it.rows, it.n, it.accumulate = ws.ptr, gp, rows, n, acc
        self._dwreds.append((it, ws, self.pgrad[weight]))
        return ws, gp, acc

    # ---------------- ops ----------------
    def conv(self, srcs, weight, Cout, k, stride=1, pad=0, dil=1, relu_in=False, bias=None, bias_n=None,
             out=None, stats=None, stats_ld=0, out_hw=None, w_choff=0, cin_total=None, fwd=True):
        """Dense conv over virtually concatenated `srcs` (list of Act).  Returns the raw output TRef.  fwd=False registers only
        the backward pass (the forward launch is part of a fused command, sep_half)."""
        lib = self.lib
        a0 = srcs[0]
        N, H, W = a0.N, a0.H, a0.W
        OH, OW = out_hw or _out_hw(H, W, k, stride, pad, dil)
        geom = (N, H, W, OH, OW, k, k, stride, pad, dil)
        csum = sum(s.C for s in srcs)
        cin_total = cin_total or csum
        if out is None:
            out = self.tensor(N, OH, OW, Cout)
        assert (out.N, out.H, out.W, out.C) == (N, OH, OW, Cout), 'conv output geometry'
        assert len(srcs) <= L.MAX_SRC
        wptr = self.param(weight)
        ldw = k * k * cin_total
        assert weight.numel() == Cout * ldw, 'weight %s does not match Cout=%d k=%d cin=%d' % (tuple(weight.shape), Cout, k, cin_total)
        if fwd:
            ar = L.ConvArgs()
            # a deferred bilinear resize in front of a 1x1 convolution (ADD.py:76-77,84-90) is sampled by the convolution itself where
            # the pointwise kernels cover the shape (addk_conv_fwd_resample_ok): no resize launch, no resized tensor at inference; in
            # training the launch also writes the resized tensor, which the backward pass reads (ADDK_FOLD_RESIZE=0: never)
            fold = (k == 1 and stride == 1 and pad == 0 and out_hw is None and any(self._pending(s) for s in srcs)
                    and _on('ADDK_FOLD_RESIZE'))
            ar.nsrc = len(srcs)
            _set_geom(ar, geom)
            ar.Cout, ar.ldw, ar.cin_total, ar.w_choff, ar.ldy = Cout, ldw, cin_total, w_choff, out.ld
            ar.w, ar.y = wptr, out.ptr
            ar.bias = self.param(bias) if bias is not None else None
            ar.bias_n, ar.stats, ar.stats_ld = _ptr(bias_n), _ptr(stats), stats_ld
            rs_out = None
            if fold:
                for i, s in enumerate(srcs):
                    assert (s.N, s.H, s.W) == (N, H, W), 'virtual concat needs equal spatial size'
                    ar.src[i] = self.src(s, relu_in, fold=True)
                if self.want_grad:                    # one copy-out slot: only src[0] may be a sampled map when a backward pass follows
                    if any(self._pending(s) for s in srcs[1:]):
                        fold = False
                    elif self._pending(srcs[0]):
                        ar.rs_y, ar.rs_ldy = srcs[0].raw.ptr, srcs[0].raw.ld
                fold = fold and int(lib.addk_conv_fwd_resample_ok(C.byref(ar))) == 1
                if not fold:
                    ar.rs_y, ar.rs_ldy = None, 0
            if not fold:
                for i, s in enumerate(srcs):
                    assert (s.N, s.H, s.W) == (N, H, W), 'virtual concat needs equal spatial size'
                    ar.src[i] = self.src(s, relu_in)  # (a still-deferred resize is emitted as its own launch here)
            rd_src = [r for s_ in srcs for r in self.lz(s_, fold=fold)]
            if fold and self.want_grad and self._pending(srcs[0]):
                rs_out = srcs[0].raw
                srcs[0].rs.done = True                # this launch writes the resized tensor
            wpk = None
            npk = 0 if fold else int(lib.addk_conv_fwd_pack_floats(C.byref(ar)))       # > 0: wide 3x3 stride-1 conv, halo-patch kernel (conv3.hip)
            if npk > 0:
                wpk = self.buf(npk)
                ar.wpack, ar.wpack_floats = wpk.ptr, npk
                self._hoist_pack(lib.addk_conv_fwd_pack_desc, ar, weight, wpk, create=True)
            self.keep.append(ar)
            cf = self._add(self.fwd, 'conv_fwd', lib.addk_conv_fwd, C.byref(ar),
                           rd=rd_src + [weight, bias, bias_n], wr=[out, stats, wpk, rs_out])
            self._batchable(cf, lib.addk_conv_fwd_batch_key, ar)
            self.meta.append(dict(kind='conv_fwd', cmd=cf, flops=2.0 * N * OH * OW * Cout * k * k * csum,
                                  bytes=4.0 * (N * H * W * csum + N * OH * OW * Cout + Cout * k * k * csum),
                                  shape=(N, H, W, csum, Cout, k, stride, dil), halo=npk > 0))
    
        if self.want_grad:
            srcs_l = list(srcs)

            def emit_bwd(dy):
                if bias is not None:
                    self._colsum(dy, bias, per_image=False)
                if bias_n is not None:
                    gbn = self.grad(bias_n)
                    self._colsum_n(dy, gbn)
                choff = w_choff
                for s in srcs_l:
                    self._defer_wgrad(dy, s, relu_in, weight, geom, ldw, cin_total, choff)
                    # data gradient
                    if s.needs_grad:
                        da = L.ConvDgradArgs()
                        da.dy, da.lddy, da.Cout = dy.ptr, dy.ld, Cout
                        _set_geom(da, geom)
                        da.w, da.ldw, da.cin_total, da.w_choff = wptr, ldw, cin_total, choff
                        da.dst = self.src(s, relu_in)
                        gs, da.accumulate, slab = self._grad_into(s, lib.addk_conv_rows(N * H * W, s.C))
                        da.g, da.ldg, da.dab = gs.ptr, gs.ld, _ptr(slab)
                        dpk = None
                        npk = int(lib.addk_conv_dgrad_pack_floats(C.byref(da)))
                        if npk > 0:
                            dpk = self.buf(npk)
                            da.wpack, da.wpack_floats = dpk.ptr, npk
                            self._hoist_pack(lib.addk_conv_dgrad_pack_desc, da, weight, dpk, create=False)
                        self.keep.append(da)
                        cd = self._add(self.bwd, 'conv_dgrad', lib.addk_conv_dgrad, C.byref(da), rd=[dy, weight] + self.lz(s),
                                       wr=[gs, slab, dpk])
                        self._batchable(cd, lib.addk_conv_dgrad_batch_key, da)
                    choff += s.C
            self._backward(out, emit_bwd)
        return out

    def _colsum(self, dy, bias, per_image):
        """bias gradient: db[c] = sum_p dy[p,c]  (via the GAP kernel over all N*H*W pixels as one 'image')."""
        lib = self.lib
        s = L.Src(); s.x, s.ld, s.C, s.relu = dy.ptr, dy.ld, dy.C, 0
        tmp = self.vec(dy.C)
        rows = lib.addk_ew_rows(dy.P, dy.C)
        ws = self.buf(rows * dy.C)
        self.keep.append(s)
        self._add(self.bwd, 'bias_grad', lib.addk_gap_fwd, C.byref(s), 1, dy.P, tmp.ptr, dy.C, ws.ptr, 0, rd=[dy], wr=[tmp, ws])
        gp, acc = self.param_grad(bias)
        one = L.AffineSumArgs()
        t = L.Src(); t.x, t.ld, t.C = tmp.ptr, dy.C, dy.C
        one.term[0] = t; one.nterm = 1; one.P = 1; one.C = dy.C
        one.out, one.ldo, one.relu_out, one.accumulate = gp, dy.C, 0, acc
        self.keep.append(one)
        self._add(self.bwd, 'bias_grad_acc', lib.addk_affine_sum_fwd, C.byref(one), rd=[tmp], wr=[self.pgrad[bias]])

    def _colsum_n(self, dy, gbn):
        """per-image bias gradient: g[n,c] = sum_{p in image n} dy[p,c]."""
        lib = self.lib
        s = L.Src(); s.x, s.ld, s.C, s.relu = dy.ptr, dy.ld, dy.C, 0
        rows = lib.addk_ew_rows(dy.H * dy.W, dy.C)
        ws = self.buf(dy.N * rows * dy.C)
        assert self.acc_flag(gbn) == 0
        self.keep.append(s)
        self._add(self.bwd, 'bias_n_grad', lib.addk_gap_fwd, C.byref(s), dy.N, dy.H * dy.W, gbn.ptr, gbn.ld, ws.ptr, 0,
                  rd=[dy], wr=[gbn, ws])

    def stats_slab(self, P, Cc):
        rows = self.lib.addk_conv_rows(P, Cc)
        return self.buf(rows * Cc * 4), rows      # fp64 [rows][C][2]

    def bn(self, raw, mod, slab=None, rows=0, post_relu=False, needs_grad=True, fuse=None):
        """Apply BatchNorm module `mod` lazily to `raw`.  Training: statistics come from `slab`.  `fuse` = (args, cmd, workgroups) of the
        producing launch when its kernel can finalize the statistics itself (last workgroup, csrc/bnfin.h): the finalize
        arguments go into `args.fin` and no bn_finalize launch is emitted (local BatchNorm only: the SyncBN exchange sits
        between the slab and the finalize)."""
        lib = self.lib
        Cc = raw.C
        a, b = self.vec(Cc), self.vec(Cc)
        training = self.training and mod.training
        count = float(raw.P)
        if TRACE_BN is not None:
            TRACE_BN.append((mod, raw))
        st = BNState(mod, Cc, a, b, training, count)
        gam = self.param(mod.weight) if mod.weight is not None else None
        bet = self.param(mod.bias) if mod.bias is not None else None
        sync = self.world is not None and getattr(mod, 'sync', False) and (self.world.size > 1 or self.world.force)      # cross-rank statistics
        if training:
            st.mean, st.invstd = self.vec(Cc), self.vec(Cc)
            fa = L.BnFinalizeArgs()
            if sync:
                red = LateVec(4 * Cc, f64=True)      # fp64 [C][2], summed over ranks
                sri = L.SlabReduceItem()
                sri.partial, sri.rows, sri.C = slab.ptr, rows, Cc
                self._add(self.fwd, 'slab_reduce', lib.addk_slab_reduce, C.byref(sri), rd=[slab], wr=[red]).payload = sri
                red.binders += [lambda p, sri=sri: setattr(sri, 'out', p), lambda p: setattr(fa, 'partial', p)]
                self.world.emit_allreduce(self, self.fwd, red)    # every rank has the same per-rank count
                fa.rows = 1
                st.count = count * self.world.size
            else:
                fa.partial, fa.rows = slab.ptr, rows
            fa.C, fa.count = Cc, st.count
            fa.gamma, fa.beta = gam, bet
            if mod.track_running_stats and mod.running_mean is not None:
                fa.running_mean, fa.running_var = mod.running_mean.data_ptr(), mod.running_var.data_ptr()
                if mod.num_batches_tracked is not None:
                    self.nbt[mod] = self.nbt.get(mod, 0) + 1
            fa.momentum = 0.1 if mod.momentum is None else mod.momentum
            fa.eps = mod.eps
            fa.a, fa.b, fa.mean, fa.invstd = a.ptr, b.ptr, st.mean.ptr, st.invstd.ptr
            self.keep.append(fa)
            stat_wr = [a, b, st.mean, st.invstd] + ([mod.running_mean, mod.running_var] if fa.running_mean else [])
            if fuse is not None and not sync and _on('ADDK_FUSE_FINALIZE', '0'):
                args, cmd, nblk = fuse
                for f_ in ('count', 'gamma', 'beta', 'running_mean', 'running_var', 'momentum', 'eps', 'a', 'b', 'mean', 'invstd'):
                    setattr(args.fin, f_, getattr(fa, f_))
                ctr = self.buf((int(lib.addk_bn_fin_ws_bytes(nblk, Cc)) + 3) // 4, zero=True)   # ticket counters + group rows of this BatchNorm call
                args.fin_counter = ctr.ptr
                cmd.rd += [r for r in (_region(mod.weight), _region(mod.bias)) if r]
                cmd.wr += [r for r in (_region(x) for x in stat_wr + [ctr]) if r]
            else:
                cfin = self._add(self.fwd, 'bn_finalize', lib.addk_bn_finalize, C.byref(fa),
                                 rd=[red if sync else slab, mod.weight, mod.bias], wr=stat_wr)
                cfin.payload = fa
        else:
            # inference: (a, b) of ALL BatchNorms come from one batched launch placed where the first one is emitted
            e = L.BnEvalItem()
            e.gamma, e.beta, e.running_mean, e.running_var = gam, bet, mod.running_mean.data_ptr(), mod.running_var.data_ptr()
            e.a, e.b, e.C, e.eps = a.ptr, b.ptr, Cc, mod.eps
            if not self._evalbn:
                self._evalbn_cmd = self._add(self.fwd, 'bn_eval_affine_batch', lib.addk_bn_eval_affine_batch, None, 0)
            self._evalbn.append(e)
            self._evalbn_cmd.rd += [_region(t) for t in (mod.weight, mod.bias, mod.running_mean, mod.running_var) if t is not None]
            self._evalbn_cmd.wr += [_region(a), _region(b)]
        act = Act(raw, st, post_relu, needs_grad and self.want_grad)

        if self.want_grad and training:
            def emit_bwd():
                if not self.grad_ready(raw) and not st.slabs:
                    return
                if not self.grad_ready(raw):
                    raise RuntimeError('BN output received (dA,dB) but no direct gradient')
                g = self.grad(raw)
                ba = L.BnBwdArgs()
                assert len(st.slabs) <= L.MAX_SLAB, 'too many consumers of one BatchNorm output (%d)' % len(st.slabs)
                for i, (p, r) in enumerate(st.slabs):
                    ba.slab[i], ba.rows[i] = p.ptr, r
                ba.nslab, ba.C, ba.count = len(st.slabs), Cc, st.count
                # dy_raw = G + c1 + c2*(x - mean): the mean is subtracted first, as the reference does (batchnorm.py:51-53), instead
                # of folding -c2*mean into c1 where it cancels against c2*x (ADDK_BN_CENTERED=0 restores the folded form)
                centered = _on('ADDK_BN_CENTERED')
                ba.centered = int(centered)
                mu = st.mean if centered else None
                ba.gamma, ba.mean, ba.invstd, ba.a = gam, st.mean.ptr, st.invstd.ptr, a.ptr
                if mod.weight is not None:
                    gp, acc = self.param_grad(mod.weight)
                    bp, acc2 = self.param_grad(mod.bias)
                    assert acc == acc2
                    ba.dgamma, ba.dbeta, ba.accumulate = gp, bp, acc
                    pg = [self.pgrad[mod.weight], self.pgrad[mod.bias]]
                else:
                    pg = []
                rd_bn = [sl for sl, _ in st.slabs] + [mod.weight, st.mean, st.invstd, a]
                c1, c2 = self.vec(Cc), self.vec(Cc)
                self.keep.append(ba)
                if sync:
                    dmv = LateVec(2 * Cc)              # (dmean, dvar) contributions of this rank, summed over ranks
                    self._add(self.bwd, 'bn_bwd', lib.addk_bn_bwd, C.byref(ba), rd=rd_bn, wr=pg + [dmv]).payload = ba
                    self.world.emit_allreduce(self, self.bwd, dmv)
                    cit = L.BnCoeffsItem()
                    cit.c1, cit.c2, cit.count, cit.C = c1.ptr, c2.ptr, st.count, Cc
                    self._add(self.bwd, 'bn_bwd_coeffs', lib.addk_bn_bwd_coeffs, C.byref(cit), rd=[dmv], wr=[c1, c2]).payload = cit
                    dmv.binders += [lambda p, ba=ba: setattr(ba, 'dmv', p), lambda p, cit=cit: setattr(cit, 'dmv', p)]
                else:
                    ba.c1, ba.c2 = c1.ptr, c2.ptr
                    self._add(self.bwd, 'bn_bwd', lib.addk_bn_bwd, C.byref(ba), rd=rd_bn, wr=pg + [c1, c2]).payload = ba
                # dy_raw = G + c1 + c2*x, in place on the accumulated gradient
                it = L.BnApplyItem()
                it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = g.ptr, raw.ptr, c1.ptr, c2.ptr, _ptr(mu), g.ptr, raw.P
                it.ldg, it.ldx, it.ldo, it.C = g.ld, raw.ld, g.ld, Cc
                cap = self._add(self.bwd, 'bn_bwd_apply', lib.addk_bn_bwd_apply, C.byref(it), rd=[g, raw, c1, c2, mu], wr=[g])
                if Cc % 4 == 0 and Cc <= 1024 and g.ld % 4 == 0 and raw.ld % 4 == 0 and g.ptr % 16 == 0 and raw.ptr % 16 == 0:
                    cap.payload = it          # vector-aligned: may join a table
            self._bwd_emitters.append(emit_bwd)
        return act

    def conv_bn(self, srcs, conv_mod, bn_mod, relu_in, post_relu=False, out=None, **kw):
        """ReLU? -> Conv -> BN (lazy).  conv_mod/bn_mod are nn.Conv2d / nn.BatchNorm2d parameter holders."""
        k = conv_mod.kernel_size[0]
        a0 = srcs[0]
        stride, pad, dil = conv_mod.stride[0], conv_mod.padding[0], conv_mod.dilation[0]
        OH, OW = _out_hw(a0.H, a0.W, k, stride, pad, dil)
        Cout = conv_mod.out_channels
        slab = rows = None
        training = self.training and bn_mod.training
        if training:
            slab, rows = self.stats_slab(a0.N * OH * OW, Cout)
        raw = self.conv(srcs, conv_mod.weight, Cout, k, stride, pad, dil, relu_in, out=out, stats=slab, **kw)
        return self.bn(raw, bn_mod, slab, rows or 0, post_relu)

    def dwconv(self, src, conv_mod, relu_in, fwd=True):
        """Depthwise conv; returns a materialised Act.  fwd=False: only the output buffer and the backward pass (sep_half)."""
        lib = self.lib
        k = conv_mod.kernel_size[0]
        stride, pad, dil = conv_mod.stride[0], conv_mod.padding[0], conv_mod.dilation[0]
        N, H, W, Cc = src.N, src.H, src.W, src.C
        OH, OW = _out_hw(H, W, k, stride, pad, dil)
        geom = (N, H, W, OH, OW, k, k, stride, pad, dil)
        out = self.tensor(N, OH, OW, Cc)
        wptr = self.param(conv_mod.weight)
        ar = L.DwArgs()
        ar.src = self.src(src, relu_in)
        _set_geom(ar, geom)
        ar.w, ar.y, ar.ldy = wptr, out.ptr, out.ld
        self.keep.append(ar)
        if fwd:
            cdw = self._add(self.fwd, 'dw_fwd', lib.addk_dw_fwd, C.byref(ar), rd=self.lz(src) + [conv_mod.weight], wr=[out])
            self._batchable(cdw, lib.addk_dw_fwd_batch_key, ar)
        act = Act(out, None, False, self.want_grad)
        if self.want_grad:
            def emit_bwd(dy):
                ba = L.DwBwdArgs()
                ba.dy, ba.lddy = dy.ptr, dy.ld
                _set_geom(ba, geom)
                ba.src = self.src(src, relu_in)
                ba.w = wptr
                rows = lib.addk_dw_rows(N * H * W, Cc)
                gs = slab = None
                if src.needs_grad:
                    gs, ba.accumulate, slab = self._grad_into(src, rows)
                    ba.g, ba.ldg, ba.dab = gs.ptr, gs.ld, _ptr(slab)
                ws, ba.dw, ba.dw_accumulate = self._defer_dw_wreduce(conv_mod.weight, rows, Cc * k * k)
                ba.ws, ba.defer_wreduce = ws.ptr, 1
                self.keep.append(ba)
                cdb = self._add(self.bwd, 'dw_bwd', lib.addk_dw_bwd, C.byref(ba), rd=[dy, conv_mod.weight] + self.lz(src),
                                wr=[gs, slab, ws])
                self._batchable(cdb, lib.addk_dw_bwd_batch_key, ba)
            self._backward(out, emit_bwd)
        return act

    def _sep_bwd_args(self, src, dw_mod, pw_mod):
        """addk_sep_bwd arguments of one SepConv half, all but the gradients and the workspace"""
        ba = L.SepBwdArgs()
        ba.N, ba.H, ba.W, ba.K, ba.Cout, ba.ldw = src.N, src.H, src.W, dw_mod.kernel_size[0], pw_mod.out_channels, src.C
        ba.src, ba.dw_w, ba.pw_w = self.src(src, True), self.param(dw_mod.weight), self.param(pw_mod.weight)
        return ba

    def _sep_bwd(self, src, dw_mod, pw_mod, raw, t, rows):
        """Backward of one SepConv half as ONE launch (addk_sep_bwd, csrc/sepb.hip): data gradient of the pointwise conv and the
        whole depthwise backward, the gradient between them staying on chip; the pointwise WEIGHT gradient joins the deferred
        weight-gradient batches.  `rows`: the launch's workgroups (addk_sep_bwd_config)."""
        lib = self.lib
        k = dw_mod.kernel_size[0]
        N, H, W, Cc = src.N, src.H, src.W, src.C
        Cout = pw_mod.out_channels

        def emit_bwd(dy):
            # pointwise weight gradient: dW[co][ci] = sum_p dy[p][co] t[p][ci]
            self._defer_wgrad(dy, t, False, pw_mod.weight, (N, H, W, H, W, 1, 1, 1, 0, 1), Cc, Cc, 0)
            # fused data gradient + depthwise backward
            ba = self._sep_bwd_args(src, dw_mod, pw_mod)
            ba.dy, ba.lddy = dy.ptr, dy.ld
            gs = slab = None
            if src.needs_grad:
                gs, ba.accumulate, slab = self._grad_into(src, rows)
                ba.g, ba.ldg, ba.dab = gs.ptr, gs.ld, _ptr(slab)
            ws = self._defer_dw_wreduce(dw_mod.weight, rows, Cc * k * k)[0]
            ba.ws = ws.ptr
            self.keep.append(ba)
            cb = self._add(self.bwd, 'sep_bwd', lib.addk_sep_bwd, C.byref(ba), rd=[dy, dw_mod.weight, pw_mod.weight] + self.lz(src),
                           wr=[gs, slab, ws])
            self._batchable(cb, lib.addk_sep_bwd_batch_key, ba)
        self._backward(raw, emit_bwd)

    def _sep_fusable(self, dw_mod, pw_mod, sum_terms, training):
        """The halves the fused kernels are written for (ADDK_FUSE_SEP=0: none); which shapes run fused is the library's decision."""
        return (_on('ADDK_FUSE_SEP') and dw_mod.stride[0] == 1 and dw_mod.dilation[0] == 1
                and dw_mod.padding[0] == dw_mod.kernel_size[0] // 2 and pw_mod.kernel_size[0] == 1
                and (sum_terms is None or not (training or self.want_grad)))

    def sep_half(self, src, dw_mod, pw_mod, bn_mod, sum_terms=None, out=None):
        """One half of SepConv (operations.py:51-54 / 55-58): ReLU -> depthwise k x k -> pointwise 1x1 -> BN (lazy), as ONE
        launch where the fused kernel covers the shape (addk_sep_fwd, csrc/sepf.hip: the depthwise output stays on chip; in
        training it is also written out because the backward pass reads it, and the launch's last workgroup finalizes the
        BatchNorm statistics itself).  Inference only: `sum_terms` (other branches of the cell block) makes the epilogue apply
        this op's frozen BatchNorm and write the block sum (ADD.py:108) into `out`."""
        lib = self.lib
        k = dw_mod.kernel_size[0]
        N, H, W, Cc = src.N, src.H, src.W, src.C
        Cout = pw_mod.out_channels
        training = self.training and bn_mod.training
        ar = L.SepArgs()
        ar.src = self.src(src, True)
        ar.N, ar.H, ar.W, ar.K, ar.Cout, ar.ldw = N, H, W, k, Cout, Cc
        ar.dw_w, ar.pw_w = self.param(dw_mod.weight), self.param(pw_mod.weight)
        fused = self._sep_fusable(dw_mod, pw_mod, sum_terms, training)
        if fused:
            raw = out if (out is not None and sum_terms is not None) else self.tensor(N, H, W, Cout)
            ar.y, ar.ldy = raw.ptr, raw.ld
            fcfg = self._config(lib.addk_sep_fwd_config, ar)          # asked once: fused or not, the launch's workgroups
            fused = fcfg[0] == 1
        if not fused:
            t = self.dwconv(src, dw_mod, relu_in=True)
            act = self.conv_bn([t], pw_mod, bn_mod, relu_in=False)
            return act if sum_terms is None else self.affine_sum(list(sum_terms) + [act], out=out)
        t = None
        slab = rows = None
        if training:
            rows = max(fcfg[6], int(lib.addk_conv_rows(N * H * W, Cout)))
            slab = self.buf(rows * Cout * 4)
            ar.stats_rows = rows
        if self.want_grad:
            bcfg = self._config(lib.addk_sep_bwd_config, self._sep_bwd_args(src, dw_mod, pw_mod)) if _on('ADDK_FUSE_SEP_BWD') else [0]
            if bcfg[0] == 1:
                t = Act(self.tensor(N, H, W, Cc), None, False, True)           # depthwise output: written by the fused forward, read by the pointwise weight gradient
                self._sep_bwd(src, dw_mod, pw_mod, raw, t, bcfg[6])
            else:
                t = self.dwconv(src, dw_mod, relu_in=True, fwd=False)
                self.conv([t], pw_mod.weight, Cout, 1, out=raw, stats=slab, fwd=False)       # backward of the pointwise half
            ar.t, ar.ldt = t.raw.ptr, t.raw.ld
        ar.stats, ar.stats_ld = _ptr(slab), 0
        rd = self.lz(src) + [dw_mod.weight, pw_mod.weight]
        if sum_terms is not None:
            # inference: y = a*acc + b (this op's frozen BatchNorm) + the other branches, written straight into the block's slot
            st = self.bn(raw, bn_mod, None, 0).bn
            terms = [tm for tm in sum_terms if not tm.zero]
            assert len(terms) <= L.MAX_TERMS and out is not None
            ar.ea, ar.eb, ar.nterm = st.a.ptr, st.b.ptr, len(terms)
            for i, tm in enumerate(terms):
                assert (tm.N, tm.H, tm.W, tm.C) == (N, H, W, Cout), 'branch shapes differ'
                ar.term[i] = self.src(tm)
                rd += self.lz(tm)
            rd += [st.a, st.b]
        self.keep.append(ar)
        c = self._add(self.fwd, 'sep_fwd', lib.addk_sep_fwd, C.byref(ar), rd=rd, wr=[raw, slab, t.raw if t is not None else None])
        act = Act(raw, None, False, False) if sum_terms is not None else self.bn(raw, bn_mod, slab, rows or 0, fuse=(ar, c, fcfg[5]))
        self._batchable(c, lib.addk_sep_fwd_batch_key, ar)        # after bn(): the fused finalize is part of the launch's validity
        return act

    def affine_sum(self, terms, out=None, relu_out=False):
        """Materialise sum_i relu_i?(a_i*x_i+b_i) (optionally ReLU'd) into `out`."""
        lib = self.lib
        terms = [t for t in terms if not t.zero]
        t0 = terms[0]
        if out is None:
            out = self.tensor(t0.N, t0.H, t0.W, t0.C)
        assert len(terms) <= L.MAX_TERMS
        ar = L.AffineSumArgs()
        for i, t in enumerate(terms):
            assert (t.N, t.H, t.W, t.C) == (out.N, out.H, out.W, out.C), 'branch shapes differ'
            ar.term[i] = self.src(t)
        ar.nterm, ar.P, ar.C = len(terms), out.P, out.C
        ar.out, ar.ldo, ar.relu_out, ar.accumulate = out.ptr, out.ld, int(relu_out), 0
        self.keep.append(ar)
        self._add(self.fwd, 'affine_sum', lib.addk_affine_sum_fwd, C.byref(ar), rd=[r for t in terms for r in self.lz(t)], wr=[out])
        ng = self.want_grad and any(t.needs_grad for t in terms)
        act = Act(out, None, False, ng)
        if ng:
            def emit_bwd(do):
                ba = L.AffineSumBwdArgs()
                rows = lib.addk_ew_rows(out.P, out.C)
                wr_ = []
                for i, t in enumerate(terms):
                    ba.term[i] = self.src(t)
                    if t.needs_grad:
                        gt, ba.accumulate[i], slab = self._grad_into(t, rows)
                        ba.g[i], ba.ldg[i], ba.dab[i] = gt.ptr, gt.ld, _ptr(slab)
                        wr_ += [gt, slab]
                ba.nterm, ba.P, ba.C = len(terms), out.P, out.C
                ba.dout, ba.lddo = do.ptr, do.ld
                ba.out, ba.ldo, ba.relu_out = out.ptr, out.ld, int(relu_out)
                self.keep.append(ba)
                self._add(self.bwd, 'affine_sum_bwd', lib.addk_affine_sum_bwd, C.byref(ba),
                          rd=[do, out] + [r for t in terms for r in self.lz(t)], wr=wr_)
            self._backward(out, emit_bwd)
        return act

    def materialize(self, act, relu_in=False):
        if act.bn is None and not (act.relu or relu_in):
            return act
        a = Act(act.raw, act.bn, act.relu or relu_in, act.needs_grad, rs=act.rs)
        return self.affine_sum([a])

    def _rs_args(self, cls, src, OH, OW, relu_in=False):
        """A ResizeArgs / ResizeBwdArgs with the prefix the two share filled in: the source and the two grids."""
        a = cls()
        a.src = self.src(src, relu_in)
        a.N, a.H, a.W, a.OH, a.OW = src.N, src.H, src.W, OH, OW
        return a

    def resize(self, src, OH, OW, relu_in=False):
        """Bilinear resize.  A lazy BN without pending ReLU passes through (affine commutes with
        interpolation); a pending ReLU forces materialisation."""
        lib = self.lib
        relu = bool(src.relu or relu_in)
        N, H, W, Cc = src.N, src.H, src.W, src.C
        out = self.tensor(N, OH, OW, Cc)
        carrier = src if relu else Act(src.raw, None, False, src.needs_grad, rs=src.rs)
        ar = self._rs_args(L.ResizeArgs, carrier, OH, OW, relu_in)
        ar.y, ar.ldy, ar.nchw_out = out.ptr, out.ld, 0
        self.keep.append(ar)
        tag = self.tag

        def emit_fwd():
            c = self._add(self.fwd, 'resize_fwd', lib.addk_resize_fwd, C.byref(ar), rd=self.lz(carrier), wr=[out])
            c.tag = tag
            if rs is not None:
                rs.done = True
        rs = None
        if relu or self._pending(src) or src.raw.H >= (1 << 15) or src.raw.W >= (1 << 16):
            emit_fwd()                    # the interpolated values are relu(a x + b): not an affine of the interpolated raw map
        else:
            rs = Resample(src.raw, emit_fwd)      # deferred: a 1x1 consumer samples src.raw itself (Graph.conv), anyone else emits it
        res = Act(out, None if relu else src.bn, False, src.needs_grad, rs=rs)
        if self.want_grad and src.needs_grad:
            def emit_bwd(dy):
                ba = self._rs_args(L.ResizeBwdArgs, carrier, OH, OW, relu_in)
                ba.dy, ba.lddy, ba.nchw_in = dy.ptr, dy.ld, 0
                # without a pending ReLU the BatchNorm passed through the interpolation: its (dA,dB) come from the consumers of `res`
                gs, ba.accumulate, slab = self._grad_into(src, lib.addk_ew_rows(N * H * W, Cc) if relu else None)
                ba.g, ba.ldg, ba.dab = gs.ptr, gs.ld, _ptr(slab)
                self.keep.append(ba)
                crb = self._add(self.bwd, 'resize_bwd', lib.addk_resize_bwd, C.byref(ba), rd=[dy] + self.lz(src), wr=[gs, slab])
                if _on('ADDK_BATCH_RESIZE_BWD'):
                    self._batchable(crb, lib.addk_resize_bwd_batch_key, ba)
            self._backward(out, emit_bwd)
        return res

    def resize_to_nchw(self, src, OH, OW):
        """Final logits resize (decoder.py:28).  Returns an OutRef.  The plan chooses who consumes the low-resolution logits (heads.py:
        HEADS names the heads, heads.logits_head says which one takes this output, the gate of an early exit among them), or nobody: the
        resize into a contiguous [N,C,OH,OW] tensor, and its backward."""
        from . import heads                      # here, not at the top: heads.py imports from this module
        assert src.bn is None and not src.relu and (self.head is None or self.head in heads.HEADS)
        out = heads.logits_head(self, src, OH, OW)
        if out is not None:
            return out
        y, emit_resize = heads._logits_resize(self, src, OH, OW)
        emit_resize()
        out = OutRef(y)
        if self.want_grad and src.needs_grad:
            def emit_bwd():
                if out.dy_ptr is None and not out.dynamic:
                    return
                ba = self._rs_args(L.ResizeBwdArgs, src, OH, OW)
                ba.dy, ba.lddy, ba.nchw_in, ba.dy_scale = out.dy_ptr, 0, 1, out.dy_scale
                gs, ba.accumulate, _ = self._grad_into(src)
                ba.g, ba.ldg = gs.ptr, gs.ld
                self.keep.append(ba)
                out.bwd_args = ba
                self._add(self.bwd, 'resize_nchw_bwd', self.lib.addk_resize_bwd, C.byref(ba), rd=self.lz(src), wr=[gs])
            self._bwd_emitters.append(emit_bwd)
        return out

    def gap(self, src, relu_in=False):
        lib = self.lib
        N, H, W, Cc = src.N, src.H, src.W, src.C
        out = self.tensor(N, 1, 1, Cc)
        s = self.src(src, relu_in)
        rows = lib.addk_ew_rows(H * W, Cc)
        ws = self.buf(N * rows * Cc)
        self.keep.append(s)
        self._add(self.fwd, 'gap_fwd', lib.addk_gap_fwd, C.byref(s), N, H * W, out.ptr, out.ld, ws.ptr, 1, rd=self.lz(src), wr=[out, ws])
        act = Act(out, None, False, self.want_grad and src.needs_grad)
        if act.needs_grad:
            def emit_bwd(dy):
                gs, acc, slab = self._grad_into(src, lib.addk_ew_rows(N * H * W, Cc))
                self._add(self.bwd, 'gap_bwd', lib.addk_gap_bwd, C.byref(s), N, H * W, dy.ptr, dy.ld, gs.ptr, gs.ld, acc,
                          _ptr(slab), rd=[dy] + self.lz(src), wr=[gs, slab])
            self._backward(out, emit_bwd)
        return act

    def edm_head(self, src, conv_w, lins, host_out=None):
        """The whole Earlier-Decision-Maker head (ADD.py:502-525) as ONE launch (csrc/edm.hip): in-place ReLU, conv 3x3 stride 2 -> 128,
        ReLU, global average pool, the three Linear layers.  Inference only.  `host_out`: pinned host tensor the confidence is also
        written to (the gate of dynamic_inference reads it there: no device-to-host copy).  Returns the [N,1,1,1] Act, or None when the
        kernel does not cover the arguments (the caller then emits the generic launches)."""
        lib = self.lib
        if self.want_grad or not _on('ADDK_FUSE_EDM'):
            return None
        N, H, W = src.N, src.H, src.W
        ar = L.EdmArgs()
        ar.src = self.src(src, True)
        ar.N, ar.H, ar.W = N, H, W
        ar.conv_w = self.param(conv_w)
        (l1, l2, l3) = lins
        ar.w1, ar.b1, ar.w2, ar.b2, ar.w3, ar.b3 = (self.param(l1.weight), self.param(l1.bias), self.param(l2.weight), self.param(l2.bias),
                                                    self.param(l3.weight), self.param(l3.bias))
        out = self.tensor(N, 1, 1, 1)
        ws = self.buf((int(lib.addk_edm_head_ws_bytes(N, H, W)) + 3) // 4, zero=True)
        ar.out, ar.ldo, ar.ws = out.ptr, out.ld, ws.ptr
        ar.out_host = host_out.data_ptr() if host_out is not None else None
        shapes_ok = (tuple(conv_w.shape[:1]) == (128,) and conv_w.numel() == 128 * 9 * src.C and tuple(l1.weight.shape) == (64, 128)
                     and tuple(l2.weight.shape) == (32, 64) and tuple(l3.weight.shape) == (1, 32))
        if not shapes_ok or int(lib.addk_edm_head_supported(C.byref(ar))) != 1:
            return None
        self.keep += [ar, host_out]
        self._add(self.fwd, 'edm_head', lib.addk_edm_head, C.byref(ar),
                  rd=self.lz(src) + [conv_w, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias], wr=[out, ws])
        return Act(out, None, False, False)

    def pool3(self, src, stride, mode):
        lib = self.lib
        N, H, W, Cc = src.N, src.H, src.W, src.C
        OH, OW = _out_hw(H, W, 3, stride, 1, 1)
        out = self.tensor(N, OH, OW, Cc)
        s = self.src(src)
        self.keep.append(s)
        self._add(self.fwd, 'pool3_fwd', lib.addk_pool3_fwd, C.byref(s), N, H, W, OH, OW, stride, mode, out.ptr, out.ld,
                  rd=self.lz(src), wr=[out])
        act = Act(out, None, False, self.want_grad and src.needs_grad)
        if act.needs_grad:
            assert src.bn is None or not src.bn.training, 'pool3 backward through a lazy training BN is not built (cold path)'

            def emit_bwd(dy):
                gs, acc, _ = self._grad_into(src)
                self._add(self.bwd, 'pool3_bwd', lib.addk_pool3_bwd, C.byref(s), N, H, W, OH, OW, stride, mode, dy.ptr, dy.ld,
                          gs.ptr, gs.ld, acc, rd=[dy] + self.lz(src), wr=[gs])
            self._backward(out, emit_bwd)
        return act

    def zeros(self, N, H, W, Cc):
        t = TRef(self.buf(N * H * W * Cc, zero=True), 0, N, H, W, Cc, Cc)
        return Act(t, None, False, False, zero=True)

    def input_nchw(self, x, requires_grad=False, ld=None):
        """Stage an NCHW torch tensor into the plan.  Returns (Act, InRef)."""
        lib = self.lib
        N, Cc, H, W = x.shape
        t = self.tensor(N, H, W, Cc, ld)
        inref = InRef(tuple(x.shape))
        self._add(self.fwd, 'nchw_to_nhwc', _in_stage, lib, inref, N, Cc, H * W, t.ptr, t.ld, wr=[t])
        act = Act(t, None, False, requires_grad and self.want_grad)
        if act.needs_grad:
            gx = torch.empty((N, Cc, H, W), dtype=torch.float32, device=self.device)
            inref.grad = gx

            def emit_bwd():
                if not self.grad_ready(t):
                    inref.grad = None
                    return
                g = self.grad(t)
                s = L.Src(); s.x, s.ld, s.C = g.ptr, g.ld, g.C
                self.keep.append(s)
                self._add(self.bwd, 'in_grad_to_nchw', lib.addk_nhwc_to_nchw, C.byref(s), N, H * W, gx.data_ptr(), rd=[g], wr=[gx])
            self._bwd_emitters.append(emit_bwd)
        return act, inref

    def output_nchw(self, act):
        """Materialise `act` (incl. its lazy BN/ReLU) as a contiguous NCHW tensor."""
        lib = self.lib
        N, H, W, Cc = act.N, act.H, act.W, act.C
        y = torch.empty((N, Cc, H, W), dtype=torch.float32, device=self.device)
        s = self.src(act)
        self.keep.append(s)
        self._add(self.fwd, 'nhwc_to_nchw', lib.addk_nhwc_to_nchw, C.byref(s), N, H * W, y.data_ptr(), rd=self.lz(act), wr=[y])
        out = OutRef(y)
        if self.want_grad and act.needs_grad:
            def emit_bwd():
                gs, acc, slab = self._grad_into(act, lib.addk_ew_rows(N * H * W, Cc))
                out.bwd_cmd = self._add(self.bwd, 'out_grad', lib.addk_nchw_grad_to_nhwc, None, C.byref(s), N, H * W, gs.ptr, gs.ld,
                                        acc, _ptr(slab), rd=self.lz(act), wr=[gs, slab])
            self._bwd_emitters.append(emit_bwd)
        return out


def require_device(x):
    """The product path is HIP-only: no CPU fallback exists (tests use oracle/ as the CPU checker)."""
    if not x.is_cuda:
        raise L.AddkError('addk runs on the MI355X HIP path only: got a tensor on %s.  There is no CPU fallback.' % x.device)


def current_stream():
    return torch.cuda.current_stream().cuda_stream


def _in_stage(lib, inref, N, Cc, HW, ptr, ld, stream):
    return lib.addk_nchw_to_nhwc(inref.ptr, N, Cc, HW, ptr, ld, stream)


class InRef:
    """Per-call input binding (pointer patched before each replay)."""

    def __init__(self, shape):
        self.shape, self.ptr, self.grad, self.keep = shape, None, None, None

    def bind(self, x):
        assert tuple(x.shape) == self.shape and x.dtype == torch.float32, 'input changed shape/dtype'
        require_device(x)
        x = x.contiguous()
        self.keep, self.ptr = x, x.data_ptr()


class OutRef:
    """A plan output: tensor + how its incoming gradient pointer is patched per backward call."""

    def __init__(self, y):
        self.y = y               # [N,C,OH,OW] logits; None where a head consumes the low-resolution logits instead; the uint8 [N,OH,OW] map of a label head
        self.dy_ptr, self.dy_scale, self.dynamic = None, None, True
        self.bwd_args = None     # ResizeBwdArgs (logits path)
        self.bwd_cmd = None      # generic nhwc path
        self.shape = None        # (N, C, OH, OW) of the logits a fused head stands for (y is None)
        self.head = None         # Graph.head of the head that consumed the logits; None: y is the real logits.  'labels': y is the label map
        self.src = None          # 'views', 'tiles', 'ce': the lazy activation of the decoder's low-resolution logits this output stands for
        # what the step binds to a 'ce' / 'score' / 'profile' head before finalize() — 'ce': target, class_w, ignore_index, wsum, scale, loss;
        # 'score': those + entropy, confusion, pred; 'profile': target, thr, nthr, entropy, share, confusion, pred and optionally temp (the
        # device word 1 / temperature: the tempered launch); 'views': N, views; 'calib': target, inv_temp, nt, bins, nll
        self.binding = None
        self.gate_out = None     # [N,2] device tensor of a gated exit: (entropy, share of pixels above the threshold)
        self.gate_scale = 1.0    # factor the host applies to gate_out[:, 0] (the stand-alone entropy kernel leaves a sum)
        self.gate_fused = False  # the gate launch writes the pinned host words itself; else the host copies gate_out
        self.gate_cut = None     # index in the forward list behind the gate: what follows runs only for an image that leaves here

    def set_grad(self, gy):
        gy = gy.contiguous()
        if self.bwd_args is not None:
            self.bwd_args.dy = gy.data_ptr()
        elif self.bwd_cmd is not None:
            self.bwd_cmd.args[0] = gy.data_ptr()
        return gy


class NbtCounter:
    """All `num_batches_tracked` counters of a plan live in ONE int64 tensor (each module's buffer is a 0-dim view
    of it), so a forward bumps them with a single add instead of one tiny launch per BatchNorm."""

    def __init__(self, nbt):
        self.mods = list(nbt)
        self.counts = [int(nbt[m]) for m in self.mods]
        self.flat = self.inc = None

    def _flatten(self):
        dev = self.mods[0].num_batches_tracked.device
        self.flat = torch.stack([m.num_batches_tracked.detach().reshape(()) for m in self.mods]).to(torch.int64)
        for i, m in enumerate(self.mods):
            m._buffers['num_batches_tracked'] = self.flat[i]
        self.inc = torch.tensor(self.counts, dtype=torch.int64, device=dev)

    def bump(self):
        if not self.mods:
            return
        m0 = self.mods[0].num_batches_tracked
        if self.flat is None or m0.data_ptr() != self.flat.data_ptr() or self.mods[-1].num_batches_tracked.data_ptr() != self.flat[-1].data_ptr():
            self._flatten()          # first use, or another plan / .to() re-pointed the buffers
        self.flat.add_(self.inc)
