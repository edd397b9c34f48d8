#!/usr/bin/env python
"""Fingerprints of the dry-built launch plans, for refactors of the planner (plan.py, heads.py, parallel.py, dynamic.py): a change that is
not meant to change a plan must leave every fingerprint as it is.  No GPU: launches are stubbed the way tests/test_plan_dryrun.py
and tests/test_sep_dispatch.py do it.

Per plan and per launch list the ordered records of every command are hashed: name, tag, tags, members, stream, waits, whether it
records an event, batch key, payload, the read / write regions and every argument.  Memory is made address-independent by what each
value is DECLARED to be, never by what its bytes look like:
  - a ctypes Structure or Array (argument struct, payload, meta array) is walked by its `_fields_`: a pointer field becomes
    Memory.word(value) = (ordinal of the known allocation it lies in, byte offset), everything else is the bytes it occupies.  A
    non-null pointer in no known allocation is an error that names plan, list, command and field: it would tie the hash to the process;
  - a positional integer argument goes through Memory.word too (a size never reaches the 2^40 and more of an address);
  - a device table is recorded as ('table', byte length, typed hash of Cmd.table), the array of argument structs the planner made
    it from.  Where the library turns that array into a blob of kernel descriptors and work lists (`*_batch_prepare`) the blob's
    bytes are NOT hashed: they are a pure function of the array, the precision mode and the library, and that side is pinned by
    tests/test_conv_dispatch.py, test_sep_dispatch.py, test_pw_dispatch.py and the *_bits fixtures.  The meta array of such a launch
    (kind, tile configuration, count, offsets, block counts: no pointer) stays in the record as bytes;
  - a region is named by the plan (sched._region): ('buf', n) is recorded as ('a', n), a LateVec as ('id', k) with k counted inside
    the plan in first-seen order, the storage of a tensor as its allocation and offset.
Known allocations are the plan's buffers in creation order, then the parameters, the plan-owned gradients, the kept tensors and the
tensors of the plan's front end (inputs, outputs, loss scalars, module buffers) in first-seen order.  Also recorded: nbytes, the
number and sizes of the buffers, the number of hoisted weight packs.

Until the fixture was re-recorded for this rule the tool scanned every struct and blob for 8-byte-aligned words that fell inside a
known allocation.  The blob of addk_conv_wgrad_batch_prepare ends in int4 work lists whose entries (i, e, flag, 0) read as the word
e << 32 | i, e.g. 0x0000554000000002: about once in six processes the address space put an allocation over such a value, data was
rewritten as (allocation, offset), and the `bwd` lists of the training plans compared unequal although the planner had made the
same plan.  tests/test_plan_fingerprint.py keeps that case as a unit test of the walk.

    python tests/tools/plan_fingerprint.py                 # writes tests/golden/plan_fingerprint.json (run it on the commit to pin)
    python tests/tools/plan_fingerprint.py --check         # compares with the fixture, exit status 1 on a difference
    python tests/tools/plan_fingerprint.py --dump DIR      # also writes every record as text, one file per list (to diff two commits)

tests/test_plan_fingerprint.py calls fingerprints() and compares with the fixture.  Every struct the planner fills is a ctypes
object (zero-initialised), so no byte needs masking: two runs of this tool in different processes give equal hashes."""
import argparse
import bisect
import collections
import ctypes as C
import gc
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(ROOT, 'tests', 'golden', 'plan_fingerprint.json')

ENVS = (('default', {}), ('no_level_batch', {'ADDK_LEVEL_BATCH': '0'}))
_BYREF = type(C.byref(C.c_int()))


class Memory:
    """The known allocations of one plan; `word(v)` makes a value that is declared an address (or a positional integer) address-independent."""

    def __init__(self):
        self.starts, self.ends, self.ords = [], [], []
        self.n = 0
        self.tables = {}          # data_ptr of a kept uint8 table -> tensor
        self.late = {}            # serial of a plan.LateVec -> its number among those of this plan, first seen

    def add(self, base, nbytes):
        o = self.n
        self.n += 1
        if nbytes <= 0:
            return o
        i = bisect.bisect_right(self.starts, base)
        if (i > 0 and self.ends[i - 1] > base) or (i < len(self.starts) and self.starts[i] < base + nbytes):
            return o              # inside / across an earlier allocation (a view of a flat buffer): the earlier one names these bytes
        self.starts.insert(i, base); self.ends.insert(i, base + nbytes); self.ords.insert(i, o)
        return o

    def add_tensor(self, t):
        if isinstance(t, torch.Tensor) and t.numel():
            self.add(t.data_ptr(), t.numel() * t.element_size())

    def word(self, v):
        i = bisect.bisect_right(self.starts, v) - 1
        if i >= 0 and v < self.ends[i]:
            return ('@', self.ords[i], v - self.starts[i])
        return v

    def name(self, key):
        """The name of a region (sched._region) in the record: the buffer's ordinal, the LateVec's number inside this plan, the
        tensor's allocation and the offset of its storage in it."""
        kind, v = key
        if kind == 'buf':
            return ('a', v)           # the buffers are the first allocations (_memory): ordinal in the plan = ordinal here
        if kind == 'late':
            return ('id', self.late.setdefault(v, len(self.late)))
        w = self.word(v) if kind == 'mem' else v
        if w == v:
            raise UnknownPointer('region %r lies in no known allocation' % (key,))
        return w


class UnknownPointer(ValueError):
    """A non-null pointer field that lies in no known allocation: its value, and so the hash, would depend on the process."""


_POINTERS = (C.c_void_p, C.c_char_p, C.c_wchar_p, C._Pointer, C._CFuncPtr)
_has_ptr = {}


def _holds_pointers(ct):
    if ct not in _has_ptr:
        _has_ptr[ct] = (issubclass(ct, _POINTERS) or (issubclass(ct, C.Array) and _holds_pointers(ct._type_)) or
                        (issubclass(ct, (C.Structure, C.Union)) and any(_holds_pointers(f[1]) for f in ct._fields_)))
    return _has_ptr[ct]


def _walk(mem, ct, raw, base, path, out):
    """The bytes raw[base:] of an object of ctypes type `ct`, appended to `out` field by field: a pointer as Memory.word(value),
    everything else as the bytes it occupies."""
    if not _holds_pointers(ct):
        out.append(raw[base:base + C.sizeof(ct)])
    elif issubclass(ct, C.Structure):
        for f in ct._fields_:
            _walk(mem, f[1], raw, base + getattr(ct, f[0]).offset, '%s.%s' % (path, f[0]), out)
    elif issubclass(ct, C.Array):
        for i in range(ct._length_):
            _walk(mem, ct._type_, raw, base + i * C.sizeof(ct._type_), '%s[%d]' % (path, i), out)
    elif issubclass(ct, _POINTERS):
        v = int.from_bytes(raw[base:base + C.sizeof(ct)], sys.byteorder)
        w = mem.word(v)
        if v and w == v:
            raise UnknownPointer('%s = %#x lies in no known allocation' % (path, v))
        out.append(w)
    else:
        raise TypeError('%s: %s' % (path, ct))


def typed(mem, obj, path=''):
    """sha256 over a ctypes Structure / Array, or a list of them, walked by its declared fields (_walk)"""
    out = []
    for i, o in enumerate(obj) if isinstance(obj, (list, tuple)) else ((None, obj),):
        _walk(mem, type(o), bytes(o), 0, '%s%s' % (path or type(o).__name__, '' if i is None else '[%d]' % i), out)
    return hashlib.sha256(repr(out).encode()).hexdigest()


def _arg(mem, a, P, table=None):
    if a is None or isinstance(a, (float, str)):
        return a
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, int):
        if table is not None and a in mem.tables:             # the device table of this command: its typed source (Cmd.table), not its address
            return ('table', mem.tables[a].numel(), typed(mem, table, 'table'))
        return mem.word(a)
    if isinstance(a, _BYREF):
        a = a._obj
    if isinstance(a, (C.Structure, C.Array)):
        return (type(a).__name__, typed(mem, a))
    if isinstance(a, torch.Tensor):
        return ('tensor', mem.word(a.data_ptr()), tuple(a.shape), str(a.dtype))
    if isinstance(a, P.LateVec):
        return ('late', a.n, a.f64, mem.word(a.ptr) if a.buf is not None else None)
    if isinstance(a, P.InRef):
        return ('inref', tuple(a.shape))
    return type(a).__name__


def _records(mem, lst, P, where=''):
    out = []
    for i, c in enumerate(lst):
        reg = lambda rs: [(mem.name(k[0]), k[1], k[2]) for k in rs]      # noqa: E731
        pay = c.payload
        try:
            args = [_arg(mem, a, P, c.table) for a in c.args]
            assert c.table is None or any(isinstance(a, tuple) and a[0] == 'table' for a in args), 'Cmd.table without a table argument'
            out.append((c.name, c.tag, sorted(c.tags) if c.tags is not None else None, c.members, c.stream, tuple(c.waits), c.event is not None,
                        c.bkey, type(pay).__name__, _arg(mem, pay, P) if isinstance(pay, (C.Structure, P.LateVec)) else None,
                        reg(c.rd), reg(c.wr), args))
        except UnknownPointer as e:
            raise UnknownPointer('%s, command %d (%s): %s' % (where, i, c.name, e)) from None
    return out


def _memory(g, extra):
    mem = Memory()
    for b in g._bufs:
        mem.add(b.ptr, 4 * max(b.n, 4))
    for p in g.params:
        mem.add_tensor(p)
    for p in g.params:
        mem.add_tensor(g.pgrad.get(p))
    for t in g.keep:
        if isinstance(t, torch.Tensor):
            mem.add_tensor(t)
            if t.dtype == torch.uint8:
                mem.tables[t.data_ptr()] = t
    for t in extra:
        mem.add_tensor(t)
    return mem


def _fingerprint(g, lists, extra, dump, label):
    import addk.plan as P
    mem = _memory(g, extra)
    res = {'nbytes': int(g.nbytes), 'bufs': len(g._bufs), 'buf_sizes': hashlib.sha256(repr([b.n for b in g._bufs]).encode()).hexdigest(),
           'packs': len(g._packs), 'lists': {}}
    for name, lst in lists:
        recs = _records(mem, lst, P, '%s/%s' % (label, name))
        text = '\n'.join(repr(r) for r in recs)
        res['lists'][name] = {'sha256': hashlib.sha256(text.encode()).hexdigest(), 'commands': len(recs),
                              'names': dict(sorted(collections.Counter(c.name for c in lst).items()))}
        if dump:
            with open(os.path.join(dump, '%s.%s.txt' % (label.replace('/', '.'), name)), 'w') as f:
                f.write(text + '\n')
    return res


# ---------------------------------------------------------------- the plans
def _model(F, sync=False, train=True, classes=19):
    from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, make_args
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F, sync_bn=sync), ARCH_C2['low_level_layer'])
    return m.train(train)


def _tensors(*objs):
    """every tensor an object of the plan's front end holds (one level of attributes, lists, dicts)"""
    out = []
    for o in objs:
        vals = list(vars(o).values()) if hasattr(o, '__dict__') else [o]
        for v in vals:
            for t in (v if isinstance(v, (list, tuple)) else v.values() if isinstance(v, dict) else [v]):
                if isinstance(t, torch.Tensor):
                    out.append(t)
                elif hasattr(t, 'y') and isinstance(getattr(t, 'y'), torch.Tensor):     # OutRef
                    out.append(t.y)
    return out


def _train_step(F, shape, sync=False, **kw):
    """the fused train step as bench.py builds it (flat gradient views, fused up-sampling + loss); `kw`: ohem=, distill=, dice="""
    import addk.train as T
    comm = None
    if sync:                       # the forced exchange at world 1 without a process group: arena binding, packed all-reduces, gradient buckets
        from addk import parallel
        comm = object.__new__(parallel.SyncBNComm)
        comm.group, comm.force, comm.size, comm.rank, comm.calls, comm.log, comm.small, comm._small_tried = None, True, 1, 0, 0, None, None, True
    m = _model(F, sync)
    ts = T.TrainStep(m, shape, sync_comm=comm, use_graph=False, nstreams=2, **kw)
    g = ts.g
    extra = _tensors(ts, ts.inref, *ts.outs) + list(m.buffers())
    return g, [('fwd', g.fwd), ('bwd', g.bwd)], extra, (ts, m)


def _module_plan(F, shape, train):
    """the nn.Module front end: model(x) (and loss.backward() in training) builds the plan"""
    m = _model(F, train=train)
    with torch.set_grad_enabled(train):
        m(torch.empty(*shape))
    plan = next(iter(m._plans().values()))
    g = plan.g
    extra = _tensors(*[o for _, o in plan.outs if not isinstance(o, int)], *plan.inrefs) + list(m.buffers())
    return g, [('fwd', g.fwd), ('bwd', g.bwd)], extra, (plan, m)


def _dynamic(F, shape, *mode):
    """the gated inference plan and every segment it replays (trunk to the gate, early head, remainder); `mode`: ('labels', table bytes
    or None) for the label-map form"""
    from addk.modeling.ADD import EDM
    m = _model(F, train=False)
    edm = EDM().eval()
    x = torch.empty(*shape)
    plan = m._dynamic_plan(x, edm, *mode)
    segs = [(0, plan.trunk_end[0]), plan.head_rng[0], (plan.head_rng[0][1], -1)]
    with torch.no_grad():
        for i0, i1 in segs:
            plan._seg(i0, i1)
    g = plan.g
    lists = [('fwd', g.fwd)] + [('seg%d' % k, plan.segs[(i0, i1 if i1 >= 0 else len(g.fwd))]) for k, (i0, i1) in enumerate(segs)]
    extra = _tensors(plan, plan.inref, *plan.conf, *plan.heads, plan.final) + list(m.buffers()) + list(edm.buffers())
    return g, lists, extra, (plan, m, edm)


def _validation(F, shape, classes=19, **kw):
    """the validation pass: one scoring head per exit (7 classes: the stand-alone kernels inside the plan), class weights and maps;
    `kw`: trimap= in place of the kept maps"""
    from addk.validate import ValidationStep
    m = _model(F, classes=classes)
    vs = ValidationStep(m, shape, class_weight=torch.ones(classes), use_graph=False, nstreams=2, **(kw or dict(keep_predictions=True)))
    g = vs.g
    extra = _tensors(vs, vs.inref) + list(m.buffers())
    return g, [('fwd', g.fwd)], extra, (vs, m)


def _exit_profile(F, shape, **kw):
    """the exit profile: one profile_upsample per exit, three top-probability thresholds, prediction maps; `kw`: temperature=, trimap=
    in place of the kept maps"""
    from addk.exit_profile import ExitProfile
    m = _model(F)
    prof = ExitProfile(m, shape, max_thresholds=(0.5, 0.9, 0.99), use_graph=False, nstreams=2, **(kw or dict(keep_predictions=True)))
    g = prof.g
    extra = _tensors(prof, prof.inref) + list(m.buffers())
    return g, [('fwd', g.fwd)], extra, (prof, m)


def _calibration(F, shape):
    """the calibration pass: one calib_upsample per exit, the default ladder of temperatures"""
    from addk.calibrate import ExitCalibration
    m = _model(F)
    cal = ExitCalibration(m, shape, use_graph=False, nstreams=2)
    g = cal.g
    extra = _tensors(cal, cal.inref) + list(m.buffers())
    return g, [('fwd', g.fwd)], extra, (cal, m)


def _segmenter(F, shape, exit=-1, lut=None, classes=19):
    """static label-map inference of one exit: the trunk up to that exit's cell and one label_upsample (7 classes: the stand-alone
    kernels and the cast in torch ops)"""
    from addk.segment import Segmenter
    m = _model(F, classes=classes)
    seg = Segmenter(m, shape, exit=exit, label_lut=lut, use_graph=False, nstreams=2)
    g = seg.g
    extra = _tensors(seg, seg.inref) + list(m.buffers())
    return g, [('fwd', g.fwd)], extra, (seg, m)


def _multi_view(F, shape):
    """multi-scale + flip label-map inference: the trunk once per scale and one label_views_upsample"""
    from addk.segment import MultiViewSegmenter
    m = _model(F)
    seg = MultiViewSegmenter(m, shape, use_graph=False, nstreams=2)
    g = seg.g
    extra = _tensors(seg, seg.inref) + [g.view_labels] + list(m.buffers())
    return g, [('fwd', g.fwd)], extra, (seg, m)


def _gate(F, shape, kind, env=None, mode=(), temperature=None):
    """dynamic inference gated by entropy / top-probability share, and the segments it replays (trunk + head + gate, resize, remainder);
    `mode` as in _dynamic; `temperature`: the tempered plan, that value at every exit"""
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        m = _model(F, train=False)
        plan = m._gate_plan(torch.empty(*shape), kind, *mode, temperature=temperature and [temperature] * m.num_exits())
        segs = [(0, plan.head_rng[0][0]), plan.head_rng[0], (plan.head_rng[0][1], -1)]
        segs = [s for s in segs if s[0] != s[1]]              # the stand-alone form leaves nothing behind the cut
        with torch.no_grad():
            for i0, i1 in segs:
                plan._seg(i0, i1)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    g = plan.g
    lists = [('fwd', g.fwd)] + [('seg%d' % k, plan.segs[(i0, i1 if i1 >= 0 else len(g.fwd))]) for k, (i0, i1) in enumerate(segs)]
    extra = _tensors(plan, plan.inref, *plan.heads, plan.final) + list(m.buffers())
    return g, lists, extra, (plan, m)


def _batched_gate(F, shape, kind, n):
    """the sub-plan of a BatchedGate at live batch `n`: the gate plan with label heads, its pinned words covering every image"""
    from addk.dynamic import BatchedGate
    m = _model(F, train=False)
    bg = BatchedGate(m, shape, kind)
    plan = bg.sub(n)
    g = plan.g
    extra = _tensors(plan, plan.inref, *plan.heads, plan.final) + list(m.buffers())
    return g, [('fwd', g.fwd)], extra, (bg, m)


def _tiled(F, tile, stride, **kw):
    """sliding-window label maps: the tile plan of a TiledSegmenter; with `threshold=` the gated tile plan (TileGatePlan), its launch
    list and every stage segment it replays (TileGatePlan.stage).  The known tensors are named one by one, so that no attribute the
    front end gains or loses moves an ordinal."""
    from addk.segment import TiledSegmenter
    m = _model(F, train=False)
    seg = TiledSegmenter(m, tile, stride, use_graph=False, nstreams=2, **kw)
    g = seg.g
    lists, extra = [('fwd', g.fwd)], [seg.x]
    if seg.threshold is None:
        extra += _tensors(seg.inref, seg.out)
    else:
        plan = seg.plan
        with torch.no_grad():
            for k in range(seg.gates + 1):
                i0, i1 = plan.stage(k)
                plan._seg(i0, i1)
                lists.append(('stage%d' % k, plan.segs[(i0, i1 if i1 >= 0 else len(g.fwd))]))
        extra += [plan.ext, plan._thr, plan._temp] + _tensors(plan.inref, *plan.outs)
        for _, pool, pext in plan.pools:
            extra += list(pool) + [pext]
    return g, lists, extra + list(m.buffers()), (seg, m)


TILE, TILE_STRIDE = (3, 3, 65, 129), (32, 71)            # what the tile dry tests use (tests/test_tile_gate_plan.py)

PLANS = (
    ('c2_train_step', lambda: _train_step(20, (2, 3, 1024, 2048))),          # the flagship: config 2, F = 20, want_grad
    ('c2_inference', lambda: _module_plan(20, (1, 3, 1024, 2048), False)),
    ('c2_module_train', lambda: _module_plan(4, (2, 3, 65, 129), True)),      # autograd front end: logits resize and its backward as launches
    ('f40_train_step', lambda: _train_step(40, (2, 3, 1024, 2048))),
    ('syncbn_forced_train_step', lambda: _train_step(4, (2, 3, 65, 129), sync=True)),
    ('dynamic_segments', lambda: _dynamic(20, (1, 3, 65, 129))),
    ('validation_step', lambda: _validation(4, (2, 3, 65, 129))),             # the scoring head: one score_upsample per exit
    ('validation_7_classes', lambda: _validation(4, (1, 3, 33, 65), 7)),      # addk_score_upsample_supported == 0: the stand-alone kernels
    ('gate_entropy', lambda: _gate(20, (1, 3, 65, 129), 'entropy')),          # the exit gate: gate_upsample, then the resize behind the cut
    ('gate_max', lambda: _gate(20, (1, 3, 65, 129), 'max')),
    ('gate_entropy_unfused', lambda: _gate(20, (1, 3, 65, 129), 'entropy', {'ADDK_FUSE_GATE': '0'})),
    ('gate_max_unfused', lambda: _gate(20, (1, 3, 65, 129), 'max', {'ADDK_FUSE_GATE': '0'})),
    ('exit_profile', lambda: _exit_profile(4, (2, 3, 65, 129))),
    ('segmenter_final_lut', lambda: _segmenter(4, (2, 3, 65, 129), -1, torch.arange(255, -1, -1, dtype=torch.uint8))),
    ('segmenter_exit0', lambda: _segmenter(4, (2, 3, 65, 129), 0)),            # the trunk stops at the first exit
    ('dynamic_labels', lambda: _dynamic(20, (1, 3, 65, 129), 'labels', None)),
    ('gate_entropy_labels', lambda: _gate(20, (1, 3, 65, 129), 'entropy', mode=('labels', None))),     # gate_label_upsample, nothing behind the cut
    ('gate_max_labels_unfused', lambda: _gate(20, (1, 3, 65, 129), 'max', {'ADDK_FUSE_GATE': '0'}, ('labels', None))),   # _labels_cold behind the cut
    ('train_step_ohem', lambda: _train_step(4, (2, 3, 65, 129), ohem=(0.7, 1000))),                     # ohem_select + ce_upsample_ohem per exit
    ('train_step_distill', lambda: _train_step(4, (2, 3, 65, 129), distill=(0.5, 2.0))),                # ce_upsample_kd for the students
    ('train_step_distill_ohem', lambda: _train_step(4, (2, 3, 65, 129), ohem=(0.7, 1000), distill=(0.5, 2.0))),
    ('multi_view_segmenter', lambda: _multi_view(4, (2, 3, 65, 129))),                                  # default scales and flip: label_views_upsample
    ('gate_entropy_tempered', lambda: _gate(20, (1, 3, 65, 129), 'entropy', temperature=1.5)),          # gate_upsample_t, then the resize behind the cut
    ('gate_max_labels_tempered', lambda: _gate(20, (1, 3, 65, 129), 'max', mode=('labels', None), temperature=1.5)),   # gate_upsample_t writes the map
    ('calibration', lambda: _calibration(4, (2, 3, 65, 129))),                                          # one calib_upsample per exit
    ('validation_trimap', lambda: _validation(4, (2, 3, 65, 129), trimap=(1, 3, 8))),                   # score_upsample + confusion_banded per exit
    ('exit_profile_tempered_trimap', lambda: _exit_profile(4, (2, 3, 65, 129), temperature=1.5, trimap=(1, 3, 8))),   # profile_upsample_t + confusion_banded
    ('batched_gate_sub2', lambda: _batched_gate(4, (2, 3, 65, 129), 'entropy', 2)),
    ('segmenter_7_classes', lambda: _segmenter(4, (1, 3, 33, 65), classes=7)),                          # addk_label_upsample_supported == 0: the cold path
    ('train_step_dice', lambda: _train_step(4, (2, 3, 65, 129), dice=(0.5, 1.0))),                      # dice_stats + ce_upsample_dice per exit
    ('train_step_dice_distill_ohem', lambda: _train_step(4, (2, 3, 65, 129), ohem=(0.7, 1000), distill=(0.5, 2.0), dice=(0.5, 1.0))),
    ('tiled_segmenter', lambda: _tiled(4, TILE, TILE_STRIDE)),                                          # the 'tiles' head: the exit's low-resolution logits
    ('tiled_segmenter_views', lambda: _tiled(4, TILE, TILE_STRIDE, scales=(0.75, 1.0), flip=True)),    # the same tile plan
    ('tiled_gate_entropy', lambda: _tiled(4, TILE, TILE_STRIDE, threshold=0.35, confidence='entropy')),   # gate_tiles_upsample, cut into stages
    ('tiled_gate_max_tempered', lambda: _tiled(4, TILE, TILE_STRIDE, threshold=0.35, confidence='max', temperature=1.5)),
)


def fingerprints(only=None, dump=None, hold=None, envs=ENVS):
    """{plan/environment: fingerprint} of every plan of PLANS (or of the names in `only`) under every environment of `envs`, built
    in f16x3 arithmetic with every fast path on (config 2's defaults on the MI355X).  `hold`: a list that receives every plan built,
    with all its front end owns, so that it stays alive (a later build then sits at other addresses)."""
    import addk
    from _util import dry_run
    from addk import _lib as L
    lib = addk.load()
    mode, fast = lib.addk_get_conv_precision(), lib.addk_get_fast_paths()
    out = {}
    try:
        L.check(lib.addk_set_conv_precision(1), 'set_conv_precision')
        lib.addk_set_fast_paths(31)
        with dry_run():
            for pname, build in PLANS:
                if only and pname not in only:
                    continue
                for ename, env in envs:
                    old = {k: os.environ.get(k) for k in env}
                    os.environ.update(env)
                    try:
                        g, lists, extra, front = build()
                        label = '%s/%s' % (pname, ename)
                        out[label] = _fingerprint(g, lists, extra, dump, label)
                    finally:
                        for k, v in old.items():
                            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
                    if hold is not None:
                        hold.append((g, front))
                    del g, lists, extra, front
                    gc.collect()
    finally:
        lib.addk_set_conv_precision(mode)
        lib.addk_set_fast_paths(fast)
    return out


def differences(got, want):
    """human-readable list of what differs between two results of fingerprints()"""
    diff = []
    for label in sorted(set(got) | set(want)):
        a, b = got.get(label), want.get(label)
        if a is None or b is None:
            diff.append('%s: %s' % (label, 'missing' if a is None else 'not in the fixture'))
            continue
        for k in ('nbytes', 'bufs', 'buf_sizes', 'packs'):
            if a[k] != b[k]:
                diff.append('%s: %s %s, fixture %s' % (label, k, a[k], b[k]))
        for name in sorted(set(a['lists']) | set(b['lists'])):
            x, y = a['lists'].get(name), b['lists'].get(name)
            if x != y:
                cnt = '' if x is None or y is None else ' names differ: %s' % sorted(
                    (n, x['names'].get(n, 0), y['names'].get(n, 0)) for n in set(x['names']) | set(y['names']) if x['names'].get(n) != y['names'].get(n))
                diff.append('%s/%s: launch list differs from the fixture%s' % (label, name, cnt))
    return diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--dump')
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--only', nargs='*')
    a = ap.parse_args()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    got = fingerprints(a.only, a.dump)
    if a.check:
        with open(a.out) as f:
            want = json.load(f)
        if a.only:
            want = {k: v for k, v in want.items() if k.split('/')[0] in a.only}
        diff = differences(got, want)
        print('\n'.join(diff) if diff else 'plan fingerprints equal the fixture (%d plans)' % len(got))
        return 1 if diff else 0
    with open(a.out, 'w') as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s (%d plans)' % (a.out, len(got)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
