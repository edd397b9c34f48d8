"""The launch-list core of a plan: one kernel launch (`Cmd`), the memory regions it reads and writes (`_region`), the hazard tracker over
those regions (`deps`) and what is derived from it: dependency levels, the level order, the stream schedule.  Nothing here knows
plan.Graph.

A region is (name, lo, hi).  The name says what memory it is and never depends on where the allocator put a Python object:
('buf', n) is the n-th buffer of the plan, ('late', n) the n-th plan.LateVec of the process, ('mem', address) the storage of a tensor
the plan does not own.  Names of different kinds never compare equal and none is handed out twice."""
import collections

import torch


class Cmd:
    """One kernel launch of a plan: fn(*args, stream).  `rd`/`wr` are the memory regions it reads / writes
    (keys from `_region`), used to schedule independent launches on parallel HIP streams."""
    __slots__ = ('name', 'fn', 'args', 'rd', 'wr', 'stream', 'waits', 'event', 'pin', 'tag', 'tags', 'payload', 'bkey', 'arena', 'members', 'table')

    def __init__(self, name, fn, args, rd=(), wr=(), pin=False):
        self.name, self.fn, self.args = name, fn, list(args)
        self.rd, self.wr = [k for k in (_region(x) for x in rd) if k], [k for k in (_region(x) for x in wr) if k]
        self.stream, self.waits, self.event, self.pin, self.tag = 0, (), None, pin, ''
        self.tags = None
        self.payload = None            # argument struct of a launch that has a table-driven batched form (level_batch)
        self.bkey = 0                  # kernel-variant key: only launches with equal keys share a batch
        self.arena, self.members = None, 1
        self.table = None              # typed source of the device table this launch reads: a ctypes array (or list) of argument structs

    def __iter__(self):                # unpacks like the (name, fn, args) triple it replaces
        return iter((self.name, self.fn, self.args))

    def __getitem__(self, i):
        return (self.name, self.fn, self.args)[i]


WHOLE = (0, 1 << 30)          # the interval of a region that stands for all of its memory


def _region(x):
    """(name, lo, hi) of what a launch reads or writes.  The plan's own memory names itself (`region` of plan.Buf, TRef, Vec, LateVec);
    a tensor is the byte interval inside its storage, so views of one flat parameter / gradient buffer (train.TrainStep) are distinct
    regions under one name; a tuple is taken as it is."""
    if x is None or isinstance(x, tuple):
        return x
    if isinstance(x, torch.Tensor):
        lo = x.storage_offset() * x.element_size()
        return (('mem', x.untyped_storage().data_ptr()), lo, lo + max(1, x.numel()) * x.element_size())
    try:
        return x.region
    except AttributeError:
        raise TypeError(type(x)) from None


def _overlap(a, b):
    return a[0] == b[0] and a[1] < b[2] and b[1] < a[2]


def deps(cmds):
    """The hazard tracker: for every command, in list order, the set of earlier indices it has to follow (every RAW, WAW and WAR
    relation on overlapping regions of the sequential list, directly or through the commands yielded)."""
    writers, readers = {}, {}            # region name -> [(region, idx)]
    for i, c in enumerate(cmds):
        d = set()
        for k in c.rd:
            d.update(j for r, j in writers.get(k[0], ()) if _overlap(r, k))
        for k in c.wr:
            d.update(j for r, j in writers.get(k[0], ()) if _overlap(r, k))
            d.update(j for r, j in readers.get(k[0], ()) if _overlap(r, k))
        yield d
        for k in c.wr:      # this write stands for the earlier accesses it FULLY covers, and only for those: a partly covered one stays listed
            covered = lambda r: r[1] >= k[1] and r[2] <= k[2]      # noqa: E731
            writers[k[0]] = [(r, j) for r, j in writers.get(k[0], ()) if not covered(r)] + [(k, i)]
            readers[k[0]] = [(r, j) for r, j in readers.get(k[0], ()) if not covered(r)]
        for k in c.rd:
            readers.setdefault(k[0], []).append((k, i))


def levels(cmds):
    """Dependency level (longest path from the inputs) of every command of a launch list."""
    level = []
    for d in deps(cmds):
        level.append(1 + max(level[j] for j in d) if d else 0)
    return level


def level_order(cmds, merge=None):
    """Re-order a launch list in place by dependency level.  Commands of one level never depend on each other, so any order inside
    a level is valid; program order of the original list is kept.  `merge(commands of one level) -> commands` may rewrite a level."""
    buckets = collections.defaultdict(list)
    for c, lv in zip(cmds, levels(cmds)):
        buckets[lv].append(c)
    cmds[:] = [c for lv in sorted(buckets) for c in (merge(buckets[lv]) if merge else buckets[lv])]


def schedule(cmds, nstreams):
    """Assign every command a stream and the cross-stream waits it needs.  A command follows the stream of its most
    recent dependency when that dependency is still the tail of its stream (a chain stays on one stream, no event);
    otherwise it opens on the least recently used stream and waits on events.  Program order inside a stream plus the
    recorded waits preserve every RAW/WAW/WAR relation of the sequential list."""
    tail = [-1] * nstreams               # index of the last command on each stream
    # vector clocks: clock[i][t] = latest command of stream t known to have completed before command i starts.  A wait
    # that a previous wait already implies TRANSITIVELY (A -> B -> C and A -> C) is dropped (fewer event edges in the graph).
    clock = []
    for i, (c, dep) in enumerate(zip(cmds, deps(cmds))):
        if c.pin or nstreams == 1:
            st = 0
        elif dep:
            last = max(dep)
            ls = cmds[last].stream
            st = ls if tail[ls] == last else min(range(nstreams), key=lambda t: tail[t])
        else:
            st = min(range(nstreams), key=lambda t: tail[t])
        # hipStreamEndCapture (ROCm 7.2) crashes when two SIDE streams wait on each other (measured with
        # scripts/capture_probe.py: 'mutual12' dumps core, 'ordered' does not).  Side stream s therefore only ever waits
        # on side streams t > s (and on the main stream 0, which may wait on anybody); a command that would need the
        # other direction runs on the main stream instead.
        if st != 0:
            vc0 = clock[tail[st]] if tail[st] >= 0 else [-1] * nstreams
            if any(0 < cmds[j].stream < st and vc0[cmds[j].stream] < j for j in dep):
                st = 0
        vc = list(clock[tail[st]]) if tail[st] >= 0 else [-1] * nstreams
        waits = []
        for j in sorted(dep, reverse=True):
            t = cmds[j].stream
            if t != st and vc[t] < j:
                waits.append(j)
                vc = [max(a, b) for a, b in zip(vc, clock[j])]
        vc[st] = i
        clock.append(vc)
        c.stream, c.waits = st, tuple(waits)
        tail[st] = i
    need = set(j for c in cmds for j in c.waits)
    for j in need:
        cmds[j].event = True
    return cmds
