"""The dry-built launch plans are the ones tests/golden/plan_fingerprint.json pins (tests/tools/plan_fingerprint.py, no GPU): config 2's
fused train step and inference plan, the F = 40 train step, the autograd front end, a SyncBN train step with the exchange forced at
world 1, the segments of a gated inference plan (EDM, entropy and top-probability gates, the latter two also with ADDK_FUSE_GATE=0),
a validation plan with its scoring heads and with the stand-alone fallback of 7 classes, an exit-profile plan, the label-map plans
(Segmenter at the final exit with a table and at exit 0, the EDM-gated and the entropy / top-probability gated plans with
output='labels', the latter also with ADDK_FUSE_GATE=0), train steps with hard example mining, with self-distillation and with both,
a MultiViewSegmenter with its default scales and flip, the tempered entropy gate and the tempered top-probability gate with
output='labels', a calibration plan, a validation plan and a tempered exit-profile plan with the trimap metric, the batch-2 sub-plan of
a BatchedGate, a Segmenter of 7 classes (the stand-alone label path), train steps with the soft-Dice term alone and with mining and
self-distillation, and the tile plans of a TiledSegmenter (single-view, with two scales and flip, gated by entropy with every stage
segment of TileGatePlan.stage, gated by the tempered top-probability share), each with and without level batching.
Every command of every list is compared: order, stream, waits, events, regions and each argument byte, with addresses replaced by
(allocation, offset); also the plan's size and its buffers.  A refactor of the planner leaves all of it as it is; a change that is
meant to alter a plan re-records the fixture with the tool and says so."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
import plan_fingerprint as FP     # noqa: E402


def test_dry_built_plans_equal_the_recorded_fingerprints():
    with open(FP.OUT) as f:
        want = json.load(f)
    assert len(want) == len(FP.PLANS) * len(FP.ENVS)
    diff = FP.differences(FP.fingerprints(), want)
    assert not diff, '\n'.join(diff)


class _Item(C.Structure):
    _fields_ = [('i', C.c_int32), ('e', C.c_int32), ('p', C.c_void_p), ('q', C.c_void_p * 2)]


def test_typed_walk_maps_pointers_and_leaves_integers_alone():
    """The fault of the byte-scanning rule this tool had: two int32 fields that together spell an address inside a known allocation
    were rewritten as (allocation, offset), so the hash followed the address space of the process.  Walked by its declared fields,
    such a pair stays data, a pointer into the allocation maps to (allocation, offset), and a pointer into nothing is an error."""
    base = 0x0000550000000000
    mem, moved, none = FP.Memory(), FP.Memory(), FP.Memory()
    mem.add(base, 0x2000)
    moved.add(base + (7 << 32), 0x2000)

    def table(at, e):
        return (_Item * 2)(_Item(3, e, at + 64, (at + 8, 0)), _Item(2, 0x5540, 0, (0, at + 0x1ff8)))
    t = table(base, base >> 32)                                       # (i, e) of the first item reads as the word base + 3
    assert int.from_bytes(bytes(t)[:8], sys.byteorder) == base + 3 and mem.word(base + 3) == ('@', 0, 3)
    out = []
    FP._walk(mem, type(t), bytes(t), 0, 'table', out)
    raw = bytes(t)
    assert out == [raw[0:4], raw[4:8], ('@', 0, 64), ('@', 0, 8), 0, raw[32:36], raw[36:40], 0, 0, ('@', 0, 0x1ff8)]
    # the same table with its memory somewhere else hashes equal; other data does not
    assert FP.typed(mem, t) == FP.typed(moved, table(base + (7 << 32), base >> 32))
    assert FP.typed(mem, t) != FP.typed(mem, table(base, 1 + (base >> 32)))
    assert FP.typed(mem, [t[0], t[1]]) == FP.typed(mem, t)            # a list of structs (conv_pack_batch) is walked like an array
    for bad in (none, moved):
        with pytest.raises(FP.UnknownPointer, match=r'table\[0\]\.p = 0x550000000040'):
            FP.typed(bad, t, 'table')


def test_fingerprints_do_not_depend_on_addresses():
    """two builds of the training plans in one process, the first still alive: other addresses, other LateVec serials, equal fingerprints"""
    held = []
    names = ('c2_module_train', 'syncbn_forced_train_step')
    first = FP.fingerprints(names, hold=held, envs=FP.ENVS[:1])
    second = FP.fingerprints(names, hold=held, envs=FP.ENVS[:1])
    assert len(first) == len(names) and first == second
    n = len(first)
    for (a, _), (b, _) in zip(held[:n], held[n:]):
        assert a is not b and {x.ptr for x in a._bufs}.isdisjoint(x.ptr for x in b._bufs)
    with open(FP.OUT) as f:
        want = json.load(f)
    assert not FP.differences(first, {k: want[k] for k in first})
