"""The per-call launches of the inference front ends (CPU, no GPU), pinned launch for launch: tests/golden/inference_call_trace.json holds,
for whole calls of segment.TiledSegmenter and dynamic.BatchedGate, the ordered command names that reach plan.Graph.run — the replays of
the plan and every launch the call adds around them.  tests/tools/plan_fingerprint.py pins what a plan IS; this pins what a call DOES with
it.  A refactor of the host side leaves both as they are; a change that is meant to alter a call re-records the fixture and says so:

    python tests/test_inference_call_trace.py            # writes tests/golden/inference_call_trace.json (run it on the commit to pin)

plan.Graph.run is wrapped here, inside the dry run of tests/_util.py.  Of `gather_tiles`, `gather_tile_views`, `gather_rows`,
`scatter_tile_logits` and the two stitching heads the record also keeps every integer or float argument that is no address: the
positional ones, the fields of the argument block, and what the launch would read through its tables — the window descriptors (without the
image address), the bytes per row of every gather_rows item and the index words.  In a dry run all of these lie in host memory.  The
descriptor table is named by its byte offset from the first gather of the call.

The calls: a static single-view segment() of two images — 40 x 100, smaller than the 65 x 129 window, and 97 x 200, whose last windows of
both axes are clamped —, the same with two scales and flip, a gated segment() of a model with two gates whose decisions are scripted
through `_conf_host` (windows leave, park, fill a batch again, and the flush runs), and a BatchedGate.run that moves 4 -> 2 -> 1.  The
gated calls also count the waits on `_conf_evt`: one per evaluated gate stage."""
import contextlib
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                     # (run as a script, to record)
    sys.path.insert(0, ROOT)
import addk                  # noqa: E402
from addk import _lib as L   # noqa: E402
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, dry_run, make_args      # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'inference_call_trace.json')
TILE, STRIDE = (3, 3, 65, 129), (32, 71)
SIZES = ((40, 100), (97, 200))
DESC = {'gather_tiles': L.TileDesc, 'gather_tile_views': L.TileViewDesc}
BLOCKS = ('gather_rows', 'scatter_tile_logits', 'label_tiles_upsample', 'label_tile_views_upsample')


def _add(arch):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, 19, make_args(4), arch['low_level_layer']).eval()


def _plain(o):
    """a ctypes value without its addresses: structs as dicts of their non-pointer fields, arrays as lists"""
    if isinstance(o, C.Structure):
        return {f: _plain(getattr(o, f)) for f, t in o._fields_ if t is not C.c_void_p}
    if isinstance(o, C.Array):
        return [_plain(v) for v in o]
    return o


def _words(ptr, n):
    return None if not ptr else list((C.c_int32 * n).from_address(ptr))


def _record(name, args):
    if name in DESC:
        table, n, Cin, th, tw, _, B = args
        return [name, {'table': table, 'n': n, 'Cin': Cin, 'th': th, 'tw': tw, 'B': B,
                       'desc': [_plain(d) for d in (DESC[name] * n).from_address(table)]}]
    if name not in BLOCKS:
        return name
    a = args[0]._obj
    rec = _plain(a)
    if name == 'gather_rows':
        rec.update(row_bytes=[it.row_bytes for it in (L.RowsItem * a.nitems).from_address(a.items)],
                   src_row=_words(a.src_row, a.nrows), dst_row=_words(a.dst_row, a.nrows))
    elif name == 'scatter_tile_logits':
        rec.update(src_row=_words(a.src_row, a.n), dst_tile=_words(a.dst_tile, a.n))
    return [name, rec]


class Waits:
    """stands in for a plan's `_conf_evt`: counts record() / synchronize(); `script`: the gate words the host finds after each wait"""

    def __init__(self, host=None, script=()):
        self.recorded = self.waited = 0
        self.host, self.script = host, list(script)

    def record(self):
        self.recorded += 1

    def synchronize(self):
        assert self.recorded == self.waited + 1, 'one record in front of every wait'
        if self.script:
            words = self.script.pop(0)
            self.host[:len(words)] = torch.tensor(words)
        self.waited += 1


@contextlib.contextmanager
def recording():
    """the dry run of tests/_util.py in the arithmetic mode and with the fast paths the fingerprints are taken in, plan.Graph.run
    recording -> the list of records"""
    import addk.plan as P
    lib = addk.load()
    mode, fast = lib.addk_get_conv_precision(), lib.addk_get_fast_paths()
    old = os.environ.get('ADDK_GRAPH_INFER')
    os.environ['ADDK_GRAPH_INFER'] = '0'                     # no device: nothing to capture
    out = []

    def run(self, cmds, stream):
        out.extend(_record(name, args) for name, fn, args in cmds)
    try:
        L.check(lib.addk_set_conv_precision(1), 'set_conv_precision')
        lib.addk_set_fast_paths(31)
        with dry_run():
            stub, P.Graph.run = P.Graph.run, run
            try:
                yield out
            finally:
                P.Graph.run = stub
    finally:
        lib.addk_set_conv_precision(mode)
        lib.addk_set_fast_paths(fast)
        os.environ.pop('ADDK_GRAPH_INFER') if old is None else os.environ.__setitem__('ADDK_GRAPH_INFER', old)


def _call(out, fn):
    """the records of one call; the descriptor table as its offset from the call's first gather"""
    del out[:]
    fn()
    base = next((r[1]['table'] for r in out if not isinstance(r, str) and r[0] in DESC), 0)
    for r in out:
        if not isinstance(r, str) and r[0] in DESC:
            r[1]['table'] -= base
    return list(out)


def _images():
    return [torch.randn(3, H, W) for H, W in SIZES]


def _static(out, **kw):
    from addk.segment import TiledSegmenter
    seg = TiledSegmenter(_add(ARCH_C2), TILE, STRIDE, **kw)
    cmds = _call(out, lambda: seg.segment(_images()))
    return {'commands': cmds, 'tiles': [list(t) for t in seg.tiles]}


def _gated(out):
    """two gates, B = 3, five windows.  Chunk 0: windows 0 and 2 leave, 1 parks.  Chunk 1: 3 and 4 stay and park: the pool holds a full
    batch, which runs gate 1 — window 1 leaves, 3 and 4 park one pool further — and the flush takes them through the last stage."""
    from addk.segment import TiledSegmenter
    seg = TiledSegmenter(_add(ARCH_C3), TILE, STRIDE, threshold=0.35, confidence='entropy')
    evt = seg.plan._conf_evt = Waits(seg.plan._conf_host, [[0.1, 0, 0.9, 0, 0.1, 0], [0.9, 0, 0.9, 0], [0.1, 0, 0.9, 0, 0.9, 0]])
    cmds = _call(out, lambda: seg.segment(_images()))
    assert seg.exits.tolist() == [0, 1, 0, 2, 2] and seg.trace == [(0, 3), (0, 2), (1, 3), (2, 2)]
    assert seg.counts['park'] == 3 and seg.counts['unpark'] == 2 and seg.counts['scatter'] == 3
    gate_stages = sum(1 for k, _ in seg.trace if k < seg.gates)
    assert evt.recorded == evt.waited == gate_stages == 3 and not evt.script
    return {'commands': cmds, 'waits': evt.waited, 'tiles': [list(t) for t in seg.tiles]}


def _batched(out):
    """N = 4, two gates: images 0 and 2 leave at gate 0, the first survivor (image 1) at gate 1, image 3 at the last exit"""
    from addk.dynamic import BatchedGate
    bg = BatchedGate(_add(ARCH_C3), (4, 3, 65, 129), 'entropy')
    evt = Waits()
    for n, words in ((4, [0.1, 0, 0.9, 0, 0.1, 0, 0.9, 0]), (2, [0.1, 0, 0.9, 0]), (1, [0.9, 0])):
        bg.sub(n)._conf_host[:] = torch.tensor(words)
        bg.sub(n)._conf_evt = evt
    got = []
    cmds = _call(out, lambda: got.extend(bg.run(torch.randn(4, 3, 65, 129), 0.5)))
    assert got[1].tolist() == [0, 1, 0, 2] and bg.moves == [(4, 2, 0, [1, 3]), (2, 1, 1, [1])]
    assert evt.recorded == evt.waited == bg.gates == 2                     # both gates were evaluated, each once
    return {'commands': cmds, 'waits': evt.waited}


CALLS = {'static': _static,
         'views': lambda out: _static(out, scales=(0.75, 1.0), flip=True),
         'gated': _gated,
         'batched_gate': _batched}


def traces(only=None):
    with recording() as out:
        return {name: json.loads(json.dumps(fn(out))) for name, fn in CALLS.items() if only is None or name in only}


@pytest.mark.parametrize('name', list(CALLS))
def test_a_call_launches_what_was_recorded(name):
    with open(OUT) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CALLS)
    got = traces((name,))[name]
    assert sorted(got) == sorted(want[name])
    for key in got:
        if key != 'commands':
            assert got[key] == want[name][key], key
    a, b = got['commands'], want[name]['commands']
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    assert first is None, 'command %d differs: %r, recorded %r' % (first, a[first], b[first])
    assert len(a) == len(b)


def test_the_records_hold_what_the_calls_are_about():
    """the fixture itself: the clamped and the padded windows, the detailed launches, the waits"""
    with open(OUT) as f:
        want = json.load(f)
    names = lambda case: [r if isinstance(r, str) else r[0] for r in want[case]['commands']]      # noqa: E731
    detail = lambda case, name: [r[1] for r in want[case]['commands'] if not isinstance(r, str) and r[0] == name]      # noqa: E731
    # 1 + 2 x 2 windows: the small image is one padded window, the last window of each axis of the other is clamped to 97 - 65, 200 - 129
    assert want['static']['tiles'] == [[0, 0, 0], [1, 0, 0], [1, 0, 71], [1, 32, 0], [1, 32, 71]]
    g = detail('static', 'gather_tiles')
    assert [(d['table'], d['n']) for d in g] == [(0, 3), (3 * C.sizeof(L.TileDesc), 2)]
    assert [(d['H'], d['W'], d['y0'], d['x0']) for d in g[0]['desc'] + g[1]['desc']] == [(40, 100, 0, 0)] + [(97, 200, y, x) for y in (0, 32) for x in (0, 71)]
    heads = detail('static', 'label_tiles_upsample')
    assert [(a['OH'], a['OW'], a['t0'], a['ny'], a['nx']) for a in heads] == [(40, 100, 0, 1, 1), (97, 200, 1, 2, 2)]
    assert names('static').count('nchw_to_nhwc') == 2 and 'gather_rows' not in names('static')
    T = len(want['views']['tiles'])
    assert T == 4 * 1 + 4 * 4 and len(detail('views', 'gather_tile_views')) == -(-T // 3) and len(detail('views', 'label_tile_views_upsample')) == 2
    assert [v['mirror'] for v in detail('views', 'label_tile_views_upsample')[1]['view'][:4]] == [0, 1, 0, 1]
    # gated: scatter at exits 0, 0 (nobody), 1, 2 -> four scatters less the empty one; park / unpark through gather_rows with their index words
    rows = detail('gated', 'gather_rows')
    assert [(r['src_row'], r['dst_row']) for r in rows] == [([1], [0]), ([0, 1], [1, 2]), ([0, 1, 2], None), ([1, 2], [0, 1]), ([0, 1], None)]
    assert [(s['src_row'], s['dst_tile']) for s in detail('gated', 'scatter_tile_logits')] == [([0, 2], [0, 2]), ([0], [1]), ([0, 1], [3, 4])]
    assert want['gated']['waits'] == 3 and names('gated').count('gate_tiles_upsample') == 3
    rows = detail('batched_gate', 'gather_rows')
    assert [(r['src_row'], r['dst_row'], r['nrows']) for r in rows] == [([0, 2], [0, 2], 2), ([1, 3], None, 2), ([0], [1], 1), ([1], None, 1), (None, [3], 1)]
    assert want['batched_gate']['waits'] == 2


if __name__ == '__main__':
    got = traces()
    with open(OUT, 'w') as f:
        f.write('{\n%s\n}\n' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(got.items())))
    print('wrote %s (%s)' % (OUT, ', '.join('%s: %d commands' % (k, len(v['commands'])) for k, v in sorted(got.items()))))
    sys.exit(0)
