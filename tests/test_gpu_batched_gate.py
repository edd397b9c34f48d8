"""GPU tests of batched dynamic inference (addk.dynamic.BatchedGate, ADD.dynamic_inference_batch): per-image exits with batch
compaction against the static batch plans (segment.Segmenter), the single-image gate (ADD.dynamic_inference) and ExitProfile.
Model, inputs and single-image references: tests/_batched_gate_ref.py."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import _batched_gate_ref as R      # noqa: E402

MARGIN = 1e-3                # least distance between a threshold's two neighbouring gate values: 100x the agreement bound below
VALUE_TOL = 1e-5             # batch gate value against the single-image one (the bound of tests/test_gpu_gate.py)
# Differing pixels per image between a map made at one batch size and at another.  Measured on the parent commit's code, Segmenter at
# batch 1 against Segmenter at batch N on these inputs, per exit and image (of 33153 pixels):
#   config 2 (N = 4)  exit 0: 0 0 0 0      final exit: 0 0 1 0
#   config 3 (N = 3)  exit 0: 0 0 0        exit 1: 0 0 0        final exit: 0 0 0
# the largest share is 1 pixel (3.0e-5); the cap is twice that and never below 4 pixels (one arg-max near-tie flips a pixel)
CAP_PIXELS = max(4, 2 * 1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _force(kind):
    # 'entropy' leaves when value < threshold; 'max' when share(threshold) > threshold: the share is 1 at a threshold <= 0 and 0 at one >= 1
    return (float('inf'), float('-inf')) if kind == 'entropy' else (-0.5, 1.5)


def _bg(m, x, kind='entropy'):
    """the cached BatchedGate behind ADD.dynamic_inference_batch"""
    return next(p for k, p in m._plans().items() if k[0] == 'dynb' and k[1] == kind and k[2] == tuple(x.shape) and k[4] is None)


@pytest.mark.parametrize('kind', ['entropy', 'max'])
def test_all_leave_and_all_stay(dev, kind):
    """Forcing thresholds: every image leaves at gate 0 and the maps are Segmenter(exit=0)'s at batch 4; forbidding ones: every image
    takes the final head, the maps are Segmenter(exit=-1)'s and no state was moved.  Bit for bit, over five calls each (the later ones
    replay captured graphs): the batch analogue of what tests/test_gpu_gate.py asserts for one image."""
    from addk.segment import Segmenter
    m, X = R.setup('c2', dev)
    force, forbid = _force(kind)
    want0 = Segmenter(m, tuple(X.shape), exit=0).step(X).clone()
    wantf = Segmenter(m, tuple(X.shape), exit=-1).step(X).clone()
    assert not torch.equal(want0, wantf)
    vals = []
    for call in range(5):
        labels, exits, secs, values = m.dynamic_inference_batch(X, force, confidence=kind)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (4, R.H, R.W) and isinstance(secs, float)
        assert exits.dtype == torch.int64 and exits.tolist() == [0, 0, 0, 0]
        assert torch.equal(labels, want0), (call, int((labels != want0).sum()))
        assert tuple(values.shape) == (4, 1) and not torch.isnan(values).any()
        vals.append(values.clone())
    bg = _bg(m, X, kind)
    assert bg.moves == [] and [t[0] for t in bg.trace] == [4]
    state0 = bg.counts['state']
    for call in range(5):
        labels, exits, secs, values = m.dynamic_inference_batch(X, forbid, confidence=kind)
        assert exits.tolist() == [1, 1, 1, 1]
        assert torch.equal(labels, wantf), (call, int((labels != wantf).sum()))
        if kind == 'entropy':
            vals.append(values.clone())
    assert bg.counts['state'] == state0 and bg.moves == [] and [t[0] for t in bg.trace] == [4, 4]  # no gather_rows ran for state
    assert len(bg.sub(4).graphs) >= 2                                                              # the later calls replayed graphs
    assert all(torch.equal(v, vals[0]) for v in vals)                                              # eager and replayed: the same words
    if kind == 'entropy':
        assert len(set(vals[0][:, 0].tolist())) == 4                                               # four images, four values


def test_gate_values_match_single_image(dev):
    """Every gate value of the batch agrees with the single-image dynamic_inference's within 1e-5, for both kinds and both configurations."""
    for cfg in ('c2', 'c3'):
        m, X = R.setup(cfg, dev)
        single, _ = R.singles(cfg, dev)
        _, exits, _, values = m.dynamic_inference_batch(X, float('-inf'), confidence='entropy')
        assert exits.tolist() == [m.num_exits() - 1] * X.shape[0]
        for i in range(X.shape[0]):
            for k in range(m.num_exits() - 1):
                print('%s image %d gate %d: batch %.9g single %.9g' % (cfg, i, k, float(values[i, k]), single[i][k]))
                assert abs(float(values[i, k]) - single[i][k]) <= VALUE_TOL
    m, X = R.setup('c2', dev)
    thr = 0.6                                       # share(0.6) of these predictions lies strictly inside (0, 1)
    _, exits, _, values = m.dynamic_inference_batch(X, thr, confidence='max')
    for i in range(4):
        _, early, _, v = m.dynamic_inference(X[i:i + 1], thr, confidence='max', output='labels')
        print('c2 image %d share(%.2f): batch %.9g single %.9g' % (i, thr, float(values[i, 0]), v))
        assert abs(float(values[i, 0]) - v) <= VALUE_TOL and 0.0 < v < 1.0
        assert int(exits[i]) == (0 if early else 1)


def _check_maps(labels, exits, maps):
    for i, e in enumerate(exits.tolist()):
        bad = int((labels[i] != maps[i][e]).sum())
        print('image %d exit %d: %d of %d pixels differ from the single-image map' % (i, e, bad, labels[i].numel()))
        assert bad <= CAP_PIXELS, (i, e, bad)


def test_mixed_decisions_c2(dev):
    """Config 2, threshold at the midpoint of the largest gap of the four single-image gate values (gap >= 1e-3 asserted first: here
    0.157 between images 1 and 2, so images 2 and 3 leave): the exits are the single-image decisions, every map differs from its
    single-image map in at most CAP_PIXELS pixels (measured shares: the comment at CAP_PIXELS), the state of the two stayers moved
    4 -> 2 in one launch and every destination row holds its source row's bits; the same again when the graphs replay."""
    m, X = R.setup('c2', dev)
    single, maps = R.singles('c2', dev)
    v = sorted(s[0] for s in single)
    gap, lo = max((b - a, a) for a, b in zip(v, v[1:]))
    assert gap >= MARGIN, v
    thr = lo + 0.5 * gap
    want = [0 if s[0] < thr else 1 for s in single]
    assert 0 < sum(want) < 4
    for call in range(4):
        labels, exits, _, values = m.dynamic_inference_batch(X, thr, confidence='entropy')
        assert exits.tolist() == want
        _check_maps(labels, exits, maps)
        bg = _bg(m, X)
        stay = [i for i in range(4) if want[i] == 1]
        assert bg.moves == [(4, len(stay), 0, stay)]
        assert [t[0] for t in bg.trace] == [4, len(stay)]
        pairs = bg.transition_pairs()
        assert len(pairs) >= 2
        for src, dst in pairs:                                                  # the transition is exact
            assert src.shape == dst.shape and src.shape[0] == len(stay) and torch.equal(src, dst)
    sizes = bg.nbytes
    assert sizes['total'] >= sum(v for k, v in sizes.items() if k != 'total') and sizes[4] > sizes[len(stay)] > 0


def test_three_way_split_c3(dev):
    """Config 3 (two gates), N = 3, one threshold per gate: gate 0's between the smallest and the second gate-0 value, gate 1's between
    the two survivors' gate-1 values (each gap >= 1e-3 asserted): one image leaves at each gate and one reaches the final head, through
    sub-plans 3 -> 2 -> 1; exits and maps as in the config 2 test."""
    m, X = R.setup('c3', dev)
    single, maps = R.singles('c3', dev)
    v0 = sorted((s[0], i) for i, s in enumerate(single))
    assert v0[1][0] - v0[0][0] >= MARGIN, v0
    t0 = 0.5 * (v0[0][0] + v0[1][0])
    rest = sorted((single[i][1], i) for _, i in v0[1:])
    assert rest[1][0] - rest[0][0] >= MARGIN, rest
    t1 = 0.5 * (rest[0][0] + rest[1][0])
    want = [0 if s[0] < t0 else 1 if s[1] < t1 else 2 for s in single]
    assert sorted(want) == [0, 1, 2]
    for call in range(4):
        labels, exits, _, values = m.dynamic_inference_batch(X, [t0, t1], confidence='entropy')
        assert exits.tolist() == want
        _check_maps(labels, exits, maps)
        for i, e in enumerate(want):
            for k in range(2):
                if k <= min(e, 1):
                    assert abs(float(values[i, k]) - single[i][k]) <= VALUE_TOL
                else:
                    assert values[i, k] != values[i, k]                         # NaN: the gate never saw this image
        bg = _bg(m, X)
        assert [(a, b, k) for a, b, k, _ in bg.moves] == [(3, 2, 0), (2, 1, 1)]
        assert [t[0] for t in bg.trace] == [3, 2, 1] and sorted(bg.subs) == [1, 2, 3]
    # the rows of the last transition (the batch-2 plan ran on behind gate 0 after the first)
    pairs = [p for p, (a, b, k, _) in zip(_per_move(bg), bg.moves) if (a, b, k) == (2, 1, 1)][0]
    assert all(torch.equal(src, dst) for src, dst in pairs)
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(X, [t0], confidence='entropy')


def test_weight_packs_behind_the_cut(dev):
    """193 x 385, N = 3: at this size the decoder's 3x3 convolutions behind the cut read hoisted weight packs, which the batch-2 sub-plan
    (entered behind the cut) must recompute (tests/test_batched_gate_plan.py checks that its replay set holds the pack launch).  One image
    leaves at gate 0; the stayers' maps are Segmenter(exit=-1)'s at batch 2 on those two images, the leaver's is its row of
    Segmenter(exit=0)'s at batch 3, bit for bit — over four calls, eager and replayed."""
    from addk.dynamic import BatchedGate
    from addk.segment import Segmenter
    from _util import rand_tensor
    m, _ = R.setup('c2', dev)
    shape = (3, 3, 193, 385)
    X = torch.cat([rand_tensor(41 + i, 'bgx', (1,) + shape[1:]) * c for i, c in enumerate((0.25, 1.0, 4.0))]).to(dev)
    bg = BatchedGate(m, shape, 'entropy')
    _, exits, values = bg.run(X, float('-inf'))
    v = sorted(values[:, 0].tolist())
    print('gate values at 193 x 385: %s' % v)
    assert exits.tolist() == [1, 1, 1] and v[1] - v[0] >= MARGIN
    thr = 0.5 * (v[0] + v[1])
    want = [0 if float(x) < thr else 1 for x in values[:, 0]]
    stay, leave = [i for i in range(3) if want[i]], [i for i in range(3) if not want[i]]
    want0 = Segmenter(m, shape, exit=0).step(X)[leave].clone()
    wantf = Segmenter(m, (2,) + shape[1:], exit=-1).step(X[stay].contiguous()).clone()
    for call in range(4):
        labels, exits, _ = bg.run(X, thr)
        assert exits.tolist() == want and bg.moves == [(3, 2, 0, stay)]
        assert 'conv_pack_batch' in [c.name for c in bg.sub(2).live(bg.sub(2).head_rng[0][1])[1]]
        assert torch.equal(labels[leave], want0)
        assert torch.equal(labels[stay], wantf), (call, int((labels[stay] != wantf).sum()))
    bg.close()


def _per_move(bg):
    """transition_pairs() of the last call, grouped by transition"""
    out, flat = [], bg.transition_pairs()
    for a, b, k, _ in bg.moves:
        n = len(bg.tables[('state', a, b, k)][2])
        out.append(flat[:n])
        flat = flat[n:]
    return out


def test_statistics_change_between_calls(dev):
    """Config 3.  running_mean of a BatchNorm between the two gates (cell 7's preprocess, which feeds exit 1) changes in place between two
    calls.  Image 2 leaves at gate 0, so the batch-2 sub-plan is entered behind that gate and never runs its own first segment: its gate-1
    values move with the statistics, and values, exits and maps are those of a freshly built BatchedGate.  Gate 1 lets nobody go
    (threshold -inf), so no decision depends on the changed values."""
    from addk.dynamic import BatchedGate
    m, X = R.setup('c3', dev)
    single, _ = R.singles('c3', dev)
    v0 = sorted(s[0] for s in single)
    assert v0[1] - v0[0] >= MARGIN
    thr = [0.5 * (v0[0] + v0[1]), float('-inf')]
    labels, exits, _, values = m.dynamic_inference_batch(X, thr, confidence='entropy')
    before, vbefore, bg = labels.clone(), values.clone(), _bg(m, X)
    assert sorted(exits.tolist()) == [0, 2, 2] and [(a, b, k) for a, b, k, _ in bg.moves] == [(3, 2, 0)]
    stay = [i for i, e in enumerate(exits.tolist()) if e == 2]
    leave = [i for i, e in enumerate(exits.tolist()) if e == 0]
    bn = [mod for mod in m.cells[7].preprocess.modules() if isinstance(mod, nn.BatchNorm2d)][0]
    saved = bn.running_mean.clone()
    try:
        with torch.no_grad():
            bn.running_mean.add_(300.0 * bn.running_var.sqrt())
        labels, exits2, _, values2 = m.dynamic_inference_batch(X, thr, confidence='entropy')
        assert _bg(m, X) is bg and len(bg.moves) == 1
        after = labels.clone()
        fresh = BatchedGate(m, tuple(X.shape), 'entropy')
        flabels, fexits, fvalues = fresh.run(X, thr)
        torch.cuda.synchronize()
        assert torch.equal(exits2, fexits) and torch.equal(exits2, exits)
        assert torch.equal(values2[stay], fvalues[stay]) and torch.equal(values2[:, 0], fvalues[:, 0])
        assert torch.equal(after, flabels)
        for i in stay:
            print('image %d gate 1: %.9g before, %.9g after the change' % (i, float(vbefore[i, 1]), float(values2[i, 1])))
            # the statistics reached the sub-plan: the gate words are reproducible to the bit from call to call (test_all_leave_and_all_stay),
            # so any other word is the change's doing (the trunk's activations are of order 1e3 here: even this shift moves the entropy little)
            assert float(values2[i, 1]) != float(vbefore[i, 1])
        assert torch.equal(values2[:, 0], vbefore[:, 0]) and torch.equal(after[leave], before[leave])     # ... and nothing in front of them
        fresh.close()
    finally:
        with torch.no_grad():
            bn.running_mean.copy_(saved)
    labels, _, _, values3 = m.dynamic_inference_batch(X, thr, confidence='entropy')
    assert torch.equal(labels, before) and torch.equal(values3[stay], vbefore[stay])


def test_consistent_with_exit_profile(dev):
    """Same images, same thresholds: the images leaving at each exit are those ExitProfile's per-image gate values predict."""
    from addk.exit_profile import ExitProfile
    for cfg in ('c2', 'c3'):
        m, X = R.setup(cfg, dev)
        single, _ = R.singles(cfg, dev)
        prof = ExitProfile(m, tuple(X.shape), max_thresholds=(0.6,))
        prof.step(X, torch.zeros((X.shape[0], R.H, R.W), dtype=torch.int64, device=dev))
        v = sorted(s[0] for s in single)
        gap, lo = max((b - a, a) for a, b in zip(v, v[1:]))
        thr = lo + 0.5 * gap                          # one number for every gate: exit_curve's rule
        pt = prof.curve('entropy', [thr])[0]
        # the margin holds at every gate the profile evaluates with this number
        ent = prof.records()['entropy'][:m.num_exits() - 1]
        assert float((ent.double() - thr).abs().min()) >= 0.5 * MARGIN
        _, exits, _, _ = m.dynamic_inference_batch(X, thr, confidence='entropy')
        assert exits.tolist() == pt['exit_of_image'].tolist()
        assert torch.bincount(exits, minlength=m.num_exits()).tolist() == pt['exit_counts']
        if cfg == 'c2':
            pm = prof.curve('max', [0.6])[0]
            _, exits, _, _ = m.dynamic_inference_batch(X, 0.6, confidence='max')
            share = prof.records()['share'][0, :, 0]
            assert float((share.double() - 0.6).abs().min()) >= 0.5 * MARGIN
            assert torch.bincount(exits, minlength=2).tolist() == pm['exit_counts']
