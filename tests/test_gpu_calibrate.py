"""End-to-end GPU tests of per-exit calibration: addk.calibrate.ExitCalibration against the model's own full-resolution logits in fp64,
and the tempered gates — model.dynamic_inference / dynamic_inference_batch / ExitProfile with `temperature=` — against fp64 and against
each other.  The F = 4 model and the batches are those of tests/test_gpu_exit_profile.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _calib_ref as R                                                                              # noqa: E402
from _util import ARCH_C3                                                                           # noqa: E402
from test_gpu_exit_profile import HW, MAX_T, SEEDS, _batch, _model                                  # noqa: E402
from test_gpu_gate import NEAR, NEAR_SHARE                                                          # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _snapshot(cal):
    torch.cuda.synchronize()
    return cal.bins.cpu().clone(), cal.nll.cpu().clone()


def test_exit_calibration_against_materialised_logits(dev):
    """Two full batches of 2 and a short one (count = 1), five images: per exit the bins and NLL sums against the definitions in fp64 on
    model(x)'s own full-resolution logits, under the kernel-level bounds.  The third step runs from the captured graph and repeats batch
    one: reset() + that step alone reproduces the eager bits, and the pass is the exact sum of its steps.  result() reports what the
    accumulators hold; the model's mode and state are untouched; config 3 yields three exits."""
    from addk.calibrate import ExitCalibration, reliability
    m = _model(dev).train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    a, b = _batch(2, 11), _batch(2, 12)
    cal = ExitCalibration(m, (2, 3) + HW, use_graph=True)
    cal.step(a[0].to(dev), a[1].to(dev))
    cal.step(b[0].to(dev), b[1].to(dev))
    assert cal.graph is None
    cal.step(a[0].to(dev), a[1].to(dev), count=1)
    assert cal.graph is not None and cal.batches == 3 and cal.images == 5 and m.training
    bins, nll = _snapshot(cal)
    res = cal.result()
    # the same steps one by one, eagerly
    eager = ExitCalibration(m, (2, 3) + HW, use_graph=False)
    parts = []
    for (x, t), count in ((a, 2), (b, 2), (a, 1)):
        eager.reset()
        eager.step(x.to(dev), t.to(dev), count=count)
        parts.append(_snapshot(eager))
    assert eager.graph is None
    assert torch.equal(bins, parts[0][0] + parts[1][0] + parts[2][0])
    assert torch.equal(nll.view(torch.int64), (parts[0][1] + parts[1][1] + parts[2][1]).view(torch.int64))
    cal.reset()
    cal.step(a[0].to(dev), a[1].to(dev), count=1)                                        # the captured replay alone
    b1, n1 = _snapshot(cal)
    assert torch.equal(b1, parts[2][0]) and torch.equal(n1.view(torch.int64), parts[2][1].view(torch.int64))
    assert int(b1[0, 0, :, 0].sum()) < int(parts[0][0][0, 0, :, 0].sum())                 # the painted image added nothing
    # fp64 on the materialised logits of the five images
    m.eval()
    with torch.no_grad():
        ya = [y.clone() for y in m(a[0].to(dev))]
        yb = [y.clone() for y in m(b[0].to(dev))]
    m.train()
    t5 = torch.cat([a[1], b[1], a[1][:1]])
    inv = R.inverse_words(cal.temperatures)
    assert len(res) == cal.nex == 2
    for k in range(cal.nex):
        y5 = torch.cat([ya[k], yb[k], ya[k][:1]])
        ref = R.reference(y5.double().cpu(), t5, inv)
        tag = 'exit %d' % k
        R.check_bins(tag, bins[k], ref)
        tv = torch.where((t5 >= 0) & (t5 < 19), t5, torch.full_like(t5, -100)).to(dev)
        unf = torch.stack([torch.nn.functional.cross_entropy(y5 * w, tv, ignore_index=-100, reduction='sum') for w in inv.to(dev)])
        R.check_nll(tag, nll[k], ref, unf.double().cpu())
        r = res[k]
        assert r['valid'] == ref['valid'] and r['temperatures'] == cal.temperatures
        assert torch.equal(r['bins'], bins[k, :, :, :2]) and torch.equal(r['conf_sum'], bins[k, :, :, 2].double() * 2.0 ** -24)
        assert torch.equal(r['nll'], nll[k] / ref['valid'])
        assert r['accuracy'] == float(bins[k, 0, :, 1].sum()) / ref['valid']
        j = cal.temperatures.index(1.0)
        rel = reliability(r['bins'][j], r['conf_sum'][j])
        assert float(r['ece'][j]) == rel['ece'] and float(r['mce'][j]) == rel['mce'] and 0.0 <= rel['ece'] <= rel['mce'] <= 1.0
        print('%s: accuracy %.4f, mean NLL %s, ECE %s' % (tag, r['accuracy'], ['%.4f' % v for v in r['nll'].tolist()],
                                                        ['%.4f' % v for v in r['ece'].tolist()]))
    fit = cal.fit()
    assert len(fit) == 2 and all(cal.temperatures[0] <= T <= cal.temperatures[-1] for T in fit)
    after = m.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    cal.close()
    eager.close()
    m3 = _model(dev, ARCH_C3)
    c3 = ExitCalibration(m3, (2, 3) + HW, temperatures=(1.0, 2.0))
    assert [c.name for c in c3.g.fwd].count('calib_upsample') == 3
    c3.step(a[0].to(dev), a[1].to(dev))
    r3 = c3.result()
    ok = int(((a[1] >= 0) & (a[1] < 19)).sum())
    assert len(r3) == 3 and all(r['valid'] == ok and tuple(r['bins'].shape) == (2, 16, 2) for r in r3) and len(c3.fit()) == 3
    c3.close()


@pytest.mark.parametrize('kind', ['entropy', 'max'])
def test_dynamic_inference_with_a_temperature(dev, kind):
    """The gate value is that of softmax(model(x)[0] / T) in fp64 under the bounds of tests/test_gpu_gate.py's end-to-end test, for eager
    calls and replays of the captured graphs alike, with both outputs; y is the exit's raw logits (or their map); temperature 1.0, as a
    scalar and per exit, returns the float, the exit and the bytes of temperature=None; another temperature reuses the cached plan."""
    m = _model(dev).eval()
    x = _batch(1, SEEDS[0])[0].to(dev)
    npix = HW[0] * HW[1]
    with torch.no_grad():
        ys = [y.clone() for y in m(x)]
        nex = len(ys)
        labels = [y.argmax(1).to(torch.uint8) for y in ys]
        thr = 0.35
        force, forbid = (float('inf'), float('-inf')) if kind == 'entropy' else (-0.5, 1.5)
        for output, want_y in (('logits', ys), ('labels', labels)):
            # temperature 1.0 is temperature None
            for t in (force, forbid, thr):
                y0, e0, _, v0 = m.dynamic_inference(x, t, kind, output=output)
                y0 = y0.clone()
                for one in (1.0, [1.0] * nex):
                    y1, e1, _, v1 = m.dynamic_inference(x, t, kind, output=output, temperature=one)
                    assert v1 == v0 and e1 == e0 and torch.equal(y1, y0), (output, t, one, v0, v1)
            mode = (output, None) if output == 'labels' else ()
            plan = m._gate_plan(x, kind, *mode, temperature=1.0)
            assert plan is not m._gate_plan(x, kind, *mode) and plan.heads[0].gate_fused
            # calls 3+ replay captured graphs: the words are read when the launch runs
            for T in (1.7, 1.7, 0.6, [2.5, 1.0], 1.7):
                ent64, pmax64 = R.tempered_gate_reference(ys[0].double().cpu(), T if isinstance(T, float) else T[0])
                t = thr if kind == 'max' else force
                y, early, _, v = m.dynamic_inference(x, t, kind, output=output, temperature=T)
                assert m._gate_plan(x, kind, *mode, temperature=T) is plan                      # the cached plan, other words
                assert isinstance(v, float)
                if kind == 'entropy':
                    print('%s T %s: entropy gate %.9g, fp64 %.9g' % (output, T, v, float(ent64[0])))
                    assert abs(v - float(ent64[0])) <= 1e-5
                    assert early == 1 and torch.equal(y, want_y[0])                             # the raw logits / their map
                else:
                    count64 = int((pmax64[0] > thr).sum())
                    near = int(((pmax64[0] - thr).abs() < NEAR).sum())
                    print('%s T %s: max gate %.9g (count %.2f), fp64 count %d, near %d of %d' % (output, T, v, v * npix, count64, near, npix))
                    assert near <= NEAR_SHARE * npix and abs(v * npix - count64) <= near + 1e-2
                    assert early == int(v > thr) and torch.equal(y, want_y[0] if early else want_y[-1])
            assert plan.calls >= 5 and len(plan.graphs) >= 1
            values = {T: m.dynamic_inference(x, forbid if kind == 'entropy' else thr, kind, output=output, temperature=T)[3] for T in (0.6, 1.0, 1.7)}
            assert len(set(values.values())) == 3, values                                      # the temperature moves the value
            if kind == 'entropy':
                assert values[0.6] < values[1.0] < values[1.7]                                 # a flatter softmax has more entropy
            y, early, _, _ = m.dynamic_inference(x, forbid, kind, output=output, temperature=1.7)
            assert early == 0 and torch.equal(y, want_y[-1])
    with pytest.raises(ValueError):
        m.dynamic_inference(x, 0.5, kind, temperature=[1.0] * (nex + 1))


def test_exit_profile_with_fitted_temperatures_equals_dynamic_inference(dev):
    """T = ExitCalibration.fit() on the four images; ExitProfile(temperature=T) then gives, for both gates and every threshold of the
    sweep of tests/test_gpu_exit_profile.py, the exits of model.dynamic_inference(..., temperature=T) image by image and its confidences
    (==)."""
    from addk.calibrate import ExitCalibration
    from addk.exit_profile import ExitProfile
    m = _model(dev).eval()
    images = [_batch(1, s) for s in SEEDS]
    cal = ExitCalibration(m, (1, 3) + HW)
    for x, t in images:
        cal.step(x.to(dev), t.to(dev))
    T, edges = cal.fit(with_edges=True)
    print('fitted temperatures %s (at the edge of the grid: %s)' % (T, edges))
    cal.close()
    plain = ExitProfile(m, (1, 3) + HW, max_thresholds=MAX_T)
    prof = ExitProfile(m, (1, 3) + HW, max_thresholds=MAX_T, temperature=T)
    for x, t in images:
        plain.step(x.to(dev), t.to(dev))
        prof.step(x.to(dev), t.to(dev))
    assert prof.graph is not None
    rec, rec0 = prof.records(), plain.records()
    M, nex = len(images), prof.nex
    assert torch.equal(rec['confusion'], rec0['confusion'])                              # the arg-max does not move
    assert all(t == 1.0 for t in T) or not torch.equal(rec['entropy'], rec0['entropy'])
    e0 = sorted(float(v) for v in rec['entropy'][0])
    print('tempered exit-0 entropies %s (untempered %s)' % (['%.9g' % v for v in rec['entropy'][0].tolist()],
                                                            ['%.9g' % v for v in rec0['entropy'][0].tolist()]))
    mids = [0.5 * (p + q) for p, q in zip(e0, e0[1:]) if q - p > 1e-6]
    assert len(mids) >= 3
    sweeps = {'entropy': [float('-inf')] + mids + [float('inf')], 'max': list(MAX_T)}
    with torch.no_grad():
        for kind, thresholds in sweeps.items():
            for pt, thr in zip(prof.curve(kind, thresholds), thresholds):
                for i, (x, t) in enumerate(images):
                    _, early, _, val = m.dynamic_inference(x.to(dev), thr, kind, temperature=T)
                    assert int(pt['exit_of_image'][i]) == (0 if early else nex - 1), (kind, thr, i)
                    assert float(pt['confidence_of_image'][i]) == val, (kind, thr, i, float(pt['confidence_of_image'][i]), val)
                print('%s thr %.9g: exits %s' % (kind, thr, pt['exit_counts']))
    # other words for the same plan: the profile follows
    g0 = prof.g
    prof.set_temperature(1.0)
    for x, t in images:
        prof.step(x.to(dev), t.to(dev))
    assert prof.g is g0 and torch.equal(prof.records()['entropy'], rec0['entropy']) and torch.equal(prof.records()['share'], rec0['share'])
    plain.close()
    prof.close()


@pytest.mark.parametrize('kind', ['entropy', 'max'])
def test_dynamic_inference_batch_with_a_temperature(dev, kind):
    """Four images at once equal the four single-image tempered calls: the same exits, == values and the same label bytes."""
    m = _model(dev).eval()
    T = [1.7, 1.0]
    xs = torch.cat([_batch(1, s)[0] for s in SEEDS]).to(dev)
    with torch.no_grad():
        singles = [m.dynamic_inference(xs[i:i + 1], float('-inf') if kind == 'entropy' else 0.35, kind, output='labels', temperature=T)[3]
                   for i in range(4)]
        thr = 0.5 * (sorted(singles)[1] + sorted(singles)[2]) if kind == 'entropy' else 0.35
        want = []
        for i in range(4):
            y, early, _, v = m.dynamic_inference(xs[i:i + 1], thr, kind, output='labels', temperature=T)
            want.append((y.clone(), early, v))
        for call in range(2):
            labels, exits, _, values = m.dynamic_inference_batch(xs, thr, kind, temperature=T)
            for i, (y, early, v) in enumerate(want):
                assert int(exits[i]) == (0 if early else 1) and float(values[i, 0]) == v, (i, exits, values, want[i][1:])
                assert torch.equal(labels[i], y[0])
        print('%s thr %.6g: exits %s values %s' % (kind, thr, exits.tolist(), values[:, 0].tolist()))
        if kind == 'entropy':
            assert sorted(exits.tolist()) == [0, 0, 1, 1]                                # the threshold splits the batch
        # the untempered batch under its own key
        _, _, _, v0 = m.dynamic_inference_batch(xs, thr, kind)
        assert not torch.equal(v0, values)
