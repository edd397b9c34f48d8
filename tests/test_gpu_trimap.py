"""GPU tests of the boundary-band ("trimap") metric: addk_boundary_dist and addk_confusion_banded through the C ABI against the numpy
reference of tests/_trimap_ref.py, and ValidationStep / ExitProfile built with `trimap=` end to end (eager calls, the capture and a replay).
Every map and matrix is an integer and is compared for equality: no tolerance exists for them anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _trimap_ref as R                                                                    # noqa: E402
from _util import ARCH_C2, GENOTYPE_AUTODEEPLAB, fill_params, make_args, rand_tensor      # noqa: E402

NC = 19
GUARD = 64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    import addk._lib as L
    return L.load(), L


# ------------------------------------------------------------------------------------------------------------------------
# addk_boundary_dist
# ------------------------------------------------------------------------------------------------------------------------
CASES = {'a': (lambda: np.random.default_rng(5).integers(0, 3, (1, 5, 7)).astype(np.int64), 64, R.dist_brute),
         'b': (R.case_b, 8, R.dist_brute),
         'c': (R.case_c, 64, R.dist_sep),
         'd': (R.case_d, 16, R.dist_brute),
         'e': (R.case_e, 5, R.dist_brute)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """target and reference distance map of one case, computed once and never modified"""
    make, radius, ref = CASES[name]
    t = make()
    want = ref(t, NC, radius)
    t.setflags(write=False)
    want.setflags(write=False)
    return t, radius, want


def _boundary_dist(t, radius, dev, fill=0xA5, ncls=NC):
    """dist and ws pre-filled with garbage; returns (rc, dist bytes [N,OH,OW], the guard bytes behind them)"""
    lib, L = _lib()
    N, OH, OW = t.shape
    ta = torch.from_numpy(np.array(t)).to(dev)
    buf = torch.full((N * OH * OW + GUARD,), fill, dtype=torch.uint8, device=dev)
    ws = torch.full((int(lib.addk_boundary_dist_ws_bytes(N, OH, OW)),), 0x5A ^ fill, dtype=torch.uint8, device=dev)
    a = L.BoundaryDistArgs()
    a.target, a.N, a.OH, a.OW, a.C, a.radius, a.dist, a.ws = ta.data_ptr(), N, OH, OW, ncls, radius, buf.data_ptr(), ws.data_ptr()
    rc = lib.addk_boundary_dist(C.byref(a), _stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return rc, host[:N * OH * OW].reshape(N, OH, OW), host[N * OH * OW:]


@pytest.mark.parametrize('name', sorted(CASES))
def test_boundary_dist_equals_reference(dev, name):
    t, radius, want = _case(name)
    rc, got, guard = _boundary_dist(t, radius, dev)
    assert rc == 0
    bad = np.argwhere(got != want)
    print('case %s: %d far bytes, %d edge bytes, %d mismatches%s' % (name, int((want == R.FAR).sum()), int((want == 0).sum()), len(bad),
                                                                    ' first %s got %d want %d' % (bad[0], got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else ''))
    assert np.array_equal(got, want)
    assert (guard == 0xA5).all()                                     # nothing behind the map is written
    if name == 'b':                                                  # partial tiles with both near and far pixels
        assert (want == R.FAR).any() and ((want > 0) & (want <= radius)).any()
    if name == 'c':                                                  # discs around the single foreign pixel of image 1
        assert got[1, 43, 74] == 5 and got[1, 45, 75] == 7 and got[1, 40, 134] == 63 and got[1, 40, 135] == 64 and got[1, 40, 136] == R.FAR
        assert int((got == R.FAR).sum()) == int((got[1] == R.FAR).sum()) == 4290
    if name == 'd':                                                  # the edge along image 0's last row does not leak into image 1
        assert (got[1] == R.FAR).all() and (got[0, 39] == 0).all() and (got[0, 38] == 0).all() and (got[0, 30] == 8).all()
    if name == 'e':                                                  # edges only where two different valid classes touch
        assert np.array_equal(got == 0, R.edges(t, NC))


def test_boundary_dist_other_fill_and_second_call_give_equal_bits(dev):
    t, radius, want = _case('b')
    _, one, _ = _boundary_dist(t, radius, dev, fill=0xA5)
    _, two, _ = _boundary_dist(t, radius, dev, fill=0x00)             # other garbage in dist and ws: every byte is written
    assert np.array_equal(one, two) and np.array_equal(one, want)


# ------------------------------------------------------------------------------------------------------------------------
# addk_confusion_banded
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pred(name):
    t, _, _ = _case(name)
    r = np.random.default_rng(23)
    p = r.integers(0, NC, t.shape).astype(np.uint8)
    flat = p.reshape(-1)
    pos = r.choice(flat.size, 60, replace=False)
    flat[pos] = np.tile(np.array([19, 77, 255], dtype=np.uint8), 20)
    p.setflags(write=False)
    return p


def _banded(t, pred, dist, widths, dev, stride=0, cm0=None, ncls=NC, null=None, nw=None):
    lib, L = _lib()
    N, OH, OW = t.shape
    nw = len(widths) if nw is None else nw
    words = (N * stride if stride else max(nw, 1) * ncls * ncls)
    cm = torch.zeros(max(words, 1), dtype=torch.int64, device=dev) if cm0 is None else torch.from_numpy(cm0.copy()).to(dev)
    ta, pa, da = (torch.from_numpy(np.array(v)).to(dev) for v in (t, pred, dist))
    a = L.ConfusionBandedArgs()
    a.target, a.pred, a.dist = ta.data_ptr(), pa.data_ptr(), da.data_ptr()
    a.N, a.OH, a.OW, a.C, a.nw = N, OH, OW, ncls, nw
    for j, w in enumerate(widths[:8]):
        a.width[j] = w
    a.cm, a.image_stride = cm.data_ptr(), stride
    if null:
        setattr(a, null, None)
    rc = lib.addk_confusion_banded(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, cm.cpu().numpy()


@pytest.mark.parametrize('name', ['c', 'b'])
@pytest.mark.parametrize('widths', [(1, 2, 4, 8, 16, 32), (3,), (0, 64)])
def test_confusion_banded_equals_reference(dev, name, widths):
    """target, dist and pred come from the host: independent of the distance kernel.  The matrices are pre-filled: the launch ADDS."""
    t, _, _ = _case(name)
    dist = R.dist_sep(t, NC, 64)                                    # the reference map at the largest radius, whatever the case's own
    pred = _pred(name)
    nw, ne = len(widths), len(widths) * NC * NC
    want_img = R.banded_confusion(t, pred, dist, NC, widths, per_image=True)
    if name == 'c' and nw == 6:                                     # no ring is empty, in either image: no empty comparison can pass
        sizes = want_img.sum((2, 3))
        print('ring sizes %s' % (sizes.tolist(),))
        assert (sizes > 0).all()
        geo = [int(((dist[1] > lo) & (dist[1] <= hi)).sum()) for lo, hi in zip((-1,) + widths, widths)]
        assert geo == [13, 12, 48, 172, 644, 2504]                  # the rings of the disc around image 1's single foreign pixel
    assert want_img.sum() > 0
    r = np.random.default_rng(9)
    # one set for the batch
    cm0 = r.integers(1, 1 << 40, ne)
    rc, got = _banded(t, pred, dist, widths, dev, cm0=cm0)
    assert rc == 0 and np.array_equal(got - cm0, want_img.sum(0).reshape(-1))
    # per-image sets with a stride above nw*C*C: the words between the sets stay
    stride = ne + 5
    cm0 = r.integers(1, 1 << 40, t.shape[0] * stride)
    rc, got = _banded(t, pred, dist, widths, dev, stride=stride, cm0=cm0)
    delta = (got - cm0).reshape(t.shape[0], stride)
    assert rc == 0 and np.array_equal(delta[:, :ne], want_img.reshape(t.shape[0], ne)) and not delta[:, ne:].any()
    # the rings sum to the plain confusion of the counted pixels
    assert np.array_equal(delta[:, :ne].reshape(-1, nw, NC, NC).sum((0, 1)), R.plain_confusion(t, pred, NC, dist <= widths[-1]))
    # twice: equal bits
    rc, again = _banded(t, pred, dist, widths, dev, stride=stride, cm0=cm0)
    assert rc == 0 and np.array_equal(again, got)


def test_invalid_arguments_launch_nothing(dev):
    lib, L = _lib()
    t, _, want = _case('b')
    pred = _pred('b')
    for radius in (0, 65):
        rc, got, guard = _boundary_dist(t, radius, dev)
        assert rc == L.load().addk_boundary_dist(None, None) == -1 and (got == 0xA5).all() and (guard == 0xA5).all()
    rc, got, _ = _boundary_dist(t, 8, dev, ncls=33)
    assert rc == -1 and (got == 0xA5).all()
    a = L.BoundaryDistArgs()
    a.N, a.OH, a.OW, a.C, a.radius = 2, 37, 53, NC, 8
    assert lib.addk_boundary_dist(C.byref(a), _stream()) == -1       # null pointers
    cm0 = np.full(10 * NC * NC, 7, dtype=np.int64)
    bad = [dict(widths=(), nw=0), dict(widths=tuple(range(1, 10)), nw=9), dict(widths=(2, 2)), dict(widths=(4, 300)), dict(widths=(-1, 3)),
           dict(widths=(1, 2), stride=2 * NC * NC - 1), dict(widths=(1, 2), ncls=33), dict(widths=(1, 2), null='pred'),
           dict(widths=(1, 2), null='dist'), dict(widths=(1, 2), null='target'), dict(widths=(1, 2), null='cm')]
    for kw in bad:
        rc, got = _banded(t, pred, want, dev=dev, cm0=cm0, **kw)
        assert rc == -1 and np.array_equal(got, cm0), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# end to end: ADD F = 4, config 2, (2, 3, 65, 129), four different batches
# ------------------------------------------------------------------------------------------------------------------------
HW = (65, 129)
WIDTHS = (1, 2, 4, 8)


def _model(dev, seed=600, scale=4e-3):
    from addk.modeling.ADD import ADD
    m = ADD(ARCH_C2['network_arch'], ARCH_C2['C_index'], GENOTYPE_AUTODEEPLAB, NC, make_args(4), ARCH_C2['low_level_layer'])
    fill_params(m, seed)
    with torch.no_grad():                      # as tests/test_gpu_exit_profile.py: entropies spread over (0, 1)
        m.decoder._conv[7].weight.mul_(scale)
        m.decoder._conv[7].bias.mul_(scale)
    return m.to(dev)


def _batch(seed):
    x = rand_tensor(seed, 'trimap_x', (2, 3) + HW)
    t = np.stack([R.voronoi(1000 + 2 * seed, *HW, sites=5), R.voronoi(1001 + 2 * seed, *HW, sites=9)])
    t[0, 10:20, 40:60] = 255
    return x, torch.from_numpy(t)


def test_validation_step_and_exit_profile_with_trimap(dev):
    """Four different batches (two eager calls, the capture, a replay).  After every step the band matrices follow on the host from
    predictions() and the targets; result()'s cumulative matrices equal their sum, lie elementwise below the full matrix, and the twin
    built without the keyword reports the same bits.  ExitProfile on the same batches: the per-image band matrices sum to ValidationStep's,
    and the curve's end points are exit 0's and the final exit's."""
    from addk.exit_profile import ExitProfile
    from addk.metrics import mean_iou
    from addk.validate import ValidationStep
    m = _model(dev).eval()
    batches = [_batch(s) for s in (1, 2, 3, 4)]
    vs = ValidationStep(m, (2, 3) + HW, trimap=WIDTHS, keep_predictions=True)
    twin = ValidationStep(m, (2, 3) + HW)
    nex, nw = vs.nex, len(WIDTHS)
    want = np.zeros((nex, nw, NC, NC), dtype=np.int64)
    for x, t in batches:
        vs.step(x.to(dev), t.to(dev))
        twin.step(x.to(dev), t.to(dev))
        dist = R.dist_sep(t.numpy(), NC, WIDTHS[-1])
        assert np.array_equal(vs.dist.cpu().numpy(), dist)
        for k, p in enumerate(vs.predictions()):
            want[k] += R.banded_confusion(t.numpy(), p.cpu().numpy(), dist, NC, WIDTHS)
    assert vs.graph is not None and vs.batches == 4
    r, r0 = vs.result(), twin.result()
    assert r['trimap_widths'] == WIDTHS and 'trimap_widths' not in r0
    cum = want.cumsum(1)
    for k, (e, e0) in enumerate(zip(r['exits'], r0['exits'])):
        assert torch.equal(e['confusion'], e0['confusion']) and e['loss'] == e0['loss'] and e['confidence'] == e0['confidence']
        full = e['confusion'].cpu().numpy()
        sizes = []
        for j, b in enumerate(e['trimap']):
            got = b['confusion'].cpu().numpy()
            assert b['width'] == WIDTHS[j] and np.array_equal(got, cum[k, j]) and (got <= full).all()
            assert b['pixels'] == int(cum[k, j].sum()) and 0.0 <= b['mIoU'] <= 1.0
            sizes.append(b['pixels'])
        print('exit %d: mIoU %.4f, band pixels %s of %d, band mIoU %s' % (k, e['mIoU'], sizes, int(full.sum()),
                                                                        ['%.4f' % b['mIoU'] for b in e['trimap']]))
        assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] < int(full.sum())
    assert r['test_loss'] == r0['test_loss'] and r['new_pred'] == r0['new_pred']
    prof = ExitProfile(m, (2, 3) + HW, max_thresholds=(0.5,), trimap=WIDTHS)
    for x, t in batches:
        prof.step(x.to(dev), t.to(dev))
    assert prof.graph is not None
    rec = prof.records()
    assert tuple(rec['band_confusion'].shape) == (nex, 8, nw, NC, NC) and rec['trimap_widths'] == WIDTHS
    for k, e in enumerate(r['exits']):
        assert torch.equal(rec['confusion'][k].sum(0), e['confusion'].cpu())
        for j, b in enumerate(e['trimap']):
            assert torch.equal(rec['band_confusion'][k, :, j].sum(0), b['confusion'].cpu())
            s = rec['static'][k]['trimap'][j]
            assert torch.equal(s['confusion'], b['confusion'].cpu()) and s['mIoU'] == b['mIoU'] and s['pixels'] == b['pixels']
    hi, lo = float(rec['entropy'].max()) + 1.0, float(rec['entropy'].min()) - 1.0
    leave, stay = prof.curve('entropy', [hi, lo])
    assert leave['exit_counts'] == [8, 0] and stay['exit_counts'] == [0, 8]
    for pt, k in ((leave, 0), (stay, nex - 1)):
        for j, b in enumerate(pt['trimap']):
            ref = r['exits'][k]['trimap'][j]
            assert torch.equal(b['confusion'], ref['confusion'].cpu()) and b['pixels'] == ref['pixels']
            # the evaluator's formula on the same matrix: exactly on the device the curve computes on (the CPU); against the figure
            # from the GPU within the roundings of a 19-term fp32 mean of ratios (21 x 2^-24 < 2e-6), as tests/test_gpu_exit_profile.py
            assert b['mIoU'] == float(mean_iou(b['confusion'])) and abs(b['mIoU'] - ref['mIoU']) <= 2e-6 * ref['mIoU']
    vs.close(); twin.close(); prof.close()
