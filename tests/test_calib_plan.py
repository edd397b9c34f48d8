"""Host-logic tests of per-exit calibration (CPU, no GPU): addk.calibrate.ExitCalibration and the tempered plans are built with the kernel
launches stubbed out (the `dry` fixture of tests/_util.py) and their launch lists are inspected; the pure host functions of the fit and
of the reliability diagram; the C ABI of the new entry points.  Arithmetic is tests/test_gpu_calib.py and tests/test_gpu_calibrate.py."""
import collections
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import addk
import addk._lib as L
from _util import ARCH_C2, ARCH_C3, GENOTYPE_AUTODEEPLAB, dry, make_args      # noqa: F401  (dry: the shared dry-run fixture)
from test_exit_profile_plan import _has_full_resolution_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 65, 129)
X1 = (1, 3, 65, 129)
GRID = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0)


def _add(F=4, arch=ARCH_C2, classes=19):
    from addk.modeling.ADD import ADD
    return ADD(arch['network_arch'], arch['C_index'], GENOTYPE_AUTODEEPLAB, classes, make_args(F), arch['low_level_layer'])


def _names(g):
    return [c.name for c in g.fwd]


# ------------------------------------------------------------------------------------------------------------------------
# ExitCalibration
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arch,nex', [(ARCH_C2, 2), (ARCH_C3, 3)], ids=['c2', 'c3'])
def test_one_calib_launch_per_exit_and_no_full_resolution_logits(dry, arch, nex):
    from addk.calibrate import TEMPERATURES, ExitCalibration
    assert TEMPERATURES == GRID
    m = _add(4, arch)
    cal = ExitCalibration(m, SHAPE)
    names = collections.Counter(_names(cal.g))
    assert names['calib_upsample'] == nex == cal.nex == len(cal.outs)
    assert names['resize_nchw'] == names['score_upsample'] == names['gate_upsample'] == names['profile_upsample'] == 0
    assert names['bn_eval_affine_batch'] == 1 and names['bn_finalize'] == 0   # inference form
    assert not cal.g.bwd
    assert all(o.y is None and o.head == 'calib' and o.binding is not None and tuple(o.shape) == (2, 19, 65, 129) for o in cal.outs)
    assert not _has_full_resolution_buffer(cal.g, (2, 19, 65, 129))
    launches = [c for c in cal.g.fwd if c.name == 'calib_upsample']
    assert all(c.tag == 'decoder' for c in launches)
    assert m.training                                                         # the model's mode is not touched
    assert tuple(cal.bins.shape) == (nex, 8, 16, 3) and cal.bins.dtype == torch.int64
    assert tuple(cal.nll.shape) == (nex, 8) and cal.nll.dtype == torch.float64
    for k, c in enumerate(launches):                                          # every exit adds into its own slice
        a = c.args[0]._obj
        assert a.nt == 8 and a.inv_temp == cal.inv_temp.data_ptr() and a.target == cal.target.data_ptr()
        assert a.bins == cal.bins[k].data_ptr() and a.nll == cal.nll[k].data_ptr() and a.ws
    # two full batches and a short one; the stubbed launches leave zeros, the bookkeeping is what is checked
    x, t = torch.randn(SHAPE), torch.zeros((2, 65, 129), dtype=torch.int64)
    cal.step(x, t)
    cal.step(x, t)
    assert int((cal.target == 255).sum()) == 0
    cal.step(x, t, count=1)
    assert dry['calib_upsample'] == 3 * nex and cal.batches == 3 and cal.images == 5
    assert int((cal.target[0] == 255).sum()) == 0 and bool((cal.target[1] == 255).all())      # the missing image is painted over
    r = cal.result()
    assert len(r) == nex and r[0]['temperatures'] == GRID and r[0]['valid'] == 0
    assert tuple(r[0]['bins'].shape) == (8, 16, 2) and r[0]['bins'].dtype == torch.int64
    assert tuple(r[0]['conf_sum'].shape) == (8, 16) and r[0]['conf_sum'].dtype == torch.float64
    assert tuple(r[0]['nll'].shape) == tuple(r[0]['ece'].shape) == tuple(r[0]['mce'].shape) == (8,) and r[0]['nll'].dtype == torch.float64
    with pytest.raises(ValueError):
        cal.step(x, t, count=3)
    cal.bins.fill_(3)
    cal.reset()
    assert cal.batches == 0 and cal.images == 0 and int(cal.bins.abs().sum()) == 0


def test_result_and_fit_from_the_accumulators(dry):
    """result() and fit() on accumulators written by hand: units of 2^-24, means per valid pixel, the fit per exit."""
    from addk.calibrate import ExitCalibration
    cal = ExitCalibration(_add(4), SHAPE)
    unit = 2 ** 24
    cal.bins[:, :, 15] = torch.tensor([80, 60, 72 * unit])                    # top bin: 80 pixels, 60 right, mean confidence 0.9
    cal.bins[:, :, 3] = torch.tensor([20, 5, 4 * unit])                       # 20 pixels, 5 right, mean confidence 0.2
    for k, t_min in enumerate((1.4, 2.5)):
        cal.nll[k] = torch.tensor([100 * ((math.log(T) - math.log(t_min)) ** 2 + 0.3) for T in GRID], dtype=torch.float64)
    r = cal.result()
    assert r[0]['valid'] == 100 and r[0]['accuracy'] == 0.65
    assert abs(float(r[0]['nll'][2]) - (math.log(1.4) ** 2 + 0.3)) < 1e-15
    assert torch.allclose(r[0]['ece'], torch.full((8,), (12 + 1) / 100, dtype=torch.float64), atol=1e-15)
    assert torch.allclose(r[0]['mce'], torch.full((8,), 0.15, dtype=torch.float64), atol=1e-15)
    assert float(r[1]['conf_sum'][4, 15]) == 72.0 and r[1]['bins'][4, 3].tolist() == [20, 5]
    T = cal.fit()
    assert len(T) == 2 and abs(T[0] - 1.4) < 1e-12 and abs(T[1] - 2.5) < 1e-12
    ts, edges = cal.fit(with_edges=True)
    assert ts == T and edges == [False, False]


def test_temperatures_live_in_a_device_buffer(dry):
    from addk.calibrate import ExitCalibration
    cal = ExitCalibration(_add(4), SHAPE, temperatures=(0.5, 1.0, 4.0))
    assert cal.inv_temp.dtype == torch.float32 and cal.inv_temp.tolist() == [2.0, 1.0, 0.25]
    g0, graph0 = cal.g, cal.graph
    cal.bins.fill_(7)
    cal.set_temperatures((1.0, 2.0, 8.0))
    assert cal.g is g0 and cal.graph is graph0                                # nothing is rebuilt or captured again
    assert cal.inv_temp.tolist() == [1.0, 0.5, 0.125] and cal.temperatures == (1.0, 2.0, 8.0)
    assert int(cal.bins.abs().sum()) == 0                                     # the accumulators belonged to the old grid
    a = [c for c in g0.fwd if c.name == 'calib_upsample'][0].args[0]._obj
    assert a.inv_temp == cal.inv_temp.data_ptr() and a.nt == 3
    with pytest.raises(ValueError):
        cal.set_temperatures((1.0, 2.0))                                      # another length is another plan
    for bad in ((), (1.0, 1.0), (2.0, 1.0), (0.0, 1.0), (-1.0, 1.0), (1.0, float('inf')), (1.0, float('nan')),
                tuple(0.5 + 0.1 * i for i in range(9))):
        with pytest.raises(ValueError):
            ExitCalibration(_add(4), SHAPE, temperatures=bad)
        with pytest.raises(ValueError):
            cal.set_temperatures(bad)
    with pytest.raises(ValueError):
        ExitCalibration(_add(4), SHAPE, ignore_index=3)                       # one of the classes the evaluator counts


def test_unsupported_class_count_is_an_error(dry):
    from addk.calibrate import ExitCalibration
    with pytest.raises(addk.AddkError, match='19 classes'):
        ExitCalibration(_add(4, classes=7), (1, 3, 33, 65))


# ------------------------------------------------------------------------------------------------------------------------
# host functions
# ------------------------------------------------------------------------------------------------------------------------
def test_fit_temperature():
    from addk.calibrate import fit_temperature
    T, edge = fit_temperature(GRID, [(math.log(t) - math.log(1.4)) ** 2 + 0.3 for t in GRID])
    assert abs(T - 1.4) <= 1e-12 and edge is False
    assert fit_temperature(GRID, [math.log(t) for t in GRID]) == (0.5, True)          # monotone: the end point, and say so
    assert fit_temperature(GRID, [-math.log(t) for t in GRID]) == (5.0, True)
    assert fit_temperature(GRID, [1.0] * 8) == (0.5, True)
    # a skewed minimum: the vertex stays inside the neighbours' interval
    T, edge = fit_temperature((1.0, 2.0, 4.0), (1.0, 0.0, 1e9))
    assert 1.0 <= T <= 2.0 and not edge
    # a tie takes the first arg-min; the parabola through (2, 1, 1) has its vertex half way between the two in log T
    T, edge = fit_temperature((1.0, 2.0, 4.0, 8.0), (2.0, 1.0, 1.0, 2.0))
    assert abs(T - math.sqrt(8.0)) < 1e-12 and not edge
    with pytest.raises(ValueError):
        fit_temperature(GRID, [1.0, 2.0])


def test_reliability_on_hand_written_bins():
    from addk.calibrate import reliability
    bins = torch.zeros((16, 2), dtype=torch.int64)
    conf = torch.zeros(16, dtype=torch.float64)
    bins[15], conf[15] = torch.tensor([80, 60]), 72.0                          # accuracy 0.75, confidence 0.9
    bins[3], conf[3] = torch.tensor([20, 5]), 4.0                              # accuracy 0.25, confidence 0.2
    r = reliability(bins, conf)
    assert abs(r['ece'] - (12 + 1) / 100) < 1e-15 and abs(r['mce'] - 0.15) < 1e-15
    assert abs(float(r['accuracy'][15]) - 0.75) < 1e-15 and abs(float(r['confidence'][15]) - 0.9) < 1e-15
    assert abs(float(r['accuracy'][3]) - 0.25) < 1e-15 and abs(float(r['confidence'][3]) - 0.2) < 1e-15
    assert bool(torch.isnan(r['accuracy'][0])) and bool(torch.isnan(r['confidence'][0]))      # an empty bin has neither
    perfect = reliability(torch.tensor([[0, 0]] * 15 + [[10, 10]]), torch.tensor([0.0] * 15 + [10.0]))
    assert perfect['ece'] == 0.0 and perfect['mce'] == 0.0
    empty = reliability(torch.zeros((16, 2), dtype=torch.int64), torch.zeros(16))
    assert math.isnan(empty['ece']) and math.isnan(empty['mce'])


# ------------------------------------------------------------------------------------------------------------------------
# tempered plans
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('output,plain', [('logits', 'gate_upsample'), ('labels', 'gate_label_upsample')])
def test_gate_plan_differs_only_in_the_gate_launch(dry, output, plain):
    from addk.dynamic import GatePlan
    m = _add(4, ARCH_C3)
    x = torch.randn(X1)
    a, b = GatePlan(m, x, 'entropy', output), GatePlan(m, x, 'entropy', output, temperature=(1.5, 2.0, 1.0))
    na, nb = _names(a.g), _names(b.g)
    assert collections.Counter(na)[plain] == 2 and 'gate_upsample_t' not in na                  # today's launch names
    assert len(na) == len(nb) and {(u, v) for u, v in zip(na, nb) if u != v} == {(plain, 'gate_upsample_t')}
    assert a.trunk_end == b.trunk_end and a.head_rng == b.head_rng
    assert a._temp is None and a.temperature is None
    assert b.temperature == (1.5, 2.0, 1.0) and b._temp.tolist() == [torch.tensor(1 / 1.5).item(), 0.5]      # the gates' words: exits 0, 1
    gates = [c.args[0]._obj for c in b.g.fwd if c.name == 'gate_upsample_t']
    assert [g.inv_temp for g in gates] == [b._temp.data_ptr(), b._temp.data_ptr() + 4]
    assert all(bool(g.labels) == (output == 'labels') for g in gates)
    g0 = b.g
    b.set_temperature(3.0)
    assert b.g is g0 and b._temp.tolist() == [torch.tensor(1 / 3.0).item()] * 2 and b.temperature == (3.0, 3.0, 3.0)
    with pytest.raises(ValueError):
        a.set_temperature(2.0)                                                                   # the untempered plan has no word
    with pytest.raises(ValueError):
        b.set_temperature(None)


def test_dynamic_inference_temperature_arguments(dry):
    from addk.modeling.ADD import EDM
    m = _add(4)
    x = torch.randn(X1)
    m.dynamic_inference(x, 0.5, confidence='entropy')
    assert dry['gate_upsample'] == 1 and dry['gate_upsample_t'] == 0
    plain = m._gate_plan(x, 'entropy')
    y, early, _, val = m.dynamic_inference(x, float('inf'), confidence='entropy', temperature=2.0)
    assert dry['gate_upsample_t'] == 1 and early == 1 and tuple(y.shape) == (1, 19, 65, 129)      # output='logits': the exit's logits
    tempered = m._gate_plan(x, 'entropy', temperature=2.0)
    assert tempered is not plain and m._gate_plan(x, 'entropy') is plain                           # None: today's plan under today's key
    assert tempered.temperature == (2.0, 2.0)
    m.dynamic_inference(x, 0.5, confidence='entropy', temperature=[1.6, 4.0])
    assert m._gate_plan(x, 'entropy', temperature=[1.6, 4.0]) is tempered                         # the key records only that it is tempered
    assert tempered.temperature == (1.6, 4.0) and tempered._temp.tolist() == [0.625]
    m.dynamic_inference(x, 0.5, confidence='max', output='labels', temperature=1.0)
    assert m._gate_plan(x, 'max', 'labels', None, temperature=1.0) is not m._gate_plan(x, 'max', 'labels')
    for bad in ([1.0], [1.0, 2.0, 3.0], 0.0, -1.0, float('inf'), float('nan'), [1.0, 0.0]):
        with pytest.raises(ValueError):
            m.dynamic_inference(x, 0.5, confidence='entropy', temperature=bad)
        with pytest.raises(ValueError):
            m.dynamic_inference_batch(torch.randn(SHAPE), 0.5, confidence='entropy', temperature=bad)
    with pytest.raises(ValueError):
        m.dynamic_inference(x, 0.5, confidence='edm', edm=EDM().eval(), temperature=2.0)
    with pytest.raises(ValueError):
        m.dynamic_inference_batch(torch.randn(SHAPE), 0.5, confidence='edm', temperature=2.0)


def test_batched_gate_temperature(dry):
    from addk.dynamic import BatchedGate
    m = _add(4)
    a, b = BatchedGate(m, SHAPE, 'max'), BatchedGate(m, SHAPE, 'max', temperature=[2.0, 1.0])
    na, nb = _names(a.sub(2).g), _names(b.sub(2).g)
    assert {(u, v) for u, v in zip(na, nb) if u != v} == {('gate_label_upsample', 'gate_upsample_t')} and len(na) == len(nb)
    assert b.sub(2)._temp.tolist() == [0.5] and b.sub(1)._temp.tolist() == [0.5]
    b.set_temperature(4.0)
    assert b.sub(2)._temp.tolist() == [0.25] and b.sub(1)._temp.tolist() == [0.25]
    assert b.sub(2).temperature == (4.0, 4.0)
    with pytest.raises(ValueError):
        a.set_temperature(2.0)
    x = torch.randn(SHAPE)
    m.dynamic_inference_batch(x, 0.5, confidence='max')
    m.dynamic_inference_batch(x, 0.5, confidence='max', temperature=2.0)
    keys = [k for k in m._plans() if k[0] == 'dynb']
    assert len(keys) == 2 and sorted(len(k) for k in keys) == [5, 6] and [k for k in keys if len(k) == 6][0][-1] == 'tempered'


def test_exit_profile_differs_only_in_the_profile_launch(dry):
    from addk.exit_profile import ExitProfile
    m = _add(4, ARCH_C3)
    a, b = ExitProfile(m, SHAPE), ExitProfile(m, SHAPE, temperature=[1.5, 2.0, 4.0])
    na, nb = _names(a.g), _names(b.g)
    assert collections.Counter(na)['profile_upsample'] == 3 and 'profile_upsample_t' not in na    # today's launch names
    assert len(na) == len(nb) and {(u, v) for u, v in zip(na, nb) if u != v} == {('profile_upsample', 'profile_upsample_t')}
    assert a.temp is None and b.temp.tolist() == [torch.tensor(1 / 1.5).item(), 0.5, 0.25]        # every exit has its word
    launches = [c.args[0]._obj for c in b.g.fwd if c.name == 'profile_upsample_t']
    assert [t.inv_temp for t in launches] == [b.temp.data_ptr() + 4 * k for k in range(3)]
    assert all(t.profile.nthr == 3 and t.profile.thr == b.thr.data_ptr() for t in launches)
    g0 = b.g
    b.step()
    b.set_temperature(2.0)
    assert b.g is g0 and b.temp.tolist() == [0.5] * 3 and b.batches == 0                           # new words, empty logs, the same plan
    with pytest.raises(ValueError):
        a.set_temperature(2.0)
    for bad in ([1.0, 2.0], 0.0, [1.0, 2.0, float('nan')]):
        with pytest.raises(ValueError):
            ExitProfile(m, SHAPE, temperature=bad)


def test_a_tempered_gate_has_no_stand_alone_form(dry, monkeypatch):
    from addk.dynamic import GatePlan
    monkeypatch.setenv('ADDK_FUSE_GATE', '0')
    GatePlan(_add(4), torch.randn(X1), 'entropy')                                                  # the untempered plan has one
    with pytest.raises(addk.AddkError, match='tempered gate'):
        GatePlan(_add(4), torch.randn(X1), 'entropy', temperature=2.0)


# ------------------------------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------------------------------
NAMES = ('addk_calib_upsample', 'addk_calib_upsample_supported', 'addk_calib_upsample_ws_bytes', 'addk_gate_upsample_t',
         'addk_profile_upsample_t')
STRUCTS = {'addk_calib_upsample_args': L.CalibUpsampleArgs, 'addk_gate_upsample_t_args': L.GateUpsampleTArgs,
           'addk_profile_upsample_t_args': L.ProfileUpsampleTArgs, 'addk_gate_upsample_args': L.GateUpsampleArgs,
           'addk_profile_upsample_args': L.ProfileUpsampleArgs}


def test_calib_abi_declared_and_exported():
    lib = addk.load()
    text = open(os.path.join(ROOT, 'include', 'addk.h')).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert int(re.search(r'#define ADDK_CALIB_MAX_T (\d+)', text).group(1)) == L.CALIB_MAX_T == 8
    assert int(re.search(r'#define ADDK_CALIB_BINS (\d+)', text).group(1)) == L.CALIB_BINS == 16
    fields = [f for f, _ in L.CalibUpsampleArgs._fields_]
    assert fields[:8] == [f for f, _ in L.GateUpsampleArgs._fields_][:8]      # the prefix the heads share
    assert fields[8:] == ['target', 'inv_temp', 'nt', 'bins', 'nll', 'ws']
    # the tempered structs embed the untempered ones, whose layout stays
    assert L.GateUpsampleTArgs._fields_[0] == ('gate', L.GateUpsampleArgs) and L.ProfileUpsampleTArgs._fields_[0] == ('profile', L.ProfileUpsampleArgs)
    assert ctypes.sizeof(L.GateUpsampleArgs) == 72 and ctypes.sizeof(L.ProfileUpsampleArgs) == 104
    sup = lib.addk_calib_upsample_supported
    score = lib.addk_score_upsample_supported
    for shape in ((2, 9, 17, 65, 129, 19), (1, 4, 4, 128, 128, 19), (2, 9, 17, 65, 129, 21), (2, 0, 17, 65, 129, 19), (70000, 9, 17, 65, 129, 19)):
        for nt in (0, 1, 8, 9, -1):
            assert sup(*shape, nt) == (1 if score(*shape) == 1 and 1 <= nt <= 8 else 0), (shape, nt)
    # the ticket, then per 64 x 32 tile eight NLL partials, then 32 replicas of the 8 x 16 x 3 counters
    assert lib.addk_calib_upsample_ws_bytes(2, 65, 129) == 16 + 32 * 2 * 3 * 3 + 32 * 8 * 16 * 3 * 8
    assert lib.addk_calib_upsample_ws_bytes(0, 65, 129) == 0


def test_calib_args_layouts_match_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "addk.h"', 'int main(void){']
    for cname, cls in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in cls._fields_]
    lines += ['return 0;}']
    c = tmp_path / 'abi.c'
    c.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
