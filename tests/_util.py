"""Shared helpers for tests and for tests/golden/make_golden.py (no reference code here)."""
import collections
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import addk  # noqa: F401  (registers the package that lives in ./auto-dynamic-deeplab_amd/)

GENOTYPE_AUTODEEPLAB = np.array(  # searched_arch/autodeeplab/genotype.npy (data; unsorted rows 8,9 — SURVEY Q1)
    [[0, 7], [1, 4], [2, 4], [3, 6], [5, 4], [8, 4], [11, 5], [13, 5], [19, 7], [18, 5]], dtype=np.int64)
GENOTYPE_BASELINE_2 = np.array(   # searched_arch/searched_baseline/genotype_2.npy (data; rows 4,5 unsorted)
    [[0, 7], [1, 4], [2, 6], [4, 4], [8, 6], [5, 4], [9, 6], [11, 7], [14, 7], [16, 5]], dtype=np.int64)
GENOTYPE_40_1 = np.array(         # searched_arch/40_5e_38_lr/genotype_1.npy (data; three unsorted pairs)
    [[1, 5], [0, 4], [2, 4], [4, 4], [5, 4], [8, 5], [13, 5], [12, 4], [18, 5], [14, 4]], dtype=np.int64)
NETWORK_PATH_BASELINE = [0, 1, 2, 2, 3, 2, 2, 1, 2, 1, 1, 2]  # searched_baseline/network_path.npy (data)
ARCH_C2 = dict(network_arch=[1, 2, 2, 2, 3, 2, 2, 1, 1, 1, 1, 2], C_index=[5], low_level_layer=0)  # train.py:75-79
ARCH_C3 = dict(network_arch=[1, 2, 3, 2, 2, 3, 2, 3, 2, 3, 2, 3], C_index=[3, 7], low_level_layer=0)  # train.py:80-83
ARCH_C4 = dict(network_arch=[1, 2, 3, 3, 2, 3, 3, 3, 3, 3, 2, 2], C_index=[2, 5, 8], low_level_layer=0)  # train.py:84-87


def make_args(F=20, B=5, sync_bn=False):
    return SimpleNamespace(F=F, B=B, sync_bn=sync_bn)


from addk.synth import _rng, fill_params, rand_tensor     # noqa: E402,F401  (the product's own synthetic-data helpers)


def probe_weights(seed, name, shape):
    """Fixed pseudo-random cotangent used to turn an output into a scalar loss."""
    return rand_tensor(seed, 'probe:' + name, shape)


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rms_err(a, b):
    """rms(a - b) / rms(b): unlike rel_err (max-abs / max-abs) every element counts, so the small-magnitude elements are constrained too
    (VERDICT r03 weak 1e).  Asserted beside rel_err by tests/test_gpu_parity.py::_chk at the same tolerance."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float(((a - b) ** 2).mean().sqrt() / ((b ** 2).mean().sqrt() + 1e-300))


@contextlib.contextmanager
def dry_run():
    """Stub the launches and accept CPU tensors, so that plans are built without a GPU exactly as they are built on one.  Yields the
    counter of the launches a replay would have made, by command name."""
    import addk.plan as P
    calls = collections.Counter()

    def fake_run(self, cmds, stream):
        for name, fn, args in cmds:
            calls[name] += 1
    saved = P.Graph.run, P.require_device, P.current_stream
    P.Graph.run, P.require_device, P.current_stream = fake_run, lambda x: None, lambda: 0
    try:
        yield calls
    finally:
        P.Graph.run, P.require_device, P.current_stream = saved


@pytest.fixture()
def dry():
    """dry_run() around one test (the plan dry-run test files import this fixture)"""
    with dry_run() as calls:
        yield calls
