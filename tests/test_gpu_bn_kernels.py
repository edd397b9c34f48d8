"""Kernel-level tests of training-mode BatchNorm and the elementwise kernels around it (csrc/bn.hip, csrc/elementwise.hip, the GAP kernels
of csrc/misc.hip), called through the C ABI and compared with fp64 evaluations, on the GPU, of the same fp32 inputs the kernels read.

Shapes: first those config 2's train plan runs at 2x1024x2048 (the NET_* tables; tests/test_bn_shapes.py dry-builds that plan and fails
when it runs a shape the tables do not list), then the rest of the C ABI contract at modest sizes.  Every output, slab and workspace holds
NaN before a launch, so an element a kernel does not write fails its comparison.

Bounds follow the arithmetic (U = 2^-24 is the fp32 unit roundoff, an fp32 ulp of S is at most 2U*S):
 * outputs computed in fp64 and rounded once to fp32 (a, b, mean, invstd, running statistics, dgamma, dbeta, c1, c2, dmv): 4U*S, with S
   the sum of the magnitudes of the terms of the defining formula, plus the fp64 summation bound (rows + 64) * 2^-53 * sum|terms|;
 * fp64 sums of exact fp32 products (slab_reduce, the dab rows of affine_sum_bwd / gap_bwd): 1e-12 of sum|terms| per channel, so one
   pixel dropped or counted twice out of 10^5 (~1e-5) cannot pass;
 * fp32 elementwise outputs (affine_sum out, g, bn_bwd_apply out, SGD): (terms + 2) fp32 ulps of the sum of the magnitudes of that
   element's terms, on every element;
 * GAP: _gap_bound.
Table-driven batched launches are held bit-identical to the single launches, the vector kernels bit-identical to the generic ones.
Every measured error / bound goes to bn_kernel_errors.txt in the directory ADDK_REPORT_DIR names (the system's temporary directory
when it is unset)."""
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import addk  # noqa: F401  (registers the package)
from addk import _lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # fp32 unit roundoff: one rounding to fp32 moves a value by at most U * |value|
ULP = 2.0 ** -23         # an fp32 ulp of S is at most ULP * S
E64 = 2.0 ** -53         # fp64 unit roundoff
MOM, EPS = C.c_float(0.1).value, C.c_float(1e-5).value      # BatchNorm momentum and eps as the kernels read them (fp32)
f64 = torch.float64

# ---- config 2's train plan at 2x1024x2048 (F = 20, ARCH_C2), one launch per BatchNorm (ADDK_LEVEL_BATCH=0) ----
# (C, count) of every BatchNorm: bn_finalize, bn_bwd and bn_bwd_apply (whose P is the count)
NET_BN = [(64, 1048576), (128, 262144), (40, 65536), (40, 63250), (80, 16384), (80, 16002), (160, 4096), (256, 16384), (256, 2),
          (48, 65536), (256, 65536)]
# (C, count, rows) of the statistics slabs bn_finalize reads
NET_FIN = [(64, 1048576, 1024), (128, 262144, 1024), (40, 65536, 1024), (40, 63250, 989), (80, 16384, 512), (80, 16002, 501),
           (160, 4096, 128), (256, 16384, 512), (256, 2, 1), (48, 65536, 1024), (256, 65536, 1024)]
# (C, count, slab rows) of every distinct slab list bn_bwd sums
NET_BWD = [
    (40, 63250, (501,)), (40, 63250, (501, 989)), (40, 63250, (501, 989, 989)), (40, 63250, (512,)), (40, 63250, (512, 512, 989)),
    (40, 63250, (512, 989)), (40, 63250, (989,)), (40, 63250, (1024,)),
    (40, 65536, (501, 989, 989, 989, 989, 501, 501, 128, 512)), (40, 65536, (512,)), (40, 65536, (512, 512, 1024)),
    (40, 65536, (512, 1024)), (40, 65536, (1024,)),
    (48, 65536, (1024, 1024)), (64, 1048576, (1024,)), (64, 1048576, (1024, 1024)),
    (80, 16002, (256,)), (80, 16002, (256, 256, 501)), (80, 16002, (256, 501)), (80, 16002, (501,)), (80, 16002, (501, 989, 989, 989)),
    (80, 16002, (501, 989, 989, 989, 989)), (80, 16002, (666,)),
    (80, 16384, (128, 501, 501, 501, 512, 989, 989, 989, 989)), (80, 16384, (128, 501, 501, 501, 989, 989, 989, 989)), (80, 16384, (256,)),
    (80, 16384, (256, 256, 512)), (80, 16384, (256, 512)), (80, 16384, (501, 501, 501, 989, 989, 989, 989)), (80, 16384, (512,)),
    (80, 16384, (682,)),
    (128, 262144, (512, 1024, 1024)),
    (160, 4096, (128,)), (160, 4096, (128, 341)), (160, 4096, (128, 341, 341)), (160, 4096, (341,)),
    (160, 4096, (501, 501, 989, 989, 989, 989)),
    (256, 2, (1,)), (256, 16384, (512,)), (256, 16384, (1024,)), (256, 65536, (1024,))]
# (P, C, nterm, ldo) of the branch sums affine_sum / affine_sum_bwd (ldo: the concat buffer's row, lddo in the backward)
NET_AFFINE = [(65536, 40, 2, 200), (63250, 40, 2, 200), (16384, 80, 2, 400), (16002, 80, 2, 400), (4096, 160, 2, 800)]
# (P, C, nterm, ldo) of affine_sum as the classifier's bias-gradient accumulation (_colsum: one plain term, accumulate)
NET_BIAS_ACC = [(1, 19, 1, 19)]
# (C, ld, N, HW, mean, relu, lazy BN) of the GAP launches: the ASPP image pool, the classifier bias gradient (_colsum), _colsum_n
NET_GAP = [(400, 400, 2, 8192, 1, 1, False), (19, 20, 1, 65536, 0, 0, False), (256, 256, 2, 8192, 0, 0, False)]

REPORT = []


def _log(fmt, *a):
    REPORT.append(fmt % a)


def teardown_module(module):
    d = os.environ.get('ADDK_REPORT_DIR') or tempfile.gettempdir()
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'bn_kernel_errors.txt'), 'w') as f:
        f.write('\n'.join(REPORT) + '\n')


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _randn(gen, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen, device='cuda', dtype=dtype)


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen, device='cuda')


def _sign(gen, *shape):
    return torch.where(_rand(gen, *shape) < 0.5, -1.0, 1.0)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _p(t):
    return None if t is None else t.data_ptr()


def _table(structs):
    """A device table of argument structs, uploaded as Graph._table does: the bytes of a ctypes array in a uint8 tensor."""
    arr = (type(structs[0]) * len(structs))(*structs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _src(x, a=None, b=None, relu=0):
    s = L.Src()
    s.x, s.a, s.b, s.ld, s.C, s.relu, s.rs_hw = x.data_ptr(), _p(a), _p(b), x.stride(0), x.shape[1], int(relu), 0
    return s


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == f64 else torch.int32)


def _same_bits(what, a, b):
    d = int((_bits(a) != _bits(b)).sum())
    assert d == 0, '%s: not bit-identical (%d elements differ)' % (what, d)


def _close(what, got, ref, bound):
    """Every element of `got` written (no NaN left) and within `bound` of the fp64 `ref`; logs the largest error / bound."""
    nn = int(torch.isnan(got).sum())
    assert nn == 0, '%s: %d elements not written' % (what, nn)
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(r.max())
    _log('%-78s err/bound %.3f  max err %.2e', what, worst, float(err.max()))
    assert worst <= 1.0, '%s: error %.3e is %.2f x its bound (flat index %d)' % (what, float(err.reshape(-1)[int(r.argmax())]), worst,
                                                                               int(r.argmax()))


def _margin(z, S):
    """Where a ReLU mask is ambiguous: the kernel decides on fmaf in fp32, the reference in fp64; keep |z| > 1e-3 * S."""
    return z.abs() <= 1e-3 * S


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. statistics -> affine (forward)
# ------------------------------------------------------------------------------------------------------------------------------------
def _samples(gen, n, Cc, loc=0.1, scale=1.0):
    """n fp32 samples of Cc channels: per-channel offsets of size ~loc, spreads of size ~scale."""
    mu = loc * (1 + _rand(gen, Cc)) * _sign(gen, Cc)
    sd = scale * (0.5 + _rand(gen, Cc))
    return (mu + sd * _randn(gen, n, Cc)).float()


def _slab(x, rows):
    """fp64 [rows][C][2] (sum x, sum x^2) of the samples x [n][C] split into `rows` consecutive pixel ranges, as a producing kernel
    writes it."""
    n, Cc = x.shape
    k = -(-n // rows)
    xd = torch.zeros(rows * k, Cc, dtype=f64, device='cuda')
    xd[:n] = x
    xd = xd.view(rows, k, Cc)
    return torch.stack((xd.sum(1), (xd * xd).sum(1)), -1).contiguous()


class Fin:
    """One bn_finalize call: a statistics slab, parameters, running statistics, NaN-filled outputs."""

    def __init__(self, gen, Cc, count, rows, loc=0.1, affine=True, running=True, stats_out=True, x=None):
        self.C, self.count, self.rows, self.stats_out = Cc, count, rows, stats_out
        self.slab = _slab(x if x is not None else _samples(gen, count, Cc, loc), rows)
        self.gamma = (1 + 0.3 * _randn(gen, Cc)) if affine else None
        self.beta = 0.5 * _randn(gen, Cc) if affine else None
        self.rm0 = 0.2 * _randn(gen, Cc) if running else None
        self.rv0 = (0.5 + _rand(gen, Cc)) if running else None
        self.reset()

    def reset(self):
        self.out = {k: _nan(self.C) for k in ('a', 'b', 'mean', 'invstd')}
        self.rm = None if self.rm0 is None else self.rm0.clone()
        self.rv = None if self.rv0 is None else self.rv0.clone()

    def args(self, partial=None):
        fa = L.BnFinalizeArgs()
        fa.partial, fa.rows = (_p(self.slab), self.rows) if partial is None else (_p(partial), 1)
        fa.C, fa.count = self.C, float(self.count)
        fa.gamma, fa.beta, fa.running_mean, fa.running_var = _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv)
        fa.momentum, fa.eps = MOM, EPS
        fa.a, fa.b = _p(self.out['a']), _p(self.out['b'])
        if self.stats_out:
            fa.mean, fa.invstd = _p(self.out['mean']), _p(self.out['invstd'])
        return fa

    def results(self):
        r = dict(self.out) if self.stats_out else {k: self.out[k] for k in 'ab'}
        if self.rm is not None:
            r['running_mean'], r['running_var'] = self.rm, self.rv
        return r

    def check(self, tag):
        s, sa = self.slab.sum(0), self.slab.abs().sum(0)
        n = float(self.count)
        tol = 4 * U + (self.rows + 64) * E64               # one rounding to fp32 (with room) + fp64 summation in any order
        mean = s[:, 0] / n
        var = (s[:, 1] / n - mean * mean).clamp_min(0)
        Sm, Sv = sa[:, 0] / n, sa[:, 1] / n + mean * mean   # magnitudes of the terms of the mean and of the variance
        ve = var + EPS
        invstd = ve.rsqrt()
        k = 1 + 0.5 * Sv / ve                               # invstd moves by k * d (relative) when the terms of var move by d
        g = self.gamma.double() if self.gamma is not None else torch.ones_like(mean)
        be = self.beta.double() if self.beta is not None else torch.zeros_like(mean)
        a = g * invstd
        _close(tag + ' a', self.out['a'], a, tol * a.abs() * k)
        _close(tag + ' b', self.out['b'], be - mean * a, tol * (be.abs() + a.abs() * (mean.abs() * k + Sm)))
        if self.stats_out:
            _close(tag + ' mean', self.out['mean'], mean, tol * Sm)
            _close(tag + ' invstd', self.out['invstd'], invstd, tol * invstd * k)
        if self.rm is not None:
            f = n / (n - 1) if n > 1 else 1.0               # the running variance is the unbiased one
            rm0, rv0 = self.rm0.double(), self.rv0.double()
            _close(tag + ' running_mean', self.rm, (1 - MOM) * rm0 + MOM * mean, tol * ((1 - MOM) * rm0.abs() + MOM * Sm))
            _close(tag + ' running_var', self.rv, (1 - MOM) * rv0 + MOM * f * var, tol * ((1 - MOM) * rv0.abs() + MOM * f * Sv))


def _finalize_all(lib, fins, tag):
    """Each call as a single launch against fp64, then all of them in ONE bn_finalize_batch table: bit-identical."""
    for f in fins:
        L.check(lib.addk_bn_finalize(C.byref(f.args()), _st()), 'bn_finalize')
        f.check('%s finalize C=%d count=%d rows=%d' % (tag, f.C, f.count, f.rows))
    single = [f.results() for f in fins]
    for f in fins:
        f.reset()
    tab = _table([f.args() for f in fins])
    L.check(lib.addk_bn_finalize_batch(tab.data_ptr(), len(fins), max(f.C for f in fins), _st()), 'bn_finalize_batch')
    for f, ref in zip(fins, single):
        for k, v in f.results().items():
            _same_bits('%s finalize_batch C=%d rows=%d %s' % (tag, f.C, f.rows, k), v, ref[k])


def test_bn_finalize_at_network_shapes(lib):
    gen = _gen(1)
    _finalize_all(lib, [Fin(gen, Cc, count, rows) for Cc, count, rows in NET_FIN], 'net')


def test_bn_finalize_edges(lib):
    """slab_sum's 8 x 64 unrolled batches (447 / 449 / 501 rows; the tail's eighth row w[7] is never in range — the unrolled loop runs
    while r + 448 < rows — so 501, 666 and 989 rows are what reach its seventh), the 2-sample BatchNorm of the image pool and its SyncBN count (16) with
    one slab row, |mean| >> std (the E[x^2] - E[x]^2 form in fp64), gamma / beta NULL, no running statistics, no mean / invstd output,
    C % 16 != 0 and C = 1 (a partly used channel block)."""
    gen = _gen(2)
    fins = [Fin(gen, 40, 447 * 3, 447), Fin(gen, 40, 449 * 3, 449), Fin(gen, 19, 501 * 2, 501),
            Fin(gen, 256, 2, 1), Fin(gen, 256, 16, 1), Fin(gen, 256, 2, 1, loc=300.0),
            Fin(gen, 80, 16002, 989, loc=100.0), Fin(gen, 160, 4096, 341, loc=1000.0),
            Fin(gen, 48, 5000, 666, affine=False), Fin(gen, 37, 3000, 128, running=False, stats_out=False),
            Fin(gen, 1, 1000, 449), Fin(gen, 1024, 2048, 512)]
    _finalize_all(lib, fins, 'edge')


def test_slab_reduce_and_the_syncbn_finalize(lib):
    """slab_reduce (single and batched) against an fp64 sum; then the SyncBN-shaped finalize (the reduced row, rows = 1) gives what the
    direct finalize gives, bit for bit: at world 1 the exchange adds nothing.  count 16 = the image pool's count at world 8 (8 ranks x 2)."""
    gen = _gen(3)
    fins = [Fin(gen, 40, 63250, 989), Fin(gen, 80, 16002, 501), Fin(gen, 256, 16, 8), Fin(gen, 64, 1048576, 1024), Fin(gen, 19, 999, 449)]
    reds = []
    for f in fins:
        red = _nan(f.C, 2, dtype=f64)
        it = L.SlabReduceItem()
        it.partial, it.out, it.rows, it.C = f.slab.data_ptr(), red.data_ptr(), f.rows, f.C
        L.check(lib.addk_slab_reduce(C.byref(it), _st()), 'slab_reduce')
        _close('slab_reduce C=%d rows=%d' % (f.C, f.rows), red, f.slab.sum(0), 1e-12 * f.slab.abs().sum(0))
        reds.append(red)
    outs = [_nan(f.C, 2, dtype=f64) for f in fins]
    items = []
    for f, o in zip(fins, outs):
        it = L.SlabReduceItem()
        it.partial, it.out, it.rows, it.C = f.slab.data_ptr(), o.data_ptr(), f.rows, f.C
        items.append(it)
    tab = _table(items)
    L.check(lib.addk_slab_reduce_batch(tab.data_ptr(), len(items), max(f.C for f in fins), _st()), 'slab_reduce_batch')
    for f, r, o in zip(fins, reds, outs):
        _same_bits('slab_reduce_batch C=%d rows=%d' % (f.C, f.rows), o, r)
    for f, red in zip(fins, reds):
        L.check(lib.addk_bn_finalize(C.byref(f.args()), _st()), 'bn_finalize')
        direct = f.results()
        f.reset()
        L.check(lib.addk_bn_finalize(C.byref(f.args(partial=red)), _st()), 'bn_finalize (reduced row)')
        f.check('syncbn-shaped finalize C=%d count=%d' % (f.C, f.count))
        for k, v in f.results().items():
            _same_bits('syncbn-shaped finalize C=%d %s' % (f.C, k), v, direct[k])


def test_bn_eval_affine(lib):
    """a = gamma / sqrt(rv + eps), b = beta - rm * a in fp32 (three roundings in a, two more in b), single and batched."""
    gen = _gen(4)
    cases = []
    for Cc, affine in ((40, True), (19, True), (256, False), (1024, True), (1600, True), (1, True)):
        e = dict(C=Cc, gamma=(1 + 0.3 * _randn(gen, Cc)) if affine else None, beta=_randn(gen, Cc) if affine else None,
                 rm=_randn(gen, Cc), rv=0.01 + 2 * _rand(gen, Cc), a=_nan(Cc), b=_nan(Cc))
        x = L.BnEvalItem()
        x.gamma, x.beta, x.running_mean, x.running_var, x.a, x.b = _p(e['gamma']), _p(e['beta']), _p(e['rm']), _p(e['rv']), _p(e['a']), _p(e['b'])
        x.C, x.eps = Cc, EPS
        L.check(lib.addk_bn_eval_affine(C.byref(x), _st()), 'bn_eval_affine')
        g = e['gamma'].double() if affine else 1.0
        be = e['beta'].double() if affine else torch.zeros(Cc, dtype=f64, device='cuda')
        rm = e['rm'].double()
        a = g / (e['rv'].double() + EPS).sqrt()
        ea = 8 * U * a.abs()
        _close('bn_eval_affine C=%d a' % Cc, e['a'], a, ea)
        _close('bn_eval_affine C=%d b' % Cc, e['b'], be - rm * a, 8 * U * (be.abs() + (rm * a).abs()) + rm.abs() * ea)
        cases.append(e)
    ents = []
    for e in cases:
        x = L.BnEvalItem()
        e['a2'], e['b2'] = _nan(e['C']), _nan(e['C'])
        x.gamma, x.beta, x.running_mean, x.running_var, x.a, x.b = _p(e['gamma']), _p(e['beta']), _p(e['rm']), _p(e['rv']), _p(e['a2']), _p(e['b2'])
        x.C, x.eps = e['C'], EPS
        ents.append(x)
    tab = _table(ents)
    L.check(lib.addk_bn_eval_affine_batch(tab.data_ptr(), len(ents), _st()), 'bn_eval_affine_batch')
    for e in cases:
        _same_bits('bn_eval_affine_batch C=%d a' % e['C'], e['a2'], e['a'])
        _same_bits('bn_eval_affine_batch C=%d b' % e['C'], e['b2'], e['b'])


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. BatchNorm backward coefficients
# ------------------------------------------------------------------------------------------------------------------------------------
class Bwd:
    """One bn_bwd call: (dA, dB) slabs [rows][C][2] as affine_sum_bwd / the dgrad kernels write them, the saved statistics, outputs.
    route 'c': c1 / c2 directly; 'dmv': (dmean, dvar) for the SyncBN exchange."""

    def __init__(self, gen, Cc, count, rows, centered=1, affine=True, accumulate=0, route='c', slabs=None, stats=None):
        self.C, self.count, self.centered, self.acc, self.route = Cc, count, centered, accumulate, route
        self.slabs = slabs if slabs is not None else [_randn(gen, r, Cc, 2, dtype=f64) + 0.1 for r in rows]
        if stats is not None:
            self.gamma, self.mean, self.invstd, self.a = stats
        else:
            self.mean = 2 * _randn(gen, Cc)
            self.invstd = 0.5 + 1.5 * _rand(gen, Cc)
            self.gamma = (1 + 0.3 * _randn(gen, Cc)) if affine else None
            self.a = (self.invstd * (self.gamma if affine else 1.0)).float()     # the lazy scale bn_finalize wrote
        self.old = (_randn(gen, Cc), _randn(gen, Cc)) if accumulate else None
        self.reset()

    def reset(self):
        Cc = self.C
        if self.gamma is not None:
            self.dg, self.db = (self.old[0].clone(), self.old[1].clone()) if self.acc else (_nan(Cc), _nan(Cc))
        else:
            self.dg = self.db = None
        self.c1, self.c2 = (_nan(Cc), _nan(Cc)) if self.route == 'c' else (None, None)
        self.dmv = _nan(Cc, 2) if self.route == 'dmv' else None

    def args(self):
        ba = L.BnBwdArgs()
        for i, s in enumerate(self.slabs):
            ba.slab[i], ba.rows[i] = s.data_ptr(), s.shape[0]
        ba.nslab, ba.C, ba.count = len(self.slabs), self.C, float(self.count)
        ba.gamma, ba.mean, ba.invstd, ba.a = _p(self.gamma), _p(self.mean), _p(self.invstd), _p(self.a)
        ba.dgamma, ba.dbeta, ba.accumulate = _p(self.dg), _p(self.db), int(self.acc)
        ba.c1, ba.c2, ba.dmv, ba.centered = _p(self.c1), _p(self.c2), _p(self.dmv), int(self.centered)
        return ba

    def results(self):
        r = {}
        for k in ('dg', 'db', 'c1', 'c2', 'dmv'):
            if getattr(self, k) is not None:
                r[k] = getattr(self, k)
        return r

    def ref(self):
        """(value, S, fp64 noise) of dgamma, dbeta, dvar, dmean, c1, c2 from the definitions:
        dA = sum dz*x, dB = sum dz, dgamma = invstd (dA - mu dB), dvar = -1/2 gamma invstd^3 (dA - mu dB),
        dmean = -a dB - [not centered] 2 mu dvar, c1 = dmean / n, c2 = 2 dvar / n."""
        allr = torch.cat(self.slabs)
        s, sa = allr.sum(0), allr.abs().sum(0)
        nz = (allr.shape[0] + 64) * E64
        dA, dB = s[:, 0], s[:, 1]
        mu, iv, av = self.mean.double(), self.invstd.double(), self.a.double()
        g = self.gamma.double() if self.gamma is not None else torch.ones_like(mu)
        n = float(self.count)
        t = dA - mu * dB
        St, Nt = dA.abs() + (mu * dB).abs(), nz * (sa[:, 0] + mu.abs() * sa[:, 1])
        k = 0.5 * g.abs() * iv ** 3
        dvar = -0.5 * g * t * iv ** 3
        nc = 0.0 if self.centered else 1.0
        R = dict(dg=(iv * t, iv * St, iv * Nt), db=(dB, dB.abs(), nz * sa[:, 1]), dvar=(dvar, k * St, k * Nt),
                 dmean=(-av * dB - nc * 2 * mu * dvar, (av * dB).abs() + nc * 2 * mu.abs() * k * St, av.abs() * nz * sa[:, 1] + nc * 2 * mu.abs() * k * Nt))
        R['c1'] = tuple(v / n for v in R['dmean'])
        R['c2'] = tuple(2 * v / n for v in R['dvar'])
        return R

    def check(self, tag):
        R = self.ref()

        def chk(name, got, key, old=None):
            v, S, N = R[key]
            if old is not None:
                v, S = old.double() + v, old.double().abs() + S
            _close('%s %s' % (tag, name), got, v, 4 * U * S + N)
        if self.dg is not None:
            chk('dgamma', self.dg, 'dg', self.old[0] if self.acc else None)
            chk('dbeta', self.db, 'db', self.old[1] if self.acc else None)
        if self.c1 is not None:
            chk('c1', self.c1, 'c1')
            chk('c2', self.c2, 'c2')
        if self.dmv is not None:
            chk('dmv.dmean', self.dmv[:, 0], 'dmean')
            chk('dmv.dvar', self.dmv[:, 1], 'dvar')
        return R


def _tag(b):
    return 'C=%d count=%d slabs=%s centered=%d acc=%d %s%s' % (b.C, b.count, tuple(s.shape[0] for s in b.slabs), b.centered, b.acc,
                                                            b.route, '' if b.gamma is not None else ' gamma=NULL')


def _bwd_all(lib, bs, tag):
    """Single launches against fp64, then all in ONE bn_bwd_batch table: bit-identical."""
    for b in bs:
        L.check(lib.addk_bn_bwd(C.byref(b.args()), _st()), 'bn_bwd')
        b.check('%s bn_bwd %s' % (tag, _tag(b)))
    single = [b.results() for b in bs]
    for b in bs:
        b.reset()
    tab = _table([b.args() for b in bs])
    L.check(lib.addk_bn_bwd_batch(tab.data_ptr(), len(bs), max(b.C for b in bs), _st()), 'bn_bwd_batch')
    for b, ref in zip(bs, single):
        for k, v in b.results().items():
            _same_bits('%s bn_bwd_batch %s %s' % (tag, _tag(b), k), v, ref[k])


def test_bn_bwd_at_network_shapes(lib):
    gen = _gen(5)
    _bwd_all(lib, [Bwd(gen, Cc, count, rows) for Cc, count, rows in NET_BWD], 'net')


NINE = (501, 989, 989, 989, 989, 501, 501, 128, 512)       # the 9-slab list of a level-1 BatchNorm, C = 40


@pytest.mark.parametrize('centered', [0, 1])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_bn_bwd_variants_and_the_dmv_route(lib, centered, accumulate):
    """centered 0 / 1, accumulate 0 / 1 into dgamma / dbeta, gamma NULL, and both outputs: c1 / c2 directly, or dmv followed by
    bn_bwd_coeffs (and its batch form).  At world 1 the dmv route gives c1 / c2 within ONE extra rounding of the direct route:
    dmv rounds (dmean, dvar) to fp32 once more before the division by the count, so the two results are at most one fp32 ulp apart."""
    gen = _gen(6 + 2 * centered + accumulate)
    cases = [(40, 63250, NINE), (80, 16002, (256, 501, 666, 682, 989)), (19, 777, (447, 449)), (256, 2, (1,)), (1024, 4096, (64, 3))]
    direct, viadmv = [], []
    for Cc, count, rows in cases:
        b = Bwd(gen, Cc, count, rows, centered=centered, accumulate=accumulate)
        direct.append(b)
        viadmv.append(Bwd(gen, Cc, count, rows, centered=centered, accumulate=accumulate, route='dmv', slabs=b.slabs,
                          stats=(b.gamma, b.mean, b.invstd, b.a)))
        viadmv[-1].old = b.old
        viadmv[-1].reset()
    nog = Bwd(gen, 40, 63250, NINE, centered=centered, affine=False)
    _bwd_all(lib, direct + [nog], 'variant')
    _bwd_all(lib, viadmv, 'variant')
    coeffs, items = [], []
    for b, d in zip(viadmv, direct):
        c1, c2 = _nan(b.C), _nan(b.C)
        one = L.BnCoeffsItem()
        one.dmv, one.c1, one.c2, one.count, one.C = b.dmv.data_ptr(), c1.data_ptr(), c2.data_ptr(), float(b.count), b.C
        L.check(lib.addk_bn_bwd_coeffs(C.byref(one), _st()), 'bn_bwd_coeffs')
        R = b.ref()
        for name, got, dir_ in (('c1', c1, d.c1), ('c2', c2, d.c2)):
            v, S, N = R[name]
            _close('variant coeffs_from_dmv %s %s' % (_tag(b), name), got, v, 4 * U * S + N)
            one_ulp = 2 * U * torch.maximum(got.double().abs(), dir_.double().abs())
            _close('variant dmv route vs direct %s %s' % (_tag(b), name), got, dir_.double(), one_ulp)
        coeffs.append((c1, c2))
        it = L.BnCoeffsItem()
        it.dmv, it.count, it.C = b.dmv.data_ptr(), float(b.count), b.C
        items.append(it)
    outs = [(_nan(b.C), _nan(b.C)) for b in viadmv]
    for it, (o1, o2) in zip(items, outs):
        it.c1, it.c2 = o1.data_ptr(), o2.data_ptr()
    tab = _table(items)
    L.check(lib.addk_bn_bwd_coeffs_batch(tab.data_ptr(), len(items), max(b.C for b in viadmv), _st()), 'bn_bwd_coeffs_batch')
    for b, (c1, c2), (o1, o2) in zip(viadmv, coeffs, outs):
        _same_bits('variant coeffs_batch %s c1' % _tag(b), o1, c1)
        _same_bits('variant coeffs_batch %s c2' % _tag(b), o2, c2)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. applying the BatchNorm backward: out = g + c1 + c2 * (x - mean)
# ------------------------------------------------------------------------------------------------------------------------------------
def _apply_ref(g, x, mean, c1, c2):
    """fp64 value and bound: three terms (g, c1, c2 * (x - mean)), three fp32 roundings (x - mean, the fma, the add): 5 ulps of S."""
    gd = g.double()
    if c1 is None:
        return gd, torch.zeros_like(gd)
    xd = x.double()
    mu = mean.double() if mean is not None else torch.zeros(g.shape[1], dtype=f64, device='cuda')
    k1, k2 = c1.double(), c2.double()
    return gd + k1 + k2 * (xd - mu), 5 * ULP * (gd.abs() + k1.abs() + k2.abs() * (xd.abs() + mu.abs()))


def _apply_vecs(gen, Cc):
    return _randn(gen, Cc), 0.5 * _randn(gen, Cc), 0.5 * _randn(gen, Cc)         # mean, c1, c2


def _apply(lib, g, x, mean, c1, c2, out):
    P, Cc = g.shape
    it = L.BnApplyItem()
    it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = g.data_ptr(), _p(x), _p(c1), _p(c2), _p(mean), out.data_ptr(), P
    it.ldg, it.ldx, it.ldo, it.C = g.stride(0), x.stride(0) if x is not None else 0, out.stride(0), Cc
    L.check(lib.addk_bn_bwd_apply(C.byref(it), _st()), 'bn_bwd_apply')


def test_bn_bwd_apply_in_place_at_network_shapes(lib):
    gen = _gen(10)
    for Cc, P in NET_BN:
        g, x = _randn(gen, P, Cc), _randn(gen, P, Cc) + 0.5
        mean, c1, c2 = _apply_vecs(gen, Cc)
        g0 = g.clone()
        _apply(lib, g, x, mean, c1, c2, g)
        _close('net bn_bwd_apply in place C=%d P=%d' % (Cc, P), g, *_apply_ref(g0, x, mean, c1, c2))
        del g, x, g0
        torch.cuda.empty_cache()


def test_bn_bwd_apply_batch_bit_identical_to_single_launches(lib):
    """Items of different P and C in one table, one of P = 1 048 576 beside items of 4 096 (the grid is sized by max_P), items with
    ld > C (a concat slot), one with mean NULL."""
    gen = _gen(11)
    specs = [(1048576, 64, 64, 64, True), (4096, 160, 160, 800, True), (4096, 40, 40, 200, False), (4096, 48, 52, 48, True),
             (2, 256, 256, 256, True), (16002, 80, 80, 400, True), (63250, 40, 44, 40, True)]       # (P, C, ldg = ldo, ldx, mean)
    items, singles, outs = [], [], []
    for P, Cc, ldg, ldx, has_mean in specs:
        gb, xb = _randn(gen, P, ldg), _randn(gen, P, ldx) + 0.5
        g, x = gb[:, :Cc], xb[:, :Cc]
        mean, c1, c2 = _apply_vecs(gen, Cc)
        mean = mean if has_mean else None
        s = gb.clone()
        _apply(lib, s[:, :Cc], x, mean, c1, c2, s[:, :Cc])
        _close('bn_bwd_apply single C=%d P=%d ldg=%d ldx=%d' % (Cc, P, ldg, ldx), s[:, :Cc], *_apply_ref(g, x, mean, c1, c2))
        _same_bits('bn_bwd_apply single: columns past C untouched', s[:, Cc:], gb[:, Cc:])
        singles.append(s)
        o = gb.clone()
        outs.append(o)
        it = L.BnApplyItem()
        it.g, it.x, it.c1, it.c2, it.mean, it.out, it.P = o.data_ptr(), x.data_ptr(), c1.data_ptr(), c2.data_ptr(), _p(mean), o.data_ptr(), P
        it.ldg, it.ldx, it.ldo, it.C = ldg, ldx, ldg, Cc
        items.append((it, x, c1, c2, mean))
    tab = _table([i[0] for i in items])
    L.check(lib.addk_bn_bwd_apply_batch(tab.data_ptr(), len(items), max(s[0] for s in specs), _st()), 'bn_bwd_apply_batch')
    for (P, Cc, ldg, ldx, _), s, o in zip(specs, singles, outs):
        _same_bits('bn_bwd_apply_batch C=%d P=%d' % (Cc, P), o, s)


@pytest.mark.parametrize('Cc,P', [(40, 4099), (64, 3), (1024, 2), (4, 1), (256, 65537)])
def test_bn_bwd_apply_vector_and_generic_kernels_agree(lib, Cc, P):
    """The same values through the vector kernel (16-byte aligned, ld % 4 == 0) and the generic one (ld % 4 != 0): bit-identical, and
    both against fp64; with mean NULL, and with c1 / c2 NULL (out = g)."""
    gen = _gen(12 + Cc + P)
    g, x = _randn(gen, P, Cc), _randn(gen, P, Cc) - 0.3
    mean, c1, c2 = _apply_vecs(gen, Cc)
    gq, xq = _nan(P, Cc + 1), _nan(P, Cc + 1)
    gq[:, :Cc], xq[:, :Cc] = g, x
    for m, k1, k2, name in ((mean, c1, c2, 'full'), (None, c1, c2, 'mean=NULL'), (mean, None, None, 'c1/c2=NULL')):
        ov, og = _nan(P, Cc), _nan(P, Cc + 1)
        _apply(lib, g, x if k1 is not None else None, m, k1, k2, ov)
        _apply(lib, gq[:, :Cc], xq[:, :Cc] if k1 is not None else None, m, k1, k2, og[:, :Cc])
        _close('bn_bwd_apply vector C=%d P=%d %s' % (Cc, P, name), ov, *_apply_ref(g, x, m, k1, k2))
        _same_bits('bn_bwd_apply generic == vector C=%d P=%d %s' % (Cc, P, name), og[:, :Cc], ov)
        assert torch.isnan(og[:, Cc]).all(), 'generic bn_bwd_apply wrote past C'


@pytest.mark.parametrize('Cc,ld,P', [(19, 20, 65536), (19, 19, 777), (1, 1, 3), (3, 5, 2), (38, 40, 1), (1021, 1023, 5)])
def test_bn_bwd_apply_generic_channel_tails(lib, Cc, ld, P):
    """C % 4 != 0: the generic kernel's guarded loads and stores (ld4g / st4g with nrem < 4)."""
    gen = _gen(13 + Cc)
    gb, xb = _randn(gen, P, ld), _randn(gen, P, ld)
    mean, c1, c2 = _apply_vecs(gen, Cc)
    ob = _nan(P, ld)
    _apply(lib, gb[:, :Cc], xb[:, :Cc], mean, c1, c2, ob[:, :Cc])
    _close('bn_bwd_apply generic C=%d ld=%d P=%d' % (Cc, ld, P), ob[:, :Cc], *_apply_ref(gb[:, :Cc], xb[:, :Cc], mean, c1, c2))
    assert torch.isnan(ob[:, Cc:]).all(), 'bn_bwd_apply wrote past C'


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. branch sum: out = relu_out?(sum_i relu_i?(a_i x_i + b_i)) (+ out), and its gradient with the per-channel (dA, dB) sums
# ------------------------------------------------------------------------------------------------------------------------------------
class Term:
    def __init__(self, gen, P, Cc, ld, lazy=True, relu=False):
        self.xb = _nan(P, ld)
        self.x = self.xb[:, :Cc]
        self.x.copy_(_randn(gen, P, Cc) + 0.2)
        self.a = ((0.5 + _rand(gen, Cc)) * _sign(gen, Cc)) if lazy else None
        self.b = 0.3 * _randn(gen, Cc) if lazy else None
        self.relu = relu

    def z(self):
        """fp64 a*x + b and the magnitude of its terms."""
        x = self.x.double()
        if self.a is None:
            return x, x.abs()
        ax = self.a.double() * x
        return ax + self.b.double(), ax.abs() + self.b.double().abs()

    def src(self):
        return _src(self.x, self.a, self.b, self.relu)


def _settle_masks(gen, terms, relu_out):
    """Redraw the x of every term where a ReLU (per term, or on the sum) would decide within 1e-3 of its terms' magnitude."""
    for _ in range(100):
        bad = torch.zeros(terms[0].x.shape, dtype=torch.bool, device='cuda')
        s, S = 0.0, 0.0
        for t in terms:
            z, Sz = t.z()
            if t.relu:
                bad |= _margin(z, Sz)
                z = z.clamp_min(0)
            s, S = s + z, S + Sz
        if relu_out:
            bad |= _margin(s, S)
        nb = int(bad.sum())
        if nb == 0:
            return
        for t in terms:
            t.x[bad] = _randn(gen, nb) + 0.2
    raise AssertionError('could not draw mask-safe data')


def _affine_fwd(lib, terms, P, Cc, ldo, slot, relu_out, accumulate, gen, tag):
    outb = _nan(P, ldo)
    out = outb[:, slot * Cc:(slot + 1) * Cc]
    old = None
    if accumulate:
        out.copy_(_randn(gen, P, Cc))
        old = out.double()
    ar = L.AffineSumArgs()
    for i, t in enumerate(terms):
        ar.term[i] = t.src()
    ar.nterm, ar.P, ar.C, ar.out, ar.ldo, ar.relu_out, ar.accumulate = len(terms), P, Cc, out.data_ptr(), ldo, int(relu_out), int(accumulate)
    L.check(lib.addk_affine_sum_fwd(C.byref(ar), _st()), 'affine_sum_fwd')
    s, S = 0.0, 0.0
    for t in terms:
        z, Sz = t.z()
        s, S = s + (z.clamp_min(0) if t.relu else z), S + Sz
    if relu_out:
        s = s.clamp_min(0)
    if old is not None:
        s, S = s + old, S + old.abs()
    _close('%s affine_sum out' % tag, out, s, (len(terms) + int(accumulate) + 2) * ULP * S)
    rest = torch.cat((outb[:, :slot * Cc], outb[:, (slot + 1) * Cc:]), 1)
    assert torch.isnan(rest).all(), '%s: affine_sum wrote outside its slot' % tag
    return outb, out


def _affine_bwd(lib, terms, P, Cc, dout, fout, relu_out, spec, gen, tag, ldg=None):
    """spec per term: string of 'g' (gradient), 'd' (dab slab), 'a' (accumulate into g).  Returns the g and dab tensors."""
    rows = int(lib.addk_ew_rows(P, Cc))
    ba = L.AffineSumBwdArgs()
    gs, gbs, dabs, olds = [], [], [], []
    for i, (t, sp) in enumerate(zip(terms, spec)):
        ba.term[i] = t.src()
        g = gb = old = dab = None
        if 'g' in sp:
            gb = _nan(P, ldg or Cc)
            g = gb[:, :Cc]
            if 'a' in sp:
                g.copy_(_randn(gen, P, Cc))
                old = g.double()
            ba.g[i], ba.ldg[i], ba.accumulate[i] = g.data_ptr(), gb.stride(0), int('a' in sp)
        if 'd' in sp:
            dab = _nan(rows, Cc, 2, dtype=f64)
            ba.dab[i] = dab.data_ptr()
        gs.append(g)
        gbs.append(gb)
        dabs.append(dab)
        olds.append(old)
    ba.nterm, ba.P, ba.C, ba.dout, ba.lddo = len(terms), P, Cc, dout.data_ptr(), dout.stride(0)
    if relu_out:
        ba.out, ba.ldo = fout.data_ptr(), fout.stride(0)
    ba.relu_out = int(relu_out)
    L.check(lib.addk_affine_sum_bwd(C.byref(ba), _st()), 'affine_sum_bwd')
    d = dout.double()
    if relu_out:
        d = d * (fout > 0)
    for i, (t, g, gb, dab, old) in enumerate(zip(terms, gs, gbs, dabs, olds)):
        z, _ = t.z()
        dm = d * (z > 0) if t.relu else d
        if g is not None:
            a = t.a.double() if t.a is not None else 1.0
            ref, S = dm * a, (dm * a).abs()
            if old is not None:
                ref, S = ref + old, S + old.abs()
            _close('%s affine_sum_bwd g[%d]' % (tag, i), g, ref, (1 + int(old is not None) + 2) * ULP * S)
            assert torch.isnan(gb[:, Cc:]).all(), '%s: affine_sum_bwd wrote g[%d] past C' % (tag, i)
        if dab is not None:
            x = t.x.double()
            nn = int(torch.isnan(dab).sum())
            assert nn == 0, '%s: %d of the %d x %d dab[%d] slab entries not written' % (tag, nn, rows, 2 * Cc, i)
            got = dab.sum(0)
            ref = torch.stack(((dm * x).sum(0), dm.sum(0)), -1)
            S = torch.stack(((dm * x).abs().sum(0), dm.abs().sum(0)), -1)
            _close('%s affine_sum_bwd dab[%d] (%d rows)' % (tag, i, rows), got, ref, 1e-12 * S)
    return gs, dabs


def _generic_copy(t, P, Cc):
    """The same term with x in a buffer of row stride C + 1: not 16-byte vectorisable, the generic kernel runs."""
    q = Term.__new__(Term)
    q.xb = _nan(P, Cc + 1)
    q.x = q.xb[:, :Cc]
    q.x.copy_(t.x)
    q.a, q.b, q.relu = t.a, t.b, t.relu
    return q


def test_affine_sum_at_network_shapes(lib):
    """The network's form: two lazy-BN terms, no ReLU, written into one slot of the 5 C concat buffer; the backward reads the slot's
    gradient and writes g and the dab slab of each term.  Then the same data through the generic kernel (x copied to row stride C + 1):
    g and dab bit-identical to the vector kernel's (the claim at affine_sum_bwd_vec_kernel)."""
    gen = _gen(20)
    for P, Cc, nterm, ldo in NET_AFFINE:
        tag = 'net P=%d C=%d nterm=%d ldo=%d' % (P, Cc, nterm, ldo)
        terms = [Term(gen, P, Cc, Cc) for _ in range(nterm)]
        slot = ldo // Cc - 2
        _affine_fwd(lib, terms, P, Cc, ldo, slot, False, False, gen, tag)
        doutb = _randn(gen, P, ldo)
        dout = doutb[:, slot * Cc:(slot + 1) * Cc]
        gv, dv = _affine_bwd(lib, terms, P, Cc, dout, None, False, ['gd'] * nterm, gen, tag + ' vector')
        gg, dg = _affine_bwd(lib, [_generic_copy(t, P, Cc) for t in terms], P, Cc, dout, None, False, ['gd'] * nterm, gen, tag + ' generic')
        for i in range(nterm):
            _same_bits('%s generic == vector g[%d]' % (tag, i), gg[i], gv[i])
            _same_bits('%s generic == vector dab[%d]' % (tag, i), dg[i], dv[i])


@pytest.mark.parametrize('P,Cc,nterm,ldo', NET_BIAS_ACC)
def test_affine_sum_bias_gradient_accumulate(lib, P, Cc, nterm, ldo):
    """_colsum adds the classifier's column sums into the bias gradient: one plain term, P = 1, C = 19, accumulate."""
    gen = _gen(21)
    terms = [Term(gen, P, Cc, Cc, lazy=False) for _ in range(nterm)]
    _affine_fwd(lib, terms, P, Cc, ldo, 0, False, True, gen, 'net bias gradient P=%d C=%d' % (P, Cc))


# (P, C, [(lazy, relu, ld)], ldo, slot, relu_out, accumulate, backward spec per term)
AFFINE_CASES = [
    (1000, 40, [(True, False, 40)], 40, 0, False, False, ['gd']),
    (3001, 40, [(True, True, 40), (False, False, 40), (True, False, 44)], 120, 1, True, True, ['gda', 'd', 'g']),
    (2050, 64, [(True, True, 64), (True, True, 68), (False, True, 64), (True, False, 64)], 64, 0, True, False, ['gd', 'ga', 'gd', 'd']),
    (777, 19, [(True, True, 19), (True, False, 20)], 20, 0, False, True, ['gda', 'gd']),
    (3, 1024, [(True, True, 1024), (True, False, 1024)], 1024, 0, True, False, ['gd', 'gd']),
    (1, 40, [(True, False, 40), (True, True, 40)], 80, 1, False, True, ['gd', 'gda']),
    (2, 80, [(True, False, 80), (True, False, 80), (True, True, 80)], 80, 0, True, False, ['d', 'g', 'gd']),
    (5003, 12, [(True, True, 12), (True, False, 12)], 60, 3, False, False, ['gd', 'gd']),
]


@pytest.mark.parametrize('case', range(len(AFFINE_CASES)))
def test_affine_sum_contract(lib, case):
    """nterm 1-4, per-term ReLU, relu_out (the backward masks by the forward output), output and per-term accumulate, g[i] NULL with dab[i]
    set and the reverse, C % 4 != 0 (generic ld4g / nrem kernels), C = 1024, P = 1, 2, 3."""
    P, Cc, tspec, ldo, slot, relu_out, acc, bspec = AFFINE_CASES[case]
    gen = _gen(30 + case)
    terms = [Term(gen, P, Cc, ld, lazy, relu) for lazy, relu, ld in tspec]
    _settle_masks(gen, terms, relu_out)
    tag = 'contract P=%d C=%d nterm=%d relu_out=%d acc=%d' % (P, Cc, len(terms), relu_out, acc)
    outb, out = _affine_fwd(lib, terms, P, Cc, ldo, slot, relu_out, acc, gen, tag)
    doutb = _randn(gen, P, ldo + 4)
    dout = doutb[:, :Cc]
    _affine_bwd(lib, terms, P, Cc, dout, out, relu_out, bspec, gen, tag, ldg=Cc + 4 if case % 2 else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. GAP and column sums
# ------------------------------------------------------------------------------------------------------------------------------------
def _ew_map(n):
    nq = min(256, (n + 3) // 4)
    return nq, max(1, 256 // nq)


def _gap_bound(Cc, N, HW, rows, Sz, y):
    """gap_partial adds a thread's ceil(HW / (rows * npl)) = L pixels in fp32, then the block adds its npl lanes one after the other in
    fp32; gap_final adds the rows in fp64 and scales: (L + npl + 1) * U * sum |terms| (the +1: the lazy prologue's fma) + 2 U |y|
    (the final rounding, and 1/HW rounded to fp32)."""
    worst = 0
    for c0 in range(0, Cc, 1024):
        nq, npl = _ew_map(min(1024, Cc - c0))
        worst = max(worst, -(-HW // (rows * npl)) + npl)
    return (worst + 1) * U * Sz + 2 * U * y.abs()


def _gap_fwd(lib, gen, Cc, ld, N, HW, mean, relu, lazy, tag, loc=0.3):
    t = Term(gen, N * HW, Cc, ld, lazy, relu)
    t.x.add_(loc)
    if relu:
        _settle_masks(gen, [t], False)
    rows = int(lib.addk_ew_rows(HW, Cc))
    y, ws = _nan(N, Cc + 3), _nan(N * rows * Cc)
    L.check(lib.addk_gap_fwd(C.byref(t.src()), N, HW, y.data_ptr(), Cc + 3, ws.data_ptr(), int(mean), _st()), 'gap_fwd')
    z, Sz = t.z()
    if relu:
        z = z.clamp_min(0)
    scale = 1.0 / HW if mean else 1.0
    ref = z.view(N, HW, Cc).sum(1) * scale
    Sz = Sz.view(N, HW, Cc).sum(1) * scale
    _close('%s gap_fwd C=%d ld=%d N=%d HW=%d mean=%d relu=%d lazy=%d' % (tag, Cc, ld, N, HW, mean, relu, lazy), y[:, :Cc], ref,
           _gap_bound(Cc, N, HW, rows, Sz, ref))
    assert torch.isnan(y[:, Cc:]).all(), 'gap_fwd wrote past C'
    z32 = z.float().view(N, HW, Cc)
    t32 = (z32.mean(1) if mean else z32.sum(1)).double()
    _log('    (torch fp32 %s of the same terms: max err %.2e, ours %.2e)', 'mean' if mean else 'sum', float((t32 - ref).abs().max()),
         float((y[:, :Cc].double() - ref).abs().max()))


@pytest.mark.parametrize('g', range(len(NET_GAP)))
def test_gap_fwd_at_network_uses(lib, g):
    """The ASPP image pool (C = 400, N = 2, HW = 8192, mean, ReLU), _colsum (the classifier's bias gradient: C = 19 at ld 20, N = 1,
    HW = 65536, plain sum — the only C % 4 != 0 launch of these kernels in the network), _colsum_n (C = 256, N = 2, HW = 8192)."""
    Cc, ld, N, HW, mean, relu, lazy = NET_GAP[g]
    _gap_fwd(lib, _gen(40 + g), Cc, ld, N, HW, mean, relu, lazy, 'net')


@pytest.mark.parametrize('Cc,ld,N,HW,mean,relu,lazy', [(1600, 1600, 2, 512, 1, 1, True), (40, 44, 3, 1000, 1, 1, True),
                                                      (1024, 1024, 1, 3, 0, 0, True), (5, 7, 2, 1, 1, 1, True)])
def test_gap_fwd_contract(lib, Cc, ld, N, HW, mean, relu, lazy):
    """C = 1600 (two channel chunks: F = 40's ASPP input), a lazy BatchNorm prologue, HW not a power of two, HW = 1."""
    _gap_fwd(lib, _gen(50 + Cc), Cc, ld, N, HW, mean, relu, lazy, 'contract')


@pytest.mark.parametrize('Cc,ld,N,HW,relu,lazy,acc,dab', [(400, 400, 2, 8192, 1, False, 0, False), (400, 400, 2, 8192, 1, True, 1, True),
                                                         (1600, 1600, 2, 512, 1, True, 0, True), (19, 20, 3, 1000, 1, True, 1, True),
                                                         (256, 256, 2, 1, 0, True, 0, True)])
def test_gap_bwd(lib, Cc, ld, N, HW, relu, lazy, acc, dab):
    """g = relu mask * (dy / HW) * a (+ g), and the (dA, dB) slab rows of the lazy BatchNorm: the ReLU prologue with and without a lazy
    BatchNorm, accumulate, C = 1600 (two chunk launches into one slab)."""
    gen = _gen(60 + Cc + HW)
    P = N * HW
    t = Term(gen, P, Cc, ld, lazy, relu)
    if relu:
        _settle_masks(gen, [t], False)
    dy = _randn(gen, N, Cc)
    gb = _nan(P, Cc + 4)
    g = gb[:, :Cc]
    old = None
    if acc:
        g.copy_(_randn(gen, P, Cc))
        old = g.double()
    rows = int(lib.addk_ew_rows(P, Cc))
    slab = _nan(rows, Cc, 2, dtype=f64) if dab else None
    L.check(lib.addk_gap_bwd(C.byref(t.src()), N, HW, dy.data_ptr(), Cc, g.data_ptr(), Cc + 4, acc, _p(slab), _st()), 'gap_bwd')
    inv = torch.ones((), device='cuda') / HW                        # 1/HW in fp32, as the kernel scales dy
    d = (dy * inv).repeat_interleave(HW, 0).double()               # dy / HW rounded to fp32: exact for the powers of two of the network
    z, _ = t.z()
    dm = d * (z > 0) if relu else d
    a = t.a.double() if lazy else 1.0
    ref, S = dm * a, (dm * a).abs()
    if old is not None:
        ref, S = ref + old, S + old.abs()
    tag = 'gap_bwd C=%d N=%d HW=%d relu=%d lazy=%d acc=%d' % (Cc, N, HW, relu, lazy, acc)
    _close(tag + ' g', g, ref, (1 + acc + 2) * ULP * S)
    assert torch.isnan(gb[:, Cc:]).all(), 'gap_bwd wrote past C'
    if dab:
        assert not torch.isnan(slab).any(), '%s: dab rows not written' % tag
        x = t.x.double()
        _close(tag + ' dab (%d rows)' % rows, slab.sum(0), torch.stack(((dm * x).sum(0), dm.sum(0)), -1),
               1e-12 * torch.stack(((dm * x).abs().sum(0), dm.abs().sum(0)), -1))


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. SGD
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nesterov', [0, 1])
@pytest.mark.parametrize('n', [1031, 4 * 1024 * 1024 + 5 * 256 + 3])
def test_sgd_step(lib, n, nesterov):
    """Three steps (first = 1, then 0) with weight decay and gscale != 1; n not a multiple of the grid (the larger n makes every thread
    take several trips).  Each step against an fp64 evaluation of torch.optim.SGD's update of the same fp32 state: d = g*gscale + wd*w,
    buf = d (first) or mom*buf + d, step = d + mom*buf (nesterov) or buf, w -= lr*step — six fp32 roundings, 8 ulps of the magnitudes.
    After three steps against torch.optim.SGD itself in fp32 on the GPU."""
    gen = _gen(70 + nesterov)
    mom, wd, gscale = C.c_float(0.9).value, C.c_float(4e-5).value, C.c_float(0.125).value
    lr = torch.tensor([0.05], device='cuda')
    lrv = float(lr)
    p = _randn(gen, n)
    buf = _nan(n)
    pt = torch.nn.Parameter(p.clone())
    opt = torch.optim.SGD([pt], lr=lrv, momentum=mom, weight_decay=wd, nesterov=bool(nesterov), foreach=False)
    Smax = 0.0
    for step in range(3):
        g = _randn(gen, n)
        p0, b0 = p.double(), buf.double()
        first = int(step == 0)
        L.check(lib.addk_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, lr.data_ptr(), mom, wd, nesterov, first, gscale, _st()),
                'sgd_step')
        gd = g.double() * gscale
        d, Sd = gd + wd * p0, gd.abs() + wd * p0.abs()
        b, Sb = (d, Sd) if first else (mom * b0 + d, mom * b0.abs() + Sd)
        s, Ss = (d + mom * b, Sd + mom * Sb) if nesterov else (b, Sb)
        tag = 'sgd n=%d nesterov=%d step %d' % (n, nesterov, step)
        _close(tag + ' buf', buf, b, 8 * ULP * Sb)
        Sp = p0.abs() + lrv * Ss
        _close(tag + ' param', p, p0 - lrv * s, 8 * ULP * Sp)
        Smax = max(Smax, float(Sp.max()))
        pt.grad = g * gscale
        opt.step()
    diff = float((p.double() - pt.detach().double()).abs().max())
    _log('sgd n=%d nesterov=%d: max |addk - torch.optim.SGD fp32| after 3 steps %.2e (bound %.2e)', n, nesterov, diff, 3 * 16 * ULP * Smax)
    assert diff <= 3 * 16 * ULP * Smax


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. the chain: statistics -> affine -> branch sum -> its backward -> BatchNorm backward, against fp64 autograd
# ------------------------------------------------------------------------------------------------------------------------------------
def _errs(got, ref):
    e = got.double() - ref
    return float(e.pow(2).mean().sqrt()), float(e.abs().max())


def _compare(tag, ours, t32, ref, floor):
    """rms and max-abs error of ours within 2x PyTorch fp32's own error on the same inputs, plus a floor of `floor` ulps of the output's
    scale."""
    (ro, mo), (rt, mt) = _errs(ours, ref), _errs(t32, ref)
    fl = floor * ULP * float(ref.abs().max())
    _log('%-56s rms %.2e (torch fp32 %.2e, ratio %.2f)  max %.2e (torch fp32 %.2e, ratio %.2f)', tag, ro, rt, ro / max(rt, 1e-300), mo, mt,
         mo / max(mt, 1e-300))
    assert ro <= 2 * rt + fl and mo <= 2 * mt + fl, (tag, ro, rt, mo, mt, fl)


def _bn_torch(xs, gams, bets, dy, dtype, relu=False):
    """fp64 / fp32 autograd of sum_i relu?(batch_norm(x_i, training=True)) against dy."""
    xs, ws, bs = ([v.detach().to(dtype).clone().requires_grad_() for v in vs] for vs in (xs, gams, bets))
    rms = [torch.zeros(x.shape[1], dtype=dtype, device='cuda') for x in xs]
    rvs = [torch.ones(x.shape[1], dtype=dtype, device='cuda') for x in xs]
    y = 0
    for x, w, b, rm, rv in zip(xs, ws, bs, rms, rvs):
        z = F.batch_norm(x, rm, rv, w, b, True, MOM, EPS)
        y = y + (F.relu(z) if relu else z)
    (y * dy.to(dtype)).sum().backward()
    return dict(y=y.detach(), dx=[x.grad for x in xs], dgamma=[w.grad for w in ws], dbeta=[b.grad for b in bs], rm=rms, rv=rvs)


def _chain_stats(lib, gen, xs, rows, gams, bets):
    fins = []
    for x, g, b in zip(xs, gams, bets):
        f = Fin(gen, x.shape[1], x.shape[0], rows, x=x)
        f.gamma, f.beta = g, b
        f.rm0, f.rv0 = torch.zeros_like(g), torch.ones_like(g)
        f.reset()
        L.check(lib.addk_bn_finalize(C.byref(f.args()), _st()), 'bn_finalize')
        fins.append(f)
    return fins


def _chain_bwd(lib, fins, xs, gs, dabs, rows):
    out = []
    for f, x, g, dab in zip(fins, xs, gs, dabs):
        b = Bwd(None, f.C, f.count, None, slabs=[dab], stats=(f.gamma, f.out['mean'], f.out['invstd'], f.out['a']))
        L.check(lib.addk_bn_bwd(C.byref(b.args()), _st()), 'bn_bwd')
        _apply(lib, g, x, f.out['mean'], b.c1, b.c2, g)
        out.append(b)
    return out


@pytest.mark.parametrize('P,Cc,ldo', [(63250, 40, 200), (16002, 80, 400), (4096, 160, 800)])
def test_chain_against_fp64_autograd(lib, P, Cc, ldo):
    """A cell block's branch sum batch_norm(x1) + batch_norm(x2) (training mode), end to end through the kernels the plan runs:
    fp64 statistics slabs -> bn_finalize -> affine_sum into the concat slot -> affine_sum_bwd (g and dab per term) -> bn_bwd ->
    bn_bwd_apply in place.  dx, dgamma, dbeta, the running statistics and the forward output against fp64 autograd, each in rms and
    max-abs within 2x of PyTorch fp32's own error on the same inputs (plus a 4-ulp floor).
    Measured on an MI355X, ours / PyTorch fp32, the largest over the three shapes and both terms (rms, max-abs): y 0.76, 0.56;
    dx 0.73, 1.24; dgamma 0.37, 0.78; dbeta 0.31, 0.47; running mean 0.55, 0.33; running var 0.93, 0.87."""
    gen = _gen(80 + Cc)
    xs = [_samples(gen, P, Cc, loc=0.5) for _ in range(2)]
    gams = [1 + 0.2 * _randn(gen, Cc) for _ in range(2)]
    bets = [0.2 * _randn(gen, Cc) for _ in range(2)]
    dycat = _randn(gen, P, ldo)
    slot = 1
    dy = dycat[:, slot * Cc:(slot + 1) * Cc]
    fins = _chain_stats(lib, gen, xs, int(lib.addk_conv_rows(P, Cc)), gams, bets)
    terms = []
    for x, f in zip(xs, fins):
        t = Term.__new__(Term)
        t.xb, t.x, t.a, t.b, t.relu = x, x, f.out['a'], f.out['b'], False
        terms.append(t)
    outb = _nan(P, ldo)
    ar = L.AffineSumArgs()
    for i, t in enumerate(terms):
        ar.term[i] = t.src()
    ar.nterm, ar.P, ar.C, ar.out, ar.ldo, ar.relu_out, ar.accumulate = 2, P, Cc, outb[:, slot * Cc].data_ptr(), ldo, 0, 0
    L.check(lib.addk_affine_sum_fwd(C.byref(ar), _st()), 'affine_sum_fwd')
    rows = int(lib.addk_ew_rows(P, Cc))
    gs = [_nan(P, Cc) for _ in range(2)]
    dabs = [_nan(rows, Cc, 2, dtype=f64) for _ in range(2)]
    ba = L.AffineSumBwdArgs()
    for i, t in enumerate(terms):
        ba.term[i] = t.src()
        ba.g[i], ba.ldg[i], ba.accumulate[i], ba.dab[i] = gs[i].data_ptr(), Cc, 0, dabs[i].data_ptr()
    ba.nterm, ba.P, ba.C, ba.dout, ba.lddo, ba.relu_out = 2, P, Cc, dy.data_ptr(), ldo, 0
    L.check(lib.addk_affine_sum_bwd(C.byref(ba), _st()), 'affine_sum_bwd')
    bws = _chain_bwd(lib, fins, xs, gs, dabs, rows)
    R64 = _bn_torch(xs, gams, bets, dy, f64)
    R32 = _bn_torch(xs, gams, bets, dy, torch.float32)
    tag = 'chain P=%d C=%d' % (P, Cc)
    _compare(tag + ' y (concat slot)', outb[:, slot * Cc:(slot + 1) * Cc], R32['y'], R64['y'], 4)
    for i in range(2):
        _compare(tag + ' dx%d' % i, gs[i], R32['dx'][i], R64['dx'][i], 4)
        _compare(tag + ' dgamma%d' % i, bws[i].dg, R32['dgamma'][i], R64['dgamma'][i], 4)
        _compare(tag + ' dbeta%d' % i, bws[i].db, R32['dbeta'][i], R64['dbeta'][i], 4)
        _compare(tag + ' running_mean%d' % i, fins[i].rm, R32['rm'][i], R64['rm'][i], 4)
        _compare(tag + ' running_var%d' % i, fins[i].rv, R32['rv'][i], R64['rv'][i], 4)


def test_chain_image_pool_count_two(lib):
    """The ASPP image pool's BatchNorm: count 2 (N = 2 images of one pixel), one slab row, ReLU; GAP backward (HW = 1) is the consumer.
    The E[x^2] - E[x]^2 form in fp64 must hold its own at 2 samples against fp64 autograd of relu(batch_norm(x)).
    Measured on an MI355X, ours / PyTorch fp32 (rms, max-abs): y 0.40, 0.20; dx 1.00, 1.00; dgamma 1.00, 1.00; dbeta exact in both;
    running mean 0.73, 0.48; running var 0.71, 0.84."""
    gen = _gen(90)
    Cc = 256
    x = _samples(gen, 2, Cc, loc=0.5)
    gam = (1 + 0.2 * _randn(gen, Cc))
    bet = 0.5 * gam * _sign(gen, Cc)            # normalised values are +-1: keep relu(gamma * (+-1) + beta) clear of 0
    dy = _randn(gen, 2, Cc)
    (f,) = _chain_stats(lib, gen, [x], 1, [gam], [bet])
    src = _src(x, f.out['a'], f.out['b'], 1)
    y = _nan(2, Cc)
    ws = _nan(2 * int(lib.addk_ew_rows(1, Cc)) * Cc)
    L.check(lib.addk_gap_fwd(C.byref(src), 2, 1, y.data_ptr(), Cc, ws.data_ptr(), 1, _st()), 'gap_fwd')
    g = _nan(2, Cc)
    rows = int(lib.addk_ew_rows(2, Cc))
    dab = _nan(rows, Cc, 2, dtype=f64)
    L.check(lib.addk_gap_bwd(C.byref(src), 2, 1, dy.data_ptr(), Cc, g.data_ptr(), Cc, 0, dab.data_ptr(), _st()), 'gap_bwd')
    (b,) = _chain_bwd(lib, [f], [x], [g], [dab], rows)
    R64 = _bn_torch([x], [gam], [bet], dy, f64, relu=True)
    R32 = _bn_torch([x], [gam], [bet], dy, torch.float32, relu=True)
    tag = 'chain image pool count 2'
    _compare(tag + ' y', y, R32['y'], R64['y'], 4)
    _compare(tag + ' dx', g, R32['dx'][0], R64['dx'][0], 4)
    _compare(tag + ' dgamma', b.dg, R32['dgamma'][0], R64['dgamma'][0], 4)
    _compare(tag + ' dbeta', b.db, R32['dbeta'][0], R64['dbeta'][0], 4)
    _compare(tag + ' running_mean', f.rm, R32['rm'][0], R64['rm'][0], 4)
    _compare(tag + ' running_var', f.rv, R32['rv'][0], R64['rv'][0], 4)
