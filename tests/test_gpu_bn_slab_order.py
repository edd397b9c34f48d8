"""The summation order of the BatchNorm slab kernels (csrc/bn.hip), pinned bit for bit, and their contract at the sizes where the
chunked, pipelined form can go wrong.

The order (header comment of csrc/bn.hip), per slab [rows][C][2] and channel:
 1. walk: row group rg (0 .. 63) adds, to a running value that starts at +0.0, one batch after the other; batch i is the eight rows
    rg + 512 i + 64 k (k = 0 .. 7, a row past the end counts as +0.0) summed as ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)), while 512 i < rows;
 2. tree: for s = 32, 16, .. 1 row group rg < s becomes (rg) + (rg + s); the slab's sum is row group 0's value;
 3. bn_bwd adds the slabs' sums one after the other in list order.
It is what makes a hipGraph replay equal the eager run, and it does not depend on how many channels a workgroup takes.

Contract cases reuse the fp64 references and bounds of test_gpu_bn_kernels.py (4U*S + (rows + 64) * 2^-53 * sum|terms|) unchanged."""
import ctypes as C

import pytest
import torch

import addk  # noqa: F401
from addk import _lib as L
import test_gpu_bn_kernels as K
from test_gpu_bn_kernels import lib  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu

f64 = torch.float64
ROWS = (1, 7, 63, 64, 65, 511, 512, 513, 989, 1024, 1537)
CS = (1, 19, 40, 250)
KC = 10      # slabs bn_bwd sums per pass over its LDS panel (BN_KC in csrc/bn.hip)


def _order_sum(slab):
    """The order above, evaluated in fp64 on the CPU: slab [rows][C][2] -> [C][2]."""
    rows = slab.shape[0]
    nb = -(-rows // 512)
    x = torch.zeros(nb * 512, *slab.shape[1:], dtype=f64)
    x[:rows] = slab
    x = x.view(nb, 8, 64, *slab.shape[1:])                   # row = rg + 512 i + 64 k  ->  [i][k][rg]
    a = torch.zeros(64, *slab.shape[1:], dtype=f64)
    for i in range(nb):
        v = x[i]
        a = a + (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
    s = 32
    while s:
        a = a[:s] + a[s:2 * s]
        s //= 2
    return a[0]


def _plain_sum(slab):
    a = torch.zeros(slab.shape[1:], dtype=f64)
    for r in range(slab.shape[0]):
        a = a + slab[r]
    return a


def _order_cases():
    """Every (rows, C): the slab N(0,1) * 2^k, k uniform in [-20, 20), its sum in the kernels' order, and a check that the case can tell
    orders apart."""
    gen = torch.Generator().manual_seed(20)
    cases = []
    for rows in ROWS:
        for Cc in CS:
            k = torch.randint(-20, 20, (rows, Cc, 2), generator=gen)
            slab = torch.randn(rows, Cc, 2, generator=gen, dtype=f64) * torch.pow(torch.tensor(2.0, dtype=f64), k)
            ref = _order_sum(slab)
            if rows >= 7:
                share = float((K._bits(ref) != K._bits(_plain_sum(slab))).double().mean())
                assert share >= 0.25, 'rows=%d C=%d: only %.0f %% of the sums depend on the order' % (rows, Cc, 100 * share)
            cases.append((rows, Cc, slab.cuda(), ref.cuda()))
    return cases


def test_slab_sums_follow_the_written_order_bit_for_bit(lib):
    cases = _order_cases()
    outs, items = [], []
    for rows, Cc, slab, ref in cases:
        red = K._nan(Cc, 2, dtype=f64)
        one = L.SlabReduceItem()
        one.partial, one.out, one.rows, one.C = slab.data_ptr(), red.data_ptr(), rows, Cc
        L.check(lib.addk_slab_reduce(C.byref(one), K._st()), 'slab_reduce')
        K._same_bits('slab_reduce rows=%d C=%d against the written order' % (rows, Cc), red, ref)
        o = K._nan(Cc, 2, dtype=f64)
        it = L.SlabReduceItem()
        it.partial, it.out, it.rows, it.C = slab.data_ptr(), o.data_ptr(), rows, Cc
        outs.append(o)
        items.append(it)
    tab = K._table(items)
    L.check(lib.addk_slab_reduce_batch(tab.data_ptr(), len(items), max(CS), K._st()), 'slab_reduce_batch')
    for (rows, Cc, slab, ref), o in zip(cases, outs):
        K._same_bits('slab_reduce_batch rows=%d C=%d against the written order' % (rows, Cc), o, ref)


# ---- contract ------------------------------------------------------------------------------------------------------------------------
POOL = (1, 989, 64, 513, 7, 1024, 63, 512, 1537, 65, 511, 3, 128, 501)


def _rows(nslab, off):
    return tuple(POOL[(3 * i + off) % len(POOL)] for i in range(nslab))


def test_bn_bwd_slab_counts_around_the_chunk(lib):
    """nslab 1, KC, KC + 1 and 32 with unequal rows (1 among them); gamma NULL, accumulate, centered, the dmv output; C = 19, 40 and
    250 in one batch table, so whole workgroups of the narrow entries leave early."""
    gen = K._gen(41)
    bs = []
    for n, (nslab, Cc) in enumerate(((1, 40), (KC, 19), (KC + 1, 250), (32, 40), (KC + 1, 19), (32, 250), (KC, 40), (1, 250))):
        bs.append(K.Bwd(gen, Cc, 4096 + n, _rows(nslab, n), centered=n & 1, accumulate=(n >> 1) & 1, route='dmv' if n % 3 == 2 else 'c'))
    bs.append(K.Bwd(gen, 40, 777, _rows(KC + 1, 5), centered=1, affine=False))
    bs.append(K.Bwd(gen, 19, 777, _rows(32, 2), centered=0, affine=False, route='dmv'))
    K._bwd_all(lib, bs, 'chunk')


@pytest.mark.parametrize('accumulate', [0, 1])
def test_bn_bwd_without_slabs(lib, accumulate):
    """nslab = 0: dA = dB = 0, so dgamma / dbeta keep their old value (or become 0) and c1 = c2 = 0, exactly."""
    gen = K._gen(42 + accumulate)
    for route in ('c', 'dmv'):
        b = K.Bwd(gen, 40, 1000, (), accumulate=accumulate, route=route, slabs=[])
        L.check(lib.addk_bn_bwd(C.byref(b.args()), K._st()), 'bn_bwd')
        zero = torch.zeros(40, device='cuda')
        assert torch.equal(b.dg, b.old[0] if accumulate else zero) and torch.equal(b.db, b.old[1] if accumulate else zero)
        for o in ((b.c1, b.c2) if route == 'c' else (b.dmv,)):
            assert torch.equal(o, torch.zeros_like(o))
        single = {k: v.clone() for k, v in b.results().items()}
        b.reset()
        other = K.Bwd(gen, 250, 1000, _rows(2, 0))
        tab = K._table([other.args(), b.args()])
        L.check(lib.addk_bn_bwd_batch(tab.data_ptr(), 2, 250, K._st()), 'bn_bwd_batch')
        for k, v in b.results().items():
            K._same_bits('bn_bwd_batch nslab=0 %s' % k, v, single[k])


def test_bn_finalize_mixed_widths(lib):
    """With and without running statistics, rows on both sides of a batch boundary, C = 19, 40 and 250 in one batch table."""
    gen = K._gen(44)
    fins = [K.Fin(gen, 19, 2 * 1537, 1537), K.Fin(gen, 250, 5000, 513, running=False, stats_out=False), K.Fin(gen, 40, 63250, 989),
            K.Fin(gen, 40, 64, 1, running=False), K.Fin(gen, 250, 2048, 512), K.Fin(gen, 19, 650, 65, affine=False)]
    K._finalize_all(lib, fins, 'mixed')


# ---- replay --------------------------------------------------------------------------------------------------------------------------
def test_bn_bwd_same_bytes_beside_a_busy_device(lib):
    """The same launches alone, then while chip-filling kernels of another stream hold the device: identical bytes."""
    gen = K._gen(45)
    bs = [K.Bwd(gen, 40, 65536, K.NINE), K.Bwd(gen, 250, 4096, _rows(32, 1), route='dmv'), K.Bwd(gen, 19, 777, _rows(KC + 1, 4))]

    def run(stream):
        with torch.cuda.stream(stream):                      # the NaN fills of reset() go in front of the launch on its own stream
            for b in bs:
                b.reset()
                L.check(lib.addk_bn_bwd(C.byref(b.args()), stream.cuda_stream), 'bn_bwd')

    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    run(main)
    torch.cuda.synchronize()
    alone = [{k: v.clone() for k, v in b.results().items()} for b in bs]
    big = torch.ones(1 << 28, device='cuda')                 # 1 GiB: every multiply fills the chip for a few hundred microseconds
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(12):
            big.mul_(1.0001)
    run(main)
    busy = not side.query()
    torch.cuda.synchronize()
    assert busy, 'the other stream had drained before bn_bwd was launched'
    for b, ref in zip(bs, alone):
        for k, v in b.results().items():
            assert not torch.isnan(v).any()
            K._same_bits('bn_bwd beside a busy device %s %s' % (K._tag(b), k), v, ref[k])
