"""The statistics tail of the forward kernels (csrc/common.h: rs16, used by sepf.hip and pw.hip) against the butterfly it replaced, as numpy
models of the two schedules over the 16 pixel lanes of a DPP row.  No GPU.

The butterfly (the parent's `for (m = 1; m < 16; m <<= 1) a += __shfl_xor(a, m)`): every lane i computes, for every one of its V values,

    T1[i] = x[i] + x[i ^ 1];  T2[i] = T1[i] + T1[i ^ 2];  T3[i] = T2[i] + T2[i ^ 4];  T4[i] = T3[i] + T3[i ^ 8]

and lane 0 writes T4.  The reduce-scatter keeps the partial sums of each level and halves the values a lane carries:

    level  partner of lane i           a lane keeps the UPPER half of its values if
      1    i ^ 1  (quad_perm [1,0,3,2])   bit 0 of i  xor  bit 2 of i
      2    i ^ 2  (quad_perm [2,3,0,1])   bit 1 of i  xor  bit 2 of i
      3    i ^ 7  (row_half_mirror)       bit 2 of i
      4    i ^ 8  (row_ror:8)             bit 3 of i

With n values in, a lane leaves a level with ceil(n / 2): slot s holds value s (lower half) or s + ceil(n / 2) (upper half), its own partial
sum plus the partner's partial sum of the same value; where n is odd the last slot has no sibling, both lanes add it and the lower-half lane
owns it.  Bit 2 flips the choices of levels 1 and 2, so the lane that row_half_mirror pairs with i (i ^ 7, the other quad of the same half
row) holds the values i ^ 4 would hold in a plain layout, and what meets at level 3 are the two quad sums T2 of one value, as in the tree.
Each sum adds the same two numbers as the butterfly, possibly in the other order; IEEE addition is commutative, so the bits are the same.
rs_index mirrors rs16_index of common.h: the value a final slot of a lane holds, or None for a copy that another lane owns."""
import numpy as np
import pytest

LEVELS = ((1, lambda i: ((i >> 0) ^ (i >> 2)) & 1), (2, lambda i: ((i >> 1) ^ (i >> 2)) & 1), (7, lambda i: (i >> 2) & 1), (8, lambda i: (i >> 3) & 1))
LANES = np.arange(16)


def butterfly(x):
    """x[lane, value] -> the totals lane 0 holds after the four xor levels."""
    t = x.copy()
    for m in (1, 2, 4, 8):
        t = t + t[LANES ^ m]
    return t[0]


def sizes(V):
    out = [V]
    for _ in range(4):
        out.append((out[-1] + 1) // 2)
    return out


def reduce_scatter(x):
    """x[lane, value] -> v[lane, slot]: the slots every lane holds after the four levels (rs16 of common.h)."""
    v = x.copy()
    nin = x.shape[1]
    for partner, upper_of in LEVELS:
        nout = (nin + 1) // 2
        upper = np.array([upper_of(i) for i in LANES], dtype=bool)
        src = LANES ^ partner
        new = v.copy()
        for s in range(nout):
            if s + nout < nin:
                keep = np.where(upper, v[:, s + nout], v[:, s])
                send = np.where(upper, v[:, s], v[:, s + nout])
                new[:, s] = keep + send[src]
            else:
                new[:, s] = v[:, s] + v[src, s]
        v, nin = new, nout
    return v[:, :nin]


def rs_index(V, slot, lane):
    n = sizes(V)
    idx, own = slot, True
    for lvl in (3, 2, 1, 0):
        nin, nout = n[lvl], n[lvl + 1]
        if LEVELS[lvl][1](lane):
            if idx + nout < nin:
                idx += nout
            else:
                own = False
    return idx if own else None


def scattered_totals(x):
    V = x.shape[1]
    v = reduce_scatter(x)
    out, owners = np.empty(V, dtype=x.dtype), np.zeros(V, dtype=int)
    for lane in LANES:
        for slot in range(v.shape[1]):
            idx = rs_index(V, slot, lane)
            if idx is not None:
                out[idx] = v[lane, slot]
                owners[idx] += 1
    assert (owners == 1).all(), 'every value has exactly one owning lane: %s' % owners
    return out


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def inputs(V, dtype, seed):
    rs = np.random.RandomState(seed)
    plain = rs.standard_normal((16, V))
    wide = plain * np.where(rs.rand(16, V) < 0.3, 2.0 ** 40, 1.0)               # neighbours 2^40 apart: every level rounds
    zeros = np.where(rs.rand(16, V) < 0.5, 0.0, -0.0)                           # signed zeros only: the sign of the total depends on the tree
    zeros[:, ::3] = -0.0
    mixed = np.where(rs.rand(16, V) < 0.4, zeros, plain)
    nan = wide.copy()
    nan[5, :] = np.nan                                                            # a NaN lane poisons every total, with one payload
    sums = np.abs(plain) * 1e3 + plain ** 2                                       # like (sum, sum of squares) partials: one sign, cancellation-free
    return [a.astype(dtype) for a in (plain, wide, zeros, mixed, nan, sums)]


@pytest.mark.parametrize('V', [24, 40, 8, 16, 32])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_reduce_scatter_totals_equal_the_butterfly_bit_for_bit(V, dtype):
    """24 / 40 values per lane are sepf's CT = 3 / 5 in fp64; 8, 16, 24, 32 are pw.hip's CT = 1..4, in fp64 and in fp32 lane sums."""
    for k, x in enumerate(inputs(V, dtype, 1000 + V)):
        with np.errstate(invalid='ignore'):
            want, got = butterfly(x), scattered_totals(x)
        assert want.dtype == got.dtype == dtype
        assert np.array_equal(bits(want), bits(got)), 'input set %d: %d of %d totals differ' % (k, int((bits(want) != bits(got)).sum()), V)


def test_the_tree_is_not_order_free():
    """The check above has teeth: a plain left-to-right sum of the 16 lanes differs from the tree on the wide inputs."""
    x = inputs(24, np.float64, 7)[1]
    serial = np.zeros(24)
    for lane in LANES:
        serial = serial + x[lane]
    assert (bits(serial) != bits(butterfly(x))).any()


@pytest.mark.parametrize('V', [24, 40, 8, 16, 32])
def test_exchange_counts(V):
    """12 + 6 + 3 + 2 exchanges for 24 values (20 + 10 + 5 + 3 for 40) where the butterfly takes 4 V; at most ceil(V / 16) + 1 LDS writes per lane."""
    n = sizes(V)
    assert sum(n[1:]) < V + 4 and n[4] <= (V + 15) // 16 + 1
    if V == 24:
        assert n[1:] == [12, 6, 3, 2]
    if V == 40:
        assert n[1:] == [20, 10, 5, 3]
