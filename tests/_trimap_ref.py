"""numpy reference of the boundary-band ("trimap") metric, written from the definition in include/addk.h ("Boundary-band confusion"):
edge pixels, the distance byte by brute force over all edge pixels (small shapes) and in the separable form (larger shapes), and the
ring confusion matrices.  Everything is integer arithmetic on int64.  Also the seeded targets the tests share."""
import numpy as np

FAR = 255


def valid(t, C):
    t = np.asarray(t, dtype=np.int64)
    return (t >= 0) & (t < C)


def edges(t, C):
    """bool [N,OH,OW]: valid(p) and a 4-neighbour q inside the same image with valid(q) and t(q) != t(p)"""
    t = np.asarray(t, dtype=np.int64)
    v = valid(t, C)
    e = np.zeros(t.shape, dtype=bool)

    def against(a, b, va, vb):          # a, b: views of neighbouring pixels
        return va & vb & (a != b)
    d = against(t[:, 1:, :], t[:, :-1, :], v[:, 1:, :], v[:, :-1, :])
    e[:, 1:, :] |= d
    e[:, :-1, :] |= d
    d = against(t[:, :, 1:], t[:, :, :-1], v[:, :, 1:], v[:, :, :-1])
    e[:, :, 1:] |= d
    e[:, :, :-1] |= d
    return e


def k_of(d2):
    """the smallest integer k >= 0 with k*k >= d2, elementwise on non-negative int64"""
    d2 = np.asarray(d2, dtype=np.int64)
    k = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    k = np.where(k * k > d2, k - 1, k)                  # k = floor(sqrt(d2)) whatever the float root did
    k = np.where((k + 1) * (k + 1) <= d2, k + 1, k)
    return np.where(k * k < d2, k + 1, k)


def _to_bytes(d2, R):
    k = k_of(np.minimum(d2, np.int64(1) << 40))
    return np.where((d2 >= 0) & (k <= R), k, FAR).astype(np.uint8)


def dist_brute(t, C, R):
    """uint8 [N,OH,OW]: the minimum over ALL edge pixels of the image"""
    t = np.asarray(t, dtype=np.int64)
    N, OH, OW = t.shape
    e = edges(t, C)
    out = np.full(t.shape, FAR, dtype=np.uint8)
    yy, xx = np.mgrid[0:OH, 0:OW]
    for n in range(N):
        ey, ex = np.nonzero(e[n])
        if ey.size == 0:
            continue
        d2 = np.full((OH, OW), np.iinfo(np.int64).max, dtype=np.int64)
        for s in range(0, ey.size, 256):
            dy = yy[:, :, None] - ey[None, None, s:s + 256]
            dx = xx[:, :, None] - ex[None, None, s:s + 256]
            d2 = np.minimum(d2, (dy * dy + dx * dx).min(-1))
        out[n] = _to_bytes(d2, R)
    return out


def dist_sep(t, C, R):
    """uint8 [N,OH,OW]: the separable form, h(y,x) = min |x-x'| over E(y,x') kept where <= R, D2 = min over |dy| <= R of dy^2 + h^2"""
    t = np.asarray(t, dtype=np.int64)
    N, OH, OW = t.shape
    e = edges(t, C)
    INF = np.int64(1) << 20
    x = np.arange(OW, dtype=np.int64)
    # nearest edge column to the left / right of every pixel
    left = np.where(e, x[None, None, :], -INF)
    left = np.maximum.accumulate(left, axis=2)
    right = np.where(e, x[None, None, :], INF)
    right = np.minimum.accumulate(right[:, :, ::-1], axis=2)[:, :, ::-1]
    h = np.minimum(x[None, None, :] - left, right - x[None, None, :])
    h = np.where(h <= R, h, INF)
    d2 = np.full(t.shape, INF * INF, dtype=np.int64)
    for dy in range(-R, R + 1):
        lo, hi = max(0, -dy), min(OH, OH - dy)           # rows y with y + dy inside the image
        if lo >= hi:
            continue
        src = h[:, lo + dy:hi + dy, :]
        d2[:, lo:hi, :] = np.minimum(d2[:, lo:hi, :], dy * dy + src * src)
    return _to_bytes(d2, R)


def banded_confusion(t, pred, dist, C, widths, per_image=False):
    """int64 ring matrices [nw,C,C] (or [N,nw,C,C]): ring j holds w[j-1] < dist <= w[j]; a pixel counts when valid(t), pred < C and
    dist <= w[-1]"""
    t = np.asarray(t, dtype=np.int64)
    pred = np.asarray(pred).astype(np.int64)
    dist = np.asarray(dist).astype(np.int64)
    N = t.shape[0]
    nw = len(widths)
    out = np.zeros((N, nw, C, C), dtype=np.int64)
    ok = valid(t, C) & (pred < C) & (pred >= 0)
    prev = -1
    for j, w in enumerate(widths):
        ring = ok & (dist > prev) & (dist <= w)
        for n in range(N):
            m = ring[n]
            out[n, j] = np.bincount(t[n][m] * C + pred[n][m], minlength=C * C).reshape(C, C)
        prev = w
    return out if per_image else out.sum(0)


def plain_confusion(t, pred, C, mask):
    t = np.asarray(t, dtype=np.int64)
    pred = np.asarray(pred).astype(np.int64)
    m = valid(t, C) & (pred < C) & mask
    return np.bincount(t[m] * C + pred[m], minlength=C * C).reshape(C, C)


# ---- seeded targets -------------------------------------------------------------------------------------------------------------
def voronoi(seed, OH, OW, sites=12, C=19):
    """int64 [OH,OW]: every pixel takes the class of the nearest of `sites` seeded points (blobs with straight contours)"""
    r = np.random.default_rng(seed)
    sy, sx = r.integers(0, OH, sites), r.integers(0, OW, sites)
    cls = r.integers(0, C, sites)
    yy, xx = np.mgrid[0:OH, 0:OW]
    d2 = (yy[:, :, None] - sy) ** 2 + (xx[:, :, None] - sx) ** 2
    return cls[d2.argmin(-1)].astype(np.int64)


def case_b():
    """2 x 37 x 53: few, large blobs with a patch of 255: near and far pixels at radius 8"""
    t = np.stack([voronoi(101, 37, 53, 3), voronoi(102, 37, 53, 4)])
    t[0, 5:12, 30:41] = 255
    return t


def case_c():
    """2 x 96 x 160: image 0 blobs; image 1 uniform class 7 with one pixel of class 3 at (40, 70)"""
    t = np.stack([voronoi(103, 96, 160, 14), np.full((96, 160), 7, dtype=np.int64)])
    t[1, 40, 70] = 3
    return t


def case_d():
    """2 x 40 x 64: image 0 has an edge along its LAST row, image 1 is uniform"""
    t = np.full((2, 40, 64), 4, dtype=np.int64)
    t[0, 39, :] = 9
    return t


def case_e():
    """1 x 16 x 24: out-of-range values beside valid classes and beside each other"""
    t = np.full((1, 16, 24), 2, dtype=np.int64)
    t[0, :, 12:] = 5                                     # one real contour down the middle
    odd = [19, 20, 254, 255, 256, 2 ** 40, -1, -2 ** 40]
    for i, v in enumerate(odd):
        t[0, 2, 1 + i] = v                               # a run of different invalid values inside class 2
        t[0, 6 + (i % 4) * 2, 16 + (i // 4) * 3] = v     # single ones inside class 5
    t[0, 12, 2:5] = [255, 3, 256]                        # a valid class between two invalid ones
    return t
