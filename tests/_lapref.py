"""The Laplacian content term of csrc/lap.hip restated in numpy, rounding for rounding (include/st3d.h states the arithmetic):

    pool(x, p, dtype)                 the p x p block average: every row of a block summed left to right, the row sums added top
                                      to bottom, one product with dtype(1 / p^2)
    D(P)                              4 P - ((up + down) + (left + right)), indices clamped to the plane
    fwd(x, p, dtype)                  D(pool(x))
    loss_grad(x, T, p, scale, tile)   fp32((ordered fp64 sum of r^2) * scale) and k * D(r) spread over the blocks, r = fwd(x) - T,
                                      k = fp32(2 scale / p^2); the sum in the kernel's order over tiles of ``tile`` fine pixels
    loss_grad64(x, T, p, scale)       the same in fp64 throughout, sums in numpy's order: the reference of the bounds
    bound_fwd / bound_loss_grad       per-element bounds of the fp32 results against the fp64 ones, from the roundings counted

Arrays are (..., H, W); every leading axis is a plane of its own.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24          # the unit roundoff of fp32
THREADS = 256
POOLS = (1, 2, 4, 8, 16)


def pool(x, p, dtype=F32):
    x = np.asarray(x, dtype=dtype)
    H, W = x.shape[-2:]
    assert H % p == 0 and W % p == 0
    b = x.reshape(x.shape[:-2] + (H // p, p, W // p, p))
    rows = b[..., 0].copy()
    for q in range(1, p):                   # a row of the block, left to right
        rows = rows + b[..., q]
    s = rows[..., 0, :].copy()
    for r in range(1, p):                   # the row sums, top to bottom
        s = s + rows[..., r, :]
    return s if p == 1 else s * dtype(1.0 / (p * p))


def _shift(P, axis, d):
    """P at index i + d along ``axis``, clamped to the plane"""
    n = P.shape[axis]
    return np.take(P, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def D(P):
    four = P.dtype.type(4)
    return four * P - ((_shift(P, -2, -1) + _shift(P, -2, 1)) + (_shift(P, -1, -1) + _shift(P, -1, 1)))


def D_abs(A):
    """the stencil with every coefficient made positive: what the magnitudes of D's terms add up to"""
    return 4 * A + _shift(A, -2, -1) + _shift(A, -2, 1) + _shift(A, -1, -1) + _shift(A, -1, 1)


def fwd(x, p, dtype=F32):
    return D(pool(x, p, dtype))


def _fold(acc):
    acc = acc.copy()
    s = THREADS // 2
    while s > 0:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def _strided_sum(values):
    """thread t adds values t, t + 256, ... in ascending order, then the 256 sums are folded by halving strides"""
    n = -(-len(values) // THREADS) * THREADS
    v = np.zeros(n, F64)
    v[:len(values)] = values
    v = v.reshape(-1, THREADS)
    acc = np.zeros(THREADS, F64)
    for row in v:
        acc = acc + row
    return _fold(acc)


def ordered_sum_sq(r, p, tile):
    """the sum of (double) r^2 in the kernel's order: r (..., h, w) fp32, ``tile`` = lap_tile(p) in fine pixels"""
    th, tw = tile[0] // p, tile[1] // p
    h, w = r.shape[-2:]
    planes = r.reshape((-1, h, w)).astype(F64)
    partials = []
    for plane in planes:
        for i0 in range(0, h, th):
            for j0 in range(0, w, tw):
                cells = np.zeros((th, tw), F64)         # cells off the plane are skipped: adding +0.0 changes no sum
                blk = plane[i0:i0 + th, j0:j0 + tw]
                cells[:blk.shape[0], :blk.shape[1]] = blk * blk
                partials.append(_strided_sum(cells.reshape(-1)))
    return _strided_sum(np.array(partials, F64))


def spread(g, p):
    return np.repeat(np.repeat(g, p, axis=-2), p, axis=-1)


def loss_grad(x, T, p, scale, tile):
    r = fwd(x, p, F32) - np.asarray(T, F32)
    loss = F32(ordered_sum_sq(r, p, tile) * F64(scale))
    k = F32(2.0 * float(scale) / (p * p))
    return loss, spread(k * D(r), p), r


def loss_grad64(x, T, p, scale):
    r = fwd(x, p, F64) - np.asarray(T, F64)
    return float((r * r).sum() * scale), spread((2.0 * float(scale) / (p * p)) * D(r), p), r


# ---------------------------------------------------------------------------- bounds from the roundings the source writes
def _gamma(n):
    return n * U / (1.0 - n * U)


def bound_fwd(x, p):
    """|fp32 fwd - fp64 fwd| per element, for the same fp32 input.  A pooled cell passes p^2 - 1 additions and the scaling;
    in the stencil every term passes at most three more roundings (the product or a pair sum, the sum of the pairs, the
    final difference): p^2 + 3 roundings on any path, each relative to a partial result no larger than the sum of the
    magnitudes, D_abs(pool(|x|))."""
    return 1.01 * _gamma(p * p + 3) * D_abs(pool(np.abs(np.asarray(x, F64)), p, F64))


def bound_loss_grad(x, c, p, scale):
    """-> (bound of the loss, bound of the gradient per pixel, bound of r per cell) against loss_grad64 with the fp64
    target fwd(c, p, fp64).  r = L(x) - T: both Laplacians' bounds and one rounding; the gradient applies D to r (the errors
    pass through D_abs, three roundings as above) and multiplies by k (k's own rounding and the product's): five roundings
    relative to D_abs(|r|); the loss sums exact fp64 squares of the fp32 r (2 |r| e + e^2 each), the fp64 sum's own error is
    below 1e-12 of it, and one rounding to fp32."""
    r64 = fwd(x, p, F64) - fwd(c, p, F64)
    e_r = bound_fwd(x, p) + bound_fwd(c, p) + 1.01 * U * np.abs(r64)
    k = 2.0 * float(scale) / (p * p)
    e_g = 1.01 * k * (D_abs(e_r) + 5 * U * D_abs(np.abs(r64) + e_r))
    loss64 = float((r64 * r64).sum() * scale)
    e_loss = float(scale) * float((2 * np.abs(r64) * e_r + e_r * e_r).sum()) * (1 + 1e-12)
    e_loss = e_loss + 1.01 * U * (loss64 + e_loss) + 1e-12 * loss64
    return e_loss, spread(e_g, p), e_r
