"""numpy restatement of the image-pyramid step of csrc/imgpyr.hip (include/st3d.h, "image pyramid step"): the step, its
transpose and the need rule.  ``dtype=np.float32`` repeats the kernels' roundings in their order (bit-equal results),
``dtype=np.float64`` is the reference the error bounds are taken against."""
import numpy as np


def _clamped(n, offset):
    """fine indices 2i + offset for i in 0..n/2, clamped to the axis"""
    return np.clip(2 * np.arange(n // 2) + offset, 0, n - 1)


def down(x, dtype=np.float32):
    """(..., H, W) -> (..., H/2, W/2): per row h = (x[-1] + x[2]) + 3 (x[0] + x[1]), over the four h the same, * 1/64"""
    x = np.asarray(x, dtype)
    H, W = x.shape[-2:]
    assert H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0, x.shape
    three = dtype(3)
    with np.errstate(invalid="ignore", over="ignore"):
        xm, x0, x1, x2 = (x[..., :, _clamped(W, o)] for o in (-1, 0, 1, 2))
        h = (xm + x2) + three * (x0 + x1)
        hm, h0, h1, h2 = (h[..., _clamped(H, o), :] for o in (-1, 0, 1, 2))
        v = (hm + h2) + three * (h0 + h1)
        return (v * dtype(1.0 / 64.0)).astype(dtype)


def axis_taps(n):
    """for the n fine indices of an axis: near coarse index, far coarse index, near weight (3 or 4), far exists"""
    y = np.arange(n)
    near = y >> 1
    far = np.where(y & 1, near + 1, near - 1)
    has_far = (far >= 0) & (far < n // 2)
    return near, np.clip(far, 0, n // 2 - 1), np.where(has_far, 3.0, 4.0), has_far


def down_transpose(g, dtype=np.float32):
    """(..., H/2, W/2) -> (..., H, W): every fine pixel sums (wy wx / 64) g over (near,near), (near,far), (far,near),
    (far,far) in (row, column), in that order; a tap that does not exist is skipped"""
    g = np.asarray(g, dtype)
    Ho, Wo = g.shape[-2:]
    yn, yf, wy, hy = axis_taps(2 * Ho)
    xn, xf, wx, hx = axis_taps(2 * Wo)
    wy, wx = wy[:, None], wx[None, :]
    hy, hx = hy[:, None], hx[None, :]
    c = 1.0 / 64.0
    with np.errstate(invalid="ignore", over="ignore"):
        s = (wy * wx * c).astype(dtype) * g[..., yn[:, None], xn[None, :]]
        s = np.where(hx, s + (wy * c).astype(dtype) * g[..., yn[:, None], xf[None, :]], s).astype(dtype)
        s = np.where(hy, s + (wx * c).astype(dtype) * g[..., yf[:, None], xn[None, :]], s).astype(dtype)
        s = np.where(hy & hx, s + dtype(c) * g[..., yf[:, None], xf[None, :]], s).astype(dtype)
    return s


def transpose_weight_mass(g_abs):
    """sum |w| |g| of down_transpose per fine pixel in fp64: what an error bound of the transpose scales with"""
    return down_transpose(np.abs(np.asarray(g_abs, np.float64)), np.float64)


def matrix(H, W):
    """the step as a dense fp64 matrix (H/2 W/2, H W), built tap by tap from the definition (not from down())"""
    D = np.zeros((H // 2 * (W // 2), H * W))
    k = (1.0, 3.0, 3.0, 1.0)
    for i in range(H // 2):
        for j in range(W // 2):
            for a in range(4):
                for b in range(4):
                    y, x = min(max(2 * i - 1 + a, 0), H - 1), min(max(2 * j - 1 + b, 0), W - 1)
                    D[i * (W // 2) + j, y * W + x] += k[a] * k[b] / 64.0
    return D


def need(mask):
    """(..., H, W) -> (..., H/2, W/2) uint8: 1 where any pixel of the clamped 4 x 4 footprint is non-zero"""
    m = np.asarray(mask) != 0
    H, W = m.shape[-2:]
    cols = np.zeros(m.shape[:-1] + (W // 2,), bool)
    for o in (-1, 0, 1, 2):
        cols |= m[..., :, _clamped(W, o)]
    out = np.zeros(m.shape[:-2] + (H // 2, W // 2), bool)
    for o in (-1, 0, 1, 2):
        out |= cols[..., _clamped(H, o), :]
    return out.astype(np.uint8)


def footprint_outputs(H, W, y, x):
    """the coarse pixels (i, j) whose clamped 4 x 4 footprint holds fine pixel (y, x)"""
    hit = set()
    for i in range(H // 2):
        for j in range(W // 2):
            ys = {min(max(2 * i - 1 + a, 0), H - 1) for a in range(4)}
            xs = {min(max(2 * j - 1 + b, 0), W - 1) for b in range(4)}
            if y in ys and x in xs:
                hit.add((i, j))
    return hit
