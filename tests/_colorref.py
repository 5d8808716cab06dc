"""numpy restatement of csrc/color.hip and of the host-side match of st3d/color.py (include/st3d.h states the arithmetic).

Images are planar (B,3,P) float32.  The fp32 fma is emulated through fp64.  The product of two fp32 values has at most 48
significant bits and is exact in fp64.  Adding the fp32 addend to it in fp64 and rounding the result to fp32 is NOT always
the correctly rounded fmaf: the fp64 sum is rounded once to 53 bits and then again to 24, and when the first rounding lands
exactly on an fp32 tie the second one cannot know on which side the exact value lay (1 + (2^-24 + 2^-60) is such a case:
fmaf gives 1 + 2^-23, the naive form 1).  So the fp64 sum is taken with round-to-odd instead: TwoSum gives the exact error e
of s = p + c; when e != 0 and the last bit of s is even, s moves one fp64 ulp towards the exact value (that neighbour is
the odd one).  A value rounded to odd at 53 >= 24 + 2 bits rounds to fp32 as the exact value does (Boldo and Melquiond,
"Emulation of FMA and correctly rounded sums: proved algorithms using rounding to odd", 2008), so fma() below is fmaf
bit for bit, for finite operands without fp64 overflow (fp32 operands cannot overflow fp64).
The moments are taken in exact rational arithmetic (fractions) or with math.fsum, which is correctly rounded."""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
W = (F32(0.299), F32(0.587), F32(0.114))        # Rec. 601, as the kernels hold them
EIG_FLOOR = 1e-8                                # a definition: a flat image has no palette to stretch
# the standard RGB -> YIQ matrix (NTSC), fp64: row 0 is the luminance above
YIQ = np.array([[0.299, 0.587, 0.114],
                [0.595716, -0.274453, -0.321263],
                [0.211456, -0.522591, 0.311135]], F64)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def fma(a, b, c):
    """fmaf(a, b, c) on fp32 arrays, correctly rounded (see the module docstring)"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)     # exact
        c = np.broadcast_to(np.asarray(c, F32).astype(F64), p.shape)
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                                             # TwoSum: s + e == p + c exactly
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        move = np.isfinite(e) & (e != 0) & even
        s = np.where(move, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def luma_plane(x):
    """(B,3,P) float32 -> (B,P): Y = fmaf(W2, b, fmaf(W1, g, W0 * r))"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return fma(W[2], x[:, 2], fma(W[1], x[:, 1], W[0] * x[:, 0]))


def luma_fwd(x):
    y = luma_plane(x)
    return np.stack([y, y, y], axis=1)


def luma_bwd(g):
    """the exact transpose: s = (g0 + g1) + g2, out_c = W_c * s"""
    g = np.asarray(g, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (g[:, 0] + g[:, 1]) + g[:, 2]
        return np.stack([W[0] * s, W[1] * s, W[2] * s], axis=1).astype(F32)


def recombine(opt, orig):
    """d = Y(opt) - Y(orig) (one fp32 subtraction), out_c = orig_c + d"""
    orig = np.asarray(orig, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (luma_plane(opt) - luma_plane(orig)).astype(F32)
        return (orig + d[:, None, :]).astype(F32)


def affine(x, A, b, clamp):
    """out_c = fmaf(A[c][2], x2, fmaf(A[c][1], x1, fmaf(A[c][0], x0, b_c))); clamp: v < 0 ? 0 : (v > 1 ? 1 : v), NaN stays"""
    x = np.asarray(x, F32)
    A = np.asarray(A, F64).reshape(3, 3).astype(F32)
    b = np.asarray(b, F64).reshape(3).astype(F32)
    out = np.empty_like(x)
    for c in range(3):
        v = fma(A[c, 2], x[:, 2], fma(A[c, 1], x[:, 1], fma(A[c, 0], x[:, 0], b[c])))
        if clamp:
            with np.errstate(invalid="ignore"):
                v = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v))
        out[:, c] = v
    return out


def moment_terms(x, mask=None):
    """(B,3,P) float32, mask (B,P) or None -> list of ten fp64 arrays: the terms of the ten sums over the selected pixels
    (ones, x_c, x_c x_d for c <= d; every product of two fp32 values is exact in fp64)"""
    x = np.asarray(x, F32).astype(F64)
    sel = np.ones(x.shape[::2], bool) if mask is None else np.asarray(mask).reshape(x.shape[0], x.shape[2]) != 0
    ch = [x[:, c][sel] for c in range(3)]
    return [np.ones(ch[0].shape, F64)] + ch + [ch[c] * ch[d] for c, d in PAIRS]


def moments_exact(x, mask=None):
    """-> (ten exact sums as Fractions, ten sums of |terms| as floats)"""
    terms = moment_terms(x, mask)
    return [sum((Fraction(float(v)) for v in t), Fraction(0)) for t in terms], [math.fsum(np.abs(t)) for t in terms]


def moments(x, mask=None):
    """the ten sums, correctly rounded (math.fsum)"""
    return np.array([math.fsum(t) for t in moment_terms(x, mask)], F64)


def stats(sums):
    """ten sums -> {'n', 'mean', 'cov'}: the population covariance S_cd / n - mu_c mu_d"""
    s = np.asarray([float(v) for v in sums], F64)
    n = s[0]
    mean = s[1:4] / n
    second = np.empty((3, 3), F64)
    for k, (c, d) in enumerate(PAIRS):
        second[c, d] = second[d, c] = s[4 + k] / n
    return {"n": int(n), "mean": mean, "cov": second - np.outer(mean, mean)}


def sym_power(cov, power):
    w, v = np.linalg.eigh(np.asarray(cov, F64))
    return (v * np.maximum(w, EIG_FLOOR) ** power) @ v.T


def match_matrix(src, dst):
    """A = Sigma_dst^(1/2) Sigma_src^(-1/2) (symmetric roots, eigenvalues floored at EIG_FLOOR), b = mu_dst - A mu_src"""
    A = sym_power(dst["cov"], 0.5) @ sym_power(src["cov"], -0.5)
    return A, np.asarray(dst["mean"], F64) - A @ np.asarray(src["mean"], F64)


def luma_match(src, dst):
    k = math.sqrt(max(float(dst["cov"][0][0]), EIG_FLOOR)) / math.sqrt(max(float(src["cov"][0][0]), EIG_FLOOR))
    return k, float(dst["mean"][0]) - k * float(src["mean"][0])
