"""numpy restatement of the sliced Wasserstein style loss (include/st3d.h, "sliced Wasserstein style loss"):
a render tap F (B,C,N) and a style tap S (Bs,C,M) are projected onto K unit directions V (K,C), every projected row is sorted
by the total order (inactive, key, index), rank r of a row meets the style quantile j(r), and the loss is the mean squared
difference.

  project      fp64: the dot products; fp32: each value ONE fma chain in ascending c from 0.  The fma is emulated as
               round32(fp64(a) * fp64(b) + fp64(acc)) (the construction of _nnfmref.sims): the product is exact in fp64, the
               sum is rounded to 53 bits and then to 24, which differs from a real fma only on an exact tie of the fp32 grid.
  key / order  the order-preserving map of the fp32 bits to uint32 with every NaN as 0x7FC00000; np.lexsort on the triple
  quantile     j(r) = ((2r+1) M) // (2 n) in integers
  loss / grad  fp64
"""
import numpy as np

F32, F64 = np.float32, np.float64


def relu_like(rng, shape):
    """seeded post-ReLU-like features: max(randn + 0.3, 0)"""
    return np.maximum(rng.standard_normal(shape).astype(F32) + F32(0.3), F32(0)).astype(F32)


def unit_rows(rng, K, C):
    """(K,C) fp32 rows of unit norm (to fp32 rounding)"""
    v = rng.standard_normal((K, C))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


# ---------------------------------------------------------------------------- projection
def project(x, a, dtype=F64):
    """x (B,Q,N), a (R,Q) -> (B,R,N).  fp64: the dot products; fp32: the ascending fma chain from 0"""
    x, a = np.asarray(x, F32), np.asarray(a, F32)
    with np.errstate(all="ignore"):
        if dtype == F64:
            return np.einsum("rq,bqn->brn", a.astype(F64), x.astype(F64))
        acc = np.zeros((x.shape[0], a.shape[0], x.shape[2]), F32)
        for q in range(x.shape[1]):
            acc = (a[:, q].astype(F64)[None, :, None] * x[:, q].astype(F64)[:, None, :] + acc.astype(F64)).astype(F32)
        return acc


def project_bound(x, a):
    """the standard bound of a length-Q fp32 chain against fp64: (Q+1) 2^-24 sum_q |a_rq x_qn|, per element"""
    x, a = np.abs(np.asarray(x, F64)), np.abs(np.asarray(a, F64))
    return (x.shape[1] + 1) * 2.0 ** -24 * np.einsum("rq,bqn->brn", a, x)


# ---------------------------------------------------------------------------- order
def key(v):
    """fp32 values -> uint32 keys: NaN -> 0x7FC00000 first, then all bits flipped if the sign bit is set, else the sign bit"""
    u = np.ascontiguousarray(np.asarray(v, F32)).view(np.uint32).copy()
    u[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0x7FC00000)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sort_rows(proj, w=None):
    """proj (B,K,N) fp32, w (B,N) or None -> (sorted (B,K,N) fp32 = the original values in order, perm (B,K,N) int32,
    count (B) int32): every row ascending by (inactive, key, index), inactive = not w > 0"""
    proj = np.asarray(proj, F32)
    B, K, N = proj.shape
    inactive = np.zeros((B, N), bool) if w is None else ~(np.asarray(w, F32) > 0)
    keys = key(proj)
    perm = np.empty((B, K, N), np.int32)
    index = np.arange(N)
    for b in range(B):
        for k in range(K):
            perm[b, k] = np.lexsort((index, keys[b, k], inactive[b]))          # the last key is the primary one
    return np.take_along_axis(proj, perm.astype(np.int64), axis=2), perm, (~inactive).sum(axis=1).astype(np.int32)


def quantile(n, M):
    """j(r) for r < n: ((2r+1) M) // (2n)"""
    r = np.arange(n, dtype=np.int64)
    return ((2 * r + 1) * M) // (2 * n)


# ---------------------------------------------------------------------------- loss and gradient (fp64)
def loss(srt, count, tsorted, batch_denom=None):
    """srt (B,K,N), count (B), tsorted (Bs,K,M) -> L = (1 / batch_denom) sum_b (1 / (K n_b)) sum_k sum_{r<n_b} (.)^2"""
    srt, tsorted = np.asarray(srt, F64), np.asarray(tsorted, F64)
    B, K, N = srt.shape
    M = tsorted.shape[2]
    total = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            n = int(count[b])
            if n == 0:
                continue
            t = tsorted[b if tsorted.shape[0] > 1 else 0][:, quantile(n, M)]
            total += ((srt[b, :, :n] - t) ** 2).sum() / (K * n)
    return total / float(batch_denom if batch_denom is not None else B)


def grad_proj(srt, perm, count, tsorted, batch_denom=None, g=1.0):
    """d L / d proj (B,K,N) in fp64: g 2 / (batch_denom K n_b) (sorted_kbr - tsorted_{k,j(r)}) at position perm[r], r < n_b;
    zero elsewhere"""
    srt, tsorted = np.asarray(srt, F64), np.asarray(tsorted, F64)
    B, K, N = srt.shape
    M = tsorted.shape[2]
    inv = 1.0 / float(batch_denom if batch_denom is not None else B)
    out = np.zeros((B, K, N), F64)
    with np.errstate(all="ignore"):
        for b in range(B):
            n = int(count[b])
            if n == 0:
                continue
            t = tsorted[b if tsorted.shape[0] > 1 else 0][:, quantile(n, M)]
            cf = (g * 2.0 * inv) / (K * n)
            vals = cf * (srt[b, :, :n] - t)
            np.put_along_axis(out[b], perm[b, :, :n].astype(np.int64), vals, axis=1)
    return out


# ---------------------------------------------------------------------------- the whole term
def term(F, S, V, w=None, batch_denom=None, dtype=F64):
    """F (B,C,N), S (Bs,C,M), V (K,C), w (B,N) or None -> (L, dL/dF (B,C,N) fp64).  dtype: the precision of the projections
    (the order is taken on their fp32 roundings, as on the GPU)"""
    p = project(F, V, dtype)
    t = project(S, V, dtype)
    _, perm, count = sort_rows(p.astype(F32), w)
    srt = np.take_along_axis(p, perm.astype(np.int64), axis=2)
    tperm = sort_rows(t.astype(F32))[1]
    tsorted = np.take_along_axis(t, tperm.astype(np.int64), axis=2)
    L = loss(srt, count, tsorted, batch_denom)
    gp = grad_proj(srt, perm, count, tsorted, batch_denom)
    return L, np.einsum("kc,bkn->bcn", np.asarray(V, F64), gp)
