"""numpy restatement of the NNFM style loss (include/st3d.h, "NNFM style loss"): nearest-neighbour feature
matching of a render tap F (B,C,N) against a style tap S (Bs,C,M) by cosine distance, with optional position weights.

Two precisions:
  * fp64 -- norms, similarities and sums in fp64: what the GPU tests measure against;
  * fp32 -- the roundings of the kernels: squares rounded and added in ascending channel order, sqrtf, the division, and each
    similarity ONE fma chain in ascending channel order starting from 0.  The fma is emulated as round32(fp64(a) * fp64(b) +
    fp64(acc)): the product is exact in fp64, the sum is rounded to 53 bits and then to 24, which differs from the single
    rounding of a real fma only when the fp64 sum lands exactly on a tie of the fp32 grid (about one case in 2^29).
"""
import numpy as np

F32, F64 = np.float32, np.float64


def E(C):
    """the fp32 chain's bound on a similarity of two non-negative unit vectors: C roundings of partial sums <= 1, and 8 ulps
    for the two normalisations"""
    return (C + 8) * 2.0 ** -24


# ---------------------------------------------------------------------------- norms
def norms(x, dtype=F64):
    """x (C, M) -> n (M): sqrt of the squares added in ascending channel order, every operation rounded to `dtype`"""
    x = np.asarray(x).astype(dtype)
    acc = np.zeros(x.shape[1], dtype)
    with np.errstate(all="ignore"):
        for c in range(x.shape[0]):
            acc = (acc + (x[c] * x[c]).astype(dtype)).astype(dtype)
        return np.sqrt(acc).astype(dtype)


def normalise(x, dtype=F64):
    """-> (xhat (C, M), n (M)); a zero vector stays zero"""
    x = np.asarray(x).astype(dtype)
    n = norms(x, dtype)
    with np.errstate(all="ignore"):
        hat = np.where(n[None, :] == 0, dtype(0), x / np.where(n == 0, dtype(1), n)[None, :]).astype(dtype)
    return hat, n


# ---------------------------------------------------------------------------- similarities
def sims(fhat, shat, dtype=F64):
    """fhat (C, N), shat (C, M) -> sim (N, M).  fp64: the dot products; fp32: the ascending fma chain from 0"""
    if dtype == F64:
        with np.errstate(all="ignore"):
            return np.asarray(fhat, F64).T @ np.asarray(shat, F64)
    f, s = np.asarray(fhat, F32), np.asarray(shat, F32)
    acc = np.zeros((f.shape[1], s.shape[1]), F32)
    with np.errstate(all="ignore"):
        for c in range(f.shape[0]):
            acc = (f[c].astype(F64)[:, None] * s[c].astype(F64)[None, :] + acc.astype(F64)).astype(F32)
    return acc


def scan(sim):
    """the search of one image: j ascending from best = -Inf, idx = 0, j replaces the best when sim_ij > best.  NaN never
    passes the test.  -> idx (N) int32"""
    masked = np.where(np.isnan(sim), -np.inf, sim)
    return np.argmax(masked, axis=1).astype(np.int32)          # argmax returns the first of equal maxima; all -Inf -> 0


def search_image(F, S, w=None, dtype=F64):
    """F (C, N), S (C, M), w (N) or None -> (idx (N) int32, d (N) dtype, n (N) dtype)"""
    fhat, n = normalise(F, dtype)
    shat, _ = normalise(S, dtype)
    sim = sims(fhat, shat, dtype)
    idx = scan(sim)
    with np.errstate(all="ignore"):
        d = (dtype(1) - sim[np.arange(sim.shape[0]), idx]).astype(dtype)
    zero = n == 0
    idx = np.where(zero, -1, idx).astype(np.int32)
    d = np.where(zero, dtype(1), d).astype(dtype)
    if w is not None:
        off = np.asarray(w) == 0
        idx = np.where(off, -1, idx).astype(np.int32)
        d = np.where(off, dtype(0), d).astype(dtype)
    return idx, d, n


def search(F, S, w=None, dtype=F64):
    """F (B, C, N), S (Bs, C, M), Bs in {1, B}, w (B, N) or None -> (idx (B, N), d (B, N))"""
    B = F.shape[0]
    out = [search_image(F[b], S[b if S.shape[0] > 1 else 0], None if w is None else w[b], dtype) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------------------- loss and gradient (fp64)
def loss(d, w=None, batch_denom=None):
    """d (B, N), w (B, N) or None -> L = (1 / batch_denom) sum_b (sum_i w_i d_i / sum_i w_i); an image of sum w = 0 adds 0"""
    d = np.asarray(d, F64)
    w = np.ones_like(d) if w is None else np.asarray(w, F64)
    total = 0.0
    for b in range(d.shape[0]):
        W = w[b].sum()
        if W > 0:
            total += (w[b][w[b] != 0] * d[b][w[b] != 0]).sum() / W
    return total / float(batch_denom if batch_denom is not None else d.shape[0])


def grad(F, S, idx, w=None, batch_denom=None):
    """d L / d F (B, C, N) in fp64 for the given indices (constants):
    -(w_i / (W_b batch_denom n_i)) (s^_j - sim_ij f^_i), j = idx_i; zero where idx_i = -1 or W_b = 0"""
    B, C, N = F.shape
    denom = float(batch_denom if batch_denom is not None else B)
    out = np.zeros((B, C, N), F64)
    for b in range(B):
        fhat, n = normalise(F[b], F64)
        shat, _ = normalise(S[b if S.shape[0] > 1 else 0], F64)
        wb = np.ones(N, F64) if w is None else np.asarray(w[b], F64)
        W = wb.sum()
        on = (idx[b] >= 0) & (wb != 0)
        if not W > 0 or not on.any():
            continue
        sj = shat[:, idx[b][on]]
        with np.errstate(all="ignore"):
            sim = (fhat[:, on] * sj).sum(axis=0)
            out[b][:, on] = -(wb[on] / (W * denom * n[on]))[None, :] * (sj - sim[None, :] * fhat[:, on])
    return out


def grad_bound(F, S, idx, w=None, batch_denom=None):
    """the per-element bound of the GPU gradient against `grad`:
    (w_i / (W_b denom n_i)) (16 2^-24 (|s^_jc| + |f^_ic|) + E(C) |f^_ic|)"""
    B, C, N = F.shape
    denom = float(batch_denom if batch_denom is not None else B)
    out = np.zeros((B, C, N), F64)
    for b in range(B):
        fhat, n = normalise(F[b], F64)
        shat, _ = normalise(S[b if S.shape[0] > 1 else 0], F64)
        wb = np.ones(N, F64) if w is None else np.asarray(w[b], F64)
        W = wb.sum()
        on = (idx[b] >= 0) & (wb != 0)
        if not W > 0 or not on.any():
            continue
        sj, fh = np.abs(shat[:, idx[b][on]]), np.abs(fhat[:, on])
        out[b][:, on] = (wb[on] / (W * denom * n[on]))[None, :] * (16 * 2.0 ** -24 * (sj + fh) + E(C) * fh)
    return out


# ---------------------------------------------------------------------------- mask pooling
def pool_mask(mask, H, W):
    """mask (B, S, S') fp32 -> (B, H, W): successive 2x2 averages in fp32"""
    m = np.asarray(mask, F32)
    while m.shape[1] > H:
        m = ((m[:, 0::2, 0::2] + m[:, 0::2, 1::2] + m[:, 1::2, 0::2] + m[:, 1::2, 1::2]) * F32(0.25)).astype(F32)
    assert m.shape[1:] == (H, W), (m.shape, H, W)
    return m


def relu_like(rng, shape):
    """seeded post-ReLU-like features: max(randn + 0.3, 0)"""
    return np.maximum(rng.standard_normal(shape).astype(F32) + F32(0.3), F32(0)).astype(F32)
