"""numpy restatement of csrc/cover.hip: which texels a view's hard K = 1 fragments touch (mark), the greedy choice of views
(greedy) and the per-texel count (count).  Integer results: the GPU tests compare them bit for bit.

mark restates frag_uv and uv_footprint of csrc/shadek1.h in fp32, operation for operation; the rule of record is: a texel of
the pixel's bilinear footprint is marked when it is inside the map and both of its weights are > 0 -- the texels to which
shade_bwd of a positive gradient adds a non-zero weight (tests/test_cover_ref.py checks that against the C oracle).

Layout: W = words(T) uint32 words per view, texel (row r, column x) of the map as stored = bit (r*T + x) & 31 of word
(r*T + x) >> 5.  Masks are handed around as int32 (torch has no uint32 arithmetic); as_u32 / as_i32 reinterpret."""
import numpy as np

F32 = np.float32


def words(T):
    return (T * T + 31) // 32


def as_u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def as_i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def touched(frag, verts_uvs, faces_uvs, T):
    """one view's fragments (p2f (S,S), zbuf, bary (S,S,3), dists) -> bool (T,T): [r, x] = texel (row r, column x) is marked"""
    p2f, _, bary, _ = frag
    cov = np.asarray(p2f) >= 0
    out = np.zeros((T, T), bool)
    if not cov.any():
        return out
    f = np.asarray(p2f)[cov]
    b = np.asarray(bary, F32)[cov]
    uvs = np.asarray(verts_uvs, F32).reshape(-1, 2)
    corner = np.asarray(faces_uvs).reshape(-1, 3)[f]
    b0, b1, b2 = b[:, 0], b[:, 1], b[:, 2]
    one, two = F32(1), F32(2)
    # frag_uv: the three products added from left to right, every operation rounded to fp32
    u = (b0 * uvs[corner[:, 0], 0] + b1 * uvs[corner[:, 1], 0]).astype(F32) + b2 * uvs[corner[:, 2], 0]
    v = (b0 * uvs[corner[:, 0], 1] + b1 * uvs[corner[:, 1], 1]).astype(F32) + b2 * uvs[corner[:, 2], 1]
    # uv_footprint
    hi = F32(T - 1)
    with np.errstate(invalid="ignore"):
        gx, gy = u * two - one, v * two - one
        ix, iy = ((gx + one) / two) * hi, ((gy + one) / two) * hi
        ix = np.where(~(ix >= 0), F32(0), np.where(ix > hi, hi, ix)).astype(F32)
        iy = np.where(~(iy >= 0), F32(0), np.where(iy > hi, hi, iy)).astype(F32)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, yf0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, yf1 = x0 + 1, yf0 + 1
    wx1, wy1 = ix - fx, iy - fy
    wx0, wy0 = one - wx1, one - wy1
    assert all(a.dtype == F32 for a in (u, v, ix, iy, wx0, wx1, wy0, wy1))
    vx0, vx1 = (x0 >= 0) & (x0 < T), (x1 >= 0) & (x1 < T)
    vy0, vy1 = (yf0 >= 0) & (yf0 < T), (yf1 >= 0) & (yf1 < T)
    r0, r1 = (T - 1) - yf0, (T - 1) - yf1
    for ok, r, x in ((vy0 & vx0 & (wy0 > 0) & (wx0 > 0), r0, x0), (vy0 & vx1 & (wy0 > 0) & (wx1 > 0), r0, x1),
                     (vy1 & vx0 & (wy1 > 0) & (wx0 > 0), r1, x0), (vy1 & vx1 & (wy1 > 0) & (wx1 > 0), r1, x1)):
        out[r[ok], x[ok]] = True
    return out


def pack(touch):
    """bool (C,T,T) -> masks (C, words(T)) int32"""
    touch = np.asarray(touch, bool)
    C, T = touch.shape[0], touch.shape[1]
    W = words(T)
    bits = np.zeros((C, W * 32), np.uint32)
    bits[:, :T * T] = touch.reshape(C, T * T)
    return as_i32((bits.reshape(C, W, 32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32))


def unpack(masks, T):
    """masks (C, W) -> bool (C,T,T)"""
    m = as_u32(masks)
    bits = (m[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(m.shape[0], -1)[:, :T * T].reshape(m.shape[0], T, T).astype(bool)


def mark(frags, verts_uvs, faces_uvs, T, masks=None):
    """a list of B views' fragments -> masks (B, words(T)) int32, ORed into `masks` when given"""
    new = pack(np.stack([touched(fr, verts_uvs, faces_uvs, T) for fr in frags]))
    return new if masks is None else as_i32(as_u32(masks) | as_u32(new))


def popcount(a):
    return int(np.unpackbits(as_u32(a).view(np.uint8)).sum())


def greedy(masks, n, covered=None):
    """-> (picks (n,) int32, gains (n,) int32, covered (W,) int32): every round takes the untaken row that adds the most bits
    to covered, the lowest index among equals; a taken row is never taken again."""
    m = as_u32(masks)
    C, W = m.shape
    assert 1 <= n <= C
    cov = np.zeros(W, np.uint32) if covered is None else as_u32(covered).copy()
    taken = np.zeros(C, bool)
    picks, gains = [], []
    for _ in range(n):
        gain = np.unpackbits(np.ascontiguousarray(m & ~cov).view(np.uint8), axis=1).sum(1, dtype=np.int64)
        gain[taken] = -1
        best = int(np.argmax(gain))             # the first of the largest
        picks.append(best)
        gains.append(int(gain[best]))
        taken[best] = True
        cov |= m[best]
    return np.array(picks, np.int32), np.array(gains, np.int32), as_i32(cov)


def count(masks, T):
    """-> (T,T) int32: how many rows touch each texel"""
    return unpack(masks, T).sum(0).astype(np.int32)


def reached(masks):
    """texels any row touches"""
    return popcount(np.bitwise_or.reduce(as_u32(masks), axis=0))
