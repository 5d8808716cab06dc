"""CPU restatement of the Chamfer contract (csrc/chamfer.hip repeats these roundings): point sampling by inverse
CDF of the fp64 face areas, the fp32 brute-force nearest neighbour, the Chamfer loss and its gradients.  numpy / torch only.
Nothing here is tuned to the code under test: every function is the contract's sentence written out."""
import math

import numpy as np
import torch

F32 = np.float32


# ---------------------------------------------------------------------------- meshes
def cow(cow_npz):
    """the golden cow -> verts (V,3) fp32, faces (F,3) int64 (numpy)"""
    return cow_npz["verts"].astype(F32), cow_npz["faces"].astype(np.int64)


def icosphere(level=2):
    """unit icosphere -> verts fp32 (all of length 1 to fp32), faces int64"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v).astype(F32), np.array(f, dtype=np.int64)


# ---------------------------------------------------------------------------- sampling
def uniforms(n, seed):
    """(3,N) fp32 from ONE torch.rand((3,N), generator=), row 0 sorted ascending"""
    r = torch.rand((3, n), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    r[0] = torch.sort(r[0]).values
    return r.numpy()


def face_areas(verts, faces):
    """area_f = |(v1 - v0) x (v2 - v0)| / 2 in fp64 from the fp32 vertices"""
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    return 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def area_cdf(verts, faces):
    return np.cumsum(face_areas(verts, faces))


def bary(r):
    """-> w (N,3) fp32: s = sqrtf(r1), w0 = 1 - s, w1 = s (1 - r2), w2 = s r2"""
    s = np.sqrt(r[1].astype(F32))
    return np.stack([F32(1.0) - s, s * (F32(1.0) - r[2]), s * r[2]], 1).astype(F32)


def sample(verts, faces, r, cdf=None):
    """-> points (N,3) fp32, face_idx (N) int32, w (N,3) fp32.  face = the smallest f with cdf_f > (double)r0 * total.
    A total that is not finite (a NaN / Inf vertex) draws no face: every point is NaN."""
    cdf = area_cdf(verts, faces) if cdf is None else cdf
    w = bary(r)
    if not np.isfinite(cdf[-1]):
        return np.full((r.shape[1], 3), np.nan, F32), np.full(r.shape[1], faces.shape[0] - 1, np.int32), w
    u = r[0].astype(np.float64) * cdf[-1]
    f = np.minimum(np.searchsorted(cdf, u, side="right"), faces.shape[0] - 1)
    a, b, c = verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]]
    p = (w[:, 0:1] * a + w[:, 1:2] * b) + w[:, 2:3] * c
    assert p.dtype == F32
    return p, f.astype(np.int32), w


def sample_grad64(g, face_idx, w, faces, V):
    """d <g, points> / d verts in fp64 -> (grad (V,3), sum of |terms| (V,3))"""
    out, mag = np.zeros((V, 3)), np.zeros((V, 3))
    for k in range(3):
        t = w[:, k:k + 1].astype(np.float64) * g.astype(np.float64)
        np.add.at(out, faces[face_idx, k], t)
        np.add.at(mag, faces[face_idx, k], np.abs(t))
    return out, mag


# ---------------------------------------------------------------------------- nearest neighbour
def dist2(a, b):
    """(dx dx + dy dy) + dz dz in fp32, broadcasting"""
    d = a.astype(F32) - b.astype(F32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn1(x, y, chunk=512):
    """the contract's scan -> idx (P1) int32, dist2 (P1) fp32.  best = +Inf, idx = 0; j replaces the best when d < best: the
    first minimum of the distances with every NaN read as +Inf (a NaN never passes d < best), 0 when there is none below
    +Inf.  The distance is recomputed from x_i and y[idx]."""
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    idx = np.zeros(x.shape[0], np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, x.shape[0], chunk):
            d = dist2(x[s:s + chunk, None, :], y[None, :, :])
            d = np.where(np.isnan(d), F32(np.inf), d)
            idx[s:s + chunk] = np.argmin(d, axis=1)          # the first occurrence of the minimum
        return idx, dist2(x, y[idx])


# ---------------------------------------------------------------------------- chamfer
def chamfer(x, y, single_directional=False, point_reduction="mean"):
    """-> (loss fp32, (idx_x, d_x), (idx_y, d_y) or None).  Each direction's sum in fp64; the first term is rounded to fp32,
    the second is added to it in fp64 and the total rounded once more (one rounding per st3d_chamfer_sum call)."""
    ix, dx = knn1(x, y)
    sx = 1.0 / x.shape[0] if point_reduction == "mean" else 1.0
    loss = F32(sx * dx.astype(np.float64).sum())
    back = None
    if not single_directional:
        iy, dy = knn1(y, x)
        sy = 1.0 / y.shape[0] if point_reduction == "mean" else 1.0
        loss = F32(np.float64(loss) + sy * dy.astype(np.float64).sum())
        back = (iy, dy)
    return loss, (ix, dx), back


def chamfer_grad64(x, y, nn_x, nn_y, sx, sy):
    """d loss / d x in fp64 with the indices held: 2 sx (x_i - y_nn(i)) + 2 sy sum_{j: nn_y(j) = i} (x_i - y_j)
    -> (grad (P1,3), sum of |terms| (P1,3)).  nn_y None: the first term alone; nn_x None: the second alone."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    g, mag = np.zeros_like(x64), np.zeros_like(x64)
    if nn_x is not None:
        t = 2.0 * sx * (x64 - y64[nn_x])
        g, mag = g + t, mag + np.abs(t)
    if nn_y is not None:
        t = 2.0 * sy * (x64[nn_y] - y64)
        np.add.at(g, nn_y, t)
        np.add.at(mag, nn_y, np.abs(t))
    return g, mag


def chamfer_torch64(x, y, nn_x, nn_y, sx, sy):
    """gather-then-square in torch fp64 (differentiable in x and y, the indices constants)"""
    loss = sx * ((x - y[torch.as_tensor(nn_x, dtype=torch.int64)]) ** 2).sum()
    if nn_y is not None:
        loss = loss + sy * ((y - x[torch.as_tensor(nn_y, dtype=torch.int64)]) ** 2).sum()
    return loss


def sample_torch64(verts, faces, face_idx, w):
    """points from their faces and weights in torch fp64 (differentiable in verts)"""
    f = torch.as_tensor(faces)[torch.as_tensor(face_idx, dtype=torch.int64)]
    w = torch.as_tensor(w, dtype=torch.float64)
    return w[:, 0:1] * verts[f[:, 0]] + w[:, 1:2] * verts[f[:, 1]] + w[:, 2:3] * verts[f[:, 2]]


def floor(area, n):
    """2 A / (pi N)"""
    return 2.0 * area / (math.pi * n)
