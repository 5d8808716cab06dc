"""fp64 numpy restatement of csrc/bake.hip: the texel -> surface map (surface) and the bake of a batch of views (bake), the
rule of DESIGN 7 "Baking views into the texture" spelled a second time, with, for every decision, whether it was taken with
margin (the GPU tests compare only those).

Texel (row r, column x) of the map as stored sits at (x, T-1-r) in texel units, UV x (T-1).  The squared distances of the
surface stage are compared as rounded to fp32 (they are half of the kernel's 64-bit key); everything else is fp64.
"""
import numpy as np

F32, F64 = np.float32, np.float64
INV_TAN_HALF_FOV = float(1.0 / np.tan(np.radians(60.0) / 2.0))
EDGE_MARGIN = 1e-5          # an edge function within this, relative, of 0
D2_MARGIN = 1e-5            # a squared distance within this, relative, of pad^2 or of the runner-up's
RINT_MARGIN = 1e-3          # ix / iy within this of an integer (floor flips) or of a half (rint flips)
DEPTH_MARGIN = 1e-4         # | |zv - z| - depth_tol zv | within this x zv
COS_MARGIN = 1e-4           # c within this of min_cos
BEST_MARGIN = 1e-5          # the two largest weights of 'best' within this, relative
NEAR_D2 = 1e-4              # an edge function decides inside against outside: it is looked at for faces within 0.01 texel


def _seg(px, py, ax, ay, bx, by):
    ex, ey = bx - ax, by - ay
    den = ex * ex + ey * ey
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(den > 0, ((px - ax) * ex + (py - ay) * ey) / np.where(den > 0, den, 1.0), 0.0)
    t = np.minimum(np.maximum(t, 0.0), 1.0)
    dx, dy = px - np.where(t < 1.0, ax + t * ex, bx), py - np.where(t < 1.0, ay + t * ey, by)      # at t = 1: b itself
    return dx * dx + dy * dy, t


def closest(px, py, ax, ay, bx, by, cx, cy):
    """closest point of the triangles (a, b, c) to the points p (broadcast) -> d2, (b0, b1, b2), ok, edge_close.
    d2 is exactly 0 inside or on the triangle (the edge functions, signed by the winding, all >= 0); outside, the nearest of
    ab, bc, ca decides, the first among equals.  ok = False: no area.  edge_close: an edge function within EDGE_MARGIN,
    relative to its two products, of 0."""
    px, py, ax, ay, bx, by, cx, cy = np.broadcast_arrays(*(np.asarray(v, F64) for v in (px, py, ax, ay, bx, by, cx, cy)))
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    ok = area != 0
    sign = np.where(area < 0, -1.0, 1.0)
    es, close = [], np.zeros(area.shape, bool)
    for (qx, qy, rx, ry) in ((bx, by, cx, cy), (cx, cy, ax, ay), (ax, ay, bx, by)):
        m1, m2 = (qx - px) * (ry - py), (qy - py) * (rx - px)
        e = m1 - m2
        close |= np.abs(e) <= EDGE_MARGIN * (np.abs(m1) + np.abs(m2))
        es.append(e * sign)
    A = np.where(ok, area * sign, 1.0)
    inside = (es[0] >= 0) & (es[1] >= 0) & (es[2] >= 0)
    d_ab, t_ab = _seg(px, py, ax, ay, bx, by)
    d_bc, t_bc = _seg(px, py, bx, by, cx, cy)
    d_ca, t_ca = _seg(px, py, cx, cy, ax, ay)
    zero, one = np.zeros_like(d_ab), np.ones_like(d_ab)
    d2 = d_ab
    b = [one - t_ab, t_ab, zero]
    take = d_bc < d2
    d2 = np.where(take, d_bc, d2)
    b = [np.where(take, v, w) for v, w in zip((zero, one - t_bc, t_bc), b)]
    take = d_ca < d2
    d2 = np.where(take, d_ca, d2)
    b = [np.where(take, v, w) for v, w in zip((t_ca, zero, one - t_ca), b)]
    d2 = np.where(inside, 0.0, d2)
    b = [np.where(inside, e / A, w) for e, w in zip(es, b)]
    return d2, b, ok, close


def surface(verts_uvs, faces_uvs, T, pad=1.5, chunk=256):
    """-> t2f (T,T) int32, tbary (T,T,3) float64, unsure (T,T) bool.  unsure: the decision had no margin -- an edge function
    of a face the texel lies on or within 0.01 texel of was within EDGE_MARGIN of 0, or the winner's d2 within D2_MARGIN of
    pad^2 or of a different runner-up d2."""
    uv = np.asarray(verts_uvs, F32).reshape(-1, 2).astype(F64) * F64(T - 1)
    fuv = np.asarray(faces_uvs).reshape(-1, 3).astype(np.int64)
    pad2 = F32(F32(pad) * F32(pad))
    N = T * T
    r, x = np.divmod(np.arange(N), T)
    px, py = x.astype(F64)[:, None], (T - 1 - r).astype(F64)[:, None]
    best = np.full(N, np.inf, F32)
    second = np.full(N, np.inf, F32)
    face = np.full(N, -1, np.int64)
    unsure = np.zeros(N, bool)
    for lo in range(0, fuv.shape[0], chunk):
        c = uv[fuv[lo:lo + chunk]]                                   # (Fc, 3, 2)
        d2, _, ok, close = closest(px, py, c[None, :, 0, 0], c[None, :, 0, 1], c[None, :, 1, 0], c[None, :, 1, 1],
                                   c[None, :, 2, 0], c[None, :, 2, 1])
        d2 = np.where(ok, d2, np.inf).astype(F32)
        unsure |= (ok & close & (d2 <= NEAR_D2)).any(1)
        k = d2.argmin(1)                                             # the first (lowest) face among equals
        cb = d2[np.arange(N), k]
        rest = d2.copy()
        rest[np.arange(N), k] = np.inf
        cs = rest.min(1) if d2.shape[1] > 1 else np.full(N, np.inf, F32)
        wins = cb < best                                             # an earlier (lower) face keeps a tie
        second = np.where(wins, np.minimum(best, cs), np.minimum(second, cb))
        face = np.where(wins, lo + k, face)
        best = np.where(wins, cb, best)
    taken = best <= pad2
    with np.errstate(invalid="ignore"):
        if pad2 > 0:
            unsure |= np.abs(best.astype(F64) - F64(pad2)) <= D2_MARGIN * F64(pad2)
        # an exact tie is the rule's own case (the lowest face), not a doubt: the faces around a vertex or an edge find the
        # same distance to it from the same operands, in any arithmetic
        reach = best.astype(F64) <= F64(pad2) * (1 + D2_MARGIN)
        unsure |= reach & np.isfinite(second) & (second > best) & ((second.astype(F64) - best.astype(F64)) <= D2_MARGIN * second.astype(F64))
    t2f = np.where(taken, face, -1).astype(np.int32)
    tbary = np.zeros((N, 3), F64)
    idx = np.nonzero(taken)[0]
    if idx.size:
        c = uv[fuv[t2f[idx]]]
        _, b, _, _ = closest(px[idx, 0], py[idx, 0], c[:, 0, 0], c[:, 0, 1], c[:, 1, 0], c[:, 1, 1], c[:, 2, 0], c[:, 2, 1])
        tbary[idx] = np.stack(b, -1)
    return t2f.reshape(T, T), tbary.reshape(T, T, 3), unsure.reshape(T, T)


def texel_uv_units(T):
    """-> (T,T,2) float64: the position of texel (row r, column x) in texel units, (x, T-1-r)"""
    r, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    return np.stack([x, T - 1 - r], -1).astype(F64)


def _unit(v):
    return v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-12)


def views(verts, faces, t2f, tbary, R, T, images, p2f, zbuf, min_cos=0.1, depth_tol=0.01, power=2.0, s=INV_TAN_HALF_FOV):
    """Per view and texel, in fp64 -> dict: used (B,N) bool, w (B,N), colour (B,N,3), unsure (B,N) bool, c (B,N), valid (N,)
    bool = t2f >= 0.  unsure: a decision of that texel-view had no margin (see the constants above); such a texel-view may
    be used or not."""
    verts = np.asarray(verts, F32).astype(F64)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    t2f = np.asarray(t2f).reshape(-1)
    tb = np.asarray(tbary).reshape(-1, 3).astype(F64)
    R, T = np.asarray(R, F32).astype(F64).reshape(-1, 3, 3), np.asarray(T, F32).astype(F64).reshape(-1, 3)
    images = np.asarray(images, F32).astype(F64)
    p2f, zbuf = np.asarray(p2f), np.asarray(zbuf, F32).astype(F64)
    B, S = images.shape[0], images.shape[2]
    N = t2f.shape[0]
    valid = t2f >= 0
    f = np.where(valid, t2f, 0)
    v0, v1, v2 = verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]]
    P = tb[:, 0:1] * v0 + tb[:, 1:2] * v1 + tb[:, 2:3] * v2
    n = _unit(np.cross(v1 - v0, v2 - v0))
    out = {k: np.zeros((B, N), t) for k, t in (("used", bool), ("w", F64), ("unsure", bool), ("c", F64))}
    out["colour"] = np.zeros((B, N, 3), F64)
    out["valid"] = valid
    for b in range(B):
        alive, unsure = valid.copy(), np.zeros(N, bool)
        view = P @ R[b] + T[b]
        zv = view[:, 2]
        alive &= zv > 0.5
        zs = np.where(zv > 0.5, zv, 1.0)
        ix = ((1.0 - (s * view[:, 0]) / zs) * S - 1.0) / 2.0
        iy = ((1.0 - (s * view[:, 1]) / zs) * S - 1.0) / 2.0
        for q in (ix, iy):
            frac = q - np.floor(q)
            unsure |= alive & ((np.abs(frac - 0.5) <= RINT_MARGIN) | (np.minimum(frac, 1.0 - frac) <= RINT_MARGIN))
        rx, ry = np.rint(ix), np.rint(iy)
        alive &= (rx >= 0) & (rx < S) & (ry >= 0) & (ry < S)
        px, py = np.where(alive, rx, 0).astype(np.int64), np.where(alive, ry, 0).astype(np.int64)
        g, z = p2f[b, py, px], zbuf[b, py, px]
        alive &= g >= 0
        other = alive & (g != f)
        gap = np.abs(zv - z) - depth_tol * zv
        unsure |= other & (np.abs(gap) <= DEPTH_MARGIN * zv)
        alive &= (g == f) | (gap <= 0)
        C = -(R[b] @ T[b])                                           # C = -T R^T
        c = np.abs((n * _unit(C[None] - P)).sum(-1))
        unsure |= alive & (np.abs(c - min_cos) <= COS_MARGIN)
        alive &= c >= min_cos
        fx, fy = np.floor(ix), np.floor(iy)
        wx1, wy1 = ix - fx, iy - fy
        wx0, wy0 = 1.0 - wx1, 1.0 - wy1
        x0 = np.clip(np.where(alive, fx, 0), 0, S - 1).astype(np.int64)
        x1 = np.clip(np.where(alive, fx + 1, 0), 0, S - 1).astype(np.int64)
        y0 = np.clip(np.where(alive, fy, 0), 0, S - 1).astype(np.int64)
        y1 = np.clip(np.where(alive, fy + 1, 0), 0, S - 1).astype(np.int64)
        col, tot = np.zeros((N, 3), F64), np.zeros(N, F64)
        for yy, xx, w in ((y0, x0, wy0 * wx0), (y0, x1, wy0 * wx1), (y1, x0, wy1 * wx0), (y1, x1, wy1 * wx1)):
            w = np.where(p2f[b, yy, xx] >= 0, w, 0.0)
            col += w[:, None] * images[b][:, yy, xx].T
            tot += w
        alive &= tot > 0
        col = col / np.where(tot > 0, tot, 1.0)[:, None]
        out["used"][b] = alive
        out["unsure"][b] = unsure
        out["c"][b] = c
        out["w"][b] = np.where(alive, np.power(np.where(alive, c, 1.0), power), 0.0)
        out["colour"][b] = np.where(alive[:, None], col, 0.0)
    return out


def accumulate(detail, mode="mean", acc=None):
    """the per-view figures of views() -> acc (N,4) float64, unsure (N,) bool.  'mean': sums in view order; 'best': the view
    of the largest weight, the earliest among equals.  acc continues an earlier result.  unsure: a view of the texel was, or
    ('best') the two largest weights -- the carried one included -- are within BEST_MARGIN, relative."""
    used, w, col = detail["used"], detail["w"], detail["colour"]
    B, N = used.shape
    acc = np.zeros((N, 4), F64) if acc is None else np.array(acc, F64).reshape(N, 4)
    unsure = detail["unsure"].any(0)
    for b in range(B):
        if mode == "mean":
            acc[:, :3] += np.where(used[b][:, None], w[b][:, None] * col[b], 0.0)
            acc[:, 3] += np.where(used[b], w[b], 0.0)
        else:
            hi, lo = np.maximum(w[b], acc[:, 3]), np.minimum(w[b], acc[:, 3])
            unsure |= used[b] & (acc[:, 3] > 0) & ((hi - lo) <= BEST_MARGIN * hi)
            take = used[b] & (w[b] > acc[:, 3])
            acc[:, :3] = np.where(take[:, None], w[b][:, None] * col[b], acc[:, :3])
            acc[:, 3] = np.where(take, w[b], acc[:, 3])
    return acc, unsure


def bake(verts, faces, t2f, tbary, R, T, images, p2f, zbuf, mode="mean", power=2.0, min_cos=0.1, depth_tol=0.01, acc=None):
    """-> acc (Tt,Tt,4) float64, unsure (Tt,Tt) bool, detail (views())"""
    side = np.asarray(t2f).shape[0]
    detail = views(verts, faces, t2f, tbary, R, T, images, p2f, zbuf, min_cos, depth_tol, power)
    out, unsure = accumulate(detail, mode, None if acc is None else np.asarray(acc).reshape(-1, 4))
    return out.reshape(side, side, 4), unsure.reshape(side, side), detail


def resolve(acc, fallback):
    acc, fallback = np.asarray(acc, F64), np.asarray(fallback)
    w = acc[..., 3:4]
    return np.where(w > 0, acc[..., :3] / np.where(w > 0, w, 1.0), fallback)


def cpu_fragments(verts, faces, R, T, S):
    """the CPU oracle's hard K = 1 fragments of the views (R (B,3,3), T (B,3)) at side S -> p2f (B,S,S) int32, zbuf (B,S,S)"""
    from oracle import render_ref as RR
    frags = [RR.rasterize(RR.project_verts(verts, R[b], T[b]), faces, S) for b in range(len(R))]
    return np.stack([f[0] for f in frags]), np.stack([f[1] for f in frags])


# ---------------------------------------------------------------------------------------------------------- scenes
def quad_chart():
    """one quad as two triangles over a generic (no texel on an edge) part of the UV square -> verts_uvs (4,2) f32, faces_uvs
    (2,3) i32"""
    uvs = np.array([[0.21, 0.27], [0.83, 0.22], [0.87, 0.79], [0.16, 0.74]], F32)
    return uvs, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def facing_quad(z=0.0, half=0.6, cx=0.013, cy=0.029):
    """a quad in the plane z around (cx, cy), with quad_chart's UVs -> verts (4,3) f32, faces (2,3) i32.  Slightly off the
    axis: seen from front_camera, a centred quad's diagonal would run through pixel centres, which the rasteriser gives to
    neither triangle"""
    verts = np.array([[cx - half, cy - half, z], [cx + half, cy - half, z], [cx + half, cy + half, z], [cx - half, cy + half, z]], F32)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def front_camera(dist=2.5):
    """a camera on the +z axis looking at the origin (PyTorch3D's look_at_view_transform(dist, 0, 0)) -> R (1,3,3), T (1,3)"""
    R = np.array([[[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]], F32)
    return R, np.array([[0.0, 0.0, dist]], F32)


def ramp_images(B, S):
    """(B,3,S,S) float32 ramps: channel 0 along x, 1 along y, 2 along the diagonal, a different slope per view; the largest
    difference between adjacent pixels (any of the 8 neighbours) is returned with them"""
    y, x = np.meshgrid(np.arange(S, dtype=F64), np.arange(S, dtype=F64), indexing="ij")
    imgs = np.stack([np.stack([(0.2 + 0.6 * x / S) / (b + 1), (0.9 - 0.5 * y / S) / (b + 1), (0.1 + 0.4 * (x + y) / S) / (b + 1)])
                     for b in range(B)]).astype(F32)
    return imgs, adjacent_difference(imgs)


def adjacent_difference(imgs):
    """G: the largest |difference| between pixels one step apart along x or y"""
    imgs = np.asarray(imgs, F64)
    return float(max(np.abs(np.diff(imgs, axis=-1)).max(), np.abs(np.diff(imgs, axis=-2)).max()))
