"""TEST INFRASTRUCTURE ONLY: vectorised numpy restatement of the silhouette rasteriser's semantics (csrc/silraster.hip).

"All candidates of every pixel": every decision, the depth pz and the edge distance d in fp32 in the operation order of
oracle/raster_ref.c:ref_rasterize_k3 (numpy float32 arithmetic rounds every operation and never contracts a multiply-add);
the clipped records come from the C oracle's own ref_clip_face.  Then: of the two halves of a quadrilateral split by the near
plane the one nearer in the image plane stays ("halves first"), the K nearest by (pz, record slot) are the fragments, and
sigmoid_alpha_blend over them in fp64.

The C oracle's per-pixel lists hold 16 entries, so it can serve as a check only for K <= 16 (tests/test_silraster_ref.py pins
this module to it there); this module has no such limit."""
import ctypes

import numpy as np

F32 = np.float32
K_EPS = F32(1e-8)


def _pix_to_ndc(i, S):
    return F32(-1.0) + (F32(2.0) * i.astype(F32) + F32(1.0)) / F32(S)


def records(ndc, faces, z_clip=0.5, perspective_correct=True):
    """-> tri (2F,9) float32, code (2F,) int32: the two record slots per face of ref_rasterize_k3 (z_clip None: no clipping)"""
    from oracle import render_ref as rr
    ndc = np.ascontiguousarray(ndc, F32)
    faces = np.asarray(faces)
    Fn = faces.shape[0]
    v = ndc[faces].reshape(Fn, 9)
    tri = np.zeros((Fn, 2, 9), F32)
    code = np.zeros((Fn, 2), np.int32)
    tri[:, 0] = v
    code[:, 0] = 1
    if z_clip is not None:
        fn = rr.lib().ref_clip_face
        fp = ctypes.POINTER(ctypes.c_float)
        t = np.zeros((2, 9), F32)
        c = np.zeros(2, np.int32)
        w = np.zeros(2, F32)
        for f in np.nonzero((v[:, 2::3] < F32(z_clip)).any(axis=1))[0]:
            vf = np.ascontiguousarray(v[f])
            fn(vf.ctypes.data_as(fp), ctypes.c_float(z_clip), ctypes.c_int(1 if perspective_correct else 0),
               t.ctypes.data_as(fp), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), w.ctypes.data_as(fp))
            tri[f], code[f] = t, c
    return tri.reshape(2 * Fn, 9), code.reshape(2 * Fn)


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _pld2(px, py, ax, ay, bx, by):
    bax, bay = bx - ax, by - ay
    l2 = bax * bax + bay * bay
    deg = l2 <= K_EPS
    dxb, dyb = px - bx, py - by
    d_deg = dxb * dxb + dyb * dyb
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (bax * (px - ax) + bay * (py - ay)) / l2
    t = np.where(t < 0, F32(0), np.where(t > 1, F32(1), t)).astype(F32)
    qx, qy = ax + t * bax, ay + t * bay
    dx, dy = qx - px, qy - py
    return np.where(deg, d_deg, dx * dx + dy * dy).astype(F32)


def _eval(t, xf, yf, blur, clip_bary, cull, persp):
    """t (n,9) records, xf (S,) pixel centres of one row at yf -> candidate (n,S) bool, pz, d (unsigned), inside"""
    x0, y0, z0, x1, y1, z1, x2, y2, z2 = (t[:, k:k + 1] for k in range(9))
    pad = np.sqrt(F32(blur)).astype(F32)
    xmin, xmax = np.minimum(x0, np.minimum(x1, x2)) - pad, np.maximum(x0, np.maximum(x1, x2)) + pad
    ymin, ymax = np.minimum(y0, np.minimum(y1, y2)) - pad, np.maximum(y0, np.maximum(y1, y2)) + pad
    xf = xf[None, :]
    ok = ~((xf > xmax) | (xf < xmin) | (yf > ymax) | (yf < ymin))
    ok &= ~(np.maximum(z0, np.maximum(z1, z2)) < K_EPS)
    face_area = _edge(x2, y2, x0, y0, x1, y1)
    ok &= ~((face_area <= K_EPS) & (face_area >= -K_EPS))
    if cull:
        ok &= ~(face_area < 0)
    area = face_area + K_EPS
    with np.errstate(all="ignore"):
        w0 = _edge(xf, yf, x1, y1, x2, y2) / area
        w1 = _edge(xf, yf, x2, y2, x0, y0) / area
        w2 = _edge(xf, yf, x0, y0, x1, y1) / area
        b0, b1, b2 = w0, w1, w2
        if persp:
            t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
            den = np.maximum(t0 + t1 + t2, K_EPS)
            b0, b1, b2 = t0 / den, t1 / den, t2 / den
        c0, c1, c2 = b0, b1, b2
        if clip_bary:
            c0, c1, c2 = (np.minimum(np.maximum(b, F32(0)), F32(1)) for b in (b0, b1, b2))
            s = np.maximum(c0 + c1 + c2, K_EPS)
            c0, c1, c2 = c0 / s, c1 / s, c2 / s
        pz = c0 * z0 + c1 * z1 + c2 * z2
        ok &= ~(pz < 0)
        inside = (b0 > 0) & (b1 > 0) & (b2 > 0)
        d = np.minimum(_pld2(xf, yf, x0, y0, x1, y1), np.minimum(_pld2(xf, yf, x1, y1, x2, y2), _pld2(xf, yf, x2, y2, x0, y0)))
    ok &= inside | ~(d >= F32(blur))
    assert pz.dtype == F32 and d.dtype == F32
    return ok, pz, d, inside


class Candidates:
    """all candidates of one view, sorted by (pixel, pz, slot): pix = y * S + x, slot = 2 * face + sub, pz, sd (signed d)"""

    def __init__(self, S, pix, slot, pz, sd, code):
        self.S, self.pix, self.slot, self.pz, self.sd, self.code = S, pix, slot, pz, sd, code
        self.count = np.bincount(pix, minlength=S * S)                       # candidates per pixel
        start = np.concatenate([[0], np.cumsum(self.count)[:-1]])
        self.rank = np.arange(pix.size) - start[pix]                         # depth rank within the pixel

    def alpha(self, K, sigma=1e-4):
        """(S,S) float64: sigmoid_alpha_blend over the K nearest candidates of every pixel"""
        take = self.rank < K
        prob = 1.0 / (1.0 + np.exp(self.sd[take].astype(np.float64) / sigma))
        keep = np.ones(self.S * self.S)
        np.multiply.at(keep, self.pix[take], 1.0 - prob)
        return (1.0 - keep).reshape(self.S, self.S)

    def fragments(self, K):
        """-> slots (S,S,K) int64 (-1 = empty), pz (S,S,K) f32, sd (S,S,K) f32: the K nearest, in depth order"""
        S = self.S
        slots = np.full((S * S, K), -1, np.int64)
        pz = np.full((S * S, K), -1, F32)
        sd = np.full((S * S, K), -1, F32)
        take = self.rank < K
        slots[self.pix[take], self.rank[take]] = self.slot[take]
        pz[self.pix[take], self.rank[take]] = self.pz[take]
        sd[self.pix[take], self.rank[take]] = self.sd[take]
        return slots.reshape(S, S, K), pz.reshape(S, S, K), sd.reshape(S, S, K)


def candidates(ndc, faces, S, blur, clip_bary=True, cull_backfaces=False, perspective_correct=True, z_clip=0.5):
    tri, code = records(ndc, faces, z_clip, perspective_correct)
    live = np.nonzero(code != 0)[0]
    tl = tri[live]
    pad = np.sqrt(F32(blur)).astype(F32)
    rymin = np.minimum(tl[:, 1], np.minimum(tl[:, 4], tl[:, 7])) - pad
    rymax = np.maximum(tl[:, 1], np.maximum(tl[:, 4], tl[:, 7])) + pad
    xf = _pix_to_ndc(S - 1 - np.arange(S), S)
    yfs = _pix_to_ndc(S - 1 - np.arange(S), S)
    out = [[], [], [], []]
    for yi in range(S):
        yf = yfs[yi]
        row = live[~((yf > rymax) | (yf < rymin))]
        if row.size == 0:
            continue
        # the siblings of clipped halves must be evaluated too, wherever their own bbox lies
        halves = row[(code[row] >= 2) & (code[row] < 8)]
        row = np.union1d(row, halves ^ 1)
        row = row[code[row] != 0]
        ok, pz, d, inside = _eval(tri[row], xf, yf, blur, clip_bary, cull_backfaces, perspective_correct)
        pos = {int(s): i for i, s in enumerate(row)}
        drop = np.zeros_like(ok)
        for s in halves:
            i, j = pos[int(s)], pos.get(int(s) ^ 1)
            if j is None:
                continue
            # the oracle keeps the earlier (even) half unless the later one is strictly nearer in the image plane
            drop[i] = ok[j] & (~(d[i] < d[j]) if s & 1 else (d[j] < d[i]))
        ok &= ~drop
        ri, xi = np.nonzero(ok)
        if ri.size == 0:
            continue
        slot, z = row[ri], pz[ri, xi]
        order = np.lexsort((slot, z, xi))
        out[0].append(yi * S + xi[order])
        out[1].append(slot[order])
        out[2].append(z[order])
        out[3].append(np.where(inside[ri, xi], -d[ri, xi], d[ri, xi])[order])
    if not out[0]:
        z = np.zeros(0, F32)
        return Candidates(S, np.zeros(0, np.int64), np.zeros(0, np.int64), z, z, code)
    return Candidates(S, np.concatenate(out[0]).astype(np.int64), np.concatenate(out[1]).astype(np.int64),
                      np.concatenate(out[2]), np.concatenate(out[3]), code)


# ------------------------------------------------------------------ scenes
def deck(n=20, z0=2.0, dz=0.05):
    """n copies of one view-space triangle at depths z0, z0 + dz, ...: every copy has the SAME projection, so a covered pixel
    has exactly n candidates with the same d.  -> (ndc (3n,3) float32 = (x_ndc, y_ndc, z_view), faces (n,3) int32)"""
    base = np.array([[-0.55, -0.45], [0.6, -0.35], [0.05, 0.62]], F32)
    ndc = np.concatenate([np.concatenate([base, np.full((3, 1), z0 + dz * k, F32)], axis=1) for k in range(n)]).astype(F32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return ndc, faces


OBLIQUE = dict(dist=2.1, elev=[35.0], azim=[65.0], at=(0, 0.10, 0.25))
