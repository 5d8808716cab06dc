"""The vertex-path backward restated in numpy, rounding for rounding: the per-fragment arithmetic of raster_bwd_kernel
(csrc/raster.hip) and raster_k_frag_grad (csrc/soft.hip), the fixed-point scatter of csrc/det.h and project_verts_bwd_kernel.

raster.hip and soft.hip are built without FMA contraction and with correctly rounded division, and the backward uses only
+ - * /, comparisons, fminf and fmaxf, so with dt = np.float32 every value below is the value the kernel computes: numpy
rounds each fp32 operation correctly, and the expressions keep the kernels' order and association (C++ evaluates
a*b + c*d + e*f as ((a*b)+(c*d))+(e*f) and a*b*c as (a*b)*c).  With dt = np.float64 the same text states the definition
(the checker against the C oracle and against autograd).  In both precisions the pixel centre is the fp32 value of
pix_to_ndc, promoted afterwards, and kEps is float32(1e-8), as in oracle/raster_ref.c:ref_raster_bwd.

No torch is needed except for dt = np.float64 through clipped faces, where the cut is taken from oracle/soft_ref.py."""
import ctypes
import math

import numpy as np

F32, F64 = np.float32, np.float64
K_EPS = np.float32(1e-8)
INV_TAN_HALF_FOV = np.float32(1.0 / math.tan(math.radians(60.0) / 2.0))     # st3d.ops.INV_TAN_HALF_FOV as a C float


def pix_to_ndc(i, S):
    """softgeom.h:pix_to_ndc in fp32: -1 + (2 i + 1) / S"""
    i = np.asarray(i).astype(F32)
    return (F32(-1.0) + ((F32(2.0) * i).astype(F32) + F32(1.0)).astype(F32) / F32(S)).astype(F32)


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


# ------------------------------------------------------------------------------------------------ raster_bwd_kernel (K = 1)
def frag_grad_hard(ndc_b, faces, p2f_b, gbary_b, S, dt):
    """One view.  ndc_b (V,3) fp32, faces (F,3), p2f_b (S,S), gbary_b (S,S,3) fp32 ->
    (frag_index (P,) = yi * S + xi, face (P,), c9 (P,9) in dt, live (P,)) for the P covered pixels, c9 in the face's own
    vertex order {d/dx0, d/dy0, d/dz0, d/dx1, ...}.  Fragments with den <= kEps are not live and their c9 is 0."""
    assert dt in (F32, F64)
    ndc_b, p2f_b, gbary_b = np.asarray(ndc_b), np.asarray(p2f_b), np.asarray(gbary_b)
    assert ndc_b.dtype == F32 and gbary_b.dtype == F32 and p2f_b.shape == (S, S)
    faces = np.asarray(faces).astype(np.int64)
    yi, xi = np.nonzero(p2f_b >= 0)
    f = p2f_b[yi, xi].astype(np.int64)
    px, py = pix_to_ndc(S - 1 - xi, S).astype(dt), pix_to_ndc(S - 1 - yi, S).astype(dt)
    v = ndc_b.astype(dt)[faces[f]]                                   # (P, corner, xyz)
    x0, y0, z0 = v[:, 0, 0], v[:, 0, 1], v[:, 0, 2]
    x1, y1, z1 = v[:, 1, 0], v[:, 1, 1], v[:, 1, 2]
    x2, y2, z2 = v[:, 2, 0], v[:, 2, 1], v[:, 2, 2]
    g = gbary_b[yi, xi].astype(dt)
    g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
    eps = dt(K_EPS)
    with np.errstate(all="ignore"):
        A = _edge(x2, y2, x0, y0, x1, y1) + eps
        w0 = _edge(px, py, x1, y1, x2, y2) / A
        w1 = _edge(px, py, x2, y2, x0, y0) / A
        w2 = _edge(px, py, x0, y0, x1, y1) / A
        t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
        den = t0 + t1 + t2
        live = den > eps
        b0, b1, b2 = t0 / den, t1 / den, t2 / den
        gs = g0 * b0 + g1 * b1 + g2 * b2
        dt0, dt1, dt2 = (g0 - gs) / den, (g1 - gs) / den, (g2 - gs) / den
        dw0, dw1, dw2 = dt0 * z1 * z2, dt1 * z0 * z2, dt2 * z0 * z1
        dz0 = dt1 * w1 * z2 + dt2 * z1 * w2
        dz1 = dt0 * w0 * z2 + dt2 * z0 * w2
        dz2 = dt0 * w0 * z1 + dt1 * z0 * w1
        de0, de1, de2 = dw0 / A, dw1 / A, dw2 / A
        dA = -(dw0 * w0 + dw1 * w1 + dw2 * w2) / A
        c9 = np.stack([
            de1 * -(py - y2) + de2 * (py - y1) + dA * (y2 - y1),
            de1 * (px - x2) + de2 * (x1 - px) + dA * (x1 - x2),
            dz0,
            de0 * (py - y2) + de2 * -(py - y0) + dA * -(y2 - y0),
            de0 * (x2 - px) + de2 * (px - x0) + dA * (x2 - x0),
            dz1,
            de0 * -(py - y1) + de1 * (py - y0) + dA * (y1 - y0),
            de0 * (px - x1) + de1 * (x0 - px) + dA * -(x1 - x0),
            dz2], axis=1)
    c9[~live] = 0
    assert c9.dtype == dt, c9.dtype
    return yi * S + xi, f, c9, live


# ------------------------------------------------------------------------------------------ raster_k_frag_grad (general path)
def _clip_face_f32(ov, z_clip, persp):
    """oracle/raster_ref.c:ref_clip_face (pinned bit-equal to clip_face_dev by the forward clipping test)
    -> (tri (2,9) fp32, code (2,), (w2, w3) fp32)"""
    from oracle import render_ref as rr
    v = (ctypes.c_float * 9)(*[float(x) for x in ov])
    tri = ((ctypes.c_float * 9) * 2)()
    code = (ctypes.c_int * 2)()
    w = (ctypes.c_float * 2)()
    fn = rr.lib().ref_clip_face
    fn.restype = None
    fn(v, ctypes.c_float(float(z_clip)), ctypes.c_int(1 if persp else 0), tri, code, w)
    return np.array([list(tri[0]), list(tri[1])], F32), (int(code[0]), int(code[1])), (F32(w[0]), F32(w[1]))


def _clip_face_f64(ov, code, z_clip, persp):
    """the same cut in fp64 (oracle/soft_ref.py:clip_face on the fp32 vertices): -> (tri (n,9) fp64, (w2, w3) fp64); the
    codes -- which vertices are behind the plane -- are comparisons of fp32 inputs and stay those of ref_clip_face"""
    import torch
    from oracle import soft_ref as SR
    subs = SR.clip_face(torch.tensor(np.asarray(ov, F64).reshape(3, 3)), float(z_clip), bool(persp))
    tri = np.stack([t.numpy().reshape(9) for t, _ in subs])
    if code[0] <= 1:
        return tri, (F64(0), F64(0))
    i1, kind = (code[0] - 2) % 3, (code[0] - 2) // 3
    M = subs[0][1].numpy()                       # kind 0: rows (b4, b2, b5); kind 2: rows (b1, b4, b5)
    w2 = M[0 if kind == 0 else 1][(i1 + 1) % 3]
    w3 = M[2][(i1 + 2) % 3]
    return tri, (F64(w2), F64(w3))


def _pld2(px, py, ax, ay, bx, by, eps):
    bax, bay = bx - ax, by - ay
    l2 = bax * bax + bay * bay
    if l2 <= eps:
        dx, dy = px - bx, py - by
        return dx * dx + dy * dy
    t = (bax * (px - ax) + bay * (py - ay)) / l2
    t = type(t)(0) if t < 0 else (type(t)(1) if t > 1 else t)
    qx, qy = ax + t * bax, ay + t * bay
    dx, dy = qx - px, qy - py
    return dx * dx + dy * dy


def _frag_soft_one(px, py, ov, tri, ccode, cw2, cw3, go, gzk, gdv, clip, persp, zc, dt):
    """raster_k_frag_grad for one fragment, line by line.  px, py, ov (9), tri (9), cw2, cw3, go (3), gzk, zc: dt scalars;
    gdv: dt scalar or None (no distance gradient) -> c9 (list of 9 dt scalars)"""
    Z, ONE, TWO, eps = dt(0), dt(1), dt(2), dt(K_EPS)
    x0, y0, z0, x1, y1, z1, x2, y2, z2 = tri
    A = _edge(x2, y2, x0, y0, x1, y1) + eps
    w0 = _edge(px, py, x1, y1, x2, y2) / A
    w1 = _edge(px, py, x2, y2, x0, y0) / A
    w2 = _edge(px, py, x0, y0, x1, y1) / A
    t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
    den = t0 + t1 + t2
    gx0 = gy0 = gx1 = gy1 = gx2 = gy2 = dz0 = dz1 = dz2 = Z
    if persp:
        dm = max(den, eps)
        b0, b1, b2 = t0 / dm, t1 / dm, t2 / dm
    else:
        b0, b1, b2 = w0, w1, w2
    # ---- clipped barycentrics + depth
    c0, c1, c2, s = b0, b1, b2, ONE
    if clip:
        c0, c1, c2 = min(max(b0, Z), ONE), min(max(b1, Z), ONE), min(max(b2, Z), ONE)
        s = max(c0 + c1 + c2, eps)
        c0, c1, c2 = c0 / s, c1 / s, c2 / s
    gq0, gq1, gq2 = go
    k1, k2, k3, kind = 0, 1, 2, -1
    if ccode > 1:                                    # bary_orig = c . M  =>  d c = M . g
        k1, kind = (ccode - 2) % 3, (ccode - 2) // 3
        k2, k3 = (k1 + 1) % 3, (k1 + 2) % 3
        g1, g2, g3 = go[k1], go[k2], go[k3]
        g4 = (ONE - cw2) * g1 + cw2 * g2
        g5 = (ONE - cw3) * g1 + cw3 * g3
        if kind == 0:
            gq0, gq1, gq2 = g4, g2, g5
        elif kind == 1:
            gq0, gq1, gq2 = g5, g2, g3
        else:
            gq0, gq1, gq2 = g1, g4, g5
    dc0 = gq0 + gzk * z0
    dc1 = gq1 + gzk * z1
    dc2 = gq2 + gzk * z2
    dz0, dz1, dz2 = dz0 + gzk * c0, dz1 + gzk * c1, dz2 + gzk * c2
    db0, db1, db2 = dc0, dc1, dc2
    if clip:
        dot = dc0 * c0 + dc1 * c1 + dc2 * c2
        live = (min(max(b0, Z), ONE) + min(max(b1, Z), ONE) + min(max(b2, Z), ONE)) > eps
        e0 = (dc0 - dot) / s if live else Z
        e1 = (dc1 - dot) / s if live else Z
        e2 = (dc2 - dot) / s if live else Z
        db0 = e0 if (b0 > Z and b0 < ONE) else Z
        db1 = e1 if (b1 > Z and b1 < ONE) else Z
        db2 = e2 if (b2 > Z and b2 < ONE) else Z
    if (not persp) or den > eps:
        dw0, dw1, dw2 = db0, db1, db2                # perspective_correct = False: b = w
        if persp:
            gs = db0 * b0 + db1 * b1 + db2 * b2
            dt0, dt1, dt2 = (db0 - gs) / den, (db1 - gs) / den, (db2 - gs) / den
            dw0, dw1, dw2 = dt0 * z1 * z2, dt1 * z0 * z2, dt2 * z0 * z1
            dz0 = dz0 + (dt1 * w1 * z2 + dt2 * z1 * w2)
            dz1 = dz1 + (dt0 * w0 * z2 + dt2 * z0 * w2)
            dz2 = dz2 + (dt0 * w0 * z1 + dt1 * z0 * w1)
        de0, de1, de2 = dw0 / A, dw1 / A, dw2 / A
        dA = -(dw0 * w0 + dw1 * w1 + dw2 * w2) / A
        gx0 = gx0 + (de1 * -(py - y2) + de2 * (py - y1) + dA * (y2 - y1))
        gy0 = gy0 + (de1 * (px - x2) + de2 * (x1 - px) + dA * (x1 - x2))
        gx1 = gx1 + (de0 * (py - y2) + de2 * -(py - y0) + dA * -(y2 - y0))
        gy1 = gy1 + (de0 * (x2 - px) + de2 * (px - x0) + dA * (x2 - x0))
        gx2 = gx2 + (de0 * -(py - y1) + de1 * (py - y0) + dA * (y1 - y0))
        gy2 = gy2 + (de0 * (px - x1) + de1 * (x0 - px) + dA * -(x1 - x0))
    # ---- signed squared distance to the nearest edge (first minimum), projection parameter constant
    if gdv is not None:
        inside = (b0 > Z) and (b1 > Z) and (b2 > Z)
        gdd = -gdv if inside else gdv
        d01, d12, d20 = (_pld2(px, py, x0, y0, x1, y1, eps), _pld2(px, py, x1, y1, x2, y2, eps),
                         _pld2(px, py, x2, y2, x0, y0, eps))
        e, dmin = 0, d01
        if d12 < dmin:
            dmin, e = d12, 1
        if d20 < dmin:
            dmin, e = d20, 2
        ax, ay = (x0, y0) if e == 0 else ((x1, y1) if e == 1 else (x2, y2))
        bx, by = (x1, y1) if e == 0 else ((x2, y2) if e == 1 else (x0, y0))
        bax, bay = bx - ax, by - ay
        l2 = bax * bax + bay * bay
        if l2 <= eps:
            gax, gay, gbx, gby = Z, Z, gdd * TWO * (bx - px), gdd * TWO * (by - py)
        else:
            t = (bax * (px - ax) + bay * (py - ay)) / l2
            t = Z if t < Z else (ONE if t > ONE else t)
            qx, qy = ax + t * bax - px, ay + t * bay - py
            gax, gay = gdd * (ONE - t) * TWO * qx, gdd * (ONE - t) * TWO * qy
            gbx, gby = gdd * t * TWO * qx, gdd * t * TWO * qy
        if e == 0:
            gx0, gy0, gx1, gy1 = gx0 + gax, gy0 + gay, gx1 + gbx, gy1 + gby
        elif e == 1:
            gx1, gy1, gx2, gy2 = gx1 + gax, gy1 + gay, gx2 + gbx, gy2 + gby
        else:
            gx2, gy2, gx0, gy0 = gx2 + gax, gy2 + gay, gx0 + gbx, gy0 + gby
    if ccode > 1:
        # sub-triangle vertices q0 q1 q2 -> the face's p1 p2 p3 (indices k1 k2 k3 in the face) through the cut points
        gq = ((gx0, gy0, dz0), (gx1, gy1, dz1), (gx2, gy2, dz2))
        gp = [[Z, Z, Z], [Z, Z, Z], [Z, Z, Z]]                     # [p1, p2, p3][x, y, z]
        P = tuple(tuple(ov[3 * k + a] for a in range(3)) for k in (k1, k2, k3))
        dw2 = dw3 = Z
        who = (4 if kind == 0 else (5 if kind == 1 else 0), 4 if kind == 2 else 1, 2 if kind == 1 else 5)
        cq = (c0, c1, c2) if clip else (b0, b1, b2)
        for q in range(3):
            wq = who[q]
            if wq < 3:
                for c in range(3):
                    gp[wq][c] = gp[wq][c] + gq[q][c]
                continue
            o = 1 if wq == 4 else 2                                 # the edge's far end: p2 for p4, p3 for p5
            w = cw2 if wq == 4 else cw3
            dw = Z
            for a in range(2):                                      # x, y
                g = gq[q][a]
                if persp:
                    gp[0][a] = gp[0][a] + g * (ONE - w) * P[0][2] / zc
                    gp[0][2] = gp[0][2] + g * (ONE - w) * P[0][a] / zc
                    gp[o][a] = gp[o][a] + g * w * P[o][2] / zc
                    gp[o][2] = gp[o][2] + g * w * P[o][a] / zc
                    dw = dw + g * (P[o][a] * P[o][2] - P[0][a] * P[0][2]) / zc
                else:
                    gp[0][a] = gp[0][a] + g * (ONE - w)
                    gp[o][a] = gp[o][a] + g * w
                    dw = dw + g * (P[o][a] - P[0][a])
            dw = dw + cq[q] * (go[k2 if wq == 4 else k3] - go[k1])  # M's row for this vertex: (1 - w) e_p1 + w e_far
            if wq == 4:
                dw2 = dw2 + dw
            else:
                dw3 = dw3 + dw
        d12, d13 = P[0][2] - P[1][2], P[0][2] - P[2][2]
        gp[0][2] = gp[0][2] + (dw2 * (zc - P[1][2]) / (d12 * d12) + dw3 * (zc - P[2][2]) / (d13 * d13))
        gp[1][2] = gp[1][2] + dw2 * (P[0][2] - zc) / (d12 * d12)
        gp[2][2] = gp[2][2] + dw3 * (P[0][2] - zc) / (d13 * d13)
        c9 = [Z] * 9
        for r, k in enumerate((k1, k2, k3)):                        # gp[r] belongs to the face's vertex number k
            for c in range(3):
                c9[3 * k + c] = gp[r][c]
        return c9
    return [gx0, gy0, dz0, gx1, gy1, dz1, gx2, gy2, dz2]


def frag_grad_soft(ndc_b, faces, p2f_b, gbary_b, gzb_b, gdist_b, S, dt, clip, persp=True, slots_b=None, z_clip=None):
    """One view of the general path.  ndc_b (V,3) fp32, p2f_b (S,S,K), gbary_b (S,S,K,3) / gzb_b / gdist_b (S,S,K) fp32 or
    None (that gradient absent, as a null pointer of the kernel), slots_b (S,S,K) record slots of a clipped rasterisation or
    None -> (frag_index (P,) = (yi * S + xi) * K + k, face (P,), c9 (P,9) in dt, live (P,) all True)."""
    assert dt in (F32, F64)
    ndc_b, p2f_b = np.asarray(ndc_b), np.asarray(p2f_b)
    assert ndc_b.dtype == F32 and p2f_b.shape[:2] == (S, S)
    for g in (gbary_b, gzb_b, gdist_b):
        assert g is None or np.asarray(g).dtype == F32
    K = p2f_b.shape[2]
    faces = np.asarray(faces).astype(np.int64)
    yi, xi, ki = np.nonzero(p2f_b >= 0)
    f = p2f_b[yi, xi, ki].astype(np.int64)
    pxs, pys = pix_to_ndc(S - 1 - xi, S).astype(dt), pix_to_ndc(S - 1 - yi, S).astype(dt)
    vd = ndc_b.astype(dt)
    zc = dt(F32(z_clip)) if z_clip is not None else dt(0)
    c9 = np.zeros((f.size, 9), dt)
    cache = {}
    with np.errstate(all="ignore"):
        for n in range(f.size):
            y, x, k, fn = int(yi[n]), int(xi[n]), int(ki[n]), int(f[n])
            ov = tuple(vd[faces[fn]].reshape(9))
            tri, ccode, cw2, cw3 = ov, 1, dt(0), dt(0)
            if slots_b is not None:
                if fn not in cache:
                    tris, code, ws = _clip_face_f32(ndc_b[faces[fn]].reshape(9), z_clip, persp)
                    if dt is F64:
                        tris, ws = _clip_face_f64(ov, code, z_clip, persp)
                    cache[fn] = (tris, code, ws)
                tris, code, (cw2, cw3) = cache[fn]
                sub = int(slots_b[y, x, k]) & 1
                ccode, tri = code[sub], tuple(tris[sub])
            go = tuple(dt(v) for v in gbary_b[y, x, k]) if gbary_b is not None else (dt(0), dt(0), dt(0))
            gzk = dt(gzb_b[y, x, k]) if gzb_b is not None else dt(0)
            gdv = dt(gdist_b[y, x, k]) if gdist_b is not None else None
            row = _frag_soft_one(pxs[n], pys[n], ov, tri, ccode, cw2, cw3, go, gzk, gdv, clip, persp, zc, dt)
            assert all(type(v) is dt for v in row), [type(v) for v in row]          # no silent promotion on the way
            c9[n] = row
    assert c9.dtype == dt
    return (yi * S + xi) * K + ki, f, c9, np.ones(f.size, bool)


# ---------------------------------------------------------------------------------------------------------------- det.h
class BoundNearPowerOfTwo(ValueError):
    """the bound's mantissa is so close to a power of two that the kernel's fp32 partial sums may land in the other binade"""


MANTISSA_LO, MANTISSA_HI = 0.5 * (1.0 + 2.0 ** -12), 1.0 - 2.0 ** -12


def det_scatter(index, values_f32, n_out, bound=None):
    """The fixed-point scatter-add of csrc/det.h, exactly: bound = sum |values| over ALL values of the call (or `bound`, for
    the entry points that take theirs from the upstream gradient: the texture scatters, tests/_texpath_ref.py), scale
    2^(60 - e) with bound = m 2^e, 0.5 <= m < 1; every value quantised with round-to-nearest-even (__double2ll_rn), summed as
    int64 (any order: integer addition), converted back through fp64 to fp32 (nearest even, as the C casts).

    The kernel forms its bound from fp32 block sums, so only the bound's binary exponent is shared with this fp64 sum.  The
    kernel's bound is within 100 * 2^-24 relative of the exact one (at most 72 terms per thread, an 8-level tree, fp64
    after that), so a bound whose mantissa lies outside [0.5 (1 + 2^-12), 1 - 2^-12] is refused (BoundNearPowerOfTwo): the
    caller rescales its upstream gradient and tries again.  This is a condition on the input, not a tolerance."""
    index = np.asarray(index).astype(np.int64).reshape(-1)
    v = np.asarray(values_f32)
    assert v.dtype == F32, v.dtype
    v = v.reshape(-1).astype(F64)
    assert index.shape == v.shape
    own = float(np.abs(v).sum(dtype=F64))
    bound = own if bound is None else float(bound)
    assert np.isfinite(bound) and bound >= 0.0
    k = 0
    if bound > 0.0:
        m, e = np.frexp(bound)
        if not (MANTISSA_LO <= m <= MANTISSA_HI):
            raise BoundNearPowerOfTwo(f"bound {bound!r} = {m!r} * 2^{e}")
        k = 60 - int(e)
    assert np.abs(np.ldexp(v, k)).sum() < 2.0 ** 63              # a bound given from outside covers every partial sum
    q = np.rint(np.ldexp(v, k)).astype(np.int64)
    acc = np.zeros(n_out, np.int64)
    np.add.at(acc, index, q)
    return np.ldexp(acc.astype(F64), -k).astype(F32)


def exact_sums(index, values, n_out):
    """per element of the output: the exact sum of its terms (rounded once to fp64, math.fsum), the exact sum of their
    magnitudes and the number of nonzero terms"""
    flat, val = np.asarray(index).ravel(), np.asarray(values).ravel().astype(F64)
    order = np.argsort(flat, kind="stable")
    flat, val = flat[order], val[order]
    total, mag, cnt = np.zeros(n_out, F64), np.zeros(n_out, F64), np.zeros(n_out, np.int64)
    if flat.size == 0:
        return total, mag, cnt
    starts = np.nonzero(np.r_[True, flat[1:] != flat[:-1]])[0]
    for a, b in zip(starts, np.r_[starts[1:], flat.size]):
        total[flat[a]] = math.fsum(val[a:b])
        mag[flat[a]] = math.fsum(np.abs(val[a:b]))
        cnt[flat[a]] = np.count_nonzero(val[a:b])
    return total, mag, cnt


def assert_within_summation_bound(got, index, values, what, where):
    """Float atomics: per element |got - sum| <= n 2^-24 sum|c|, n the number of nonzero terms of the element, sum and sum|c|
    the exact sums of the restated fp32 terms -- the textbook bound of an fp32 summation in any order; elements without a
    term are exactly 0.  `where(j)` describes element j for the failure message.  -> the largest error / bound ratio."""
    got = np.asarray(got).reshape(-1)
    total, mag, cnt = exact_sums(index, values, got.size)
    assert cnt.max() * (cnt.max() - 1) * 2.0 ** -24 <= 1.0              # where n u sum|c| covers (n-1) u / (1 - (n-1) u)
    zero = cnt == 0
    assert (got[zero] == 0).all(), f"{what}: an element without a contribution is not 0"
    err, bound = np.abs(got.astype(F64) - total), cnt * 2.0 ** -24 * mag
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f"{what}: float atomics, largest error / bound over {int((~zero).sum())} elements: {ratio:.3f} (most terms: {cnt.max()})")
    bad = np.nonzero(err > bound)[0]
    if bad.size:
        j = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} elements beyond n 2^-24 sum|c|; first: got {got[j]!r}, sum {total[j]!r}, "
                             f"bound {bound[j]:.3e}; {where(j)}")
    return ratio


def scatter_index(b, face, faces, V):
    """flat (b, vertex, component) index of the nine contributions of fragments of view b on faces `face` -> (P,9)"""
    faces = np.asarray(faces).astype(np.int64)
    vtx = faces[np.asarray(face)]                                   # (P,3)
    return (b * V * 3 + 3 * vtx[:, :, None] + np.arange(3)[None, None, :]).reshape(-1, 9)


# ------------------------------------------------------------------------------------------------ project_verts_bwd_kernel
def project_verts_bwd_f32(verts, R, T, s, gndc, out=None):
    """verts (V,3), R (B,3,3), T (B,3), s, gndc (B,V,3), all fp32 -> (V,3) fp32 in the kernel's order: per view
    dxv = (s g0) / zv, dzv = g2 - (s ((g0 xv) + (g1 yv))) / (zv zv), ax += ((dxv r0) + (dyv r1)) + (dzv r2); `out` is added last."""
    verts, R, T, gndc = np.asarray(verts), np.asarray(R), np.asarray(T), np.asarray(gndc)
    for a in (verts, R, T, gndc):
        assert a.dtype == F32
    s = F32(s)
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    acc = [np.zeros(verts.shape[0], F32) for _ in range(3)]
    with np.errstate(all="ignore"):
        for b in range(R.shape[0]):
            r, t = R[b].reshape(9), T[b]
            xv = x * r[0] + y * r[3] + z * r[6] + t[0]
            yv = x * r[1] + y * r[4] + z * r[7] + t[1]
            zv = x * r[2] + y * r[5] + z * r[8] + t[2]
            g0, g1, g2 = gndc[b, :, 0], gndc[b, :, 1], gndc[b, :, 2]
            dxv, dyv = s * g0 / zv, s * g1 / zv
            dzv = g2 - s * (g0 * xv + g1 * yv) / (zv * zv)
            for j in range(3):
                acc[j] = acc[j] + (dxv * r[3 * j] + dyv * r[3 * j + 1] + dzv * r[3 * j + 2])
        res = np.stack(acc, axis=1)
        if out is not None:
            out = np.asarray(out)
            assert out.dtype == F32
            res = res + out
    assert res.dtype == F32
    return res


# ------------------------------------------------------------------------------------------ whole calls: all views at once
def restate_hard(ndc, faces, p2f, gbary, dt=F32):
    """ops.raster_bwd's contributions: ndc (B,V,3), p2f (B,S,S), gbary (B,S,S,3) ->
    (index (P,9) flat into (B,V,3), c9 (P,9), where (P,3) = (view, frag_index, face)) over the live fragments of all views"""
    B, V = ndc.shape[0], ndc.shape[1]
    S = p2f.shape[1]
    idx, val, where = [], [], []
    for b in range(B):
        fi, f, c9, live = frag_grad_hard(ndc[b], faces, p2f[b], gbary[b], S, dt)
        idx.append(scatter_index(b, f[live], faces, V))
        val.append(c9[live])
        where.append(np.stack([np.full(live.sum(), b), fi[live], f[live]], 1))
    return np.concatenate(idx), np.concatenate(val), np.concatenate(where)


def restate_soft(ndc, faces, p2f, grads, clip, persp=True, slots=None, z_clip=None, dt=F32):
    """ops.raster_soft_bwd's contributions: p2f (B,S,S,K), grads = (gbary, gzb, gdist), each (B,...) or None -> as restate_hard"""
    B, V = ndc.shape[0], ndc.shape[1]
    S = p2f.shape[1]
    idx, val, where = [], [], []
    for b in range(B):
        gb, gz, gd = (None if g is None else g[b] for g in grads)
        fi, f, c9, _ = frag_grad_soft(ndc[b], faces, p2f[b], gb, gz, gd, S, dt, clip, persp,
                                      None if slots is None else slots[b], z_clip)
        idx.append(scatter_index(b, f, faces, V))
        val.append(c9)
        where.append(np.stack([np.full(f.size, b), fi, f], 1))
    return np.concatenate(idx), np.concatenate(val), np.concatenate(where)


def vertex_groups(where, faces):
    """Greedy partition of the fragments `where` (P,3) = (view, frag_index, face) into groups in which no two fragments
    share a (view, vertex): -> list of index arrays into `where`, every fragment in exactly one group"""
    faces = np.asarray(faces)
    used, groups = [], []
    for n, (b, _, f) in enumerate(where):
        key = {(int(b), int(v)) for v in faces[f]}
        for u, g in zip(used, groups):
            if not (u & key):
                u |= key
                g.append(n)
                break
        else:
            used.append(set(key))
            groups.append([n])
    return [np.array(g) for g in groups]


# ----------------------------------------------------------------------------------------------------- the shared scenes
HARD_CASES = [("cow", 17), ("cow", 32), ("cow", 48), ("quad", 16), ("quad", 48), ("sub", 24)]

# name -> (scene, S, K, blur, clip, persp, z_clip)
SOFT_CASES = {
    "k1": ("cow", 32, 1, 0.0, False, True, None),
    "k4-clip": ("cow", 32, 4, 3e-4, True, True, None),
    "k3-clip": ("cow", 32, 3, 1e-3, True, True, None),
    "k2-nonpersp": ("cow", 32, 2, 0.0, False, False, None),
    "overflow": ("sub1", 16, 8, 1e-3, True, True, None),
}
NEAR_SETTINGS = ((True, 1, 0.0), (False, 1, 0.0), (True, 2, 3e-3))          # (persp, K, blur)
NEAR_SCENES = ("one behind", "two behind", "cow from inside")
NEAR_S, Z_CLIP = 40, 0.5
for _scene in NEAR_SCENES:
    for _persp, _K, _blur in NEAR_SETTINGS:
        SOFT_CASES[f"{_scene}/{'p' if _persp else 'n'}{_K}"] = (_scene, NEAR_S, _K, _blur, _blur > 0, _persp, Z_CLIP)


def scene(name):
    """-> (verts (V,3) or None, faces (F,3) int32, R, T, ndc (B,V,3) or None): the near scenes are given in projected
    coordinates (ndc), every other one by vertices and cameras"""
    import _scenes
    import _vcolref as VC
    from oracle import render_ref as rr
    if name == "quad":
        verts, faces, R, T = VC.two_triangles()
        return verts, faces, R, T, None
    if name in ("cow", "sub", "sub1"):
        verts, faces = (VC.cow()["verts"], VC.cow()["faces"]) if name == "cow" else VC.cow_subdivided(2)
        R, T = _scenes.random_cameras(2, 11)
        if name == "sub1":                       # one view: the one whose single 16 x 16 tile sees the most faces
            R, T = R[1:], T[1:]
        return np.asarray(verts, F32), np.asarray(faces, np.int32), R, T, None
    if name == "cow from inside":
        R, T = rr.look_at_view_transform(0.75, [10.0], [35.0], at=(0, 0.10, 0.25))
        return None, np.asarray(VC.cow()["faces"], np.int32), None, None, rr.project_verts(VC.cow()["verts"], R[0], T[0])[None]
    from test_oracle_soft import _straddling_scene
    ndc, faces = _straddling_scene({"one behind": 1, "two behind": 2}[name])
    return None, faces, None, None, ndc[None]


def upstream(shape, seed):
    return np.random.default_rng(4100 + seed).standard_normal(shape).astype(F32)
