"""The texture-path backward restated in numpy, rounding for rounding: the per-fragment arithmetic of the K = 1 shading
kernels that share csrc/shadek1.h and csrc/tilebins.h -- shade_bwd_kernel (plain and supersampled, csrc/shade.hip),
shade_mip_bwd_kernel (csrc/mipmap.hip), shade_vc_bwd_kernel (csrc/vcolor.hip), shade_atlas_bwd_kernel (csrc/atlas.hip) --
and the bound every entry point hands to the fixed-point scatter of csrc/det.h (_vertexpath_ref.det_scatter, bound=).

These files are built without FMA contraction and with correctly rounded division, and apart from the blend factor the
backward has only + - * /, comparisons and floorf, so with dt = np.float32 every value below is the value the kernel
computes: numpy rounds each fp32 operation correctly and the expressions keep the kernels' order and association (C++
evaluates a*b + c*d + e*f as ((a*b)+(c*d))+(e*f); `gix += x` three times from 0.f is ((0+x0)+x1)+x2).  With dt = np.float64
the same text states the definition (the checker against tests/_mipref.py, _vcolref.py, _atlasref.py and the C oracle).
The footprints, the UV position and the level split are _mipref's (foot0, footl, _corner, _uv, _split): they are these
expressions already.

The blend factor k = wnum / denom of blend_k1 is the one place with expf, and the device's expf is not numpy's, so k is an
INPUT here: (B,S,S) in dt.  The GPU tests read the kernel's own k back bit for bit (tests/test_gpu_texpath_exact.py:
probe_k), the CPU tests take it from _mipref._blend (blend_k below).

Every restate_* returns a dict over the P covered fragments of all views, in (view, pixel) order:
    idx, c, valid  (P, D*3): the flat output element, the deposited value in dt and whether the deposit exists; column
                   3 * d + channel, d the deposit (footprint corner, face corner, ...), D = 4 texels, 8 mip (lower level,
                   then upper), 3 vertex colours, 1 atlas
    where          (P, 3) = (view, pixel index y * side + x at the fragments' side, face)
    guv (P,2), gbary (P,3): the per-pixel outputs the kernel writes directly (those it has)
    n_out          the number of elements of the scattered output
    bound          the entry point's fixed-point bound, restated from its source (exact in fp64)
No torch is needed."""
import numpy as np

import _atlasref as AT
import _mipref as M

F32, F64 = np.float32, np.float64


def _same(dt, *arrays):
    """the guard against silent promotion: every intermediate handed in is an array of dt"""
    for a in arrays:
        assert isinstance(a, np.ndarray) and a.dtype == dt, (dt, getattr(a, "dtype", type(a)))


def blend_k(frag, dt):
    """k = wnum / denom of blend_k1 with numpy's (correctly rounded) exp: (B,S,S) in dt; what the CPU tests use for k"""
    _, zbuf, _, dists = frag
    with np.errstate(all="ignore"):
        _, wnum, _, denom = M._blend(np.asarray(dists, F32), np.asarray(zbuf, F32), dt)
        k = (wnum / denom).astype(dt)
    return k


def _views(frag):
    p2f, zbuf, bary, dists = (np.asarray(a) for a in frag)
    assert p2f.ndim == 3 and p2f.shape[1] == p2f.shape[2] and bary.dtype == F32
    return [(p2f[b], zbuf[b], bary[b], dists[b]) for b in range(p2f.shape[0])]


def _upstream(grad_rgb, b, cov, a, dt):
    """the three upstream values of the covered (sub-)pixels of view b: g, or g / (float)(a*a) of the pixel's a x a block"""
    g = np.asarray(grad_rgb)
    assert g.dtype == F32
    yi, xi = np.nonzero(cov)
    gs = g[b][:, yi // a, xi // a].T.astype(dt)                       # (n,3)
    if a != 1:
        gs = gs / dt(a * a)
    _same(dt, gs)
    return np.ascontiguousarray(gs)


def _level(flat, q, off, l, g, dt):
    """level_bwd of mipmap.hip (the plain kernel's body at l = 0): the deposits g_c * (wx * wy) of one level, (n,4,3) index /
    value / valid, and the level's d/d(ix_0, iy_0): gx = ((0 + g_0 dx_0) + g_1 dx_1) + g_2 dx_2 with
    dx_c = (t01 - t00) * wy0 + (t11 - t10) * wy1, a tap that does not exist read as 0; l > 0: * 2^-l, 0 where the level's
    own clamp acted"""
    n = g.shape[0]
    idx, c, ok = np.zeros((n, 4, 3), np.int64), np.zeros((n, 4, 3), dt), np.zeros((n, 4, 3), bool)
    taps = []
    for kk in range(4):
        valid, texel, w = M._corner(q, off, kk, dt)
        _same(dt, w)
        idx[:, kk] = texel[:, None] * 3 + np.arange(3)[None]
        c[:, kk] = g * w[:, None]
        ok[:, kk] = valid[:, None]
        taps.append(np.where(valid[:, None], flat[idx[:, kk]], dt(0)))
    t00, t01, t10, t11 = taps
    wx0, wx1, wy0, wy1 = (q[name][:, None] for name in ("wx0", "wx1", "wy0", "wy1"))
    dx = (t01 - t00) * wy0 + (t11 - t10) * wy1
    dy = (t10 - t00) * wx0 + (t11 - t01) * wx1
    gx, gy = np.zeros(n, dt), np.zeros(n, dt)
    for ch in range(3):
        gx = gx + g[:, ch] * dx[:, ch]
        gy = gy + g[:, ch] * dy[:, ch]
    _same(dt, t00, t01, t10, t11, dx, dy, gx, gy)
    l = np.broadcast_to(np.asarray(l, np.int64), (n,))
    inv = (dt(1) / np.left_shift(1, l).astype(dt)).astype(dt)
    gx = np.where(l > 0, np.where(q["cx"], dt(0), gx * inv), gx)
    gy = np.where(l > 0, np.where(q["cy"], dt(0), gy * inv), gy)
    _same(dt, c, gx, gy)
    return idx, c, ok, gx, gy


def _uv_tail(q0, gix, giy, T, fr, verts_uvs, faces_uvs, dt):
    """gu = cx ? 0 : gix * (float)(T - 1); gbary_j = gu * u_j + gv * v_j"""
    gu = np.where(q0["cx"], dt(0), gix * dt(T - 1))
    gv = np.where(q0["cy"], dt(0), giy * dt(T - 1))
    p2f = fr[0]
    t = np.asarray(verts_uvs, F32).astype(dt)[np.asarray(faces_uvs)[p2f[p2f >= 0]]]           # (n,3,2)
    gbary = gu[:, None] * t[:, :, 0] + gv[:, None] * t[:, :, 1]
    guv = np.stack([gu, gv], 1)
    _same(dt, guv, gbary)
    return guv, gbary


def _where(b, fr):
    p2f = fr[0]
    side = p2f.shape[0]
    yi, xi = np.nonzero(p2f >= 0)
    return np.stack([np.full(yi.size, b, np.int64), yi * side + xi, p2f[yi, xi].astype(np.int64)], 1)


def _collect(parts, n_out, bound):
    out = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    out["n_out"], out["bound"] = int(n_out), float(bound)
    return out


def _k_of(k, b, cov, dt):
    k = np.asarray(k)
    assert k.dtype == dt, (k.dtype, dt)
    return k[b][cov]


def _abs_sum(g, weight=None):
    """sum |g| (* weight per pixel) in fp64: weight (B,S,S) against g (B,3,S,S)"""
    a = np.abs(np.asarray(g).astype(F64))
    return float((a if weight is None else a * np.asarray(weight, F64)[:, None]).sum(dtype=F64))


# ------------------------------------------------------------------------------------ shade_bwd_kernel (plain and supersampled)
def restate_shade(grad_rgb, frag, verts_uvs, faces_uvs, tex, k, dt=F32, a=1):
    """ops.shade_bwd (a = 1) / ops.shade_ss_bwd: grad_rgb (B,3,S,S) fp32, frag at side a*S, tex (T,T,3), k (B,aS,aS) in dt.
    Bound (st3d_shade_ss_bwd_det): sum |grad_rgb| over all B*3*S^2 values at a = 1 (det_abs_sum_kernel), over the pixels
    one of whose a x a sub-pixels holds a face at a > 1 (ss_abs_sum_kernel)."""
    assert dt in (F32, F64)
    tex = np.asarray(tex)
    assert tex.dtype == F32
    T = tex.shape[0]
    flat = tex.astype(dt).reshape(-1)
    parts = []
    for b, fr in enumerate(_views(frag)):
        cov, u, v = M._uv(fr, verts_uvs, faces_uvs, dt)
        q0 = M.foot0(u, v, T, dt)
        gk = _upstream(grad_rgb, b, cov, a, dt) * _k_of(k, b, cov, dt)[:, None]
        _same(dt, u, v, gk)
        idx, c, ok, gix, giy = _level(flat, q0, 0, 0, gk, dt)
        guv, gbary = _uv_tail(q0, gix, giy, T, fr, verts_uvs, faces_uvs, dt)
        n = gk.shape[0]
        parts.append(dict(idx=idx.reshape(n, 12), c=c.reshape(n, 12), valid=ok.reshape(n, 12), where=_where(b, fr), guv=guv,
                          gbary=gbary, cx=q0["cx"], cy=q0["cy"], vx1=q0["vx1"], vy1=q0["vy1"], ix=q0["ix"], iy=q0["iy"]))
    p2f = np.asarray(frag[0])
    if a == 1:
        bound = _abs_sum(grad_rgb)
    else:
        B, SS, _ = p2f.shape
        block = (p2f >= 0).reshape(B, SS // a, a, SS // a, a).any(axis=(2, 4))
        bound = _abs_sum(grad_rgb, block)
    return _collect(parts, T * T * 3, bound)


# ------------------------------------------------------------------------------------------------------ shade_mip_bwd_kernel
def restate_mip(grad_rgb, frag, verts_uvs, faces_uvs, pyr, lam, T, L, k, dt=F32):
    """ops.shade_mip_bwd(want_levels=True): pyr the packed chain fp32, lam (B,S,S) fp32 -> deposits into the packed per-level
    gradient: columns 0..11 the lower level l0, 12..23 the upper level l0 + 1 (valid only where t = lambda - l0 != 0).
    t == 0: the lower level takes g k; else g k (1 - t) and g k t.  d/d(ix, iy): the lower level's first, then `gix + gx` of
    the upper (level_bwd's `first ? gx : gix + gx`).  Bound (st3d_shade_mip_bwd): sum |grad_rgb| over all B*3*S^2 values."""
    assert dt in (F32, F64)
    pyr, lam = np.asarray(pyr), np.asarray(lam)
    assert pyr.dtype == F32 and lam.dtype == F32
    flat = pyr.astype(dt)
    off = M.texel_offsets(T, L)
    parts = []
    for b, fr in enumerate(_views(frag)):
        cov, u, v = M._uv(fr, verts_uvs, faces_uvs, dt)
        q0 = M.foot0(u, v, T, dt)
        gk = _upstream(grad_rgb, b, cov, 1, dt) * _k_of(k, b, cov, dt)[:, None]
        l0, t = M._split(lam[b][cov], L, dt)
        two = t != 0
        tt = t[:, None]
        ga = np.where(tt != 0, gk * (dt(1) - tt), gk)
        gb = gk * tt
        _same(dt, t, ga, gb)
        n = gk.shape[0]
        idx, c, ok = np.zeros((n, 8, 3), np.int64), np.zeros((n, 8, 3), dt), np.zeros((n, 8, 3), bool)
        idx[:, :4], c[:, :4], ok[:, :4], gix, giy = _level(flat, M._level_foot(q0, l0, T, dt), off[l0], l0, ga, dt)
        if two.any():
            l1 = (l0 + 1)[two]
            qb = M.footl(q0["ix"][two], q0["iy"][two], l1, T, dt)
            iu, cu, oku, ux, uy = _level(flat, qb, off[l1], l1, gb[two], dt)
            idx[two, 4:], c[two, 4:], ok[two, 4:] = iu, cu, oku
            gix[two] = gix[two] + ux
            giy[two] = giy[two] + uy
        _same(dt, c, gix, giy)
        guv, gbary = _uv_tail(q0, gix, giy, T, fr, verts_uvs, faces_uvs, dt)
        parts.append(dict(idx=idx.reshape(n, 24), c=c.reshape(n, 24), valid=ok.reshape(n, 24), where=_where(b, fr), guv=guv,
                          gbary=gbary))
    return _collect(parts, M.numel(T, L), _abs_sum(grad_rgb))


# -------------------------------------------------------------------------------------------------------- shade_vc_bwd_kernel
def restate_vc(grad_rgb, frag, faces, colours, k, dt=F32):
    """ops.shade_vc_bwd: deposits b_j * (g_c k) into colours[faces[f][j]][c] (column 3 j + c), gbary_j = (gk_0 C_j0 + gk_1 C_j1)
    + gk_2 C_j2.  Bound (vc_abs_sum_kernel): sum over covered pixels of (|g_0| + |g_1| + |g_2|) max(1, max_j |b_j|)."""
    assert dt in (F32, F64)
    colours, faces = np.asarray(colours), np.asarray(faces).astype(np.int64)
    assert colours.dtype == F32
    col = colours.astype(dt)
    parts = []
    weight = []
    for b, fr in enumerate(_views(frag)):
        p2f, _, bary, _ = fr
        cov = p2f >= 0
        vtx = faces[p2f[cov]]                                               # (n,3)
        bw = bary[cov].astype(dt)                                           # (n,3)
        gk = _upstream(grad_rgb, b, cov, 1, dt) * _k_of(k, b, cov, dt)[:, None]
        c = gk[:, None, :] * bw[:, :, None]                                 # (n, corner, channel): dep_g[ch] * dep_w[j]
        C = col[vtx]                                                        # (n, corner, channel)
        gbary = (gk[:, None, 0] * C[:, :, 0] + gk[:, None, 1] * C[:, :, 1]) + gk[:, None, 2] * C[:, :, 2]
        _same(dt, gk, c, gbary)
        n = gk.shape[0]
        idx = vtx[:, :, None] * 3 + np.arange(3)[None, None]
        parts.append(dict(idx=idx.reshape(n, 9), c=np.ascontiguousarray(c).reshape(n, 9), valid=np.ones((n, 9), bool),
                          where=_where(b, fr), gbary=gbary))
        weight.append(np.where(cov, np.maximum(np.abs(bary.astype(F64)).max(-1), 1.0), 0.0))
    return _collect(parts, colours.shape[0] * 3, _abs_sum(grad_rgb, np.stack(weight)))


# ----------------------------------------------------------------------------------------------------- shade_atlas_bwd_kernel
def restate_atlas(grad_rgb, frag, R, n_faces, k, dt=F32):
    """ops.shade_atlas_bwd: one deposit (g_c k) * 1.0f per covered pixel into atlas[f][wy][wx][c], (wy, wx) =
    _atlasref.texel_index (atlas.h).  Bound (atlas_abs_sum_kernel): sum |grad_rgb| over the covered pixels."""
    assert dt in (F32, F64)
    parts = []
    for b, fr in enumerate(_views(frag)):
        p2f, _, bary, _ = fr
        cov = p2f >= 0
        f = p2f[cov].astype(np.int64)
        wy, wx = AT.texel_index(bary[cov][:, 0], bary[cov][:, 1], R)
        gk = _upstream(grad_rgb, b, cov, 1, dt) * _k_of(k, b, cov, dt)[:, None]
        c = gk * dt(1)
        _same(dt, c)
        idx = (((f * R + wy) * R + wx) * 3)[:, None] + np.arange(3)[None]
        parts.append(dict(idx=idx, c=c, valid=np.ones(idx.shape, bool), where=_where(b, fr)))
    return _collect(parts, n_faces * R * R * 3, _abs_sum(grad_rgb, np.asarray(frag[0]) >= 0))


# ------------------------------------------------------------------------------------------------------------- what tests share
def deposits(r):
    """the deposits that exist, flat: (index, value)"""
    return r["idx"][r["valid"]], r["c"][r["valid"]]


def scatter64(r):
    """every deposit added in fp64 (np.add.at) -> (n_out,)"""
    out = np.zeros(r["n_out"], F64)
    i, c = deposits(r)
    np.add.at(out, i, c.astype(F64))
    return out


def dense(r, key, frag):
    """a per-pixel output on the whole (B,S,S,n) grid, +0 where there is no face"""
    p2f = np.asarray(frag[0])
    B, S, _ = p2f.shape
    val = r[key]
    out = np.zeros((B * S * S, val.shape[1]), val.dtype)
    out[r["where"][:, 0] * S * S + r["where"][:, 1]] = val
    return out.reshape(B, S, S, val.shape[1])


def disjoint_groups(r):
    """Greedy partition of the fragments into groups in which no two share an output location (texel, vertex: idx // 3 of
    the deposits that exist) -> list of index arrays, every fragment in exactly one group"""
    used, groups = [], []
    for n in range(r["idx"].shape[0]):
        key = set((r["idx"][n][r["valid"][n]] // 3).tolist())
        for u, g in zip(used, groups):
            if not (u & key):
                u |= key
                g.append(n)
                break
        else:
            used.append(set(key))
            groups.append([n])
    return [np.array(g) for g in groups]


# the "clamped" copy of the cow: its UV table through uv -> CLAMP_A uv + CLAMP_B, so that part of the chart leaves [0,1]^2 at
# both ends of u and of v (uv_footprint's cx / cy branches) and footprints end on x1 = T / yf1 = T (the vx1 / vy1 masks)
# (u -> 1.3 u - 0.15; the visible part of the cow's chart has v in [0.135, 0.978], so 1.3 v - 0.15 clamps no fragment at the
# low end of v: v -> 1.45 v - 0.30 does, below v = 0.207)
CLAMP_A, CLAMP_B = np.array([1.3, 1.45], np.float32), np.array([-0.15, -0.30], np.float32)
CLAMP_MIN = 5


def clamped_uvs(verts_uvs):
    return (np.asarray(verts_uvs, F32) * CLAMP_A[None] + CLAMP_B[None]).astype(F32)


def clamp_counts(r, T):
    """fragments clamped at (u low, u high, v low, v high), and with x1 == T, yf1 == T, of a restate_shade result"""
    cx, cy, ix, iy = r["cx"], r["cy"], r["ix"], r["iy"]
    return (int((cx & (ix == 0)).sum()), int((cx & (ix == T - 1)).sum()), int((cy & (iy == 0)).sum()),
            int((cy & (iy == T - 1)).sum()), int((~r["vx1"]).sum()), int((~r["vy1"]).sum()))


def edge_fragments():
    """The scatter scene's fragments (tests/_scatter_scene.py) with every covered pixel moved OUTSIDE its face:
    dists = +3e-3 * hash in [0, 3e-3), so dist / sigma lies in [0, 30), prob = 1 / (1 + exp(dist / sigma)) runs from 1/2 down
    to 1e-13 and k = prob / (prob + 1e-10) from 1 down to 1e-3.  On every rasterised scene of these tests -- and on the
    scatter scene as it is -- dist <= 0, prob >= 1/2 and k rounds to exactly 1.0f: this is the one set on which the blend
    factor is not 1 and the device's expf reaches the gradients."""
    import _scatter_scene as sc
    p2f, zbuf, bary, dists = sc.fragments()
    d = (np.float32(3e-3) * sc.hash01(sc.S * sc.S, 9)).astype(F32).reshape(sc.S, sc.S)
    return p2f, zbuf, bary, np.where(p2f >= 0, d[None], dists).astype(F32)
