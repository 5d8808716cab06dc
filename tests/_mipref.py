"""Mip-mapped trilinear sampling restated in numpy: the chain and its adjoint, the analytic level of detail, the
sample and its backward.  `dt` is the number format of every operation that the kernels do in fp32: np.float64 states the
definitions (the checker of the GPU tests, the subject of the finite-difference tests), np.float32 rounds every step as
oracle/raster_ref.c and the kernels do (numpy rounds each fp32 operation correctly), so that lambda == 0 reproduces the
oracle's own shade_fwd / shade_bwd exactly and the chain is the ordered fp32 sum bit for bit.  The level of detail is
always fp64."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
SIGMA = GAMMA = 1e-4
BLEND_EPS, ZNEAR, ZFAR = 1e-10, 1.0, 100.0
MAX_LEVELS = 16


# ----------------------------------------------------------------------------------------------------- layout
def max_levels(T):
    L = 1
    while L < MAX_LEVELS and T % (1 << L) == 0 and T >> L >= 2:
        L += 1
    return L


def shape_ok(T, L):
    if T < 2 or not 1 <= L <= MAX_LEVELS:
        return False
    return L == 1 or (T % (1 << (L - 1)) == 0 and T >> (L - 1) >= 2)


def texel_offsets(T, L):
    """texel offset of every level in the packed chain, the total at [L]"""
    off = [0]
    for l in range(L):
        off.append(off[-1] + (T >> l) ** 2)
    return np.asarray(off, np.int64)


def numel(T, L):
    return int(3 * texel_offsets(T, L)[L]) if shape_ok(T, L) else 0


def pack(levels):
    return np.concatenate([np.ascontiguousarray(x).reshape(-1) for x in levels])


def unpack(flat, T, L):
    off = texel_offsets(T, L) * 3
    return [flat[off[l]:off[l + 1]].reshape(T >> l, T >> l, 3) for l in range(L)]


# ----------------------------------------------------------------------------------------------------- chain
def build(tex, L, dt=F32):
    """[level_0 .. level_{L-1}]: level_{l+1}[r][x] = ((a + b) + (c + d)) * 0.25 over the 2 x 2 block, every step in dt"""
    lv = [np.asarray(tex, dt)]
    assert shape_ok(lv[0].shape[0], L)
    for _ in range(1, L):
        p = lv[-1]
        a, b, c, d = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
        lv.append(((a + b).astype(dt) + (c + d).astype(dt)).astype(dt) * dt(0.25))
    return lv


def adjoint(glevels, dt=F32):
    """acc_{L-1} = g_{L-1}; acc_l[r][x] = g_l[r][x] + 0.25 * acc_{l+1}[r>>1][x>>1] -> acc_0, every step in dt"""
    acc = np.asarray(glevels[-1], dt)
    for g in reversed(glevels[:-1]):
        up = np.repeat(np.repeat(acc, 2, axis=0), 2, axis=1)
        acc = (np.asarray(g, dt) + (dt(0.25) * up).astype(dt)).astype(dt)
    return acc


# ----------------------------------------------------------------------------------------------------- level of detail
def lod(frag, verts_ndc, faces, verts_uvs, faces_uvs, T, L, bias=0.0):
    """lambda (S,S) fp64 of one view's fragments: analytic, from the face's projected vertices (x_ndc, y_ndc, view depth)"""
    p2f, zbuf, bary, _ = frag
    S = p2f.shape[0]
    out = np.zeros((S, S), F64)
    cov = p2f >= 0
    f = p2f[cov]
    P = np.asarray(verts_ndc, F64)[np.asarray(faces)[f]]                    # (n,3,3)
    x, y, z = P[:, :, 0], P[:, :, 1], P[:, :, 2]
    uv = np.asarray(verts_uvs, F64)[np.asarray(faces_uvs)[f]]              # (n,3,2)
    b = np.asarray(bary, F64)[cov]
    zp = np.asarray(zbuf, F64)[cov]
    A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    with np.errstate(all="ignore"):
        dax = np.stack([y[:, 1] - y[:, 2], y[:, 2] - y[:, 0], y[:, 0] - y[:, 1]], 1) / A[:, None]
        day = np.stack([x[:, 2] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 0]], 1) / A[:, None]
        rho = []
        for da in (dax, day):
            q = da / z
            s = q[:, 0] + q[:, 1] + q[:, 2]
            db = zp[:, None] * (q - b * s[:, None])
            du = db[:, 0] * uv[:, 0, 0] + db[:, 1] * uv[:, 1, 0] + db[:, 2] * uv[:, 2, 0]
            dv = db[:, 0] * uv[:, 0, 1] + db[:, 1] * uv[:, 1, 1] + db[:, 2] * uv[:, 2, 1]
            rho.append(np.hypot(du, dv) * ((T - 1) * 2.0 / S))
        r = np.where(rho[0] > rho[1], rho[0], rho[1])
        lam = np.where(r > 1.0, np.clip(np.log2(np.where(r > 1.0, r, 2.0)) + bias, 0.0, L - 1.0), 0.0)
    lam[A == 0.0] = 0.0
    out[cov] = lam
    return out


# ----------------------------------------------------------------------------------------------------- footprints
def _finish(ix, iy, n, dt):
    fx, fy = np.floor(ix), np.floor(iy)
    x0, yf0 = fx.astype(np.int64), fy.astype(np.int64)
    wx1, wy1 = (ix - fx).astype(dt), (iy - fy).astype(dt)
    q = dict(x0=x0, x1=x0 + 1, r0=(n - 1) - yf0, r1=(n - 1) - (yf0 + 1), wx1=wx1, wx0=(dt(1) - wx1).astype(dt), wy1=wy1,
             wy0=(dt(1) - wy1).astype(dt), vx0=(x0 >= 0) & (x0 < n), vx1=(x0 + 1 >= 0) & (x0 + 1 < n),
             vy0=(yf0 >= 0) & (yf0 < n), vy1=(yf0 + 1 >= 0) & (yf0 + 1 < n), ix=ix, iy=iy)
    return q


def _clamp(i, hi, dt):
    hi = np.asarray(hi).astype(dt)
    low, high = ~(i >= 0), i > hi
    return np.where(low, dt(0), np.where(high, hi, i)).astype(dt), low | high


def foot0(u, v, T, dt):
    """uv_footprint of shade.hip / raster_ref.c"""
    gx, gy = (u * dt(2) - dt(1)).astype(dt), (v * dt(2) - dt(1)).astype(dt)
    ix = (((gx + dt(1)) / dt(2)).astype(dt) * dt(T - 1)).astype(dt)
    iy = (((gy + dt(1)) / dt(2)).astype(dt) * dt(T - 1)).astype(dt)
    ix, cx = _clamp(ix, T - 1, dt)
    iy, cy = _clamp(iy, T - 1, dt)
    q = _finish(ix, iy, np.full(ix.shape, T, np.int64), dt)
    q.update(cx=cx, cy=cy, n=np.full(ix.shape, T, np.int64))
    return q


def footl(ix, iy, l, T, dt):
    """level l >= 1 (per-pixel array) at ix_l = (ix + 0.5) / 2^l - 0.5, clamped to [0, T_l - 1]"""
    n = T >> l
    inv = (dt(1) / (1 << l).astype(dt)).astype(dt)
    jx = ((ix + dt(0.5)).astype(dt) * inv - dt(0.5)).astype(dt)
    jy = ((iy + dt(0.5)).astype(dt) * inv - dt(0.5)).astype(dt)
    jx, cx = _clamp(jx, n - 1, dt)
    jy, cy = _clamp(jy, n - 1, dt)
    q = _finish(jx, jy, n, dt)
    q.update(cx=cx, cy=cy, n=n)
    return q


def _select(m, a, b):
    return {k: np.where(m, a[k], b[k]) for k in a}


def _level_foot(q0, l, T, dt):
    """the footprint on per-pixel level l: q0 itself where l == 0"""
    ql = footl(q0["ix"], q0["iy"], np.maximum(l, 1), T, dt)
    return _select(l == 0, q0, ql)


_CORNERS = (("vy0", "vx0", "r0", "x0", "wx0", "wy0"), ("vy0", "vx1", "r0", "x1", "wx1", "wy0"),
            ("vy1", "vx0", "r1", "x0", "wx0", "wy1"), ("vy1", "vx1", "r1", "x1", "wx1", "wy1"))


def _corner(q, off, k, dt):
    vy, vx, r, x, wx, wy = _CORNERS[k]
    valid = q[vy] & q[vx]
    n = q["n"]
    texel = off + np.clip(q[r], 0, n - 1) * n + np.clip(q[x], 0, n - 1)
    return valid, texel, (q[wx] * q[wy]).astype(dt)


def _bil(pyr, q, off, dt):
    """(n,3): the taps in the kernels' order; a tap that does not exist is not multiplied"""
    t = np.zeros((q["x0"].shape[0], 3), dt)
    for k in range(4):
        valid, texel, w = _corner(q, off, k, dt)
        tap = pyr[texel[:, None] * 3 + np.arange(3)[None]]
        t = np.where(valid[:, None], (t + (tap * w[:, None]).astype(dt)).astype(dt), t)
    return t


def _split(lam, L, dt):
    lam = np.asarray(lam, dt)
    lam = np.where(lam > 0, np.minimum(lam, dt(L - 1)), dt(0)).astype(dt)
    l0 = np.minimum(np.floor(lam).astype(np.int64), L - 1)
    return l0, (lam - l0.astype(dt)).astype(dt)


def sample(u, v, pyr, T, L, lam, dt=F64):
    """texel (n,3) = (1 - t) bil(l0) + t bil(l0 + 1) at per-point (u, v, lambda); pyr: the packed chain in dt"""
    off = texel_offsets(T, L)
    l0, t = _split(lam, L, dt)
    q0 = foot0(np.asarray(u, dt), np.asarray(v, dt), T, dt)
    lo = _bil(pyr, _level_foot(q0, l0, T, dt), off[l0], dt)
    l1 = np.minimum(l0 + 1, L - 1)
    up = _bil(pyr, _level_foot(q0, l1, T, dt), off[l1], dt)
    tt = t[:, None]
    mix = (((dt(1) - tt).astype(dt) * lo).astype(dt) + (tt * up).astype(dt)).astype(dt)
    return np.where(tt != 0, mix, lo)


def _level_bwd(pyr, q, off, l, g, gpyr, dt):
    """deposits g * (wx * wy) of one level into gpyr (fp64, in pixel, channel, corner order) -> this level's d/d(ix_0, iy_0) fp64"""
    n_px = g.shape[0]
    idx = np.zeros((n_px, 3, 4), np.int64)
    val = np.zeros((n_px, 3, 4), F64)
    ok = np.zeros((n_px, 3, 4), bool)
    taps = []
    for k in range(4):
        valid, texel, w = _corner(q, off, k, dt)
        idx[:, :, k] = texel[:, None] * 3 + np.arange(3)[None]
        val[:, :, k] = (g * w[:, None]).astype(dt)
        ok[:, :, k] = valid[:, None]
        taps.append(np.where(valid[:, None], pyr[idx[:, :, k]], dt(0)))
    np.add.at(gpyr, idx[ok], val[ok])
    t00, t01, t10, t11 = taps
    g64 = g.astype(F64)
    dx = (t01 - t00).astype(dt).astype(F64) * q["wy0"][:, None].astype(F64) + (t11 - t10).astype(dt).astype(F64) * q["wy1"][:, None].astype(F64)
    dy = (t10 - t00).astype(dt).astype(F64) * q["wx0"][:, None].astype(F64) + (t11 - t01).astype(dt).astype(F64) * q["wx1"][:, None].astype(F64)
    gix, giy = np.zeros(n_px, F64), np.zeros(n_px, F64)
    for c in range(3):
        gix = gix + g64[:, c] * dx[:, c]
        giy = giy + g64[:, c] * dy[:, c]
    scale = np.ldexp(1.0, -l)
    gix = np.where((l > 0) & q["cx"], 0.0, gix * scale)
    giy = np.where((l > 0) & q["cy"], 0.0, giy * scale)
    return gix, giy


def sample_bwd(g, u, v, pyr, T, L, lam, dt=F64, gpyr=None):
    """g (n,3) = d loss / d texel -> (gpyr fp64 packed, ACCUMULATED when given; d loss / du, d loss / dv fp64); lambda is a
    constant"""
    off = texel_offsets(T, L)
    if gpyr is None:
        gpyr = np.zeros(int(off[L]) * 3, F64)
    g = np.asarray(g, dt)
    l0, t = _split(lam, L, dt)
    q0 = foot0(np.asarray(u, dt), np.asarray(v, dt), T, dt)
    tt = t[:, None]
    two = (t != 0)
    ga = np.where(tt != 0, (g * (dt(1) - tt).astype(dt)).astype(dt), g)
    gix, giy = _level_bwd(pyr, _level_foot(q0, l0, T, dt), off[l0], l0, ga, gpyr, dt)
    if two.any():
        l1 = (l0 + 1)[two]
        qb = _level_foot({k: a[two] for k, a in q0.items()}, l1, T, dt)
        ux, uy = _level_bwd(pyr, qb, off[l1], l1, (g[two] * tt[two]).astype(dt), gpyr, dt)
        gix[two] = gix[two] + ux
        giy[two] = giy[two] + uy
    gu = np.where(q0["cx"], 0.0, gix * float(T - 1))
    gv = np.where(q0["cy"], 0.0, giy * float(T - 1))
    return gpyr, gu, gv


# ----------------------------------------------------------------------------------------------------- shade
def _exp(x, dt):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, F64)).astype(dt)             # correctly rounded, as glibc's expf is


def _blend(dist, z, dt):
    dist, z = np.asarray(dist, dt), np.asarray(z, dt)
    prob = (dt(1) / (dt(1) + _exp((dist / dt(SIGMA)).astype(dt), dt)).astype(dt)).astype(dt)
    z_inv = ((dt(ZFAR) - z).astype(dt) / (dt(ZFAR) - dt(ZNEAR))).astype(dt)
    z_max = np.maximum(z_inv, dt(BLEND_EPS))
    wnum = (prob * _exp(((z_inv - z_max).astype(dt) / dt(GAMMA)).astype(dt), dt)).astype(dt)
    delta = np.maximum(_exp(((dt(BLEND_EPS) - z_max).astype(dt) / dt(GAMMA)).astype(dt), dt), dt(BLEND_EPS))
    return prob, wnum, delta, (wnum + delta).astype(dt)


def _uv(frag, verts_uvs, faces_uvs, dt):
    p2f, _, bary, _ = frag
    cov = p2f >= 0
    t = np.asarray(verts_uvs, dt)[np.asarray(faces_uvs)[p2f[cov]]]        # (n,3,2)
    b = np.asarray(bary, dt)[cov]
    u = (((b[:, 0] * t[:, 0, 0]).astype(dt) + (b[:, 1] * t[:, 1, 0]).astype(dt)).astype(dt) + (b[:, 2] * t[:, 2, 0]).astype(dt)).astype(dt)
    v = (((b[:, 0] * t[:, 0, 1]).astype(dt) + (b[:, 1] * t[:, 1, 1]).astype(dt)).astype(dt) + (b[:, 2] * t[:, 2, 1]).astype(dt)).astype(dt)
    return cov, u, v


def shade_fwd(frag, verts_uvs, faces_uvs, pyr, T, L, lam, dt=F64):
    """one view -> rgb (3,S,S), mask (1,S,S) in dt; lam (S,S)"""
    p2f, zbuf, _, dists = frag
    S = p2f.shape[0]
    cov, u, v = _uv(frag, verts_uvs, faces_uvs, dt)
    texel = sample(u, v, np.asarray(pyr, dt), T, L, np.asarray(lam)[cov], dt)
    prob, wnum, delta, denom = _blend(dists[cov], zbuf[cov], dt)
    rgb = np.ones((3, S, S), dt)
    rgb[:, cov] = (((wnum[:, None] * texel).astype(dt) + delta[:, None]).astype(dt) / denom[:, None]).astype(dt).T
    mask = np.zeros((1, S, S), dt)
    mask[0, cov] = ((dt(1) - (dt(1) - prob).astype(dt)) > 0).astype(dt)
    return rgb, mask


def shade_bwd(grad_rgb, frag, verts_uvs, faces_uvs, pyr, T, L, lam, dt=F64, gpyr=None):
    """one view: grad_rgb (3,S,S) -> (gpyr fp64 packed (accumulated when given), grad_uv (S,S,2) in dt)"""
    p2f, zbuf, _, dists = frag
    S = p2f.shape[0]
    cov, u, v = _uv(frag, verts_uvs, faces_uvs, dt)
    _, wnum, _, denom = _blend(dists[cov], zbuf[cov], dt)
    k = (wnum / denom).astype(dt)
    g = (np.asarray(grad_rgb, dt)[:, cov].T * k[:, None]).astype(dt)
    gpyr, gu, gv = sample_bwd(g, u, v, np.asarray(pyr, dt), T, L, np.asarray(lam)[cov], dt, gpyr)
    guv = np.zeros((S, S, 2), dt)
    guv[cov, 0], guv[cov, 1] = gu.astype(dt), gv.astype(dt)
    return gpyr, guv


def fold(gpyr, T, L):
    """the adjoint in fp64 on a packed per-level gradient -> (T,T,3)"""
    return adjoint(unpack(np.asarray(gpyr, F64), T, L), F64)


# ----------------------------------------------------------------------------------------------------- the shared scene
# (S, T, L): the cow under _scenes.random_cameras(2, 5); pixel classes (covered / lambda = 0 / fractional / clamped at
# L - 1) on the CPU oracle's fragments: 136/38/84/14, 152/15/113/24, 212/62/146/4, 306/40/150/116, 306/40/266/0
CASES = [(16, 32, 3), (17, 48, 3), (20, 40, 4), (24, 64, 2), (24, 64, 6)]
B = 2


def cameras():
    import _scenes
    return _scenes.random_cameras(B, 5)


def texture(T):
    return np.random.default_rng(T).random((T, T, 3), dtype=np.float32)


def upstream(S):
    return np.random.default_rng(100 + S).standard_normal((B, 3, S, S)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_case(S, T):
    """the CPU oracle's fragments and projected vertices of the shared scene at side S (read-only)"""
    import _scenes
    from oracle import render_ref as rr
    mesh = _scenes.load_asset("cow")
    R, Tt = cameras()
    tex = texture(T)
    _, _, frags = rr.render_views(mesh["verts"], mesh["faces"], mesh["verts_uvs"], mesh["faces_uvs"], tex, R, Tt, S, 8)
    ndc = [rr.project_verts(mesh["verts"], R[b], Tt[b]) for b in range(B)]
    return dict(mesh=mesh, R=R, T=Tt, tex=tex, frags=frags, ndc=ndc)


def classes(lam, cov, L):
    """(covered, lambda == 0, 0 < lambda < L - 1, lambda == L - 1) pixel counts of a lambda plane"""
    lam = np.asarray(lam)[cov]
    return int(cov.sum()), int((lam == 0).sum()), int(((lam > 0) & (lam < L - 1)).sum()), int((lam == L - 1).sum())
