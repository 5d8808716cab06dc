"""Per-vertex colours (TexturesVertex) restated in numpy: the forward and its backward, and the scenes the CPU and
GPU tests share.  `dt` is the number format of every operation the kernels do in fp32: np.float64 states the definitions
(the checker of the gradients), np.float32 rounds every step in the kernels' order (numpy rounds each fp32 operation
correctly; the products are rounded before they are added, as a build without FMA contraction does).

Forward, per covered pixel (face f, barycentrics b as rasterised):
    t_c   = b0 C[faces[f,0]][c] + b1 C[faces[f,1]][c] + b2 C[faces[f,2]][c]        (left to right)
    rgb_c = (wnum t_c + delta 1.0) / denom,   mask = (1 - (1 - prob)) > 0
with (prob, wnum, delta, denom) the K = 1 blend of the UV path; uncovered pixels are white with mask 0.
Backward, with k = wnum / denom and gk_c = g_c k:
    dC[faces[f,i]][c] += b_i gk_c  (nine deposits per covered pixel),   db_i = sum_c gk_c C[faces[f,i]][c]  (0 uncovered)."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
SIGMA = GAMMA = 1e-4
BLEND_EPS, ZNEAR, ZFAR = 1e-10, 1.0, 100.0


def _exp(x, dt):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, F64)).astype(dt)             # correctly rounded


def blend(dist, z, dt):
    """blend_k1 of the shade kernels: (prob, wnum, delta, denom), every step in dt"""
    dist, z = np.asarray(dist, dt), np.asarray(z, dt)
    prob = (dt(1) / (dt(1) + _exp((dist / dt(SIGMA)).astype(dt), dt)).astype(dt)).astype(dt)
    z_inv = ((dt(ZFAR) - z).astype(dt) / (dt(ZFAR) - dt(ZNEAR))).astype(dt)
    z_max = np.maximum(z_inv, dt(BLEND_EPS))
    wnum = (prob * _exp(((z_inv - z_max).astype(dt) / dt(GAMMA)).astype(dt), dt)).astype(dt)
    delta = np.maximum(_exp(((dt(BLEND_EPS) - z_max).astype(dt) / dt(GAMMA)).astype(dt), dt), dt(BLEND_EPS))
    return prob, wnum, delta, (wnum + delta).astype(dt)


def _gather(frag, faces, colours, dt):
    p2f, _, bary, _ = frag
    cov = p2f >= 0
    vidx = np.asarray(faces)[p2f[cov]].astype(np.int64)                 # (n,3)
    return cov, vidx, np.asarray(colours, dt)[vidx], np.asarray(bary, dt)[cov]     # (n,3,3) [pixel, corner, channel], (n,3)


def shade_fwd(frag, faces, colours, dt=F64):
    """one view -> rgb (3,S,S), mask (1,S,S) in dt"""
    p2f, zbuf, _, dists = frag
    S = p2f.shape[0]
    cov, _, C, b = _gather(frag, faces, colours, dt)
    t = (((b[:, 0, None] * C[:, 0]).astype(dt) + (b[:, 1, None] * C[:, 1]).astype(dt)).astype(dt)
         + (b[:, 2, None] * C[:, 2]).astype(dt)).astype(dt)                # (n,3)
    prob, wnum, delta, denom = blend(dists[cov], zbuf[cov], dt)
    rgb = np.ones((3, S, S), dt)
    rgb[:, cov] = (((wnum[:, None] * t).astype(dt) + (delta[:, None] * dt(1)).astype(dt)).astype(dt) / denom[:, None]).astype(dt).T
    mask = np.zeros((1, S, S), dt)
    mask[0, cov] = ((dt(1) - (dt(1) - prob).astype(dt)) > 0).astype(dt)
    return rgb, mask


def shade_bwd(grad_rgb, frag, faces, colours, dt=F64, gcol=None):
    """one view: grad_rgb (3,S,S) -> (gcol (V,3) fp64, ACCUMULATED when given; grad_bary (S,S,3) in dt).  Every deposit and
    every product is rounded to dt; the sums over pixels are fp64."""
    p2f, zbuf, _, dists = frag
    S = p2f.shape[0]
    colours = np.asarray(colours)
    if gcol is None:
        gcol = np.zeros(colours.shape, F64)
    cov, vidx, C, b = _gather(frag, faces, colours, dt)
    _, wnum, _, denom = blend(dists[cov], zbuf[cov], dt)
    k = (wnum / denom).astype(dt)
    gk = (np.asarray(grad_rgb, dt)[:, cov].T * k[:, None]).astype(dt)                  # (n,3) [pixel, channel]
    dep = (b[:, :, None] * gk[:, None, :]).astype(dt)                                   # (n,3,3) [pixel, corner, channel]
    np.add.at(gcol, (vidx[:, :, None], np.arange(3)[None, None, :]), dep.astype(F64))
    p = (gk[:, None, :] * C).astype(dt)                                                 # gk_c C[v_i][c]
    gb = ((p[:, :, 0] + p[:, :, 1]).astype(dt) + p[:, :, 2]).astype(dt)
    gbary = np.zeros((S, S, 3), dt)
    gbary[cov] = gb
    return gcol, gbary


# ----------------------------------------------------------------------------------------------------- the shared scenes
B = 2
SIDES = (16, 17, 24)                  # 17: partial tiles; 24: 2 x 2 tiles


def cameras():
    import _scenes
    return _scenes.random_cameras(B, 5)


def colours(V, seed=0):
    return np.random.default_rng(1000 + seed).random((V, 3), dtype=np.float32)


def upstream(S, n=B):
    return np.random.default_rng(200 + S).standard_normal((n, 3, S, S)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cow():
    import _scenes
    return _scenes.load_asset("cow")


@functools.lru_cache(maxsize=None)
def cow_subdivided(times=2):
    """the cow after `times` midpoint subdivisions: (verts, faces) -- 93 696 faces at 2"""
    import _scenes
    m = cow()
    v, f, uv, fuv = m["verts"], m["faces"], m["verts_uvs"], m["faces_uvs"]
    for _ in range(times):
        v, f, uv, fuv = _scenes.subdivide(v, f, uv, fuv)
    return v, f


def two_triangles():
    """a quad of two triangles that fills the image: R = I, T = (0, 0, 3) puts the plane z = 0 at view depth 3, where the
    frustum's half-width is 3 tan 30 deg = 1.73 < 4 -> (verts, faces, R (1,3,3), T (1,3)).  The quad is wider than high so that
    the shared diagonal passes through no pixel centre (a centre on an edge belongs to neither face)"""
    verts = np.array([[-4, -4, 0], [5, -4, 0], [5, 4, 0], [-4, 4, 0]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    R = np.eye(3, dtype=F32)[None]
    T = np.array([[0, 0, 3]], F32)
    return verts, faces, R, T


@functools.lru_cache(maxsize=None)
def oracle_fragments(S):
    """the CPU oracle's fragments of the cow under cameras() at side S (read-only) and the projected vertices"""
    from oracle import render_ref as rr
    m = cow()
    R, T = cameras()
    frags, ndcs = [], []
    for b in range(B):
        ndc = rr.project_verts(m["verts"], R[b], T[b])
        frag = rr.rasterize(ndc, m["faces"], S, 0.0, 4)
        for a in frag:
            a.setflags(write=False)
        frags.append(frag)
        ndcs.append(ndc)
    return frags, ndcs


# ---- the scene that pins the restatement to the C oracle: the cow with per-vertex UVs (faces_uvs = faces) and a texture
# that is affine in (u, v) per channel -- bilinear sampling reproduces an affine function, and
# sum_i b_i ramp(uv_i) = ramp(sum_i b_i uv_i), so oracle.render_ref.shade_fwd on it is the vertex-colour forward.
RAMP = np.array([[0.15, 0.55, 0.20], [0.70, -0.30, 0.25], [0.40, 0.10, 0.35]], F64)       # per channel: a + b u + c v


def ramp(uv):
    uv = np.asarray(uv, F64)
    return RAMP[:, 0][None] + uv[:, 0:1] * RAMP[:, 1][None] + uv[:, 1:2] * RAMP[:, 2][None]


def ramp_scene(T):
    """-> (verts_uvs (V,2) fp32, texture (T,T,3) fp32, colours (V,3) fp32) of the cow"""
    xy = cow()["verts"][:, :2].astype(F64)
    uv = (0.1 + 0.8 * (xy - xy.min(0)) / (xy.max(0) - xy.min(0))).astype(F32)
    # texel (row r, column x) of the ORIGINAL map is sampled at v = ((T-1) - r) / (T-1), u = x / (T-1)  (rows flipped)
    r, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    tuv = np.stack([x / (T - 1.0), ((T - 1) - r) / (T - 1.0)], -1).reshape(-1, 2)
    tex = ramp(tuv).reshape(T, T, 3).astype(F32)
    return uv, tex, ramp(uv).astype(F32)
