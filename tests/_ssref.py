"""Supersampled rendering restated with the CPU oracle: rasterise and shade at side a * S (oracle/render_ref.py), then the
a x a box filter as the ORDERED fp32 sum the kernels are pinned to:

    s = c[ay][ax];  s = s + c[ay+j][ax+i] for the other sub-pixels in row-major order;  out = s / float32(a * a)

and its transpose (every sub-pixel of a block gets g / float32(a * a)) in front of the oracle's own backward.  numpy rounds
every fp32 addition and division correctly, so this is the semantics bit for bit wherever the sub-pixel colours are."""
import functools

import numpy as np


def box_down(x, a, dtype=np.float32):
    """(..., a*S, a*S) -> (..., S, S): ordered row-major sum of each a x a block / (a * a), every step rounded to `dtype`"""
    x = np.asarray(x, dtype)
    assert x.shape[-1] == x.shape[-2] and x.shape[-1] % a == 0
    s = x[..., 0::a, 0::a].copy()
    for j in range(a):
        for i in range(a):
            if j or i:
                s = (s + x[..., j::a, i::a]).astype(dtype)
    return (s / dtype(a * a)).astype(dtype)


def box_down_t(g, a, dtype=np.float32):
    """the transpose: (..., S, S) -> (..., a*S, a*S), g / (a * a) (one division per value) at every sub-pixel"""
    gs = (np.asarray(g, dtype) / dtype(a * a)).astype(dtype)
    return np.ascontiguousarray(np.repeat(np.repeat(gs, a, axis=-2), a, axis=-1))


def render(mesh, tex, R, T, S, a, nthreads=8):
    """-> rgb (B,3,S,S), coverage (B,1,S,S), the oracle's fragments at side a * S (one tuple per view)"""
    from oracle import render_ref as rr
    hi, mask, frags = rr.render_views(mesh["verts"], mesh["faces"], mesh["verts_uvs"], mesh["faces_uvs"], tex, R, T, a * S, nthreads)
    return box_down(hi, a), box_down(mask, a), frags


def backward(g, frags, mesh, tex, R, T, a):
    """g (B,3,S,S) -> d/dtexture (T,T,3) fp64, d/dverts (V,3) fp64, d/dbary (B,aS,aS,3) fp32"""
    from oracle import render_ref as rr
    g_hi = box_down_t(g, a)
    gtex, gverts = rr.render_bwd_views(g_hi, frags, mesh["verts"], mesh["faces"], mesh["verts_uvs"], mesh["faces_uvs"], tex, R, T)
    gbary = np.stack([rr.uv_to_bary_grad(rr.shade_bwd(g_hi[b], frags[b], mesh["verts_uvs"], mesh["faces_uvs"], tex, want_uv=True)[1],
                                         frags[b][0], mesh["verts_uvs"], mesh["faces_uvs"]) for b in range(len(frags))])
    return gtex, gverts, gbary


# the shared scene of the supersampling tests: cow, two seeded views, a seeded texture and a seeded upstream gradient
CASES = [(S, T, a) for S, T in ((16, 32), (17, 37), (20, 37), (24, 32)) for a in (2, 3, 4)]
B = 2


def cameras():
    import _scenes
    return _scenes.random_cameras(B, 5)


def texture(T):
    return np.random.default_rng(T).random((T, T, 3), dtype=np.float32)


def upstream(S):
    return np.random.default_rng(100 + S).standard_normal((B, 3, S, S)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(S, T, a):
    """everything the tests compare with for one (S, T, a), computed once and never modified (read-only arrays)"""
    import _scenes
    mesh = _scenes.load_asset("cow")
    R, Tt = cameras()
    tex, g = texture(T), upstream(S)
    rgb, cov, frags = render(mesh, tex, R, Tt, S, a)
    gtex, gverts, gbary = backward(g, frags, mesh, tex, R, Tt, a)
    out = dict(mesh=mesh, R=R, T=Tt, tex=tex, g=g, rgb=rgb, cov=cov, frags=frags, gtex=gtex, gverts=gverts, gbary=gbary)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
