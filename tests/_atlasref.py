"""The per-face texel atlas (TexturesAtlas) restated in numpy: the texel of a fragment, the forward and its
backward, and the scenes the CPU and GPU tests share.  `dt` is the number format of the blend (np.float64 states the
definitions and checks the gradients, np.float32 rounds every step in the kernels' order, as in tests/_vcolref.py, whose
blend this file uses); the texel index is fp32 whatever `dt`: the barycentrics are the rasteriser's fp32 values and the
index is part of the contract.

Texel of a fragment (face f, barycentrics b0, b1 as rasterised, fp32, in this order, products rounded before sums):
    t0 = b0 R;  t0 = t0 > 0 ? t0 : 0;  t0 = t0 < R-1 ? t0 : R-1;  wx = (int) t0          (NaN -> 0)
    t1 = b1 R;  the same;                                          wy = (int) t1
    s = (b0 + b1) R;  below = (s - (float)(wx + wy)) <= 1;  if not below: wx = R-1-wx, wy = R-1-wy
    texel = atlas[f][wy][wx]
Forward, per covered pixel:  rgb_c = (wnum texel_c + delta 1.0) / denom,  mask = (1 - (1 - prob)) > 0; uncovered pixels are
white with mask 0.  Backward, with k = wnum / denom:  datlas[f][wy][wx][c] += g_c k, one deposit per covered pixel; nothing
towards the barycentrics."""
import numpy as np

import _vcolref as VC

F32, F64 = np.float32, np.float64
B, SIDES = VC.B, VC.SIDES
cow, cameras, upstream, two_triangles = VC.cow, VC.cameras, VC.upstream, VC.two_triangles


def texel_index(b0, b1, R):
    """-> (wy, wx) int64 arrays; b0, b1 are taken as fp32"""
    b0, b1 = np.asarray(b0, F32), np.asarray(b1, F32)
    fr, top = F32(R), F32(R - 1)
    with np.errstate(all="ignore"):
        def clamp(b):
            t = (b * fr).astype(F32)
            t = np.where(t > 0, t, F32(0))                  # a NaN fails the comparison
            return np.where(t < top, t, top).astype(F32)
        wx, wy = clamp(b0).astype(np.int64), clamp(b1).astype(np.int64)       # values in [0, R-1]: the conversion truncates
        s = ((b0 + b1).astype(F32) * fr).astype(F32)
        below = (s - (wx + wy).astype(F32)).astype(F32) <= F32(1)
    wx = np.where(below, wx, R - 1 - wx)
    wy = np.where(below, wy, R - 1 - wy)
    return wy, wx


def texel_centres(R):
    """the centre barycentrics of every texel, two (R,R) fp64 arrays indexed [y][x] (make_material_atlas's)"""
    y, x = np.meshgrid(np.arange(R, dtype=F64), np.arange(R, dtype=F64), indexing="ij")
    below = x + y < R
    b0 = np.where(below, x + 1.0 / 3.0, R - 1 - x + 2.0 / 3.0) / R
    b1 = np.where(below, y + 1.0 / 3.0, R - 1 - y + 2.0 / 3.0) / R
    return b0, b1


def _gather(frag, R):
    p2f, _, bary, _ = frag
    cov = p2f >= 0
    b = np.asarray(bary, F32)[cov]
    wy, wx = texel_index(b[:, 0], b[:, 1], R)
    return cov, p2f[cov].astype(np.int64), wy, wx


def shade_fwd(frag, atlas, dt=F64):
    """one view -> rgb (3,S,S), mask (1,S,S) in dt"""
    p2f, zbuf, _, dists = frag
    S, R = p2f.shape[0], atlas.shape[1]
    cov, f, wy, wx = _gather(frag, R)
    t = np.asarray(atlas, dt)[f, wy, wx]                           # (n,3)
    prob, wnum, delta, denom = VC.blend(dists[cov], zbuf[cov], dt)
    rgb = np.ones((3, S, S), dt)
    rgb[:, cov] = (((wnum[:, None] * t).astype(dt) + (delta[:, None] * dt(1)).astype(dt)).astype(dt) / denom[:, None]).astype(dt).T
    mask = np.zeros((1, S, S), dt)
    mask[0, cov] = ((dt(1) - (dt(1) - prob).astype(dt)) > 0).astype(dt)
    return rgb, mask


def shade_bwd(grad_rgb, frag, R, n_faces, dt=F64, gatlas=None):
    """one view: grad_rgb (3,S,S) -> gatlas (F,R,R,3) fp64, ACCUMULATED when given.  Every deposit is rounded to dt; the
    sums over pixels are fp64."""
    p2f, zbuf, _, dists = frag
    if gatlas is None:
        gatlas = np.zeros((n_faces, R, R, 3), F64)
    cov, f, wy, wx = _gather(frag, R)
    _, wnum, _, denom = VC.blend(dists[cov], zbuf[cov], dt)
    k = (wnum / denom).astype(dt)
    gk = (np.asarray(grad_rgb, dt)[:, cov].T * k[:, None]).astype(dt)                  # (n,3)
    np.add.at(gatlas, (f[:, None], wy[:, None], wx[:, None], np.arange(3)[None, :]), gk.astype(F64))
    return gatlas


def atlas(n_faces, R, seed=0):
    return np.random.default_rng(3000 + 7 * R + seed).random((n_faces, R, R, 3), dtype=np.float32)
