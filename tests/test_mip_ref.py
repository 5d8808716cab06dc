"""The numpy restatement of mip-mapped sampling (tests/_mipref.py) against what it restates: the CPU oracle at lambda == 0,
its own adjoint identity, one-pixel finite differences of the oracle's uv for the analytic level of detail, and central
differences for its gradients.  No GPU."""
import numpy as np
import pytest

import _mipref as M


@pytest.mark.parametrize("S,T,L", [(16, 32, 3), (17, 48, 3), (24, 64, 6)])
def test_lambda_zero_is_the_oracle_exactly(S, T, L):
    from oracle import render_ref as rr
    sc = M.oracle_case(S, T)
    mesh, g = sc["mesh"], M.upstream(S)
    pyr = M.pack(M.build(sc["tex"], L))
    for b in range(M.B):
        frag = sc["frags"][b]
        lam = np.zeros((S, S), np.float32)
        rgb, mask = M.shade_fwd(frag, mesh["verts_uvs"], mesh["faces_uvs"], pyr, T, L, lam, np.float32)
        ref_rgb, ref_mask = rr.shade_fwd(frag, mesh["verts_uvs"], mesh["faces_uvs"], sc["tex"])
        assert rgb.dtype == np.float32 and np.array_equal(rgb, ref_rgb) and np.array_equal(mask, ref_mask)
        gpyr, guv = M.shade_bwd(g[b], frag, mesh["verts_uvs"], mesh["faces_uvs"], pyr, T, L, lam, np.float32)
        ref_gtex, ref_guv = rr.shade_bwd(g[b], frag, mesh["verts_uvs"], mesh["faces_uvs"], sc["tex"], want_uv=True)
        assert np.array_equal(gpyr[:3 * T * T].reshape(T, T, 3), ref_gtex)
        assert not gpyr[3 * T * T:].any()
        assert np.array_equal(guv, ref_guv)
        assert (frag[0] >= 0).sum() > 50


@pytest.mark.parametrize("T,L", [(6, 2), (40, 4), (48, 3), (64, 6)])
def test_adjoint_identity_in_fp64(T, L):
    rng = np.random.default_rng(T + L)
    x = rng.standard_normal((T, T, 3))
    y = [rng.standard_normal((T >> l, T >> l, 3)) for l in range(L)]
    lhs = sum(float((a * b).sum()) for a, b in zip(M.build(x, L, np.float64), y))
    rhs = float((x * M.adjoint(y, np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    assert M.numel(T, L) == 3 * sum((T >> l) ** 2 for l in range(L)) and M.numel(T, L + 8) == 0


def test_chain_is_the_ordered_fp32_mean():
    tex = M.texture(6)
    l1 = M.build(tex, 2)[1]
    assert l1.dtype == np.float32 and l1.shape == (3, 3, 3)
    a, b, c, d = tex[0, 2], tex[0, 3], tex[1, 2], tex[1, 3]
    assert np.array_equal(l1[0, 1], ((a + b) + (c + d)) * np.float32(0.25))
    assert M.max_levels(64) == 6 and M.max_levels(48) == 5 and M.max_levels(40) == 4 and M.max_levels(37) == 1
    assert M.max_levels(6) == 2 and M.max_levels(1024) == 10


def test_analytic_lod_against_one_pixel_differences():
    """lambda from the face's projected vertices against log2 of the one-pixel secant of the oracle's own uv, on pixels whose
    right and lower neighbour show the same face (S = 96, T = 1024): the secant-tangent difference, <= 0.1 (measured 0.037)"""
    S, T = 96, 1024
    L = M.max_levels(T)
    sc = M.oracle_case(S, T)
    mesh = sc["mesh"]
    worst, count = 0.0, 0
    for b in range(M.B):
        p2f, _, bary, _ = sc["frags"][b]
        lam = M.lod(sc["frags"][b], sc["ndc"][b], mesh["faces"], mesh["verts_uvs"], mesh["faces_uvs"], T, L)
        f = np.where(p2f >= 0, p2f, 0)
        uv = (bary.astype(np.float64)[..., None] * mesh["verts_uvs"].astype(np.float64)[mesh["faces_uvs"][f]]).sum(2)
        same = (p2f[:-1, :-1] >= 0) & (p2f[:-1, :-1] == p2f[:-1, 1:]) & (p2f[:-1, :-1] == p2f[1:, :-1])
        dx = np.hypot(*np.moveaxis(uv[:-1, 1:] - uv[:-1, :-1], -1, 0)) * (T - 1)
        dy = np.hypot(*np.moveaxis(uv[1:, :-1] - uv[:-1, :-1], -1, 0)) * (T - 1)
        rho = np.maximum(dx, dy)
        ok = same & (rho > 1) & (lam[:-1, :-1] > 0) & (lam[:-1, :-1] < L - 1)
        worst = max(worst, float(np.abs(np.log2(rho[ok]) - lam[:-1, :-1][ok]).max()))
        count += int(ok.sum())
    print(f"lod vs one-pixel differences: {count} pixels, worst {worst:.4f}")
    assert count >= 100
    assert worst <= 0.1


def _points(T, L, n, rng):
    """(u, v, lambda) away from the texel boundaries of both levels of every pair and from the border clamp"""
    u, v = rng.uniform(0.05, 0.95, 4000), rng.uniform(0.05, 0.95, 4000)
    lam = rng.uniform(0.0, L - 1.0, 4000)
    lam[::7] = np.floor(lam[::7])                          # whole levels: one level is read
    lam[::11] = L - 1.0
    keep = np.ones(4000, bool)
    for l in range(L):
        for c in (u, v):
            j = (c * (T - 1) + 0.5) / (1 << l) - 0.5
            fr = j - np.floor(j)
            keep &= (fr > 0.02) & (fr < 0.98) & (j > 0.05) & (j < (T >> l) - 1.05)
    idx = np.flatnonzero(keep)[:n]
    assert idx.size >= n // 2
    return u[idx], v[idx], lam[idx]


@pytest.mark.parametrize("T,L", [(16, 4), (24, 3)])
def test_gradients_against_central_differences(T, L):
    rng = np.random.default_rng(7 * T + L)
    u, v, lam = _points(T, L, 40, rng)
    tex = rng.standard_normal((T, T, 3))
    w = rng.standard_normal((u.size, 3))
    assert ((lam > 0) & (lam != np.floor(lam))).sum() >= 10 and (lam == np.floor(lam)).sum() >= 3

    def loss(tex_, u_, v_):
        return float((w * M.sample(u_, v_, M.pack(M.build(tex_, L, np.float64)), T, L, lam, np.float64)).sum())

    gpyr, gu, gv = M.sample_bwd(w, u, v, M.pack(M.build(tex, L, np.float64)), T, L, lam, np.float64)
    gtex = M.fold(gpyr, T, L)
    fd = np.zeros_like(tex)
    for i in np.ndindex(*tex.shape):                       # the sample is linear in the texture: h need not be small
        e = np.zeros_like(tex)
        e[i] = 0.5
        fd[i] = loss(tex + e, u, v) - loss(tex - e, u, v)
    assert np.abs(fd - gtex).max() <= 1e-10 * max(np.abs(gtex).max(), 1.0)
    assert (np.abs(gtex) > 0).mean() > 0.2
    h = 1e-6
    for k in range(u.size):                                # piecewise bilinear and away from the kinks: linear in u at fixed v
        e = np.zeros_like(u)
        e[k] = h
        fu = (loss(tex, u + e, v) - loss(tex, u - e, v)) / (2 * h)
        fv = (loss(tex, u, v + e) - loss(tex, u, v - e)) / (2 * h)
        assert abs(fu - gu[k]) <= 1e-6 * max(abs(gu[k]), 1.0) and abs(fv - gv[k]) <= 1e-6 * max(abs(gv[k]), 1.0)
    assert np.abs(gu).max() > 0.1 and np.abs(gv).max() > 0.1
