"""The numpy restatement of the colour kernels (tests/_colorref.py) checked against itself: its fma, the adjoint identity, what
the recombination keeps and what it replaces, and the colour match on synthetic moments.  No GPU.

u = 2^-24 is the unit roundoff of fp32, eps = 2^-52 the spacing of fp64.  Every bound is derived in the comment next to it,
and the largest error / bound ratio is printed."""
import math

import numpy as np

import _colorref as CR

U = 2.0 ** -24
F32, F64 = np.float32, np.float64


def _gamma(k, u=U):
    return k * u / (1 - k * u)


def test_the_emulated_fma_is_correctly_rounded_where_the_naive_form_is_not():
    """x y = 2^-24 (1 + 2^-36) lies just above the tie between 1 and 1 + 2^-23; the fp64 sum 1 + x y rounds ONTO the tie"""
    x, y, c = F32(1 + 2.0 ** -12), F32(2.0 ** -24 * (1 - 2.0 ** -12 + 2.0 ** -24)), F32(1.0)
    assert F64(x) * F64(y) == 2.0 ** -24 + 2.0 ** -60
    naive = F32(F64(x) * F64(y) + F64(c))
    assert naive == F32(1.0)                                        # double rounding: wrong
    assert CR.fma(x, y, c)[()] == F32(1 + 2.0 ** -23)               # fmaf
    assert CR.fma(x, -y, -c)[()] == -F32(1 + 2.0 ** -23)
    assert CR.fma(F32(2.0 ** -12), F32(2.0 ** -12), c)[()] == F32(1.0)     # an exact tie goes to even
    # against exact rational arithmetic on random operands
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a, b, d = (rng.standard_normal(2000).astype(F32) * F32(10.0) ** rng.integers(-3, 4, 2000).astype(F32) for _ in range(3))
    got = CR.fma(a, b, d)
    for i in range(2000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(d[i]))
        lo, hi = np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    # NaN and Inf pass through
    assert np.isnan(CR.fma(F32(np.nan), F32(1), F32(1))) and CR.fma(F32(np.inf), F32(1), F32(1)) == F32(np.inf)


def _images(seed, B=2, P=1000, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((B, 3, P), dtype=F32) * F32(scale)).astype(F32)


def test_the_transpose_is_the_adjoint_of_the_luminance():
    """<Y x, g> = <x, Y^T g>, both sides summed in fp64 from the restatement's fp32 results.
    Left: every Y has three roundings (one product, two fma), relative to sum_c W_c |x_c|: gamma_3.  Right: s has two
    roundings relative to sum_c |g_c|, W_c * s one more: gamma_3.  Per pixel each side is therefore within
    gamma_3 (sum_c W_c |x_c|)(sum_c |g_c|) of the exact bilinear form; the fp64 accumulation of n = 3 B P terms adds
    gamma_n(eps) of the same sum.  So |left - right| <= (2 gamma_3(u) + 2 gamma_n(eps)) sum_p (sum_c W_c |x_cp|)(sum_c |g_cp|)."""
    worst = 0.0
    for seed in range(4):
        x = _images(seed) - F32(0.25)
        g = (np.random.default_rng(100 + seed).standard_normal(x.shape) * 3).astype(F32)
        left = float(np.sum(CR.luma_fwd(x).astype(F64) * g.astype(F64)))
        right = float(np.sum(x.astype(F64) * CR.luma_bwd(g).astype(F64)))
        w = np.array([float(v) for v in CR.W])[None, :, None]
        scale = float(np.sum(np.sum(w * np.abs(x), axis=1, dtype=F64) * np.sum(np.abs(g), axis=1, dtype=F64)))
        bound = (2 * _gamma(3) + 2 * _gamma(x.size, 2.0 ** -53)) * scale
        worst = max(worst, abs(left - right) / bound)
        assert abs(left - right) <= bound, (seed, left, right, bound)
    print(f"adjoint identity: largest |left - right| / bound = {worst:.3f}")


def test_recombine_keeps_the_chroma_and_takes_the_luminance():
    """out_c = fl(orig_c + d), d = fl(Y^(opt) - Y^(orig)), Y^ the fp32 luminance; checked with the standard YIQ matrix M in
    fp64 (row 0 = (0.299, 0.587, 0.114), rows 1 and 2 sum to 0).
    I and Q: out_c - orig_c = d + r_c with |r_c| <= u |orig_c + d| <= u (1 + u) |out_c| -- the common d cancels against the
      zero row sum, only the LAST rounding is left: |(M out)_k - (M orig)_k| <= u (1 + u) sum_c |M_kc| |out_c|
      + |sum_c M_kc| |d| (the row sum as fp64 holds it) + 8 eps sum_c |M_kc| (|out_c| + |orig_c|) for the two fp64 products.
    Y: Y^(x) differs from (M x)_0 by at most gamma_4 sum_c W_c |x_c| (three roundings, and W_c as fp32 is within u of M_0c);
      so |d - D| <= gamma_4 (S(opt) + S(orig)) + u |d| with D = (M opt)_0 - (M orig)_0 and S(x) = sum_c W_c |x_c|, and
      (M out)_0 - (M opt)_0 = sum_c M_0c (d - D + r_c) + (sum_c M_0c - 1) D:
      <= (gamma_4 (S(opt) + S(orig)) + u |d|) + u (1 + u) sum_c M_0c |out_c| + 4 eps |D| + 8 eps (S(out) + S(opt))."""
    M, eps = CR.YIQ, 2.0 ** -52
    worst = {"Y": 0.0, "I": 0.0, "Q": 0.0}
    for seed in range(4):
        opt, orig = _images(seed, scale=1.5) - F32(0.2), _images(50 + seed)
        out = CR.recombine(opt, orig)
        d = (CR.luma_plane(opt) - CR.luma_plane(orig)).astype(F64)
        yiq = lambda x: np.einsum("kc,bcp->bkp", M, x.astype(F64))
        S = lambda x: np.einsum("c,bcp->bp", np.abs(M[0]), np.abs(x.astype(F64)))
        o, g, r = yiq(out), yiq(orig), yiq(opt)
        for k, name in ((1, "I"), (2, "Q")):
            absrow = np.einsum("c,bcp->bp", np.abs(M[k]), np.abs(out.astype(F64)))
            absrow2 = np.einsum("c,bcp->bp", np.abs(M[k]), np.abs(orig.astype(F64)))
            bound = U * (1 + U) * absrow + abs(M[k].sum()) * np.abs(d) + 8 * eps * (absrow + absrow2)
            ratio = np.abs(o[:, k] - g[:, k]) / bound
            worst[name] = max(worst[name], float(ratio.max()))
        D = r[:, 0] - g[:, 0]
        bound = (_gamma(4) * (S(opt) + S(orig)) + U * np.abs(d)) + U * (1 + U) * S(out) + 4 * eps * np.abs(D) \
            + 8 * eps * (S(out) + S(opt))
        worst["Y"] = max(worst["Y"], float((np.abs(o[:, 0] - r[:, 0]) / bound).max()))
    print("recombine: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # a pixel that did not move keeps its bits: d = 0
    same = _images(9)
    assert np.array_equal(CR.recombine(same, same).view(np.uint32), same.view(np.uint32))


def _spd(rng, cond):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    w = np.array([1.0, math.sqrt(cond), cond]) * rng.uniform(0.01, 0.2)
    return (q * w) @ q.T


def test_match_matrix_maps_the_moments():
    """A Sigma_s A^T = Sigma_d and A mu_s + b = mu_d on covariances of condition number <= 100 (the floor is inactive).
    eigh is backward stable: each root is that of a matrix within c eps ||Sigma|| of the given one; the inverse square root
    amplifies a relative perturbation of Sigma_s by at most kappa_s, the square root of Sigma_d by at most kappa_d^(1/2)
    (<= kappa_d), and the five 3 x 3 products (two to form each root, one for A) and the two of the check each add 3 eps
    relative in norm.  With kappa = max(kappa_s, kappa_d) that is ||A Sigma_s A^T - Sigma_d||_F <= C eps kappa ||Sigma_d||_F,
    C = 2 (roots) x 8 (c of a 3 x 3 eigh, generously) + 7 x 3 (products) -> C = 64 taken.
    The mean: b = fl(mu_d - fl(A mu_s)), checked as fl(fl(A mu_s) + b): at most 3 + 1 + 1 roundings relative to
    ||A|| ||mu_s|| + ||mu_d||: 8 eps (||A||_F ||mu_s|| + ||mu_d||)."""
    rng = np.random.default_rng(5)
    eps, worst_c, worst_m = 2.0 ** -52, 0.0, 0.0
    for cond_s, cond_d in ((1, 1), (100, 1), (1, 100), (100, 100), (10, 37)):
        for _ in range(20):
            src = {"mean": rng.random(3), "cov": _spd(rng, cond_s)}
            dst = {"mean": rng.random(3), "cov": _spd(rng, cond_d)}
            A, b = CR.match_matrix(src, dst)
            kappa = max(np.linalg.cond(src["cov"]), np.linalg.cond(dst["cov"]))
            err = np.linalg.norm(A @ src["cov"] @ A.T - dst["cov"])
            bound = 64 * eps * kappa * np.linalg.norm(dst["cov"])
            worst_c = max(worst_c, err / bound)
            merr = np.linalg.norm(A @ src["mean"] + b - dst["mean"])
            mbound = 8 * eps * (np.linalg.norm(A) * np.linalg.norm(src["mean"]) + np.linalg.norm(dst["mean"]))
            worst_m = max(worst_m, merr / mbound)
    print(f"match_matrix: largest error / bound: covariance {worst_c:.3f}, mean {worst_m:.3f}")
    assert worst_c <= 1.0 and worst_m <= 1.0


def test_rank_deficient_sources_give_a_finite_map_through_the_floor():
    rng = np.random.default_rng(6)
    dst = {"mean": rng.random(3), "cov": _spd(rng, 10)}
    flat = {"mean": np.full(3, 0.5), "cov": np.zeros((3, 3))}                       # a flat image
    grey = {"mean": np.full(3, 0.4), "cov": np.full((3, 3), 0.02)}                  # three equal channels: rank 1
    for src in (flat, grey):
        A, b = CR.match_matrix(src, dst)
        assert np.isfinite(A).all() and np.isfinite(b).all()
        # ||A||_2 <= ||Sigma_d^(1/2)|| ||Sigma_s^(-1/2)|| <= sqrt(lambda_max(Sigma_d) / floor)
        assert np.abs(A).max() <= math.sqrt(np.linalg.eigvalsh(dst["cov"]).max() / CR.EIG_FLOOR) * (1 + 1e-9)
        np.testing.assert_allclose(A @ src["mean"] + b, dst["mean"], rtol=0, atol=1e-9)
    # luma_match: the one-dimensional case, and its floor
    k, b = CR.luma_match({"mean": [0.3] * 3, "cov": np.full((3, 3), 0.04)}, {"mean": [0.6] * 3, "cov": np.full((3, 3), 0.01)})
    assert abs(k - 0.5) <= 4 * 2.0 ** -52 and abs(b - (0.6 - k * 0.3)) <= 2.0 ** -52
    k, b = CR.luma_match({"mean": [0.3] * 3, "cov": np.zeros((3, 3))}, {"mean": [0.6] * 3, "cov": np.full((3, 3), 0.01)})
    assert math.isfinite(k) and abs(k - 0.1 / math.sqrt(CR.EIG_FLOOR)) <= 1e-9 * k and math.isfinite(b)


def test_moments_and_stats():
    x = _images(7, B=2, P=300)
    mask = np.random.default_rng(8).random((2, 300)) < 0.3
    exact, absum = CR.moments_exact(x, mask)
    rounded = CR.moments(x, mask)
    assert int(exact[0]) == int(mask.sum())
    for q in range(10):
        assert abs(float(exact[q]) - rounded[q]) <= 2.0 ** -52 * absum[q]
    st = CR.stats(rounded)
    sel = x.astype(F64).transpose(0, 2, 1)[mask]
    np.testing.assert_allclose(st["mean"], sel.mean(0), rtol=1e-12)
    np.testing.assert_allclose(st["cov"], np.cov(sel.T, bias=True), rtol=1e-9, atol=1e-15)
