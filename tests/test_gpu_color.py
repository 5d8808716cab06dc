"""The colour kernels (csrc/color.hip) against their numpy restatement (tests/_colorref.py), and --preserve_color built on
them: the autograd function and the tags it carries, the moments and the colour match, the 2D loop and the scripts.

u = 2^-24 is the unit roundoff of fp32.  Bounds are derived next to the assertion that uses them; the largest error / bound
ratio is printed."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import _colorref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "2d-to-3d-style-transfer_amd")
U32 = np.uint32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    import losses as L
    import style_transfer as ST
    import utils as U_
    U_.device = ST.device = L.device = dev
    return L, ST, U_, U_.get_vgg(seed=0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().cpu().numpy().view(U32)


def _shapes():
    """(B, P): the issue's images, plus one plane of chunk + 1 and one of 2 chunk - 1 pixels of the moments kernel.  Odd P
    leaves the channel planes off 16-byte boundaries (the scalar route) and gives a tail; (2,16,16) and the chunk planes
    cross wave and workgroup borders; P > chunk reaches the second reduction stage with more than one partial per image.
    (1, 2048) and (2, 4096) are added for the float4 route (P % 4 == 0), whose workgroup owns 1024 pixels: two and four
    workgroups per image, as the renders of a run have them; P = 256 alone is one partly filled workgroup."""
    from st3d import ops
    chunk = ops.color_stats_chunk()
    return [(1, 1), (2, 15), (1, 259), (2, 256), (1, 33 * 65), (1, chunk + 1), (2, 2 * chunk - 1), (1, 2048), (2, 4096)]


def _rand(rng, B, P):
    return (rng.random((B, 3, P), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


def _affine(rng):
    return rng.standard_normal((3, 3)) * 0.7, rng.standard_normal(3) * 0.3


# ---------------------------------------------------------------------------- 1. the kernels against the restatement
def test_streaming_kernels_equal_the_restatement_bit_for_bit(dev):
    from st3d import ops
    rng = np.random.default_rng(0)
    worst = 0.0
    for B, P in _shapes():
        x, y, g = _rand(rng, B, P), _rand(rng, B, P), (rng.standard_normal((B, 3, P)) * 3).astype(np.float32)
        A, b = _affine(rng)
        dx, dy, dg = _t(x, dev), _t(y, dev), _t(g, dev)
        for name, run, want in (
                ("luma_fwd", lambda: ops.luma_fwd(dx), CR.luma_fwd(x)),
                ("luma_bwd", lambda: ops.luma_bwd(dg), CR.luma_bwd(g)),
                ("luma_recombine", lambda: ops.luma_recombine(dx, dy), CR.recombine(x, y)),
                ("color_affine", lambda: ops.color_affine(dx, A, b, clamp=False), CR.affine(x, A, b, False)),
                ("color_affine clamped", lambda: ops.color_affine(dx, A, b, clamp=True), CR.affine(x, A, b, True))):
            one, two = run(), run()
            assert np.array_equal(_bits(one), want.view(U32)), (name, B, P)
            assert np.array_equal(_bits(one), _bits(two)), (name, B, P)
        # a 4-D image is the same call
        if P == 33 * 65:
            assert np.array_equal(_bits(ops.luma_fwd(dx.reshape(B, 3, 33, 65))).reshape(B, 3, P), CR.luma_fwd(x).view(U32))
        # the adjoint identity on the device results, summed in fp64: each side is within gamma_3 (sum_c W_c |x_c|)(sum_c |g_c|)
        # per pixel of the exact bilinear form (three fp32 roundings a side, tests/test_color_ref.py), the fp64 sums of
        # n = 3 B P terms add gamma_n(2^-53) of the same
        left = float((ops.luma_fwd(dx).double() * dg.double()).sum())
        right = float((dx.double() * ops.luma_bwd(dg).double()).sum())
        w = np.array([float(v) for v in CR.W])[None, :, None]
        scale = float(np.sum(np.sum(w * np.abs(x), axis=1, dtype=np.float64) * np.sum(np.abs(g), axis=1, dtype=np.float64)))
        n = x.size
        bound = (2 * 3 * U / (1 - 3 * U) + 2 * n * 2.0 ** -53 / (1 - n * 2.0 ** -53)) * scale
        worst = max(worst, abs(left - right) / bound)
        assert abs(left - right) <= bound, (B, P, left, right, bound)
    print(f"adjoint identity on the device: largest |left - right| / bound = {worst:.3f}")


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_pixels_stay_in_their_pixel(dev, value):
    from st3d import ops
    rng = np.random.default_rng(1)
    for B, P in ((2, 15), (1, 259), (2, 256), (2, 2048)):         # (the last: the float4 route past its first workgroup)
        A, b = _affine(rng)
        for b0, c0, p0 in ((0, 0, 0), (B - 1, 2, P - 1), (0, 1, P // 2)):
            x, y = _rand(rng, B, P), _rand(rng, B, P)
            x[b0, c0, p0] = value
            dx, dy = _t(x, dev), _t(y, dev)
            outs = {"luma_fwd": ops.luma_fwd(dx), "luma_bwd": ops.luma_bwd(dx), "recombine opt": ops.luma_recombine(dx, dy),
                    "recombine orig": ops.luma_recombine(dy, dx), "affine": ops.color_affine(dx, A, b, clamp=False),
                    "affine clamped": ops.color_affine(dx, A, b, clamp=True)}
            for name, out in outs.items():
                bad = ~torch.isfinite(out).cpu().numpy()
                if name == "affine clamped" and not math.isnan(value):
                    assert not bad.any(), (name, B, P)      # +-Inf is clamped like any other value; a NaN 0 * Inf stays
                    continue                                 # in the pixel (checked below through the unclamped call)
                want = np.zeros((B, 3, P), bool)
                want[b0, :, p0] = True
                assert not (bad & ~want).any(), (name, B, P, "leaked")
                assert bad[b0, :, p0].all(), (name, B, P, "lost")          # all three outputs of the pixel see it (A is dense)
            # the clamped NaN: exactly the pixel's outputs that the unclamped call makes NaN
            if math.isnan(value):
                un = torch.isnan(outs["affine"]).cpu().numpy()
                assert np.array_equal(torch.isnan(outs["affine clamped"]).cpu().numpy(), un)


def _sum_bound(m, absum):
    """|fl(sum) - sum| <= gamma_{m-1} sum |terms| for m terms summed in fp64 in ANY fixed order (Higham, 4.4)"""
    if m <= 1:
        return 0.0
    k = (m - 1) * 2.0 ** -53
    return k / (1 - k) * absum


def test_color_stats_sums(dev):
    from st3d import color, ops
    rng = np.random.default_rng(2)
    worst = 0.0
    for B, P in _shapes():
        x = _rand(rng, B, P)
        dx = _t(x, dev)
        sparse = rng.random((B, P)) < 0.05
        sparse[0, 0] = True
        for name, mask in (("5 %", sparse), ("ones", np.ones((B, P), bool)), ("NULL", None), ("zeros", np.zeros((B, P), bool))):
            dm = None if mask is None else _t(mask.astype(np.uint8), dev)
            got = ops.color_sums(dx, dm).cpu().numpy()
            again = ops.color_sums(dx, dm).cpu().numpy()
            assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), (name, B, P)
            exact, absum = CR.moments_exact(x, mask)
            m = int(exact[0])
            assert got[0] == m == (B * P if mask is None else int(mask.sum())), (name, B, P)
            for q in range(1, 10):
                bound = _sum_bound(m, absum[q])
                err = abs(Fraction(float(got[q])) - exact[q])
                assert err <= Fraction(bound), (name, B, P, q, float(err), bound)
                if bound:
                    worst = max(worst, float(err) / bound)
            if name == "zeros":
                assert not got.any()
                with pytest.raises(ValueError, match="no pixel"):
                    color.color_stats(dx, dm)
            elif name == "5 %":
                st, want = color.color_stats(dx, dm), CR.stats(CR.moments(x, mask))
                assert st["n"] == m
                np.testing.assert_allclose(st["mean"], want["mean"], rtol=1e-12)
                np.testing.assert_allclose(st["cov"], want["cov"], rtol=1e-9, atol=1e-14)
                # a bool mask is the same call
                assert np.array_equal(ops.color_sums(dx, _t(mask, dev)).cpu().numpy(), got)
        # the same pixels as B = 2 and as B = 1 of twice the pixels: other chunk borders.  The B = 1 arrangement is held to
        # the exact sums under the same bound, and the two arrangements to each other under that one bound too
        if B == 2:
            both = np.concatenate([x[0], x[1]], axis=1)[None]
            one = ops.color_sums(_t(both, dev), None).cpu().numpy()
            two = ops.color_sums(dx, None).cpu().numpy()
            exact, absum = CR.moments_exact(x, None)
            assert one[0] == two[0] == 2 * P
            for q in range(1, 10):
                bound = _sum_bound(2 * P, absum[q])
                err = abs(Fraction(float(one[q])) - exact[q])
                assert err <= Fraction(bound), (B, P, q, float(err), bound)
                assert abs(Fraction(float(one[q])) - Fraction(float(two[q]))) <= Fraction(bound), (B, P, q)
                worst = max(worst, float(err) / bound)
    print(f"color_stats: largest |sum - exact| / bound = {worst:.3f}")
    # a NaN outside the mask does not reach the sums; inside it reaches exactly the sums its channel takes part in
    x = _rand(rng, 1, 300)
    x[0, 1, 7] = np.nan
    mask = np.ones((1, 300), np.uint8)
    mask[0, 7] = 0
    assert np.isfinite(ops.color_sums(_t(x, dev), _t(mask, dev)).cpu().numpy()).all()
    got = ops.color_sums(_t(x, dev), None).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.array([0, 0, 1, 0, 0, 1, 0, 1, 1, 0], bool))


def _fp64_slack(src, dst, got, A, n):
    """(slack_mean, slack_cov) of test_match_style_reaches_the_content_moments, as its docstring derives them"""
    eps = 2.0 ** -52
    g = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    kappa = max(np.linalg.cond(src["cov"]), np.linalg.cond(dst["cov"]))
    M2 = max(float(np.max(np.diag(st["cov"]) + np.asarray(st["mean"]) ** 2)) for st in (src, dst, got))
    slack_cov = 64 * eps * kappa * np.linalg.norm(dst["cov"]) + (3 + 6 * kappa) * g * M2
    slack_mean = (8 * eps * (np.linalg.norm(A) * np.linalg.norm(src["mean"]) + np.linalg.norm(dst["mean"]))
                  + (1 + 6 * kappa) * g * math.sqrt(M2))
    return slack_mean, slack_cov


def test_match_style_reaches_the_content_moments(dev):
    """Recolour a random style towards a random masked content, unclamped, and measure the result's moments on the device.
    y = fl(A^ x + b^), A^ = fl32(A), b^ = fl32(b) (u each), three fmaf (u each): per pixel and channel
        |y_c - (A x + b)_c| <= e_c := gamma_5 R_c,   R_c = sum_d |A_cd| |x_d| + |b_c|.
    z = A x + b has the content's mean and covariance up to fp64 effects, which make the slack:
      * the host match (tests/test_color_ref.py): 64 eps kappa ||Sigma_d||_F on the covariance, 8 eps (||A||_F ||mu_s|| +
        ||mu_d||) on the mean, kappa the larger condition number of the two covariances, computed here from the data;
      * the moments: every one of the ten sums is within g = gamma_n(2^-53) of itself relatively to its sum of absolute
        values, n the larger pixel count.  A raw second moment E[v_c v_d] is then off by at most g M2, M2 the largest
        E[v_c^2] over style, content and result, and a covariance S/n - mu mu^T by at most 3 g M2 (one for S/n, two for the
        product of the means).  This enters three times: in the measured covariance of the result (3 g M2), and in the two
        covariances the map was built from, whose perturbation the roots pass on multiplied by at most kappa (as above):
        2 x 3 g kappa M2.  For the means the same with sqrt(M2): g sqrt(M2) measured, and 2 x 3 g kappa sqrt(M2) through A and b.
      slack_cov = 64 eps kappa ||Sigma_d||_F + (3 + 6 kappa) g M2,  slack_mean = 8 eps (...) + (1 + 6 kappa) g sqrt(M2).
    Mean:        |mean(y)_c - mu_d,c| <= mean(e_c) + slack_mean.
    Covariance:  Cov(y) = Cov(z) + Cov(z, d) + Cov(d, z) + Cov(d) with d = y - z, and |Cov(a, b)| <= rms(a - mean a) rms(b):
                 |Cov(y)_cd - Sigma_d,cd| <= s_c rms(e_d) + s_d rms(e_c) + rms(e_c) rms(e_d) + slack_cov, s_c = sqrt(Sigma_d,cc)."""
    from st3d import color
    rng = np.random.default_rng(3)
    worst_m = worst_c = 0.0
    for (Bs, Ps), (Bc, Pc) in (((1, 33 * 65), (2, 256)), ((1, 259), (1, 33 * 65)), ((2, 256), (2, 15))):
        mix = np.eye(3) + 0.4 * rng.standard_normal((3, 3))
        style = np.einsum("cd,bdp->bcp", mix, rng.random((Bs, 3, Ps))).astype(np.float32)
        content = (rng.random((Bc, 3, Pc)) ** 2).astype(np.float32)
        content[:, 1] = (0.6 * content[:, 0] + 0.4 * content[:, 1]).astype(np.float32)
        mask = rng.random((Bc, Pc)) < 0.6
        mask[0, :4] = True
        d_style, d_content, d_mask = _t(style, dev), _t(content, dev), _t(mask, dev)
        out = color.match_style(d_style, d_content, d_mask, clamp=False)
        got = color.color_stats(out)
        want = CR.stats(CR.moments(content, mask))
        src = CR.stats(CR.moments(style))
        A, b = CR.match_matrix(src, want)
        g5 = 5 * U / (1 - 5 * U)
        R = np.einsum("cd,bdp->bcp", np.abs(A), np.abs(style.astype(np.float64))) + np.abs(b)[None, :, None]
        e_mean = g5 * R.mean(axis=(0, 2))
        e_rms = g5 * np.sqrt((R ** 2).mean(axis=(0, 2)))
        slack_mean, slack_cov = _fp64_slack(src, want, got, A, max(Bs * Ps, int(mask.sum())))
        s = np.sqrt(np.diag(want["cov"]))
        m_ratio = np.abs(got["mean"] - want["mean"]) / (e_mean + slack_mean)
        c_bound = np.outer(s, e_rms) + np.outer(e_rms, s) + np.outer(e_rms, e_rms) + slack_cov
        c_ratio = np.abs(got["cov"] - want["cov"]) / c_bound
        worst_m, worst_c = max(worst_m, float(m_ratio.max())), max(worst_c, float(c_ratio.max()))
        assert (m_ratio <= 1).all() and (c_ratio <= 1).all(), (m_ratio, c_ratio)
        assert got["n"] == Bs * Ps
        # the result is the public pieces, bit for bit
        A_dev, b_dev = color.match_matrix(color.color_stats(d_style), color.color_stats(d_content, d_mask))
        assert np.array_equal(_bits(out), CR.affine(style, A_dev, b_dev, False).view(U32))
    print(f"match_style: largest error / bound: mean {worst_m:.3f}, covariance {worst_c:.3f}")
    # the luminance variant: three equal planes whose mean and variance are the content luminance's
    lum = color.match_style_luminance(d_style, d_content, d_mask, clamp=False)
    assert np.array_equal(_bits(lum[:, 0]), _bits(lum[:, 1])) and np.array_equal(_bits(lum[:, 0]), _bits(lum[:, 2]))
    # the same bounds with A = k I, b = (b, b, b) on the luminance planes
    ys = CR.luma_fwd(style)
    got, want = color.color_stats(lum), CR.stats(CR.moments(CR.luma_fwd(content), mask))
    k, off = CR.luma_match(CR.stats(CR.moments(ys)), want)
    R = abs(k) * np.abs(ys[:, 0].astype(np.float64)) + abs(off)
    e_mean, e_rms, s0 = g5 * R.mean(), g5 * math.sqrt((R ** 2).mean()), math.sqrt(want["cov"][0, 0])
    # (the slack in one dimension: kappa = 1, the variances and second moments of channel 0)
    one_d = lambda st: {"mean": st["mean"][:1], "cov": st["cov"][:1, :1]}      # noqa: E731
    slack_mean, slack_cov = _fp64_slack(one_d(CR.stats(CR.moments(ys))), one_d(want), one_d(got), np.array([[k]]),
                                        max(Bs * Ps, int(mask.sum())))
    m_ratio = abs(got["mean"][0] - want["mean"][0]) / (e_mean + slack_mean)
    c_ratio = abs(got["cov"][0, 0] - want["cov"][0, 0]) / (2 * s0 * e_rms + e_rms ** 2 + slack_cov)
    print(f"match_style_luminance: error / bound: mean {m_ratio:.3f}, variance {c_ratio:.3f}")
    assert m_ratio <= 1 and c_ratio <= 1, (m_ratio, c_ratio)


def test_recombine_texture_for_the_three_carriers(dev):
    from st3d import color
    rng = np.random.default_rng(4)
    for shape in ((1, 5, 7, 3), (11, 3), (6, 2, 2, 3)):
        opt, orig = rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)
        out = color.recombine_texture(_t(opt, dev), _t(orig, dev))
        planar = lambda a: np.ascontiguousarray(a.reshape(-1, 3).T)[None]
        want = CR.recombine(planar(opt), planar(orig))[0].T.reshape(shape)
        assert out.shape == tuple(shape) and out.is_contiguous() and np.array_equal(_bits(out), want.view(U32))
        same = color.recombine_texture(_t(orig, dev), _t(orig, dev))
        assert np.array_equal(_bits(same), orig.view(U32))              # a texel that never moved keeps its bits
    a = _t(rng.random((2, 3, 4, 5), dtype=np.float32), dev)
    b = _t(rng.random((2, 3, 4, 5), dtype=np.float32), dev)
    want = CR.recombine(a.cpu().numpy().reshape(2, 3, -1), b.cpu().numpy().reshape(2, 3, -1)).reshape(2, 3, 4, 5)
    assert np.array_equal(_bits(color.recombine(a, b)), want.view(U32))
    with pytest.raises(ValueError):
        color.recombine(a, b[:1])


# ---------------------------------------------------------------------------- 2. autograd, the cache, the tags
def test_autograd_of_luma(dev):
    from st3d import color, ops
    rng = np.random.default_rng(5)
    for B, H, W in ((2, 3, 5), (1, 7, 37), (2, 16, 16)):
        x = _t(_rand(rng, B, H * W).reshape(B, 3, H, W), dev).requires_grad_(True)
        g = _t((rng.standard_normal((B, 3, H, W)) * 2).astype(np.float32), dev)
        y = color.luma(x)
        y.backward(g)
        assert np.array_equal(_bits(y), _bits(ops.luma_fwd(x.detach()))) and np.array_equal(_bits(x.grad), _bits(ops.luma_bwd(g)))
        assert not hasattr(y, "_st3d_need") and not hasattr(y, "_st3d_flat")       # no tags in, no tags out


def test_luma_cached_on_the_device(dev):
    from st3d import color, imgpyr
    color.clear_cache()
    t = torch.rand(2, 3, 64, 64, device=dev)
    y = color.luma_cached(t)
    assert color.luma_cached(t) is y and not y.requires_grad and np.array_equal(_bits(y), _bits(color.luma_fwd(t)))
    assert imgpyr.reduced_cached(color.luma_cached(t), 2) is imgpyr.reduced_cached(color.luma_cached(t), 2)      # composes
    t.add_(0.1)
    assert color.luma_cached(t) is not y
    one = torch.rand(1, 3, 8, 8, device=dev)
    e = color.luma_cached(one.expand(4, -1, -1, -1))
    assert e.stride(0) == 0 and e.shape == (4, 3, 8, 8)
    color.clear_cache()
    imgpyr.clear_cache()


def _cow_scene(dev, world, S=64, B=2):
    import _scenes as SC
    L, ST, U_, vgg = world
    a = SC.load_asset("cow")
    R, T = SC.random_cameras(B, seed=0)
    mesh0, renderer, cams = SC.device_scene(U_, dev, a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], SC.texture_at(a, S),
                                            R, T, S)
    return SC, mesh0, renderer, cams


@pytest.mark.parametrize("scales", [(1,), (1, 2)])
def test_luma_carries_the_tags_and_the_tagged_loss_is_the_untagged_one(dev, world, monkeypatch, scales):
    """the golden cow at S = 64, two views, white background: with the need / flat / epoch tags on luma(render) the loss and
    the texture gradient are, bit for bit, those of the same call with ST3D_NEED_MASK=0 ST3D_FLAT=0 ST3D_EPOCHS=0 -- and the
    tags do arrive at the plan (it is handed the coverage, the luminance of white and the epoch)."""
    from st3d import color, imgpyr
    from st3d import render as RD
    from st3d import vgg as V
    L, ST, U_, _ = world
    vgg = U_.get_vgg(seed=0)
    S, B = 64, 2
    SC, mesh0, renderer, cams = _cow_scene(dev, world, S, B)
    out = U_.setup_optimizations("texture", mesh0, 0.01)
    tex = out["texture_map"]
    with torch.no_grad():
        content, _ = U_.render_meshes(renderer, mesh0, cams)
    style = color.luma_fwd(SC.style_at(1, S).to(dev)).expand(B, -1, -1, -1)
    seen, plan_loss = [], V.PerceptualPlan.loss
    monkeypatch.setattr(V.PerceptualPlan, "loss", lambda self, *a, **k: (seen.append((self.S, k.get("need_mask"), k.get("epoch", 0),
                                                                                      k.get("flat_color"))),
                                                                         plan_loss(self, *a, **k))[1])
    kw = {} if scales == (1,) else {"scales": scales}

    def run(tagged):
        for k in ("ST3D_NEED_MASK", "ST3D_FLAT", "ST3D_EPOCHS"):
            if tagged:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, "0")
        tex.grad = None
        mesh = U_.build_mesh(out["verts_uvs"], out["faces_uvs"], tex, out["verts"], out["faces"])
        cur, cov = U_.render_meshes(renderer, mesh, cams)
        y = color.luma(cur)
        need = RD.need_of(y)
        if tagged:
            white = color.luma_of_color((1.0, 1.0, 1.0))
            assert need is not None and need is RD.need_of(cur) and torch.equal(need.bool(), cov[:, 0] > 0)
            assert RD.flat_of(y) == (white, white, white) and RD.epoch_of(y, need) != 0
            assert RD.epoch_of(y, need) == RD.epoch_of(cur, need)
            bg = y.detach()[(~need.bool())[:, None].expand(-1, 3, -1, -1)]
            assert bool((bg == white).all()) and bg.numel() > 0          # the hint is true: the background holds Y(white)
        loss = L.compute_perceptual_loss(y, color.luma_cached(content), style, vgg, **kw)
        loss.backward()
        return loss.detach().clone(), tex.grad.detach().clone(), need

    l1, g1, need = run(True)
    fine = [s for s in seen if s[0] == S][-1]
    assert fine[1] is need and fine[2] != 0 and fine[3] is not None          # what the full-resolution plan was handed
    l1b, g1b, _ = run(True)                                                  # a second step of the epoch: the kept lists
    n_seen = len(seen)
    l0, g0, _ = run(False)
    fine = [s for s in seen[n_seen:] if s[0] == S][-1]
    assert fine[1] is None and fine[2] == 0
    assert np.array_equal(_bits(l1), _bits(l0)) and np.array_equal(_bits(g1), _bits(g0))
    assert np.array_equal(_bits(l1b), _bits(l0)) and np.array_equal(_bits(g1b), _bits(g0))
    assert bool((g1 != 0).any()) and torch.isfinite(g1).all()
    color.clear_cache()
    imgpyr.clear_cache()


# ---------------------------------------------------------------------------- 3. the 2D loop
def _images(dev, B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.rand(B, 3, S, S, generator=g).to(dev) for _ in range(3))


def test_style_transfer_in_luminance_is_the_public_pieces(dev, world):
    from st3d import color, ops
    from st3d import optim as st3d_optim
    L, ST, U_, vgg = world
    B, S, steps, lr = 1, 64, 3, 0.01
    x, c, s = _images(dev, B, S, seed=11)
    plain = ST.style_transfer(x, c, s, vgg, steps=steps, lr=lr).detach().clone()
    rgb = ST.style_transfer(x, c, s, vgg, steps=steps, lr=lr, color="rgb").detach().clone()
    assert np.array_equal(_bits(plain), _bits(rgb))
    lum = ST.style_transfer(x, c, s, vgg, steps=steps, lr=lr, color="luminance").detach().clone()
    again = ST.style_transfer(x, c, s, vgg, steps=steps, lr=lr, color="luminance").detach().clone()
    assert torch.isfinite(lum).all() and np.array_equal(_bits(lum), _bits(again)) and not np.array_equal(_bits(lum), _bits(plain))
    # by hand
    plan = vgg.plan(B, S)
    plan.set_content(ops.luma_fwd(c), force=True)
    plan.set_style(ops.luma_fwd(s), B, force=True)
    img = x.clone().detach().contiguous().requires_grad_(True)
    opt = st3d_optim.Adam([img], lr=lr, reduce_grads=False)
    for _ in range(steps):
        _, g = plan.loss(ops.luma_fwd(img.detach()), 1e6, 1)
        img.grad = ops.luma_bwd(g)
        opt.step()
    assert np.array_equal(_bits(color.recombine(img, c)), _bits(lum))
    # the result carries the content's chroma: I and Q of the standard YIQ matrix, to the last rounding of the recombination
    M = torch.from_numpy(CR.YIQ).to(dev)
    iq = lambda t: torch.einsum("kc,bchw->bkhw", M, t.double())[:, 1:]
    # (tests/test_color_ref.py: u (1 + u) sum_c |M_kc| |out_c|, and sum_c |M_kc| <= 1.2 for both rows)
    assert float((iq(lum) - iq(c)).abs().max()) <= 1.25 * U * float(lum.abs().max())
    # the other terms go through the same luminance
    both = ST.style_transfer(x, c, s, vgg, steps=2, lr=lr, color="luminance", nnfm_weight=1.0, swd_weight=1.0, swd_directions=8,
                             style_scales=(1, 2)).detach()
    assert torch.isfinite(both).all() and float((iq(both) - iq(c)).abs().max()) <= 1.25 * U * float(both.abs().max())
    with pytest.raises(ValueError, match="color must be"):
        ST.style_transfer(x, c, s, vgg, steps=1, color="lab")


# ---------------------------------------------------------------------------- 4. the scripts
def _write_cow_assets(tmp, cow, golden_dir, tex_size=32):
    from PIL import Image
    from st3d import io as stio
    tex = torch.from_numpy(cow["texture_u8"][::1024 // tex_size, ::1024 // tex_size].copy()).float() / 255
    obj = os.path.join(tmp, "cow.obj")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    sty = np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]
    style = os.path.join(tmp, "style.png")
    Image.fromarray(sty).save(style)
    return obj, style


def _log(d):
    return open(os.path.join(d, "log.txt"), "rb").read()


def _losses(d):
    return [line.split("Loss ")[1] for line in _log(d).decode().splitlines()[1:]]


def _final_files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith("final.")}


def test_second_approach_preserve_color(dev, world, cow, golden_dir, tmp_path, capsys):
    import second_approach as SA
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0",
              "--save_every", "0"]
    out = lambda name: str(tmp_path / name)         # noqa: E731
    SA.main(common + ["--epochs", "2", "--output_path", out("plain")])
    said_plain = capsys.readouterr().out
    SA.main(common + ["--epochs", "2", "--output_path", out("off"), "--preserve_color", "off"])
    said_off = capsys.readouterr().out
    assert _log(out("plain")) == _log(out("off")) and len(_losses(out("plain"))) == 2
    assert _final_files(out("plain")) == _final_files(out("off")) and len(_final_files(out("plain"))) >= 2
    assert "Preserve colour" not in said_off and "Recombine" not in said_off      # nothing new is printed
    assert len(said_off.splitlines()) == len(said_plain.splitlines())
    assert not os.path.exists(os.path.join(out("off"), "style_matched.png"))

    for mode in ("match", "luminance"):
        SA.main(common + ["--epochs", "2", "--output_path", out(mode), "--preserve_color", mode])
        said = capsys.readouterr().out
        assert f"Preserve colour ({mode}): content mean (" in said and "covered pixels of 2 views; style mean (" in said
        assert os.path.exists(os.path.join(out(mode), "style_matched.png"))
        got, plain = _losses(out(mode)), _losses(out("plain"))
        print(mode, "losses", got, "plain", plain)
        assert len(got) == 2 and all(math.isfinite(float(v)) for v in got) and got[0] != plain[0]
        assert ("Recombine: " in said and "texels carry a new luminance" in said) == (mode == "luminance")
        assert len(_final_files(out(mode))) >= 2

    # vertex colours and an atlas export through the recombination too
    for name, extra in (("vertex", ["--texture_type", "vertex"]), ("atlas", ["--texture_atlas", "2"])):
        SA.main(common + ["--epochs", "1", "--output_path", out(name), "--preserve_color", "luminance"] + extra)
        said = capsys.readouterr().out
        assert "Recombine: " in said and os.path.exists(os.path.join(out(name), "final.obj"))
        assert all(math.isfinite(float(v)) for v in _losses(out(name)))

    # --fill_unseen after the recombination, --style_scales and the other style terms through the luminance
    SA.main(common + ["--epochs", "1", "--output_path", out("all"), "--preserve_color", "luminance", "--fill_unseen", "map",
                      "--style_scales", "1,2", "--nnfm_weight", "1", "--swd_weight", "1", "--swd_directions", "8",
                      "--style_mask", "object"])
    said = capsys.readouterr().out
    assert said.index("Recombine: ") < said.index("Fill: ") and all(math.isfinite(float(v)) for v in _losses(out("all")))

    # a resumed run reproduces the uninterrupted one; another mode is refused
    lum = common + ["--preserve_color", "luminance"]
    SA.main(lum + ["--epochs", "3", "--output_path", out("full"), "--checkpoint_every", "2"])
    ck = os.path.join(out("full"), "checkpoint.pt")
    assert torch.load(ck, map_location="cpu", weights_only=True)["preserve_color"] == "luminance"
    SA.main(lum + ["--epochs", "3", "--output_path", out("part"), "--resume", ck])
    assert _losses(out("part")) == _losses(out("full"))[2:] and len(_losses(out("full"))) == 3
    assert _final_files(out("part")) == _final_files(out("full"))
    with pytest.raises(ValueError, match="--preserve_color luminance, this run has off"):
        SA.main(common + ["--epochs", "3", "--output_path", out("bad"), "--resume", ck])
    with pytest.raises(ValueError, match="--preserve_color luminance, this run has match"):
        SA.main(common + ["--epochs", "3", "--output_path", out("bad"), "--resume", ck, "--preserve_color", "match"])
    with pytest.raises(SystemExit):
        SA.main(lum + ["--epochs", "1", "--output_path", out("bad"), "--optimization_target", "mesh"])
    capsys.readouterr()


def test_first_and_third_approach_preserve_color(dev, world, cow, golden_dir, tmp_path, capsys):
    import first_approach as FA
    import third_approach as TA
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0"]
    steps = ["--n_style_transfer_steps", "2", "--n_mse_steps", "2"]
    logs, said = {}, {}
    for name, extra in (("plain", []), ("off", ["--preserve_color", "off"]), ("match", ["--preserve_color", "match"]),
                        ("luminance", ["--preserve_color", "luminance"])):
        FA.main(common + steps + ["--output_path", str(tmp_path / ("fa_" + name))] + extra)
        logs[name], said[name] = _losses(str(tmp_path / ("fa_" + name))), capsys.readouterr().out
    assert logs["plain"] == logs["off"] and _final_files(str(tmp_path / "fa_plain")) == _final_files(str(tmp_path / "fa_off"))
    assert "Preserve colour" not in said["off"]
    for mode in ("match", "luminance"):
        assert f"Preserve colour ({mode})" in said[mode] and os.path.exists(str(tmp_path / ("fa_" + mode) / "style_matched.png"))
        assert len(logs[mode]) == len(logs["plain"]) > 0 and logs[mode] != logs["plain"]
        assert all(math.isfinite(float(v)) for v in logs[mode])
        assert ("Recombine: " in said[mode]) == (mode == "luminance")       # the export recombines in luminance mode only
    assert "Recombine: " not in said["off"] and "Recombine: " not in said["plain"]
    TA.main(common + ["--n_rounds", "1", "--n_style_transfer_steps", "2", "--n_mse_steps", "1", "--preserve_color", "luminance",
                      "--output_path", str(tmp_path / "ta")])
    said_ta = capsys.readouterr().out
    assert "Preserve colour (luminance)" in said_ta and "Recombine: " in said_ta
    assert all(math.isfinite(float(v)) for v in _losses(str(tmp_path / "ta")))


def _run_ranks(world_size, args, port):
    env = dict(os.environ, ST3D_DIST_BACKEND="gloo", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable]
    if world_size > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world_size}", "--master-addr", "127.0.0.1",
                "--master-port", str(port)]
    cmd += [os.path.join(PKG, "second_approach.py")] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_two_ranks_reproduce_the_single_rank_run_in_luminance(cow, golden_dir, tmp_path):
    """the view batch sharded over two ranks (gloo, both on this GPU), as tests/test_gpu_imgpyr.py runs it: 3 views in batches
    of 2.  Every rank renders all views for the moments, so both prepare the same style image without communication."""
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "3", "--batch_size", "2", "--seed", "0",
              "--epochs", "2", "--lr", "0.002", "--save_every", "0", "--preserve_color", "luminance"]
    one, two = str(tmp_path / "w1"), str(tmp_path / "w2")
    said1 = _run_ranks(1, common + ["--output_path", one], 0)
    said2 = _run_ranks(2, common + ["--output_path", two], 29643)
    line = lambda said: [ln for ln in said.splitlines() if ln.startswith("Preserve colour")]      # noqa: E731
    assert len(line(said1)) == 1 and line(said1) == line(said2)
    assert open(os.path.join(one, "style_matched.png"), "rb").read() == open(os.path.join(two, "style_matched.png"), "rb").read()
    l1, l2 = [float(v) for v in _losses(one)], [float(v) for v in _losses(two)]
    assert len(l1) == len(l2) == 2
    np.testing.assert_allclose(l2, l1, rtol=2e-3)              # summation order + Adam feedback, test_gpu_imgpyr.py's bound
