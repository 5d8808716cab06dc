"""The numpy restatement of per-vertex colours (tests/_vcolref.py) checked on the CPU: at a glance, against fp64 autograd of an
independent torch restatement, and pinned to the C oracle (oracle/raster_ref.c) through a scene on which the UV path and
the vertex-colour path are the same function.  No GPU."""
import numpy as np
import pytest
import torch

import _vcolref as VC

# the largest |oracle shade_fwd - restatement| over the three (S, T) below, measured on the CPU oracle: the UV route
# interpolates uv, scales it to texels and blends four taps, the vertex-colour route interpolates three colours -- a few fp32
# roundings of values below 1 apart.  The bar is 4 x the measured value and never above the project's shaded-RGB bar.
PIN_MEASURED = 1.192e-7
PIN_BAR = min(4 * PIN_MEASURED, 2e-6)


@pytest.mark.parametrize("S", VC.SIDES)
def test_uncovered_is_white_and_one_colour_renders_itself(S):
    frags, _ = VC.oracle_fragments(S)
    m = VC.cow()
    V = m["verts"].shape[0]
    one = np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (V, 1))
    for frag in frags:
        cov = frag[0] >= 0
        assert 40 <= cov.sum() < S * S
        for dt in (np.float32, np.float64):
            rgb, mask = VC.shade_fwd(frag, m["faces"], one, dt)
            assert rgb.dtype == dt and rgb.shape == (3, S, S) and mask.shape == (1, S, S)
            assert (rgb[:, ~cov] == 1).all() and (mask[0, ~cov] == 0).all() and (mask[0, cov] == 1).all()
            err = np.abs(rgb[:, cov] - one[0][:, None].astype(np.float64)).max()
            assert err <= 1e-6, err


def _torch_forward(frag, faces, C, bary):
    """an independent fp64 statement of the forward: gather + einsum, the blend written from PyTorch3D's softmax_rgb_blend
    at K = 1 (sigma = gamma = 1e-4, white background, znear 1, zfar 100); C (V,3) and bary (S,S,3) are torch leaves"""
    p2f, zbuf, dists = (torch.from_numpy(np.array(a)) for a in (frag[0], frag[1], frag[3]))
    cov = p2f >= 0
    tri = C[torch.from_numpy(np.asarray(faces)).long()[p2f.clamp_min(0).long()]]       # (S,S,3 corners,3 channels)
    texel = torch.einsum("yxi,yxic->yxc", bary, tri)
    prob = torch.sigmoid(-dists.double() / 1e-4) * cov
    z_inv = (100.0 - zbuf.double()) / 99.0 * cov
    z_max = z_inv.clamp_min(1e-10)
    w = prob * torch.exp((z_inv - z_max) / 1e-4)
    delta = torch.exp((1e-10 - z_max) / 1e-4).clamp_min(1e-10)
    rgb = (w[..., None] * texel + delta[..., None]) / (w + delta)[..., None]
    return torch.where(cov[..., None], rgb, torch.ones_like(rgb)).permute(2, 0, 1)


@pytest.mark.parametrize("S", VC.SIDES)
def test_backward_is_fp64_autograd_of_an_independent_forward(S):
    frags, _ = VC.oracle_fragments(S)
    m = VC.cow()
    col = VC.colours(m["verts"].shape[0]).astype(np.float64)
    g = VC.upstream(S).astype(np.float64)
    for b, frag in enumerate(frags):
        C = torch.from_numpy(col).requires_grad_(True)
        bary = torch.from_numpy(np.array(frag[2])).double().requires_grad_(True)
        out = _torch_forward(frag, m["faces"], C, bary)
        ref_rgb, _ = VC.shade_fwd(frag, m["faces"], col, np.float64)
        np.testing.assert_allclose(out.detach().numpy(), ref_rgb, rtol=1e-12, atol=1e-14)
        (out * torch.from_numpy(g[b])).sum().backward()
        gcol, gbary = VC.shade_bwd(g[b], frag, m["faces"], col, np.float64)
        want_c, want_b = C.grad.numpy(), bary.grad.numpy()
        assert np.abs(want_c).max() > 0 and np.abs(want_b).max() > 0
        assert np.abs(gcol - want_c).max() <= 1e-12 * np.abs(want_c).max()
        assert np.abs(gbary - want_b).max() <= 1e-12 * np.abs(want_b).max()
        assert not gbary[frag[0] < 0].any()


def test_fp32_restatement_is_close_to_fp64():
    """the rounding of the fp32 evaluation, for the record of the GPU bars (rgb 2e-6, gradient 1e-5 of its max)"""
    S = 24
    frags, _ = VC.oracle_fragments(S)
    m = VC.cow()
    col, g = VC.colours(m["verts"].shape[0]), VC.upstream(S)
    g32, g64 = np.zeros(col.shape), np.zeros(col.shape)
    for b, frag in enumerate(frags):
        a, _ = VC.shade_fwd(frag, m["faces"], col, np.float32)
        c, _ = VC.shade_fwd(frag, m["faces"], col, np.float64)
        assert np.abs(a - c).max() <= 5e-7
        VC.shade_bwd(g[b], frag, m["faces"], col, np.float32, g32)
        VC.shade_bwd(g[b], frag, m["faces"], col, np.float64, g64)
    assert np.abs(g32 - g64).max() <= 2e-6 * np.abs(g64).max()


def test_restatement_is_pinned_to_the_c_oracle():
    """cow with per-vertex UVs (faces_uvs = faces), a texture affine in (u, v) per channel, colours = the same function at
    every vertex's UV: sum_i b_i ramp(uv_i) = ramp(sum_i b_i uv_i), so the oracle's UV shade_fwd is the vertex-colour forward"""
    from oracle import render_ref as rr
    m = VC.cow()
    worst = 0.0
    for S, T in ((16, 32), (17, 48), (24, 64)):
        uv, tex, col = VC.ramp_scene(T)
        frags, _ = VC.oracle_fragments(S)
        for frag in frags:
            want, want_mask = rr.shade_fwd(frag, uv, m["faces"], tex)
            got, mask = VC.shade_fwd(frag, m["faces"], col, np.float32)
            np.testing.assert_array_equal(mask, want_mask)
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"largest |oracle - restatement| = {worst:.3e} (bar {PIN_BAR:.2e})")
    assert worst <= PIN_BAR, worst
