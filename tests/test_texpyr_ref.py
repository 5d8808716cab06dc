"""The fp64 restatement of the texture pyramid (tests/_texpyr_ref.py) pinned to torch: synthesis to F.interpolate, the
gather adjoint to autograd of the synthesis; block offsets and sizes; the coverage experiment of DESIGN 7 (a pyramid moves
every texel of the map where the plain leaf moves under half of them); and three mutants that must be caught.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _scenes
import _texpyr_ref as TP

SHAPES = [(8, 3), (24, 3), (160, 5)]


def _interp_synth(params, T, L):
    sd = TP.sides(T, L)
    off = TP.offsets(sd)
    lv = [params[off[l]:off[l + 1]].view(sd[l], sd[l], 3) for l in range(len(sd))]
    acc = lv[-1]
    for l in range(len(sd) - 2, -1, -1):
        up = F.interpolate(acc.permute(2, 0, 1)[None], scale_factor=2, mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        acc = lv[l] + up
    return acc


def _pins(T, L, mutant=None):
    """max |restatement - torch| of the synthesis and of the adjoint at (T, L)."""
    g = torch.Generator().manual_seed(T * 31 + L)
    params = torch.randn(TP.numel(T, L), generator=g, dtype=torch.float64)
    gt = torch.randn(T, T, 3, generator=g, dtype=torch.float64)
    want = _interp_synth(params, T, L)
    got, _ = TP.synth(params, T, L, mutant)
    p = params.clone().requires_grad_(True)
    (_interp_synth(p, T, L) * gt).sum().backward()
    return float((got - want).abs().max()), float((TP.adjoint(gt, T, L, mutant) - p.grad).abs().max())


@pytest.mark.parametrize("T,L", SHAPES)
def test_restatement_is_interpolate_and_its_autograd(T, L):
    fwd, bwd = _pins(T, L)
    assert fwd <= 1e-13 and bwd <= 1e-13, (fwd, bwd)


@pytest.mark.parametrize("mutant", ["swap_odd_even", "no_clamp", "offset_off_by_one_block"])
def test_mutants_are_caught(mutant):
    fwd, bwd = _pins(24, 3, mutant)
    assert fwd > 1e-3 and bwd > 1e-3, (mutant, fwd, bwd)


def test_sides_offsets_and_numel():
    assert TP.sides(512, 0) == [512, 256, 128, 64, 32, 16, 8, 4]
    assert TP.sides(768, 0) == [768, 384, 192, 96, 48, 24, 12, 6]
    assert TP.sides(192, 0) == [192, 96, 48, 24, 12, 6]
    assert TP.sides(64, 0) == [64, 32, 16, 8, 4]
    assert TP.sides(6, 0) == [6] and TP.sides(7, 0) == [7] and TP.sides(8, 0) == [8, 4]
    assert TP.sides(24, 3) == [24, 12, 6] and TP.sides(8, 3) == [8, 4, 2] and TP.sides(5, 1) == [5]
    assert TP.offsets([24, 12, 6]) == [0, 1728, 2160, 2268]            # 108 floats: the last block is 4-byte aligned only
    assert TP.numel(160, 5) == 3 * (160 ** 2 + 80 ** 2 + 40 ** 2 + 20 ** 2 + 10 ** 2)
    for T, L in ((8, 4), (24, 5), (10, 3), (0, 1), (8, -1)):       # coarsest side 1; not divisible; odd half; no side
        with pytest.raises(ValueError):
            TP.sides(T, L)


def test_initialisation_reproduces_the_map_exactly():
    T, L = 24, 3
    tex = torch.rand(T, T, 3, dtype=torch.float64)
    params = torch.zeros(TP.numel(T, L), dtype=torch.float64)
    params[:3 * T * T] = tex.reshape(-1)
    assert torch.equal(TP.synth(params, T, L)[0], tex)


@pytest.mark.parametrize("name,plain", [("cow", 0.490), ("bob", 0.381)])
def test_a_pyramid_moves_every_texel_where_the_plain_leaf_moves_half(name, plain):
    """S = T = 64, 4 random views (seed 0), a random image gradient (seed 1), one sign step per level (Adam's first step)."""
    from oracle import render_ref as RR
    S = T = 64
    a = _scenes.load_asset(name)
    tex = _scenes.texture_at(a, T)
    R, Tt = _scenes.random_cameras(4, 0)
    _, _, frags = RR.render_views(a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], tex, R, Tt, S)
    gimg = torch.randn(4, 3, S, S, generator=torch.Generator().manual_seed(1)).numpy()
    g = np.zeros((T, T, 3), np.float64)
    for b in range(4):
        RR.shade_bwd(gimg[b], frags[b], a["verts_uvs"], a["faces_uvs"], tex, g)
    g = torch.from_numpy(g)
    leaf = TP.sign_step_coverage(g, T, 1)
    pyr = TP.sign_step_coverage(g, T, 0)
    print(f"{name}: plain leaf moves {leaf:.4f} of the texels, the 5-level pyramid {pyr:.4f}")
    assert leaf <= 0.55 and abs(leaf - plain) <= 0.02
    assert pyr >= 0.99
