"""The texture scatter's tiles (csrc/shade.hip: shade_bwd_kernel): empty tiles leave early, the others sum per texel in a
key table plus compact entries.  The scene (tests/_scatter_scene.py) has an empty view, a view with one covered pixel in a
tile corner and a fully covered view, at S = 40 (ragged last tile); texture sides 4 (every deposit on a handful of
texels), 64 and 1024 (all 4 x 256 corners of a tile distinct: the table's worst case).

Fixed point (the default): integer sums are order-free, so the texture gradient is the same twice and equal bit for bit to
tests/golden/scatter_tiles_parent.npz -- the non-zero texels (and d/d bary entries) recorded on the GPU from the build
before the table was split.  Float atomics: against the fp64 CPU oracle at 1e-5 of its max, the bound of
test_gpu_kernels.py::test_shade_fwd_bwd_match_oracle.  Per-pixel outputs of uncovered pixels are exactly zero, with
torch.empty handing out NaN-filled memory.

The variants (tests/_scatter_scene.py::variants): the same scene through the other kernels that share the K = 1 arithmetic
(csrc/shadek1.h) and the tile table (csrc/tilebins.h) -- the forward kernels, the supersampled, lit, mip-mapped and
per-vertex-colour backward and the soft backward at K = 1, all in fixed point -- twice the same bits, and the bits of
tests/golden/scatter_variants_parent.npz, recorded by tools/record_scatter_parent.py on a build of the commit before the
copies were folded together.  That file holds a SHA-256 and the non-zero count per output, not the values: stored like
the plain case's fixture they are 119 686 values and 587 KB compressed, two and a half times that fixture."""
import os

import numpy as np
import pytest
import torch

import _scatter_scene as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


@pytest.fixture(scope="module")
def scene(dev):
    frag_np = sc.fragments()
    return {"frag_np": frag_np, "frag": tuple(torch.from_numpy(a).to(dev) for a in frag_np), "g_np": sc.grad_rgb(),
            "g": torch.from_numpy(sc.grad_rgb()).to(dev), "uvs": torch.from_numpy(sc.VERTS_UVS).to(dev),
            "fuv": torch.from_numpy(sc.FACES_UVS).to(dev),
            "tex": {T: torch.from_numpy(sc.texture(T)).to(dev) for T in sc.TEX_SIDES}}


@pytest.fixture(scope="module")
def parent(golden_dir):
    d = np.load(os.path.join(golden_dir, "scatter_tiles_parent.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def oracle_gtex(scene):
    """fp64 texture gradient of the CPU oracle per texture side, computed once"""
    from oracle import render_ref as rr
    out = {}
    for T in sc.TEX_SIDES:
        acc = np.zeros((T, T, 3), np.float64)
        for b in range(sc.B):
            rr.shade_bwd(scene["g_np"][b], tuple(a[b] for a in scene["frag_np"]), sc.VERTS_UVS, sc.FACES_UVS, sc.texture(T), acc)
        out[T] = acc
    return out


def _run(ops, scene, T, want_bary):
    res = ops.shade_bwd(scene["g"], scene["frag"], scene["uvs"], scene["fuv"], scene["tex"][T], want_bary=want_bary)
    torch.cuda.synchronize()
    return (res[0], res[1]) if want_bary else (res, None)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def test_scene_is_what_the_docstring_says():
    p2f = sc.fragments()[0]
    assert (p2f[0] < 0).all() and (p2f[1] >= 0).sum() == 1 and p2f[sc.LONE] >= 0 and (p2f[2] >= 0).all()
    assert sc.LONE[1] % 16 == 0 and sc.LONE[2] % 16 == 15


@pytest.mark.parametrize("want_bary", [False, True])
@pytest.mark.parametrize("T", sc.TEX_SIDES)
def test_fixed_point_is_reproducible_and_the_parents_bits(dev, ops, scene, parent, T, want_bary):
    was = ops._DETERMINISTIC
    ops.set_deterministic(True)
    try:
        gt1, gb1 = _run(ops, scene, T, want_bary)
        gt2, gb2 = _run(ops, scene, T, want_bary)
    finally:
        ops.set_deterministic(was)
    np.testing.assert_array_equal(_bits(gt1), _bits(gt2))
    want = sc.from_sparse(parent[f"gtex_idx_{T}"], parent[f"gtex_bits_{T}"], (T, T, 3))
    assert np.count_nonzero(want) > 0
    np.testing.assert_array_equal(_bits(gt1), want.view(np.uint32))
    if want_bary:
        np.testing.assert_array_equal(_bits(gb1), _bits(gb2))
        wb = sc.from_sparse(parent[f"gbary_idx_{T}"], parent[f"gbary_bits_{T}"], (sc.B, sc.S, sc.S, 3))
        np.testing.assert_array_equal(_bits(gb1), wb.view(np.uint32))


@pytest.mark.parametrize("want_bary", [False, True])
@pytest.mark.parametrize("T", sc.TEX_SIDES)
def test_float_atomics_match_the_oracle(dev, ops, scene, oracle_gtex, T, want_bary):
    was = ops._DETERMINISTIC
    ops.set_deterministic(False)
    try:
        gt, _ = _run(ops, scene, T, want_bary)
    finally:
        ops.set_deterministic(was)
    ref = oracle_gtex[T]
    scale = np.abs(ref).max()
    err = np.abs(gt.cpu().numpy().astype(np.float64) - ref).max()
    print(f"T={T} want_bary={want_bary}: max err {err:.3e}, scale {scale:.3e}")
    assert scale > 0 and err <= 1e-5 * scale


@pytest.mark.parametrize("det", [True, False])
def test_uncovered_pixels_get_exact_zeros_over_poison(dev, ops, scene, det):
    """torch.empty filled with NaN (what ST3D_POISON_EMPTY=1 turns on for a whole session): the rows of uncovered pixels --
    whole empty tiles included -- are written, +0.0 each, and nothing non-finite is left anywhere"""
    was_det, was_alg = ops._DETERMINISTIC, torch.are_deterministic_algorithms_enabled()
    was_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    was_fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    ops.set_deterministic(det)
    try:
        assert torch.isnan(torch.empty(64, device=dev)).all()
        gt, guv, gbary = ops.shade_bwd(scene["g"], scene["frag"], scene["uvs"], scene["fuv"], scene["tex"][64], want_uv=True,
                                       want_bary=True)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was_det)
        torch.utils.deterministic.fill_uninitialized_memory = was_fill
        torch.use_deterministic_algorithms(was_alg, warn_only=was_warn)
    empty = scene["frag_np"][0] < 0
    assert not _bits(guv)[empty].any() and not _bits(gbary)[empty].any()
    assert _bits(guv)[~empty].any() and _bits(gbary)[~empty].any()
    for t in (gt, guv, gbary):
        assert torch.isfinite(t).all()


@pytest.fixture(scope="module")
def variants_parent(golden_dir):
    d = np.load(os.path.join(golden_dir, "scatter_variants_parent.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def variant_runs(dev, ops):
    """every variant, run twice, once for all the cases below"""
    return sc.variants(ops, dev), sc.variants(ops, dev)


VARIANTS = {
    "forward": ("fwd.rgb", "fwd.mask", "ss_fwd.rgb", "ss_fwd.coverage", "mip_fwd.rgb", "mip_fwd.mask", "vc_fwd.rgb",
                "vc_fwd.mask", "soft_fwd.rgb", "soft_fwd.alpha"),
    "ss_bwd": ("ss_bwd_T4.grad_texture", "ss_bwd_T4.grad_bary", "ss_bwd_T64.grad_texture", "ss_bwd_T64.grad_bary"),
    "lit_bwd": ("lit_bwd.grad_texture", "lit_bwd.grad_bary"),
    "mip_bwd": ("mip_bwd_T64.grad_texture", "mip_bwd_T64.grad_bary", "mip_bwd_T4.grad_texture", "mip_bwd_T4.grad_bary"),
    "vc_bwd": ("vc_bwd_shared.grad_colors", "vc_bwd_shared.grad_bary", "vc_bwd_own.grad_colors", "vc_bwd_own.grad_bary"),
    "soft_bwd": ("soft_bwd.grad_texture",),
}


def test_variant_cases_are_all_recorded(variants_parent):
    names = sorted(n for group in VARIANTS.values() for n in group)
    assert sorted(k[:-len(".sha256")] for k in variants_parent if k.endswith(".sha256")) == names
    own_p2f, own_faces = sc.own_faces()
    tile = own_p2f[2, :16, :16]
    assert len(np.unique(own_faces[tile.reshape(-1)])) == 768           # the vertex table's worst case: a full tile
    lod = sc.lod_plane(3)[2]
    assert lod.min() == 0 and lod.max() == 2 and (lod == 1).any() and (lod % 1 != 0).any()


@pytest.mark.parametrize("group", sorted(VARIANTS))
def test_variants_are_reproducible_and_the_parents_bits(variant_runs, variants_parent, group):
    first, second = variant_runs
    for name in VARIANTS[group]:
        np.testing.assert_array_equal(first[name].view(np.uint32), second[name].view(np.uint32), err_msg=name)
        nnz, sha = sc.digest(first[name])
        print(f"{name}: {nnz} non-zero, sha256 {sha.tobytes().hex()[:16]}")
        assert nnz > 0 and nnz == variants_parent[name + ".nnz"], name
        assert sha.tobytes() == variants_parent[name + ".sha256"].tobytes(), f"{name}: bits differ from the parent's"
