"""Host side of the texture pyramid: the flag on all three scripts and what it is refused with, setup_optimizations with and
without a pyramid, TexturePyramid's bookkeeping, and the C ABI's argument checks.  Nothing here launches a kernel."""
import ctypes

import pytest
import torch

import _texpyr_ref as TP


def _scripts():
    import first_approach
    import second_approach
    import third_approach
    return first_approach, second_approach, third_approach


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from st3d import _lib
    return _lib.load()


def test_flag_defaults_and_refusals(capsys):
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.texture_pyramid_levels == 1 and isinstance(a.texture_pyramid_levels, int)
        assert mod.build_parser().parse_args(["--texture_pyramid_levels", "0"]).texture_pyramid_levels == 0
        b = mod.build_parser().parse_args(["--texture_pyramid_levels", "4", "--optimization_target", "both"])
        assert b.texture_pyramid_levels == 4
        # 1 is "off": allowed with every target
        assert mod.build_parser().parse_args(["--optimization_target", "mesh"]).texture_pyramid_levels == 1
        for argv in (["--texture_pyramid_levels", "0", "--optimization_target", "mesh"],
                     ["--texture_pyramid_levels", "3", "--optimization_target", "mesh"],
                     ["--texture_pyramid_levels", "-1"]):
            with pytest.raises(SystemExit):
                mod.build_parser().parse_args(argv)
            assert "texture_pyramid_levels" in capsys.readouterr().err


def _mesh(T=16):
    import utils as U
    g = torch.Generator().manual_seed(0)
    verts = torch.rand(5, 3, generator=g)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4]])
    uvs = torch.rand(1, 6, 2, generator=g)
    fuv = torch.tensor([[[0, 1, 2], [3, 4, 5]]])
    tex = torch.rand(1, T, T, 3, generator=g)
    return U.build_mesh(uvs, fuv, tex, verts, faces), tex, verts


def test_setup_optimizations_default_is_unchanged():
    import utils as U
    mesh, tex, verts = _mesh()
    for target, leaves in (("texture", ["texture_map"]), ("mesh", ["verts"]), ("both", ["verts", "texture_map"])):
        for out in (U.setup_optimizations(target, mesh, 0.01), U.setup_optimizations(target, mesh, 0.01, 1),
                    U.setup_optimizations(target, mesh, 0.01, texture_pyramid_levels=1)):
            assert sorted(out) == ["faces", "faces_uvs", "optimizable_mesh", "optimizer", "texture_map", "verts", "verts_uvs"]
            assert [id(p) for p in out["optimizer"].params] == [id(out[k]) for k in leaves]
            assert out["texture_map"].requires_grad == ("texture_map" in leaves)
            assert out["verts"].requires_grad == ("verts" in leaves)
            assert torch.equal(out["texture_map"].detach(), tex) and out["texture_map"].shape == (1, 16, 16, 3)
            assert out["optimizer"].lr == 0.01 and len(out["optimizer"].param_groups) == 1


def test_setup_optimizations_with_a_pyramid():
    import utils as U
    from st3d.texpyr import TexturePyramid
    mesh, tex, verts = _mesh()
    out = U.setup_optimizations("texture", mesh, 0.01, texture_pyramid_levels=0)
    pyr = out["texture_pyramid"]
    assert isinstance(pyr, TexturePyramid) and "texture_map" not in out
    assert pyr.sides == [16, 8, 4] and pyr.levels == 3
    assert [id(p) for p in out["optimizer"].params] == [id(pyr.params)]
    assert pyr.params.is_leaf and pyr.params.requires_grad and pyr.params.shape == (TP.numel(16, 3),)
    both = U.setup_optimizations("both", mesh, 0.01, texture_pyramid_levels=2)
    assert [id(p) for p in both["optimizer"].params] == [id(both["verts"]), id(both["texture_pyramid"].params)]
    assert both["verts"].requires_grad and both["texture_pyramid"].sides == [16, 8]
    with pytest.raises(ValueError):
        U.setup_optimizations("mesh", mesh, 0.01, texture_pyramid_levels=0)
    with pytest.raises(ValueError):
        U.setup_optimizations("texture", mesh, 0.01, texture_pyramid_levels=-2)
    with pytest.raises(ValueError):
        U.setup_optimizations("texture", mesh, 0.01, texture_pyramid_levels=6)         # 16 / 32
    with pytest.raises(UnboundLocalError):                                              # the reference's own failure comes first
        U.setup_optimizations("nothing", mesh, 0.01, texture_pyramid_levels=0)


def test_texture_pyramid_bookkeeping():
    from st3d.texpyr import TexturePyramid
    tex = torch.rand(1, 24, 24, 3, generator=torch.Generator().manual_seed(1))
    pyr = TexturePyramid(tex, 3)
    assert pyr.sides == [24, 12, 6] and pyr.offsets == TP.offsets([24, 12, 6])
    assert torch.equal(pyr.level(0), tex[0])
    for l in (1, 2):
        lv = pyr.level(l)
        assert lv.shape == (pyr.sides[l], pyr.sides[l], 3)
        assert torch.equal(lv, torch.zeros_like(lv)) and not torch.signbit(lv).any()          # +0.0, not -0.0
        assert lv.data_ptr() == pyr.params.data_ptr() + 4 * pyr.offsets[l]                  # a view, not a copy
    with pytest.raises(IndexError):
        pyr.level(3)
    assert TexturePyramid(tex[0], 0).sides == [24, 12, 6]                                    # (T,T,3) is taken too
    assert TexturePyramid(tex, 1).sides == [24]
    new = torch.arange(pyr.params.numel(), dtype=torch.float32)
    leaf = pyr.params
    pyr.load_params(new)
    assert pyr.params is leaf and torch.equal(pyr.params.detach(), new)
    for bad in (new[:-1], new.view(1, -1), torch.zeros(3 * 24 * 24)):
        with pytest.raises(ValueError):
            pyr.load_params(bad)
    for T, L in ((24, 5), (8, 4), (24, -1), (10, 3)):
        with pytest.raises(ValueError):
            TexturePyramid(torch.zeros(1, T, T, 3), L)
    with pytest.raises(NotImplementedError):
        TexturePyramid(torch.zeros(1, 8, 16, 3), 2)
    with pytest.raises(ValueError):
        TexturePyramid(torch.zeros(1, 8, 8, 4), 2)


def test_ops_refuse_bad_shapes_before_any_launch(lib):
    from st3d import _lib, ops
    for T, lv, want in ((512, 0, 8), (768, 0, 8), (192, 0, 6), (64, 0, 5), (6, 0, 1), (24, 3, 3)):
        assert ops.texpyr_sides(T, lv) == TP.sides(T, lv) and len(ops.texpyr_sides(T, lv)) == want
    for T, L in ((8, 3), (24, 3), (160, 5), (192, 6), (512, 8), (7, 1)):
        assert ops.texpyr_numel(T, L) == TP.numel(T, L)
    for T, L in ((24, 5), (8, 4), (24, 0), (24, -1), (0, 1), (24, 17)):
        with pytest.raises(ValueError):
            ops.texpyr_numel(T, L)
    with pytest.raises(ValueError):
        ops.texpyr_synth(torch.zeros(10), 24, 3)                    # wrong length: refused before the pointer is looked at
    with pytest.raises(ValueError):
        ops.texpyr_adjoint(torch.zeros(24, 24), 24, 3)
    with pytest.raises(_lib.St3dError):                             # no CPU fallback
        ops.texpyr_synth(torch.zeros(TP.numel(24, 3)), 24, 3)
    with pytest.raises(_lib.St3dError):
        ops.texpyr_adjoint(torch.zeros(24, 24, 3), 24, 3)


def test_abi_argument_checks_return_minus_one(lib):
    a, b = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)           # never dereferenced: every call is refused on the host
    for fn in (lib.st3d_texpyr_synth, lib.st3d_texpyr_adjoint):
        assert fn(None, 8, 3, b, None) == -1 and b"invalid argument" in lib.st3d_last_error()
        assert fn(a, 8, 3, None, None) == -1
        assert fn(a, 8, 3, a, None) == -1                           # in place
        for T, L in ((0, 1), (-8, 2), (8, 0), (8, -1), (8, 4), (24, 5), (10, 3), (8, 17), (32768, 2)):
            assert fn(a, T, L, b, None) == -1, (T, L)
    for T, L in ((0, 1), (8, 0), (8, 4), (24, 5), (10, 3), (8, 17)):
        assert lib.st3d_texpyr_numel(T, L) == 0
    assert lib.st3d_texpyr_numel(24, 3) == 2268 and lib.st3d_texpyr_numel(6, 1) == 108
    assert lib.st3d_texpyr_numel(1024, 9) == TP.numel(1024, 9)
