"""Host side of mip-mapped texture sampling: level validation, what RasterizationSettings(texture_mip_levels=,
texture_lod_bias=) and the renderer refuse before any launch, --texture_mip_levels / --texture_lod_bias on the three
scripts, the routing of texture_mip_levels = 1, and the C ABI's argument checks.  No GPU."""
import types

import pytest
import torch


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def _cpu_mesh(T=8, z=3.0):
    from st3d import render as R
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    fuv = torch.tensor([[[0, 1, 2]]])
    tex = R.TexturesUV(maps=torch.rand(1, T, T, 3), faces_uvs=fuv, verts_uvs=torch.rand(1, 3, 2))
    return R.Meshes(verts, torch.tensor([[0, 1, 2]]), tex), R.FoVPerspectiveCameras(T=torch.tensor([[0.0, 0, z]]))


def _renderer(shader=None, **kw):
    from st3d import render as R
    return R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=8, **kw)), shader or R.SoftPhongShader())


def test_levels_are_validated_against_the_side():
    from st3d import ops
    assert [ops.check_mip(0, T) for T in (64, 48, 40, 37, 6, 2, 1024)] == [6, 5, 4, 1, 2, 1, 10]
    assert ops.check_mip(1, 37) == 1 and ops.check_mip(3, 48) == 3 and ops.check_mip(2, 6) == 2 and ops.check_mip(6, 64) == 6
    for levels, T in ((2, 37), (3, 6), (7, 64), (6, 48), (2, 2)):
        with pytest.raises(ValueError, match="texture_mip_levels"):
            ops.check_mip(levels, T)
    for bad in (-1, 17, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="texture_mip_levels"):
            ops.check_mip(bad)
        with pytest.raises(ValueError, match="texture_mip_levels"):
            ops.check_mip(bad, 64)
    with pytest.raises(ValueError, match="side"):
        ops.check_mip(0, 1)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="texture_lod_bias"):
            ops.check_lod_bias(bad)


def test_raster_settings_keywords():
    from st3d import render as R
    rs = R.RasterizationSettings(image_size=8)
    assert rs.texture_mip_levels == 1 and rs.texture_lod_bias == 0.0
    rs = R.RasterizationSettings(image_size=8, texture_mip_levels=0, texture_lod_bias=-0.5)
    assert rs.texture_mip_levels == 0 and rs.texture_lod_bias == -0.5 and rs.is_hard and rs.supersample == 1
    for bad in (-1, 17, 1.5, "0", True):
        with pytest.raises(ValueError, match="texture_mip_levels"):
            R.RasterizationSettings(image_size=8, texture_mip_levels=bad)
    with pytest.raises(ValueError, match="texture_lod_bias"):
        R.RasterizationSettings(image_size=8, texture_mip_levels=0, texture_lod_bias=float("nan"))
    assert _renderer(texture_mip_levels=4).texture_mip_levels == 4 and _renderer().texture_mip_levels == 1


def test_every_limitation_is_refused_before_a_launch():
    """CPU tensors: anything that reached a kernel would raise St3dError('no CPU fallback') instead"""
    from st3d import render as R
    mesh, cams = _cpu_mesh()
    with pytest.raises(NotImplementedError, match="supersample"):
        R.RasterizationSettings(image_size=8, texture_mip_levels=0, supersample=2)
    for lights in (R.PointLights(), R.DirectionalLights(), R.HeadLights(), R.AmbientLights(ambient_color=((0.5, 0.5, 0.5),))):
        with pytest.raises(NotImplementedError, match="unlit"):
            _renderer(texture_mip_levels=0).render(mesh, cams, lights=lights)
    for kw in (dict(faces_per_pixel=2), dict(blur_radius=1e-4), dict(cull_backfaces=True), dict(z_clip_value=0.5)):
        with pytest.raises(NotImplementedError, match="hard settings"):
            _renderer(texture_mip_levels=0, **kw).render(mesh, cams)
    with pytest.raises(NotImplementedError, match="hard settings"):
        _renderer(R.SoftPhongShader(blend_params=R.BlendParams(sigma=1e-3)), texture_mip_levels=2).render(mesh, cams)
    with pytest.raises(NotImplementedError, match="silhouette"):
        _renderer(R.SoftSilhouetteShader(), texture_mip_levels=0)
    with pytest.raises(NotImplementedError, match="silhouette"):
        R.SilhouetteRasterizationSettings(image_size=8, texture_mip_levels=2)
    with pytest.raises(NotImplementedError, match="silhouette"):
        R.render_silhouette(mesh, cams.R, cams.T, 8, R.RasterizationSettings(image_size=8, texture_mip_levels=0))
    rs = R.RasterizationSettings(image_size=8, texture_mip_levels=0)
    rs.supersample = 2                                       # (set behind the constructor's back: render time refuses too)
    with pytest.raises(NotImplementedError, match="supersample"):
        R.render_views(mesh, cams.R, cams.T, 8, rs)
    # levels that do not fit the map: ValueError at render time, once T is known
    with pytest.raises(ValueError, match="texture_mip_levels"):
        _renderer(texture_mip_levels=5).render(mesh, cams)
    # white ambient light is the unlit route: it gets as far as the kernels
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _renderer(texture_mip_levels=0).render(mesh, cams, lights=R.AmbientLights())


def test_near_plane_is_an_error_not_a_reroute(monkeypatch):
    from st3d import ops
    from st3d import render as R
    mesh, cams = _cpu_mesh(z=0.3)
    monkeypatch.setattr(ops, "NEAR_PLANE_POLICY", "clip")
    try:
        with pytest.raises(RuntimeError, match="near clipping plane.*texture_mip_levels"):
            _renderer(texture_mip_levels=0).render(mesh, cams)
        assert not ops.near_plane_triggered()
    finally:
        ops.reset_near_plane()


def test_routing(monkeypatch):
    """1 (and 0 under a side that allows one level) is _RenderFn with its old arguments; L >= 2 is _MipRenderFn"""
    from st3d import render as R
    calls = []

    def fake(name):
        def apply(*a):
            calls.append((name, a))
            S = a[7]
            return torch.zeros(1, 3, S, S), torch.zeros(1, 1, S, S)
        return types.SimpleNamespace(apply=apply)
    monkeypatch.setattr(R, "_RenderFn", fake("plain"))
    monkeypatch.setattr(R, "_MipRenderFn", fake("mip"))
    mesh, cams = _cpu_mesh(8)
    _renderer().render(mesh, cams)
    _renderer(texture_mip_levels=1, texture_lod_bias=0.0).render(mesh, cams)
    assert [c[0] for c in calls] == ["plain", "plain"] and len(calls[0][1]) == len(calls[1][1]) == 9
    assert all(x is y or x == y for x, y in zip(calls[0][1][2:], calls[1][1][2:]))
    calls.clear()
    _renderer(texture_mip_levels=0, texture_lod_bias=0.25).render(mesh, cams)
    _renderer(texture_mip_levels=2).render(mesh, cams)
    assert [c[0] for c in calls] == ["mip", "mip"]
    assert calls[0][1][7:] == (8, 3, 0.25) and calls[1][1][7:] == (8, 2, 0.0)
    calls.clear()
    odd, cams = _cpu_mesh(7)
    _renderer(texture_mip_levels=0).render(odd, cams)
    assert [c[0] for c in calls] == ["plain"]


def test_ops_wrappers_check_before_the_library():
    from st3d import _lib, ops
    frag = (torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8))
    uvs, fuv = torch.rand(3, 2), torch.zeros(1, 3, dtype=torch.int32)
    assert ops.mip_numel(8, 3) == 3 * (64 + 16 + 4) and ops.mip_numel(6, 2) == 3 * 45
    with pytest.raises(ValueError, match="texture_mip_levels"):
        ops.mip_numel(8, 4)
    with pytest.raises(ValueError, match="texture_mip_levels"):
        ops.mip_build(torch.rand(6, 6, 3), 3)
    with pytest.raises(ValueError, match="holds"):
        ops.mip_adjoint(torch.rand(10), 8, 3)
    with pytest.raises(ValueError, match="holds"):
        ops.shade_mip_fwd(frag, uvs, fuv, torch.rand(5), torch.zeros(1, 8, 8), 8, 3)
    with pytest.raises(ValueError, match="lod"):
        ops.shade_mip_fwd(frag, uvs, fuv, torch.rand(252), torch.zeros(1, 4, 4), 8, 3)
    with pytest.raises(ValueError, match="grad_rgb"):
        ops.shade_mip_bwd(torch.rand(1, 3, 4, 4), frag, uvs, fuv, torch.rand(252), torch.zeros(1, 8, 8), 8, 3)
    with pytest.raises(ValueError, match="texture_lod_bias"):
        ops.mip_lod(frag, torch.rand(1, 3, 3), fuv, uvs, fuv, 8, 3, float("nan"))
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.mip_build(torch.rand(8, 8, 3), 3)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_mip_fwd(frag, uvs, fuv, torch.rand(252), torch.zeros(1, 8, 8), 8, 3)


def test_c_abi_validates_before_any_launch():
    from st3d import _lib
    lib = _lib.load()
    one = 16        # any non-NULL value: the checks below fail before a pointer is followed
    assert lib.st3d_mip_numel(64, 6) == 3 * (4096 + 1024 + 256 + 64 + 16 + 4) and lib.st3d_mip_numel(6, 2) == 135
    assert lib.st3d_mip_numel(48, 5) == 3 * (2304 + 576 + 144 + 36 + 9) and lib.st3d_mip_numel(37, 1) == 3 * 37 * 37
    for T, L in ((64, 7), (37, 2), (6, 3), (2, 2), (1, 1), (0, 1), (64, 0), (64, 17), (32768, 1), (-4, 2)):
        assert lib.st3d_mip_numel(T, L) == 0, (T, L)
        assert lib.st3d_shade_mip_bwd_workspace_bytes(T, L) == 0
        assert lib.st3d_mip_build(one, T, L, 32, None) == -1 and b"invalid argument" in lib.st3d_last_error()
        assert lib.st3d_mip_adjoint(one, T, L, 0, 32, None) == -1
    assert lib.st3d_shade_mip_bwd_workspace_bytes(8, 3) >= 8 * 252
    assert lib.st3d_mip_build(None, 8, 3, one, None) == -1 and lib.st3d_mip_build(one, 8, 3, None, None) == -1
    assert lib.st3d_mip_build(one, 8, 3, one, None) == -1                  # in place
    assert lib.st3d_mip_adjoint(one, 8, 3, 0, None, None) == -1
    p = [one] * 7
    assert lib.st3d_mip_lod(*p, 1, 8, 8, 4, 3, 1, 3, 0.0, one, None) == -1             # L = 4 under T = 8
    assert lib.st3d_mip_lod(*p, 1, 8, 8, 3, 3, 1, 3, 0.0, None, None) == -1
    assert lib.st3d_mip_lod(*p, 1, 4097, 8, 3, 3, 1, 3, 0.0, one, None) == -1
    assert lib.st3d_mip_lod(*p, 1, 8, 8, 3, 3, 1, 3, float("nan"), one, None) == -1
    f = [one] * 8
    assert lib.st3d_shade_mip_fwd(*f, 1, 8, 8, 4, 1, 3, one, one, None) == -1
    assert lib.st3d_shade_mip_fwd(*f, 1, 8, 8, 3, 1, 3, None, one, None) == -1
    assert lib.st3d_shade_mip_fwd(*f[:7], None, 1, 8, 8, 3, 1, 3, one, one, None) == -1
    g = [one] * 9
    assert lib.st3d_shade_mip_bwd(*g, 1, 8, 8, 4, 1, 3, one, one, None, None, None, 0, None) == -1
    assert lib.st3d_shade_mip_bwd(*g, 1, 8, 8, 3, 1, 3, None, None, None, None, None, 0, None) == -1    # nothing wanted
    assert lib.st3d_shade_mip_bwd(*g, 1, 8, 8, 3, 1, 3, None, one, None, None, None, 0, None) == -1     # no grad_pyramid
    assert lib.st3d_shade_mip_bwd(*g, 1, 8, 8, 3, 1, 3, one, one, None, None, one, 8, None) == -1       # workspace too small
    assert lib.st3d_shade_mip_bwd(*g, 1, 8, 8, 3, 1, 3, None, None, None, one, one, 1 << 20, None) == -1  # fixed point of nothing


@pytest.mark.parametrize("k", [0, 1, 2])
def test_flags_reach_all_three_scripts(k):
    p = _scripts()[k].build_parser()
    a = p.parse_args([])
    assert a.texture_mip_levels == 1 and a.texture_lod_bias == 0.0
    a = p.parse_args(["--texture_mip_levels", "0", "--texture_lod_bias", "-0.5"])
    assert a.texture_mip_levels == 0 and a.texture_lod_bias == -0.5
    assert p.parse_args(["--texture_mip_levels", "4", "--size", "64"]).texture_mip_levels == 4
    for argv in (["--texture_mip_levels", "-1"], ["--texture_mip_levels", "17"],
                 ["--texture_mip_levels", "0", "--supersample", "2"], ["--texture_mip_levels", "0", "--lights", "point"],
                 ["--texture_mip_levels", "3", "--lights", "headlight"], ["--texture_mip_levels", "4", "--size", "36"],
                 ["--texture_mip_levels", "0", "--texture_lod_bias", "nan"], ["--texture_lod_bias", "1.0"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_check_args_names_the_conflict():
    from st3d import cli
    base = dict(silhouette_weight=0.0, optimization_target="texture", silhouette_sigma=1e-4, silhouette_faces_per_pixel=None,
                texture_pyramid_levels=1, size=768, supersample=1, texture_mip_levels=1, texture_lod_bias=0.0, lights="ambient",
                resize_texture=True)
    ns = lambda **kw: types.SimpleNamespace(**dict(base, **kw))      # noqa: E731
    assert cli.check_args(ns()) is None and cli.check_args(ns(texture_mip_levels=0, texture_lod_bias=-1.0)) is None
    assert cli.check_args(ns(texture_mip_levels=9)) is None           # 768 = 3 * 2^8
    assert "16" in cli.check_args(ns(texture_mip_levels=20))
    assert "supersample" in cli.check_args(ns(texture_mip_levels=0, supersample=2))
    assert "lights" in cli.check_args(ns(texture_mip_levels=0, lights="directional"))
    assert "divisible" in cli.check_args(ns(texture_mip_levels=10))
    assert cli.check_args(ns(texture_mip_levels=10, resize_texture=False)) is None      # the map's own side decides, at render time
    assert "finite" in cli.check_args(ns(texture_mip_levels=0, texture_lod_bias=float("inf")))
    assert "texture_mip_levels" in cli.check_args(ns(texture_lod_bias=0.5))
    # the pyramid parametrisation, the style mask and a silhouette term are independent of the sampling
    assert cli.check_args(ns(texture_mip_levels=0, texture_pyramid_levels=0)) is None
    assert cli.check_args(ns(texture_mip_levels=0, silhouette_weight=1.0, optimization_target="both")) is None
    names = {f.name: f.default for f in cli.SHARED_FLAGS}
    assert names["texture_mip_levels"] == 1 and names["texture_lod_bias"] == 0.0
