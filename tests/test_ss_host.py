"""Host side of supersampled rendering: the doors of the Python surface (RasterizationSettings(supersample=), the
renderer, --supersample, the ops wrappers) and the C ABI's argument checks.  No GPU."""
import pytest
import torch


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def _cpu_mesh():
    from st3d import render as R
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    fuv = torch.tensor([[[0, 1, 2]]])
    tex = R.TexturesUV(maps=torch.rand(1, 4, 4, 3), faces_uvs=fuv, verts_uvs=torch.rand(1, 3, 2))
    return R.Meshes(verts, torch.tensor([[0, 1, 2]]), tex), R.FoVPerspectiveCameras(T=torch.tensor([[0.0, 0, 3]]))


def test_raster_settings_take_an_int_in_1_to_4():
    from st3d import render as R
    assert R.RasterizationSettings(image_size=8).supersample == 1
    for a in (1, 2, 3, 4):
        rs = R.RasterizationSettings(image_size=8, supersample=a)
        assert rs.supersample == a and rs.image_size == 8 and rs.is_hard
    for bad in (0, 5, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="supersample"):
            R.RasterizationSettings(image_size=8, supersample=bad)


def test_the_rasterisers_side_limit_is_refused_on_the_host():
    from st3d import render as R
    assert R.RasterizationSettings(image_size=1024, supersample=4).supersample == 4
    assert R.RasterizationSettings(image_size=4096).supersample == 1
    for S, a in ((1025, 4), (2049, 2), (1366, 3)):
        with pytest.raises(ValueError, match="4096"):
            R.RasterizationSettings(image_size=S, supersample=a)


def test_alpha_only_renders_are_out_of_scope():
    from st3d import render as R
    with pytest.raises(NotImplementedError, match="supersample"):
        R.SilhouetteRasterizationSettings(image_size=8, supersample=2)
    assert R.SilhouetteRasterizationSettings(image_size=8, supersample=1).supersample == 1
    rs = R.RasterizationSettings(image_size=8, supersample=2)
    with pytest.raises(NotImplementedError, match="supersample"):
        R.MeshRenderer(R.MeshRasterizer(None, rs), R.SoftSilhouetteShader())
    mesh, cams = _cpu_mesh()
    with pytest.raises(NotImplementedError, match="supersample"):
        R.render_silhouette(mesh, cams.R, cams.T, 8, rs)
    R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=8)), R.SoftSilhouetteShader())


def test_renderer_reports_supersample_and_keeps_is_hard():
    from st3d import render as R
    r1 = R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=8)), R.SoftPhongShader())
    r2 = R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=8, supersample=3)), R.SoftPhongShader())
    assert r1.supersample == 1 and r2.supersample == 3 and r1.is_hard and r2.is_hard and r2.image_size == 8


def test_render_meshes_thresholds_a_fractional_coverage():
    """utils.render_meshes keeps mask = (alpha > 0) of the reference whenever the coverage can be fractional"""
    import utils as U

    class Fake:
        is_hard = True

        def __init__(self, a):
            self.supersample = a

        def render(self, meshes, cameras):
            return torch.zeros(1, 3, 2, 2), torch.tensor([[[[0.0, 0.25], [0.5, 1.0]]]])
    _, m = U.render_meshes(Fake(2), None, None)
    assert m.tolist() == [[[[0.0, 1.0], [1.0, 1.0]]]]
    _, m = U.render_meshes(Fake(1), None, None)
    assert m.tolist() == [[[[0.0, 0.25], [0.5, 1.0]]]]         # supersample = 1 under hard settings: untouched, as before


def test_cpu_tensors_are_refused_not_rendered():
    from st3d import _lib, ops
    from st3d import render as R
    mesh, cams = _cpu_mesh()
    for rs in (R.RasterizationSettings(image_size=8, supersample=2),
               R.RasterizationSettings(image_size=8, supersample=2, faces_per_pixel=2)):
        r = R.MeshRenderer(R.MeshRasterizer(None, rs), R.SoftPhongShader())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            r.render(mesh, cams)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.box_down_fwd(torch.rand(1, 3, 8, 8), 2)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.box_down_bwd(torch.rand(1, 3, 4, 4), 2)
    frag = (torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8))
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_ss_fwd(frag, torch.rand(3, 2), torch.zeros(1, 3, dtype=torch.int32), torch.rand(4, 4, 3), 2)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_ss_bwd(torch.rand(1, 3, 4, 4), frag, torch.rand(3, 2), torch.zeros(1, 3, dtype=torch.int32), torch.rand(4, 4, 3), 2)


def test_ops_wrappers_check_shapes_and_the_factor_first():
    from st3d import ops
    for bad in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="supersample"):
            ops.box_down_fwd(torch.rand(1, 3, 8, 8), bad)
    with pytest.raises(ValueError, match="multiple"):
        ops.box_down_fwd(torch.rand(1, 3, 9, 9), 2)
    with pytest.raises(ValueError, match="square"):
        ops.box_down_bwd(torch.rand(1, 3, 4, 5), 2)
    with pytest.raises(ValueError, match="4096"):
        ops.box_down_bwd(torch.rand(1, 1, 1025, 1025), 4)
    frag = (torch.zeros(1, 9, 9, dtype=torch.int32), torch.zeros(1, 9, 9), torch.zeros(1, 9, 9, 3), torch.zeros(1, 9, 9))
    with pytest.raises(ValueError, match="multiple"):
        ops.shade_ss_fwd(frag, torch.rand(3, 2), torch.zeros(1, 3, dtype=torch.int32), torch.rand(4, 4, 3), 2)
    with pytest.raises(ValueError, match="grad_rgb"):
        ops.shade_ss_bwd(torch.rand(1, 3, 9, 9), frag, torch.rand(3, 2), torch.zeros(1, 3, dtype=torch.int32), torch.rand(4, 4, 3), 3)


def test_c_abi_validates_before_any_launch():
    from st3d import _lib
    lib = _lib.load()
    one = 16        # any non-NULL value: the checks below fail before a pointer is followed
    for fn in (lib.st3d_box_down_fwd, lib.st3d_box_down_bwd):
        assert fn(None, 1, 3, 8, 2, one, None) == -1 and b"invalid argument" in lib.st3d_last_error()
        assert fn(one, 1, 3, 8, 2, None, None) == -1
        for a in (0, 5, -1):
            assert fn(one, 1, 3, 8, a, one, None) == -1
        assert fn(one, 1, 3, 1025, 4, one, None) == -1 and fn(one, 0, 3, 8, 2, one, None) == -1
        assert fn(one, 1, 0, 8, 2, one, None) == -1 and fn(one, 1, 3, 0, 2, one, None) == -1
    p = [one] * 7
    assert lib.st3d_shade_ss_fwd(*p, 1, 8, 5, 4, 1, 3, one, one, None) == -1
    assert lib.st3d_shade_ss_fwd(*p, 1, 2049, 2, 4, 1, 3, one, one, None) == -1
    assert lib.st3d_shade_ss_fwd(*p, 1, 8, 2, 4, 1, 3, None, one, None) == -1
    g = [one] * 8
    assert lib.st3d_shade_ss_bwd(*g, 1, 8, 0, 4, 1, 3, one, None, None, None) == -1
    assert lib.st3d_shade_ss_bwd(*g, 1, 8, 2, 4, 1, 3, None, None, None, None) == -1
    assert lib.st3d_shade_ss_bwd_det(*g, 1, 8, 5, 4, 1, 3, one, None, None, one, 1 << 20, None) == -1
    assert lib.st3d_shade_ss_bwd_det(*g, 1, 8, 2, 4, 1, 3, one, None, None, None, 0, None) == -1
    lit = [one, one, one, one, one, one, 1, 1]
    assert lib.st3d_shade_ss_lit_fwd(*p, 1, 8, 5, 4, 1, 3, *lit, one, one, None) == -1
    assert lib.st3d_shade_ss_lit_bwd(*g, 1, 8, 5, 4, 1, 3, *lit, 1.0, one, None, None, None, 0, None) == -1
    assert lib.st3d_shade_ss_lit_bwd(*g, 1, 1366, 3, 4, 1, 3, *lit, 1.0, one, None, None, None, 0, None) == -1


@pytest.mark.parametrize("k", [0, 1, 2])
def test_flag_reaches_all_three_scripts(k):
    script = _scripts()[k]
    p = script.build_parser()
    assert p.parse_args([]).supersample == 1
    assert p.parse_args(["--supersample", "3"]).supersample == 3
    for argv in (["--supersample", "0"], ["--supersample", "5"], ["--supersample", "2", "--size", "2049"],
                 ["--supersample", "4", "--size", "1025"],
                 ["--supersample", "2", "--silhouette_weight", "1", "--optimization_target", "mesh"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert p.parse_args(["--supersample", "4", "--size", "1024"]).supersample == 4
    assert p.parse_args(["--supersample", "1", "--silhouette_weight", "1", "--optimization_target", "mesh"]).supersample == 1


def test_check_args_names_the_conflict():
    import types
    from st3d import cli
    base = dict(silhouette_weight=0.0, optimization_target="texture", silhouette_sigma=1e-4, silhouette_faces_per_pixel=None,
                texture_pyramid_levels=1, size=768, supersample=1)
    assert cli.check_args(types.SimpleNamespace(**base)) is None
    assert "1..4" in cli.check_args(types.SimpleNamespace(**dict(base, supersample=7)))
    assert "4096" in cli.check_args(types.SimpleNamespace(**dict(base, supersample=4, size=1100)))
    assert "silhouette" in cli.check_args(types.SimpleNamespace(**dict(base, supersample=2, silhouette_weight=0.5,
                                                                       optimization_target="both")))
    assert any(f.name == "supersample" and f.default == 1 for f in cli.SHARED_FLAGS)


def test_fused_switch_is_read_from_the_environment(monkeypatch):
    from st3d import render as R
    monkeypatch.delenv("ST3D_SS_FUSED", raising=False)
    assert R.ss_fused()
    monkeypatch.setenv("ST3D_SS_FUSED", "0")
    assert not R.ss_fused()
    monkeypatch.setenv("ST3D_SS_FUSED", "1")
    assert R.ss_fused()
