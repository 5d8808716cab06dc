"""Host side of the silhouette rasteriser (csrc/silraster.hip): the doors of the Python surface (faces_per_pixel of
compute_silhouette_loss, SilhouetteRasterizationSettings, --silhouette_faces_per_pixel), and the C ABI's argument checks.
No GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_mesh():
    from st3d import render as R
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    return R.Meshes(verts, torch.tensor([[0, 1, 2]])), R.FoVPerspectiveCameras(T=torch.tensor([[0.0, 0, 3]]))


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


# ---------------------------------------------------------------------------- 1. compute_silhouette_loss(faces_per_pixel=)
def test_faces_per_pixel_range_of_the_loss():
    import losses as L
    from st3d import render as R
    mesh, cams = _cpu_mesh()
    a = torch.zeros(1, 1, 4, 4)
    rs = R.RasterizationSettings(image_size=4)
    for bad in (0, 65, -1, 1000, 8.0, "8", True):
        with pytest.raises(ValueError, match="faces_per_pixel"):
            L.compute_silhouette_loss(rs, mesh, cams, a, faces_per_pixel=bad)
    for good in (1, 8, 50, 64):
        # in range: accepted up to the device check (CPU tensors are refused, there is no CPU path)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            L.compute_silhouette_loss(rs, mesh, cams, a, faces_per_pixel=good)
    assert L.SILHOUETTE_FACES_PER_PIXEL == 8 and L.SILHOUETTE_RASTER_MAX_FACES_PER_PIXEL == 64


def test_none_keeps_the_fragment_path_and_an_integer_takes_the_rasteriser(monkeypatch):
    import losses as L
    from st3d import render as R
    taken = []

    class Stop(Exception):
        pass

    def spy(name):
        def apply(*a):
            taken.append((name, a))
            raise Stop
        return apply
    monkeypatch.setattr(L._SilhouetteLossFn, "apply", spy("fragments"))
    monkeypatch.setattr(L._SilhouetteRasterLossFn, "apply", spy("rasteriser"))
    class OnDevice(torch.Tensor):                   # a CPU tensor that passes the device check
        is_cuda = property(lambda self: True)
    _, cams = _cpu_mesh()
    verts = torch.zeros(3, 3).as_subclass(OnDevice)
    mesh = types.SimpleNamespace(verts_packed=lambda: verts, faces_i32=lambda: torch.zeros(1, 3, dtype=torch.int32))
    rs = R.RasterizationSettings(image_size=4)
    a = torch.zeros(1, 1, 4, 4).as_subclass(OnDevice)
    for k, name in ((None, "fragments"), (8, "rasteriser"), (50, "rasteriser")):
        with pytest.raises(Stop):
            L.compute_silhouette_loss(rs, mesh, cams, a, faces_per_pixel=k)
        assert taken[-1][0] == name
    assert taken[0][1][6] == 8                      # the fragment path's K stays SILHOUETTE_FACES_PER_PIXEL
    assert taken[2][1][5] == 50 and taken[2][1][6] == pytest.approx(L.silhouette_blur_radius(1e-4))


def test_ops_refuse_bad_k_and_sigma_before_any_launch():
    from st3d import _lib, ops
    ndc = torch.zeros(1, 3, 3)
    faces = torch.zeros(1, 3, dtype=torch.int32)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            ops.silraster_fwd(ndc, faces, 4, bad, 1e-3)
        with pytest.raises(ValueError):
            ops.silraster_loss(ndc, faces, torch.zeros(1, 1, 4, 4), bad, 1e-3)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.silraster_fwd(ndc, faces, 4, 8, 1e-3, sigma=bad)
        with pytest.raises(ValueError):
            ops.silraster_bwd(torch.zeros(3, 1, 4, 4), ndc, faces, 1e-3, sigma=bad, grad_alpha=torch.zeros(1, 1, 4, 4))
    with pytest.raises(_lib.St3dError):             # CPU tensors
        ops.silraster_fwd(ndc, faces, 4, 8, 1e-3)


# ---------------------------------------------------------------------------- 2. SilhouetteRasterizationSettings
def test_silhouette_rasterization_settings():
    from st3d import render as R
    assert issubclass(R.SilhouetteRasterizationSettings, R.RasterizationSettings)
    assert R.SilhouetteRasterizationSettings.MAX_FACES_PER_PIXEL == 64 and R.RasterizationSettings.MAX_FACES_PER_PIXEL == 8
    rs = R.SilhouetteRasterizationSettings(image_size=32, blur_radius=9.21e-4, faces_per_pixel=50)
    assert rs.faces_per_pixel == 50 and rs.clip_barycentric_coords and not rs.is_hard and rs.z_clip == 0.5
    assert R.SilhouetteRasterizationSettings(image_size=32, faces_per_pixel=64).faces_per_pixel == 64
    for bad in (0, 65):
        with pytest.raises(NotImplementedError):
            R.SilhouetteRasterizationSettings(image_size=32, faces_per_pixel=bad)
    with pytest.raises(NotImplementedError):
        R.RasterizationSettings(faces_per_pixel=9)              # the general rasteriser stays at 8
    renderer = R.MeshRenderer(R.MeshRasterizer(None, rs), R.SoftSilhouetteShader())
    assert renderer.image_size == 32 and not renderer.is_hard
    with pytest.raises(NotImplementedError, match="SoftSilhouetteShader"):
        R.MeshRenderer(R.MeshRasterizer(None, rs), R.SoftPhongShader())


def test_other_shaders_are_refused_before_any_launch(monkeypatch):
    from st3d import ops, render as R

    def boom(*a, **k):
        raise AssertionError("a kernel was launched")
    for name in ("project_verts", "raster_soft_fwd", "raster_fwd", "silraster_fwd"):
        monkeypatch.setattr(ops, name, boom)
    rs = R.SilhouetteRasterizationSettings(image_size=8, faces_per_pixel=50)
    renderer = R.MeshRenderer(R.MeshRasterizer(None, rs), R.SoftSilhouetteShader())
    renderer.shader = R.SoftPhongShader()           # swapped behind the constructor's back
    mesh, cams = _cpu_mesh()
    with pytest.raises(NotImplementedError, match="SoftSilhouetteShader"):
        renderer.render(mesh, cams)


# ---------------------------------------------------------------------------- 3. the CLI
def test_all_three_parsers_carry_the_flag():
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.silhouette_faces_per_pixel is None
        b = mod.build_parser().parse_args(["--silhouette_weight", "10", "--silhouette_faces_per_pixel", "50",
                                           "--optimization_target", "both"])
        assert b.silhouette_faces_per_pixel == 50 and isinstance(b.silhouette_faces_per_pixel, int)
        for k in ("1", "64"):
            assert mod.build_parser().parse_args(["--silhouette_faces_per_pixel", k]).silhouette_faces_per_pixel == int(k)


def test_a_value_outside_the_range_is_refused_before_any_gpu_work(monkeypatch, capsys):
    import st3d.cli as cli

    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    for mod in _scripts():
        monkeypatch.setattr(mod, "Run", no_gpu)
        for k in ("0", "65", "-3"):
            with pytest.raises(SystemExit) as e:
                mod.main(["--silhouette_weight", "1", "--optimization_target", "mesh", "--silhouette_faces_per_pixel", k])
            assert e.value.code == 2
            assert "silhouette_faces_per_pixel" in capsys.readouterr().err
    args = _scripts()[1].build_parser().parse_args(["--silhouette_weight", "1", "--optimization_target", "mesh",
                                                    "--silhouette_faces_per_pixel", "50"])
    assert cli.check_args(args) is None


def test_weight_zero_runs_no_silhouette_op_of_either_family(monkeypatch):
    import st3d.cli as cli
    from st3d import ops

    def boom(*a, **k):
        raise AssertionError("a silhouette op ran at weight 0")
    for name in ("silhouette_fwd", "silhouette_bwd", "silhouette_loss", "raster_soft_fwd", "silraster_fwd", "silraster_loss",
                 "silraster_bwd"):
        monkeypatch.setattr(ops, name, boom)
    run = cli.Run.__new__(cli.Run)
    run.args = _scripts()[1].build_parser().parse_args(["--optimization_target", "both", "--silhouette_faces_per_pixel", "50"])
    mesh, cams = _cpu_mesh()
    assert run.silhouette_term(mesh, cams, torch.zeros(1, 1, 4, 4), 1) == 0
    run.args.silhouette_weight = 2.0
    assert run.silhouette_term(mesh, None, None, 1) == 0            # a rank without views adds nothing


def test_the_term_hands_the_flag_to_the_loss(monkeypatch):
    import losses as L
    import st3d.cli as cli
    seen = {}

    def fake(renderer, mesh, cams, target, sigma=None, batch_denom=None, faces_per_pixel="missing"):
        seen.update(sigma=sigma, batch_denom=batch_denom, faces_per_pixel=faces_per_pixel)
        return 1.5
    monkeypatch.setattr(L, "compute_silhouette_loss", fake)
    run = cli.Run.__new__(cli.Run)
    run.renderer = None
    mesh, cams = _cpu_mesh()
    for argv, want in ((["--silhouette_faces_per_pixel", "50"], 50), ([], None)):
        run.args = _scripts()[1].build_parser().parse_args(["--optimization_target", "both", "--silhouette_weight", "2"] + argv)
        assert run.silhouette_term(mesh, cams, torch.zeros(1, 1, 4, 4), 4) == 3.0
        assert seen == dict(sigma=1e-4, batch_denom=4, faces_per_pixel=want)


# ---------------------------------------------------------------------------- 4. the C ABI
def test_symbols_are_declared_bound_and_validate_their_arguments():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in ("st3d_silraster_fwd", "st3d_silraster_loss", "st3d_silraster_bwd", "st3d_silraster_bwd_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    lib = _lib.load()
    p = ctypes.c_void_p(4096)           # never dereferenced: validation comes before any launch
    nan = float("nan")
    fwd = lambda *a: lib.st3d_silraster_fwd(*a)
    loss = lambda *a: lib.st3d_silraster_loss(*a)
    bwd = lambda *a: lib.st3d_silraster_bwd(*a)
    # fwd(rec, B, F, S, K, blur, clip, cull, persp, sigma, alpha, state, stream)
    # loss(rec, B, F, S, K, blur, clip, cull, persp, sigma, target, scale, state, partials, loss_out, stream)
    # bwd(rec, ndc, faces, B, V, F, S, blur, clip, cull, persp, z_clip, sigma, state, grad_alpha, grad_scale, g, ws, ws_bytes, stream)
    bad_calls = [
        (fwd, (None, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, p, None)), (fwd, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, None, p, None)),
        (fwd, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, None, None)),
        (fwd, (p, 0, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, p, None)), (fwd, (p, 1, 0, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, p, None)),
        (fwd, (p, 1, 2, 0, 8, 1e-3, 1, 0, 1, 1e-4, p, p, None)),
        (fwd, (p, 1, 2, 4, 0, 1e-3, 1, 0, 1, 1e-4, p, p, None)), (fwd, (p, 1, 2, 4, 65, 1e-3, 1, 0, 1, 1e-4, p, p, None)),
        (fwd, (p, 1, 2, 4, 8, -1e-3, 1, 0, 1, 1e-4, p, p, None)), (fwd, (p, 1, 2, 4, 8, nan, 1, 0, 1, 1e-4, p, p, None)),
        (fwd, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 0.0, p, p, None)), (fwd, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, -1.0, p, p, None)),
        (fwd, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, nan, p, p, None)),
        (fwd, (ctypes.c_void_p(4100), 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, p, None)),             # records not 16-byte aligned
        (loss, (None, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, 1.0, p, p, p, None)), (loss, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, None, 1.0, p, p, p, None)),
        (loss, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, 1.0, None, p, p, None)), (loss, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, 1.0, p, None, p, None)),
        (loss, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, 1.0, p, p, None, None)),
        (loss, (p, 1, 2, 4, 0, 1e-3, 1, 0, 1, 1e-4, p, 1.0, p, p, p, None)), (loss, (p, 1, 2, 4, 65, 1e-3, 1, 0, 1, 1e-4, p, 1.0, p, p, p, None)),
        (loss, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, 0.0, p, 1.0, p, p, p, None)), (loss, (p, 1, 2, 4, 8, 1e-3, 1, 0, 1, nan, p, 1.0, p, p, p, None)),
        (loss, (p, -1, 2, 4, 8, 1e-3, 1, 0, 1, 1e-4, p, 1.0, p, p, p, None)),
        (bwd, (None, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, None, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, None, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, None, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, p, p, 1.0, None, None, 0, None)),
        (bwd, (p, p, p, 1, 0, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.0, 1e-4, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 0.0, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, nan, p, p, 1.0, p, None, 0, None)),
        (bwd, (p, p, p, 1, 3, 2, 4, 1e-3, 1, 0, 1, 0.5, 1e-4, p, p, 1.0, p, p, 16, None)),       # workspace too small
    ]
    for fn, args in bad_calls:
        assert fn(*args) == -1, args
        assert b"invalid argument" in lib.st3d_last_error()
    tiles = 2
    assert lib.st3d_silraster_bwd_workspace_bytes(2, 100, 20) == 16 + ((tiles * tiles * 2 * 4 + 15) & ~15) + 2 * 100 * 3 * 8
