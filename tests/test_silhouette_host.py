"""Host side of the silhouette feature: the fp64 restatement (tests/_silhouette_ref.py) pinned to softmax_rgb_blend's alpha
and to analytic cases, SoftSilhouetteShader's defaults and validation, the CLI flags, the C ABI's argument checks, and the
silhouette fit on the CPU reference.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _silhouette_ref as SIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_fragments(seed, n=1000, K=8, sigma=1e-4):
    g = torch.Generator().manual_seed(seed)
    dists = (torch.rand(n, K, generator=g, dtype=torch.float64) * 2 - 1) * 6 * sigma
    mask = torch.rand(n, K, generator=g) > 0.3
    mask[:5] = False                                    # some pixels without any face
    return dists, mask


# ---------------------------------------------------------------------------- 1. the restatement
def test_restatement_equals_the_alpha_of_softmax_rgb_blend():
    from oracle import soft_ref as SR
    for sigma in (1e-4, 1e-3):
        dists, mask = _random_fragments(0, sigma=sigma)
        g = torch.Generator().manual_seed(1)
        colors = torch.rand(dists.shape + (3,), generator=g, dtype=torch.float64)
        zbuf = 1.0 + torch.rand(dists.shape, generator=g, dtype=torch.float64)
        _, alpha = SR.softmax_rgb_blend(colors, zbuf, dists, mask, sigma, 1e-4)
        assert float((SIL.sigmoid_alpha_blend(dists, mask, sigma) - alpha).abs().max()) <= 1e-14


def test_restatement_analytic_cases():
    s = 1e-4
    one = SIL.sigmoid_alpha_blend(torch.zeros(1, 1, dtype=torch.float64), torch.ones(1, 1, dtype=torch.bool), s)
    assert float(one) == 0.5                                             # one layer on the edge
    d = torch.tensor([[-0.7e-4, 1.3e-4]], dtype=torch.float64)
    p1, p2 = 1 / (1 + math.exp(-0.7)), 1 / (1 + math.exp(1.3))
    both = SIL.sigmoid_alpha_blend(d, torch.ones(1, 2, dtype=torch.bool), s)
    assert abs(float(both) - (1 - (1 - p1) * (1 - p2))) <= 1e-15
    only_second = SIL.sigmoid_alpha_blend(d, torch.tensor([[False, True]]), s)
    assert abs(float(only_second) - p2) <= 1e-15                         # masked layers are ignored
    assert float(SIL.sigmoid_alpha_blend(d, torch.zeros(1, 2, dtype=torch.bool), s)) == 0.0      # nothing covers the pixel
    deep = SIL.sigmoid_alpha_blend(torch.tensor([[-1.0]], dtype=torch.float64), torch.ones(1, 1, dtype=torch.bool), s)
    assert float(deep) == 1.0


def test_closed_form_gradient_equals_autograd():
    """d alpha / d dists_k = -prob_k * prod_j (1 - prob_j) / sigma, the form the kernels use (no division by 1 - prob_k)."""
    dists, mask = _random_fragments(2)
    d = dists.clone().requires_grad_(True)
    w = torch.rand(d.shape[0], generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (SIL.sigmoid_alpha_blend(d, mask, 1e-4) * w).sum().backward()
    closed = SIL.alpha_grad_closed_form(dists, mask, 1e-4) * w[:, None]
    assert float((closed - d.grad).norm()) <= 1e-12 * float(d.grad.norm())
    assert float(d.grad[~mask].abs().max()) == 0.0 and float(closed[~mask].abs().max()) == 0.0
    # saturated layer (prob -> 1): finite and zero, where dividing the product by (1 - prob) would give 0 / 0
    sat = SIL.alpha_grad_closed_form(torch.tensor([[-1.0, 0.0]], dtype=torch.float64), torch.ones(1, 2, dtype=torch.bool), 1e-4)
    assert torch.isfinite(sat).all() and float(sat.abs().max()) == 0.0


# ---------------------------------------------------------------------------- 2. the Python surface
def test_soft_silhouette_shader_defaults_and_renderer():
    from st3d import render as R
    sh = R.SoftSilhouetteShader()
    assert sh.blend_params.sigma == 1e-4
    assert R.SoftSilhouetteShader(blend_params=R.BlendParams(sigma=3e-4)).blend_params.sigma == 3e-4
    rs = R.RasterizationSettings(image_size=32)
    renderer = R.MeshRenderer(R.MeshRasterizer(None, rs), sh)
    assert renderer.image_size == 32
    assert not renderer.is_hard                 # always the general rasteriser: render_meshes thresholds its alpha
    assert R.MeshRenderer(R.MeshRasterizer(None, rs), R.SoftPhongShader()).is_hard
    with pytest.raises(ValueError):
        R.SoftSilhouetteShader(blend_params=R.BlendParams(sigma=0.0))


def _cpu_mesh():
    from st3d import render as R
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    return R.Meshes(verts, torch.tensor([[0, 1, 2]])), R.FoVPerspectiveCameras(T=torch.tensor([[0.0, 0, 3]]))


def test_cpu_tensors_are_refused():
    import losses as L
    from st3d import _lib, ops, render as R
    p2f = torch.zeros(1, 4, 4, 2, dtype=torch.int32)
    d = torch.zeros(1, 4, 4, 2)
    a = torch.zeros(1, 1, 4, 4)
    with pytest.raises(_lib.St3dError):
        ops.silhouette_fwd(p2f, d, 1e-4)
    with pytest.raises(_lib.St3dError):
        ops.silhouette_bwd(a, p2f, d, 1e-4)
    with pytest.raises(_lib.St3dError):
        ops.silhouette_loss(p2f, d, a, 1e-4, 1.0)
    mesh, cams = _cpu_mesh()                    # a mesh without textures is accepted up to the first device call
    renderer = R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=4)), R.SoftSilhouetteShader())
    with pytest.raises(_lib.St3dError):
        renderer.render(mesh, cams)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.compute_silhouette_loss(renderer, mesh, cams, a)


def test_sigma_must_be_positive():
    import losses as L
    from st3d import ops, render as R
    p2f = torch.zeros(1, 4, 4, 2, dtype=torch.int32)
    d = torch.zeros(1, 4, 4, 2)
    a = torch.zeros(1, 1, 4, 4)
    for bad in (0.0, -1e-4, float("nan")):
        with pytest.raises(ValueError):
            ops.silhouette_fwd(p2f, d, bad)
        with pytest.raises(ValueError):
            ops.silhouette_bwd(a, p2f, d, bad)
        with pytest.raises(ValueError):
            ops.silhouette_loss(p2f, d, a, bad, 1.0)
        mesh, cams = _cpu_mesh()
        with pytest.raises(ValueError):
            L.compute_silhouette_loss(R.RasterizationSettings(image_size=4), mesh, cams, a, sigma=bad)


def test_silhouette_pass_raster_settings():
    import losses as L
    assert L.SILHOUETTE_FACES_PER_PIXEL == 8
    assert L.silhouette_blur_radius(1e-4) == pytest.approx(math.log(1.0 / 1e-4 - 1.0) * 1e-4, rel=1e-15)
    assert L.silhouette_blur_radius(1e-4) == pytest.approx(9.21e-4, rel=1e-3)


# ---------------------------------------------------------------------------- 3. the CLI
def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_all_three_parsers_carry_the_flags_with_their_defaults():
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.silhouette_weight == 0.0 and a.silhouette_sigma == 1e-4
        b = mod.build_parser().parse_args(["--silhouette_weight", "10", "--silhouette_sigma", "3e-4",
                                           "--optimization_target", "both"])
        assert b.silhouette_weight == 10.0 and b.silhouette_sigma == 3e-4


def test_silhouette_weight_with_texture_target_is_refused_before_any_gpu_work(monkeypatch, capsys):
    import st3d.cli as cli

    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    for mod in _scripts():
        monkeypatch.setattr(mod, "Run", no_gpu)
        for argv in (["--silhouette_weight", "1", "--optimization_target", "texture"], ["--silhouette_weight", "1"],
                     ["--silhouette_sigma", "0", "--optimization_target", "mesh"]):
            with pytest.raises(SystemExit) as e:
                mod.main(argv)
            assert e.value.code == 2
        assert "silhouette" in capsys.readouterr().err
    ok = cli.check_args(_scripts()[1].build_parser().parse_args(["--silhouette_weight", "1", "--optimization_target", "mesh"]))
    assert ok is None


def test_weight_zero_runs_no_silhouette_op(monkeypatch):
    import st3d.cli as cli
    from st3d import ops

    def boom(*a, **k):
        raise AssertionError("a silhouette op ran at weight 0")
    for name in ("silhouette_fwd", "silhouette_bwd", "silhouette_loss", "raster_soft_fwd"):
        monkeypatch.setattr(ops, name, boom)
    run = cli.Run.__new__(cli.Run)
    run.args = _scripts()[1].build_parser().parse_args(["--optimization_target", "both"])
    mesh, cams = _cpu_mesh()
    assert run.silhouette_term(mesh, cams, torch.zeros(1, 1, 4, 4), 1) == 0
    run.args.silhouette_weight = 2.0
    assert run.silhouette_term(mesh, None, None, 1) == 0            # a rank without views adds nothing


# ---------------------------------------------------------------------------- 4. the C ABI
def test_symbols_are_declared_bound_and_validate_their_arguments():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    names = ("st3d_silhouette_fwd", "st3d_silhouette_bwd", "st3d_silhouette_loss")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    lib = _lib.load()
    p = ctypes.c_void_p(4096)           # never dereferenced: validation comes before any launch
    fwd = lambda *a: lib.st3d_silhouette_fwd(*a)
    bwd = lambda *a: lib.st3d_silhouette_bwd(*a)
    loss = lambda *a: lib.st3d_silhouette_loss(*a)
    bad_calls = [
        (fwd, (None, p, 1, 4, 2, 1e-4, p, None)), (fwd, (p, None, 1, 4, 2, 1e-4, p, None)), (fwd, (p, p, 1, 4, 2, 1e-4, None, None)),
        (fwd, (p, p, 0, 4, 2, 1e-4, p, None)), (fwd, (p, p, 1, 0, 2, 1e-4, p, None)), (fwd, (p, p, 1, 4, 0, 1e-4, p, None)),
        (fwd, (p, p, 1, 4, 9, 1e-4, p, None)), (fwd, (p, p, 1, 4, 2, 0.0, p, None)), (fwd, (p, p, 1, 4, 2, -1.0, p, None)),
        (fwd, (p, p, 1, 4, 2, float("nan"), p, None)),
        (bwd, (None, p, p, 1, 4, 2, 1e-4, 0, p, None)), (bwd, (p, p, p, 1, 4, 2, 1e-4, 0, None, None)),
        (bwd, (p, p, p, 1, 4, 9, 1e-4, 0, p, None)), (bwd, (p, p, p, 1, 4, 2, 0.0, 1, p, None)), (bwd, (p, p, p, -1, 4, 2, 1e-4, 1, p, None)),
        (loss, (p, p, None, 1, 4, 2, 1e-4, 1.0, p, p, p, None)), (loss, (p, p, p, 1, 4, 2, 1e-4, 1.0, p, None, p, None)),
        (loss, (p, p, p, 1, 4, 2, 1e-4, 1.0, p, p, None, None)), (loss, (p, p, p, 1, 4, 0, 1e-4, 1.0, None, p, p, None)),
        (loss, (p, p, p, 1, 4, 2, 0.0, 1.0, None, p, p, None)), (loss, (p, p, p, 1, 0, 2, 1e-4, 1.0, None, p, p, None)),
    ]
    for fn, args in bad_calls:
        assert fn(*args) == -1, args
        assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 5. the fit on the CPU reference
@pytest.mark.parametrize("displacement", ["shift", "scale"])
def test_silhouette_fit_on_the_reference_recovers_the_outline(cow, displacement):
    """Cow displaced by (0.06, 0.03, 0) / scaled by 1.08, S = 64, four views, K = 8, sigma 1e-4, targets = hard coverage of
    the undisplaced cow, Adam(lr 0.005), 40 steps on the fp64 restatement: the loss falls to <= 0.45 of its first value
    (measured: 0.338 shifted, 0.321 scaled)."""
    losses = SIL.fit_on_the_reference(cow, displacement, nthreads=min(8, os.cpu_count() or 1))
    assert all(np.isfinite(losses))
    print(f"{displacement}: first {losses[0]:.6f} last {losses[-1]:.6f} ratio {losses[-1] / losses[0]:.4f}")
    assert losses[-1] / losses[0] <= SIL.FIT["bound"], (losses[0], losses[-1])
