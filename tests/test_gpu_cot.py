"""GPU tests of st3d_mesh_reg_ex: the cotangent Laplacians ('cot', 'cotcurv') and the edge target length against the fp64
restatement (tests/_cotref.py), on the small analytic meshes, the twice-refined icosphere and the cow.

The parity bars are not derived -- Heron's formula in fp32 is ill-conditioned on needle triangles -- but measured: FP32_TORCH
holds, per mesh and method, the error of the same formulas evaluated in fp32 torch on the CPU against fp64 (relative error of
the loss, relative L2 error of the gradient), i.e. what a PyTorch3D user gets in fp32; the kernels may be at most twice as far
off.  (The figures are recorded in DESIGN.md 7 too.  On the tiny meshes fp32 torch happens to return the fp32 number nearest
the fp64 loss; the kernels meet that because they compute in fp64 and round each output once.)"""
import os

import numpy as np
import pytest
import torch

import _cotref as C

pytestmark = pytest.mark.gpu

METHODS = ("cot", "cotcurv")
# (mesh, method) -> (relative loss error, relative L2 gradient error) of fp32 torch against fp64, measured on the CPU
FP32_TORCH = {
    ("tetrahedron", "cot"): (1.615e-08, 9.244e-08), ("tetrahedron", "cotcurv"): (2.388e-08, 2.626e-07),
    ("fan", "cot"): (4.128e-09, 2.643e-07), ("fan", "cotcurv"): (1.856e-07, 4.594e-07),
    ("strip", "cot"): (2.914e-08, 2.054e-07), ("strip", "cotcurv"): (7.325e-08, 2.301e-07),
    ("non_manifold", "cot"): (4.359e-08, 8.608e-08), ("non_manifold", "cotcurv"): (2.767e-07, 4.722e-07),
    ("degenerate", "cot"): (9.997e-08, 9.750e-03), ("degenerate", "cotcurv"): (4.628e-03, 3.419e-02),
    ("unused_vertex", "cot"): (6.961e-08, 9.229e-08), ("unused_vertex", "cotcurv"): (2.388e-08, 2.531e-07),
    ("icosphere2", "cot"): (3.927e-07, 2.251e-05), ("icosphere2", "cotcurv"): (4.106e-07, 1.255e-05),
    ("cow", "cot"): (6.511e-08, 2.553e-05), ("cow", "cotcurv"): (8.403e-07, 4.373e-05),
}
HEADROOM = 2.0
# the four weighted terms together (weights W, edge target = the cow's mean edge length) on the cow, measured the same way
W = [0.7, 1.3, 0.9, 1.1]
FP32_TORCH_ALL_TERMS = {"cot": (4.152e-08, 4.210e-07), "cotcurv": (8.095e-07, 4.259e-05)}
# the edge term with a target: the kernel computes in fp64 from the fp32 vertices and rounds the loss and every gradient
# component to fp32 once (relative error <= 2^-24 = 6e-8 each; the relative L2 error of a vector of such components is no
# larger); 1e-7 leaves room for the fp64 arithmetic itself
EDGE_BAR = 1e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def meshes(cow):
    out = {name: make() for name, make in C.SMALL_MESHES.items()}
    out["cow"] = C.cow_mesh(cow)[:2]
    out["zero_length_edge"] = C.zero_length_edge()       # not a parity mesh of the Laplacian: see its docstring
    return out


@pytest.fixture(scope="module")
def reference(meshes):
    """fp64 loss and gradient of every (mesh, method), computed once"""
    ref = {}
    for name, (v, f) in meshes.items():
        for method in METHODS:
            ref[name, method] = C.loss_and_grad(v.double(), f, lambda a, b: C.laplacian_loss(a, b, method))
    return ref


_TOPOS = {}


def _topos(faces, V, dev):
    from st3d import mesh_losses as ML
    key = (id(faces), V)
    if key not in _TOPOS:
        _TOPOS[key] = (ML.build_topology(faces.to(dev), V), ML.build_cot_topology(faces.to(dev), V), faces)
    return _TOPOS[key][:2]


def _reg_ex(v, f, dev, w, method="uniform", t=0.0, target=None):
    from st3d import ops
    topo, cot = _topos(f, v.shape[0], dev)
    vd = v.to(dev)
    out, grad = ops.mesh_reg_ex(vd, vd if target is None else target.to(dev), topo, cot, w, method, t)
    torch.cuda.synchronize()
    return out.cpu(), grad.cpu()


def _mean_edge(v, f):
    e = C.unique_edges(f)
    return float(np.float32((v.double()[e[:, 0]] - v.double()[e[:, 1]]).norm(dim=1).mean()))


# ---------------------------------------------------------------------------- parity
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(C.SMALL_MESHES) + ["cow"])
def test_laplacian_matches_the_fp64_restatement(dev, meshes, reference, name, method):
    v, f = meshes[name]
    out, grad = _reg_ex(v, f, dev, [0.0, 0.0, 1.0, 0.0], method)
    loss64, grad64 = reference[name, method]
    rel_loss = abs(float(out[3].double()) - float(loss64)) / abs(float(loss64))
    rel_grad = float((grad.double() - grad64).norm() / grad64.norm())
    bar_loss, bar_grad = (HEADROOM * x for x in FP32_TORCH[name, method])
    print(f"{name} {method}: loss {float(out[3]):.9g} rel {rel_loss:.3e} (bar {bar_loss:.3e}), grad rel L2 {rel_grad:.3e} (bar {bar_grad:.3e})")
    assert float(out[0]) == float(out[3]) and float(out[1]) == 0.0          # unit Laplacian weight; target = verts: mse 0
    assert rel_loss <= bar_loss and rel_grad <= bar_grad


@pytest.mark.parametrize("name", ["zero_length_edge", "degenerate", "strip", "cow"])
def test_edge_target_length_matches_the_fp64_restatement(dev, meshes, name):
    v, f = meshes[name]
    for t in (_mean_edge(v, f), 0.75):                                       # fp32 numbers: the C ABI takes the length as a float
        out, grad = _reg_ex(v, f, dev, [0.0, 1.0, 0.0, 0.0], "uniform", t)
        loss64, grad64 = C.loss_and_grad(v.double(), f, lambda a, b: C.edge_loss(a, b, t))
        rel_loss = abs(float(out[2].double()) - float(loss64)) / abs(float(loss64))
        rel_grad = float((grad.double() - grad64).norm() / grad64.norm())
        print(f"{name} t={t:.6g}: edge loss {float(out[2]):.9g} rel {rel_loss:.3e}, grad rel L2 {rel_grad:.3e}")
        assert torch.isfinite(grad).all()                                   # zero_length_edge has one
        assert rel_loss <= EDGE_BAR and rel_grad <= EDGE_BAR


# ---------------------------------------------------------------------------- the defaults, reproducibility, non-finite input
def test_method_uniform_and_target_zero_are_st3d_mesh_reg_bit_for_bit(dev, cow):
    from st3d import ops
    v, f, target = C.cow_mesh(cow)
    topo, cot = _topos(f, v.shape[0], dev)
    vd, td = v.to(dev), target.to(dev)
    for cot_lists in (cot, None):
        for want_grad in (True, False):
            a, ga = ops.mesh_reg(vd, td, topo, W, want_grad=want_grad)
            b, gb = ops.mesh_reg_ex(vd, td, topo, cot_lists, W, "uniform", 0.0, want_grad=want_grad)
            assert torch.equal(a, b) and float(a[0]) > 0.0
            if want_grad:
                assert torch.equal(ga, gb) and bool((ga != 0).any())
            else:
                assert ga is None and gb is None


@pytest.mark.parametrize("name", ["non_manifold", "icosphere2", "cow"])
def test_two_runs_are_bit_equal(dev, meshes, name):
    v, f = meshes[name]
    for method, t in (("uniform", 0.05), ("cot", 0.0), ("cotcurv", 0.0), ("cot", 0.05), ("cotcurv", 0.75)):
        a, ga = _reg_ex(v, f, dev, W, method, t, target=v * 1.01)
        b, gb = _reg_ex(v, f, dev, W, method, t, target=v * 1.01)
        assert torch.equal(a, b) and torch.equal(ga, gb), (method, t)
        assert torch.isfinite(a).all() and torch.isfinite(ga).all()


def test_nan_vertex_gives_nan_loss_and_the_degenerate_face_finite_output(dev, meshes):
    v, f = meshes["tetrahedron"]
    bad = v.clone()
    bad[2, 1] = float("nan")
    for method in METHODS:
        out, _ = _reg_ex(bad, f, dev, [0.0, 0.0, 1.0, 0.0], method)
        assert torch.isnan(out[3]) and torch.isnan(out[0]), method
    out, _ = _reg_ex(bad, f, dev, [0.0, 1.0, 0.0, 0.0], "uniform", 0.5)
    assert torch.isnan(out[2]) and torch.isnan(out[0])
    for name in ("degenerate", "zero_length_edge"):
        v, f = meshes[name]
        for method, t in (("cot", 0.0), ("cotcurv", 0.0), ("cot", 0.5), ("uniform", 0.5)):
            out, grad = _reg_ex(v, f, dev, W, method, t, target=v * 1.01)
            assert torch.isfinite(out).all() and torch.isfinite(grad).all(), (name, method, t)
    # the unused vertex: r = -v under cot (it is pulled to the origin with unit force / V), nothing under cotcurv
    v, f = meshes["unused_vertex"]
    _, grad = _reg_ex(v, f, dev, [0.0, 0.0, 1.0, 0.0], "cot")
    expect = v[4].double() / v[4].double().norm() / v.shape[0]
    assert float((grad[4].double() - expect).abs().max()) <= 1e-7 * float(expect.abs().max())
    _, grad = _reg_ex(v, f, dev, [0.0, 0.0, 1.0, 0.0], "cotcurv")
    assert float(grad[4].abs().max()) == 0.0


# ---------------------------------------------------------------------------- the public functions
def _weights(**kw):
    w = {'mesh_verts_weight': 0.0, 'mesh_edge_loss_weight': 0.0, 'mesh_laplacian_smoothing_weight': 0.0,
         'mesh_normal_consistency_weight': 0.0, 'main_loss_weight': 3.0}
    w.update(kw)
    return w


def test_public_functions_give_the_gradient_of_mesh_terms_with_the_matching_weight(dev, cow):
    from st3d import mesh_losses as ML, render as R
    v, f, target = C.cow_mesh(cow)
    t = _mean_edge(target, f)
    cases = [(lambda m: ML.mesh_laplacian_smoothing(m, method="cot"), _weights(mesh_laplacian_smoothing_weight=1.0, mesh_laplacian_method="cot")),
             (lambda m: ML.mesh_laplacian_smoothing(m, method="cotcurv"), _weights(mesh_laplacian_smoothing_weight=1.0, mesh_laplacian_method="cotcurv")),
             (lambda m: ML.mesh_edge_loss(m, target_length=t), _weights(mesh_edge_loss_weight=1.0, mesh_edge_target_length=t))]
    for fn, weights in cases:
        a = v.to(dev).requires_grad_(True)
        la = fn(R.Meshes(a, f.to(dev)))
        la.backward()
        b = v.to(dev).requires_grad_(True)
        lb = ML.mesh_terms(b, target.to(dev), R.Meshes(b, f.to(dev)), weights)
        lb.backward()
        assert float(la.detach()) == float(lb.detach()) and float(la.detach()) > 0 and torch.equal(a.grad, b.grad) and bool((a.grad != 0).any())
    # the defaults still go where they went
    a = v.to(dev).requires_grad_(True)
    ML.mesh_laplacian_smoothing(R.Meshes(a, f.to(dev))).backward()
    b = v.to(dev).requires_grad_(True)
    ML.mesh_laplacian_smoothing(R.Meshes(b, f.to(dev)), method="uniform").backward()
    c = v.to(dev).requires_grad_(True)
    ML.mesh_terms(c, target.to(dev), R.Meshes(c, f.to(dev)), _weights(mesh_laplacian_smoothing_weight=1.0)).backward()
    assert torch.equal(a.grad, b.grad) and torch.equal(a.grad, c.grad)


@pytest.mark.parametrize("method", METHODS)
def test_mesh_terms_with_everything_on_is_the_weighted_sum_of_the_separate_terms(dev, cow, method):
    from st3d import mesh_losses as ML, render as R
    v, f, target = C.cow_mesh(cow)
    t = _mean_edge(target, f)
    weights = _weights(mesh_verts_weight=W[0], mesh_edge_loss_weight=W[1], mesh_laplacian_smoothing_weight=W[2],
                       mesh_normal_consistency_weight=W[3], mesh_laplacian_method=method, mesh_edge_target_length=t)
    a = v.to(dev).requires_grad_(True)
    fused = ML.mesh_terms(a, target.to(dev), R.Meshes(a, f.to(dev)), weights)
    fused.backward()
    b = v.to(dev).requires_grad_(True)
    mesh = R.Meshes(b, f.to(dev))
    terms = [ML.verts_mse(b, target.to(dev)), ML.mesh_edge_loss(mesh, target_length=t), ML.mesh_laplacian_smoothing(mesh, method=method),
             ML.mesh_normal_consistency(mesh)]
    sum(wk * term for wk, term in zip(W, terms)).backward()
    separate = sum(float(np.float32(wk)) * float(term.detach().double()) for wk, term in zip(W, terms))       # summed in fp64 on the host
    rel_loss = abs(float(fused.detach().double()) - separate) / abs(separate)
    rel_grad = float((a.grad.double() - b.grad.double()).norm() / b.grad.double().norm())
    bar_loss, bar_grad = (HEADROOM * x for x in FP32_TORCH_ALL_TERMS[method])
    print(f"all terms, {method}: fused {float(fused.detach()):.9g} separate {separate:.9g} rel {rel_loss:.3e} (bar {bar_loss:.3e}), "
          f"grad rel L2 {rel_grad:.3e} (bar {bar_grad:.3e})")
    assert rel_loss <= bar_loss and rel_grad <= bar_grad
    # and against the fp64 restatement of the whole objective
    from oracle import mesh_ref as M
    loss64, grad64 = C.loss_and_grad(v.double(), f, lambda x, y: (
        W[0] * M.verts_mse_ref(x, target.double()) + W[1] * C.edge_loss(x, y, t) + W[2] * C.laplacian_loss(x, y, method)
        + W[3] * M.mesh_normal_consistency_ref(x, y)))
    assert abs(float(fused.detach().double()) - float(loss64)) <= 1e-5 * abs(float(loss64))          # tests/test_gpu_kernels.py's bars for
    assert float((a.grad.double().cpu() - grad64).norm() / grad64.norm()) <= 1e-4            # the four fp32 terms together


# ---------------------------------------------------------------------------- one run
def test_second_approach_runs_with_cot_and_the_mean_edge_length(dev, cow, golden_dir, tmp_path, capsys):
    from PIL import Image
    from st3d import io as stio
    import second_approach as SA
    tex = torch.from_numpy(cow["texture_u8"][::16, ::16].copy()).float() / 255
    obj, style = str(tmp_path / "cow.obj"), str(tmp_path / "style.png")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    out = str(tmp_path / "out")
    SA.main(["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "2", "--epochs", "3", "--seed", "0",
             "--optimization_target", "both", "--save_every", "0", "--output_path", out, "--laplacian_method", "cot",
             "--edge_target_length", "mean"])
    assert "Mean edge length of the loaded mesh: 0.0476" in capsys.readouterr().out
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    losses = [float(line.split("Loss ")[1]) for line in lines[1:]]
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert os.path.exists(os.path.join(out, "final.obj"))
    final = stio.load_obj(os.path.join(out, "final.obj"))[0]
    assert torch.isfinite(final).all() and not torch.equal(final, torch.from_numpy(cow["verts"]))
