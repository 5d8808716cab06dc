"""csrc/diffuse.hip and st3d/largesteps.py on the GPU against tests/_largesteps_ref.py: what the row form makes exact (a
constant right-hand side, b = 0, determinism, LDS against global memory, the iteration cap, a NaN column), the accuracy
against the fp64 direct solve with the bound the fp32 restatement sets, the backward, two properties of M^-1, the Adam with
one denominator, the public API with a checkpoint and a resume, and every new wrapper between guard zones."""
import math
import os

import numpy as np
import pytest
import torch

import _guarded as G
import _largesteps_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
LAMBDAS = (1.0, 19.0, 100.0)
TOL = 1e-6
MODULES = ("st3d.largesteps",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def LS():
    from st3d import largesteps
    return largesteps


class _Case:
    """one mesh: its vertices, the device adjacency of build_topology and the numpy restatement's tables (computed once)"""

    def __init__(self, name, verts, faces, dev):
        from st3d.mesh_losses import build_topology
        self.name, self.v, self.f, self.V = name, verts, faces, len(verts)
        topo = build_topology(torch.from_numpy(faces).to(dev), self.V)
        self.off, self.idx = topo["nbr_off"], topo["nbr_idx"]
        self.rows = R.Rows(faces, self.V)
        self._solvers = {}

    def exact(self, lam, b):
        if lam not in self._solvers:
            self._solvers[lam] = R.direct_solver(self.f, self.V, lam)
        return self._solvers[lam](b)

    def cap(self, lam, tol=TOL):
        return R.iteration_cap(lam, self.rows.d_max, tol)


@pytest.fixture(scope="module")
def cases(dev):
    out = {name: _Case(name, v, f, dev) for name, (v, f) in R.meshes().items()}
    for c in out.values():              # the device adjacency is the restatement's, entry for entry
        assert np.array_equal(c.off.cpu().numpy(), c.rows.off) and np.array_equal(c.idx.cpu().numpy(), c.rows.idx), c.name
    assert out["tetrahedron"].V == 4 and out["grid33x32"].V == 1056 and out["cow_loose_vertex"].V == out["cow"].V + 1
    assert out["cow_loose_vertex"].rows.off[-1] == out["cow_loose_vertex"].rows.off[-2]          # degree 0
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _solve(LS, c, b, lam, dev, tol=TOL, max_iter=None):
    x, info = LS.diffuse_solve(c.off, c.idx, _t(b, dev), lam, tol, c.cap(lam, tol) if max_iter is None else max_iter)
    return x, info


# ---------------------------------------------------------------------------- 1. exact
def test_apply_annihilates_constants_and_matches_the_restatement_bit_for_bit(LS, cases, dev):
    rng = np.random.default_rng(0)
    for c in cases.values():
        for const in (1.0, 0.1, -3.7):
            x = np.full((c.V, 3), const, F32)
            assert np.array_equal(_bits(LS.diffuse_apply(c.off, c.idx, _t(x, dev), 19.0)), x.view(np.uint32)), (c.name, const)
        x = rng.standard_normal((c.V, 3)).astype(F32)
        want = np.stack([c.rows.apply32(19.0, x[:, k]) for k in range(3)], 1)
        assert np.array_equal(_bits(LS.diffuse_apply(c.off, c.idx, _t(x, dev), 19.0)), want.view(np.uint32)), c.name
    x = _t(cases["cow"].v, dev)
    assert torch.equal(LS.diffuse_apply(cases["cow"].off, cases["cow"].idx, x, 0.0), x)          # lambda 0: the identity


def test_a_constant_right_hand_side_takes_one_iteration_and_comes_back_bit_for_bit(LS, cases, dev):
    """Ap = p exactly, so alpha = 1, x = b and r = 0"""
    for c in cases.values():
        for const in (1.0, 0.1, -3.7):
            b = np.full((c.V, 3), const, F32)
            x, info = _solve(LS, c, b, 19.0, dev)
            got = LS.read_info(info)
            assert np.array_equal(_bits(x), b.view(np.uint32)), (c.name, const)
            assert got == {"iterations": [1, 1, 1], "converged": [True, True, True], "residual": [0.0, 0.0, 0.0]}, (c.name, const)


def test_a_zero_right_hand_side_takes_no_iteration(LS, cases, dev):
    for c in cases.values():
        x, info = _solve(LS, c, np.zeros((c.V, 3), F32), 19.0, dev)
        assert not _bits(x).any(), c.name                   # +0.0
        assert LS.read_info(info) == {"iterations": [0, 0, 0], "converged": [True, True, True], "residual": [0.0, 0.0, 0.0]}
    c = cases["cow"]
    b = np.zeros((c.V, 3), F32)
    b[:, 1] = np.random.default_rng(2).standard_normal(c.V)             # the columns are independent solves
    x, info = _solve(LS, c, b, 19.0, dev)
    got = LS.read_info(info)
    assert got["iterations"][0] == 0 == got["iterations"][2] and got["iterations"][1] > 10 and got["converged"] == [True] * 3
    assert not _bits(x)[:, [0, 2]].any() and np.isfinite(x.cpu().numpy()).all()


def test_two_runs_and_both_homes_of_the_search_direction_give_the_same_bits(LS, cases, dev, monkeypatch):
    rng = np.random.default_rng(3)
    for c in cases.values():
        b = rng.standard_normal((c.V, 3)).astype(F32)
        monkeypatch.delenv("ST3D_DIFFUSE_LDS", raising=False)
        monkeypatch.delenv("ST3D_DIFFUSE_REGS", raising=False)
        x0, i0 = _solve(LS, c, b, 19.0, dev)                # these meshes: p in LDS; x, r, A p in registers
        x1, i1 = _solve(LS, c, b, 19.0, dev)
        monkeypatch.setenv("ST3D_DIFFUSE_LDS", "0")         # everything in global memory
        x2, i2 = _solve(LS, c, b, 19.0, dev)
        monkeypatch.setenv("ST3D_DIFFUSE_LDS", "1")
        monkeypatch.setenv("ST3D_DIFFUSE_REGS", "0")        # p in LDS; x, r, A p in global memory (what a larger mesh takes)
        x3, i3 = _solve(LS, c, b, 19.0, dev)
        for x, i, what in ((x1, i1, "second run"), (x2, i2, "global memory"), (x3, i3, "LDS without registers")):
            assert torch.equal(x0.view(torch.int32), x.view(torch.int32)) and torch.equal(i0, i), (c.name, what)
        assert all(LS.read_info(i0)["converged"]), c.name


def test_the_loop_ends_at_max_iter_and_says_so(LS, cases, dev):
    c = cases["cow"]
    b = np.random.default_rng(4).standard_normal((c.V, 3)).astype(F32)
    x, info = _solve(LS, c, b, 19.0, dev, max_iter=2)
    got = LS.read_info(info)
    assert got["iterations"] == [2, 2, 2] and got["converged"] == [False] * 3 and all(r > TOL for r in got["residual"])
    assert np.isfinite(x.cpu().numpy()).all()
    want = np.stack([R.cg32(c.rows, 19.0, b[:, k], TOL, 2)[0] for k in range(3)], 1)           # two steps of the restatement
    np.testing.assert_allclose(x.cpu().numpy(), want, rtol=1e-5, atol=1e-6)


def test_a_nan_runs_to_max_iter_in_its_column_alone(LS, cases, dev):
    c = cases["cow"]
    b = np.random.default_rng(5).standard_normal((c.V, 3)).astype(F32)
    clean, clean_info = _solve(LS, c, b, 19.0, dev, max_iter=40)
    bad = b.copy()
    bad[1234, 1] = np.nan
    x, info = _solve(LS, c, bad, 19.0, dev, max_iter=40)
    got, ref = LS.read_info(info), LS.read_info(clean_info)
    assert got["iterations"][1] == 40 and got["converged"][1] is False and math.isnan(got["residual"][1])
    assert torch.isnan(x[:, 1]).all()                       # the first dot product carries it to every row
    for k in (0, 2):
        assert torch.equal(x[:, k].view(torch.int32), clean[:, k].view(torch.int32))
        assert got["iterations"][k] == ref["iterations"][k] and got["residual"][k] == ref["residual"][k]


# ---------------------------------------------------------------------------- 2. accuracy
def _inputs(c, lam, seed):
    rng = np.random.default_rng(seed)
    return (("noise", rng.standard_normal((c.V, 3)).astype(F32)),
            ("M verts", (R.system(c.f, c.V, lam) @ c.v.astype(F64)).astype(F32)))


@pytest.mark.parametrize("name", ["tetrahedron", "grid33x32", "teapot", "cow", "cow_loose_vertex", "two_tetrahedra"])
def test_the_solution_is_as_close_to_the_direct_solve_as_the_restatement(LS, cases, dev, name):
    """||x - x*||_inf / ||x*||_inf against the fp64 sparse LU.  lambda_min(M) >= 1 bounds the error by the true residual,
    which in fp32 stalls near eps kappa for a smooth b, so the residual itself is no yardstick: the bound is 4 x the error
    the fp32 restatement makes on the same input at the same tol (the factor covers another order of the fp64 sums), and
    the iterations stay within the derived cap.
    Measured on an MI355X: see DESIGN 7."""
    c = cases[name]
    for lam in LAMBDAS:
        cap = c.cap(lam)
        for what, b in _inputs(c, lam, 6):
            exact = c.exact(lam, b)
            ref, ref_its, ref_ok = R.cg32_columns(c.rows, lam, b, TOL, cap)
            ref_err = R.relative_max_error(ref, exact)
            x, info = _solve(LS, c, b, lam, dev)
            got = LS.read_info(info)
            err = R.relative_max_error(x.cpu().numpy(), exact)
            print(f"{name} lambda {lam:g} {what}: GPU error {err:.3e} in {got['iterations']} iterations, restatement "
                  f"{ref_err:.3e} in {ref_its}, cap {cap}, residual {max(got['residual']):.2e}")
            assert all(ref_ok) and all(got["converged"]) and max(got["iterations"]) <= cap, (lam, what, got)
            assert all(r <= TOL * (1 + 1e-6) for r in got["residual"])          # sqrt(rr / bb) rounded to fp32
            assert err <= 4.0 * ref_err, (lam, what, err, ref_err)


def test_the_backward_is_the_same_solve(LS, cases, dev):
    """loss = sum w * verts(): d loss / d params = M^-T w = M^-1 w, under the bound of the forward test"""
    c = cases["cow"]
    dv = LS.DiffusedVertices(_t(c.v, dev), _t(c.f, dev), 19.0)
    assert dv.max_iter == c.cap(19.0) and dv.params.is_leaf and dv.params.device.type == "cuda"
    w = np.random.default_rng(7).standard_normal((c.V, 3)).astype(F32)
    verts = dv.verts()
    (verts * _t(w, dev)).sum().backward()
    exact = c.exact(19.0, w)
    ref_err = R.relative_max_error(R.cg32_columns(c.rows, 19.0, w, TOL, dv.max_iter)[0], exact)
    err = R.relative_max_error(dv.params.grad.cpu().numpy(), exact)
    print(f"backward: GPU error {err:.3e}, restatement {ref_err:.3e}")
    assert err <= 4.0 * ref_err
    fwd, bwd = dv.last_info(), dv.last_info(backward=True)
    assert all(fwd["converged"]) and all(bwd["converged"]) and max(fwd["iterations"] + bwd["iterations"]) <= dv.max_iter
    # v(u0) is the loaded mesh to the solve's error, relative to the extent
    u = dv.params.detach().cpu().numpy()
    ref_fwd = R.relative_max_error(R.cg32_columns(c.rows, 19.0, u, TOL, dv.max_iter)[0], c.exact(19.0, u))
    assert R.relative_max_error(verts.detach().cpu().numpy(), c.exact(19.0, u)) <= 4.0 * ref_fwd
    assert np.abs(verts.detach().cpu().numpy() - c.v).max() <= 1e-5 * np.abs(c.v).max()


def test_the_solve_smooths_and_never_overshoots(LS, cases, dev):
    """evaluated in fp64 on the host: x^T L x <= b^T L b (every eigen-component is scaled by 1 / (1 + lam mu) <= 1), and
    max |x| <= max |b| (1 + 4 tol) (M^-1 is entrywise non-negative with unit row sums; the rest is the solve's error)"""
    for c in cases.values():
        b = np.random.default_rng(8).standard_normal((c.V, 3)).astype(F32)
        x = _solve(LS, c, b, 19.0, dev)[0].cpu().numpy().astype(F64)
        L = R.laplacian(c.f, c.V)
        b64 = b.astype(F64)
        for k in range(3):
            assert x[:, k] @ (L @ x[:, k]) <= b64[:, k] @ (L @ b64[:, k]), (c.name, k)
            assert np.abs(x[:, k]).max() <= np.abs(b64[:, k]).max() * (1.0 + 4.0 * TOL), (c.name, k)


# ---------------------------------------------------------------------------- 3. Adam with one denominator
@pytest.mark.parametrize("n", [5000, 300001])           # one pass of the grid, and more elements than the grid has threads
def test_the_uniform_adam_matches_its_restatement(LS, dev, n):
    """three steps; the tolerance of test_gpu_kernels.test_adam_matches_torch_optim"""
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.1 + i) for i in range(3)]
    pr, mr, sr = p0.clone(), torch.zeros(n), torch.zeros(n)
    p = p0.clone().to(dev)
    m, s = torch.zeros_like(p), torch.zeros_like(p)
    for i, g in enumerate(grads):
        R.adam_uniform_step(pr, g, mr, sr, i + 1, 0.01)
        LS.adam_step_uniform(p, g.to(dev), m, s, i + 1, 0.01)
    torch.testing.assert_close(p.cpu(), pr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m.cpu(), mr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(s.cpu(), sr, rtol=1e-5, atol=1e-6)


def test_the_uniform_adam_has_one_denominator_and_is_deterministic(LS, dev):
    n, lr = 70000, 0.01
    g = torch.zeros(n)
    g[n - 3] = 10.0                                         # one-hot, in the last block
    p, m, s = (torch.zeros(n, device=dev) for _ in range(3))
    LS.adam_step_uniform(p, g.to(dev), m, s, 1, lr)
    moved = p.cpu()
    assert int((moved != 0).sum()) == 1 and abs(float(moved[n - 3]) + lr) <= 1e-8           # lr g / (eps + |g|)
    g2 = 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(1))
    before = p.clone()
    LS.adam_step_uniform(p, g2.to(dev), m, s, 2, lr)
    denom = 1e-8 + math.sqrt(float(s[n - 3]) / (1 - 0.999 ** 2))          # the one large second moment sets it for everybody
    want = lr * (m.cpu().double() / (1 - 0.9 ** 2)) / denom
    keep = torch.arange(n) != n - 3
    torch.testing.assert_close((before - p).cpu().double()[keep], want[keep], rtol=1e-5, atol=1e-10)
    # plain Adam would have moved every one of them by about lr
    assert float((before - p).abs().cpu()[keep].max()) < 0.01 * lr
    q, mq, sq = (torch.zeros(n, device=dev) for _ in range(3))
    LS.adam_step_uniform(q, g.to(dev), mq, sq, 1, lr)
    LS.adam_step_uniform(q, g2.to(dev), mq, sq, 2, lr)
    assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    bad = g2.clone()
    bad[17] = float("nan")
    LS.adam_step_uniform(q, bad.to(dev), mq, sq, 3, lr)
    assert torch.isnan(q).all()                             # a NaN moment is the maximum: it reaches every parameter


# ---------------------------------------------------------------------------- 4. through the public API
def _cow_mesh(cow, dev, T=32):
    import utils as U
    tex = torch.from_numpy(cow["texture_u8"][::1024 // T, ::1024 // T].copy()).float().div(255)[None].to(dev)
    return U.build_mesh(torch.from_numpy(cow["verts_uvs"])[None].to(dev),
                        torch.from_numpy(cow["faces_uvs"].astype(np.int64))[None].to(dev), tex,
                        torch.from_numpy(cow["verts"]).to(dev), torch.from_numpy(cow["faces"].astype(np.int64)).to(dev))


def test_one_step_from_a_render_gradient_moves_no_vertex_further_than_lr(LS, cow, dev):
    """Adam's first uniform step moves every entry of u by lr |g| / (eps + max |g|) <= lr, and M^-1 is entrywise non-negative
    with unit row sums, so no coordinate of any vertex moves by more than lr (1 + 4 tol)"""
    import losses as L
    import style_transfer as ST
    import utils as U
    from oracle import render_ref as RR
    from st3d.render import FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    U.device = ST.device = L.device = dev
    lr, S, B = 0.01, 64, 2
    mesh0 = _cow_mesh(cow, dev)
    out = U.setup_optimizations('mesh', mesh0, lr, verts_diffusion=19)
    dv = out["verts_diffusion"]
    assert isinstance(dv, LS.DiffusedVertices) and len(out["optimizer"].params) == 1 and out["optimizer"].params[0] is dv.params
    assert out["optimizer"].param_groups[0]["uniform"] is True and not out["texture_map"].requires_grad
    g = torch.Generator().manual_seed(0)
    elev, azim = RR.random_camera_angles(B, lambda k: torch.rand(k, generator=g).numpy())
    Rm, Tt = RR.look_at_view_transform(2.10, elev, azim, at=(0, 0.10, 0.25))
    cams = FoVPerspectiveCameras(R=torch.from_numpy(Rm), T=torch.from_numpy(Tt), device=dev)
    renderer = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftPhongShader())
    before = out["verts"].detach().clone()
    mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
    img, _ = U.render_meshes(renderer, mesh, cams)
    target = torch.rand(img.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    out["optimizer"].zero_grad()
    ((img - target) ** 2).mean().backward()
    grad = dv.params.grad
    assert grad is not None and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    u_before = dv.params.detach().clone()
    out["optimizer"].step()
    # lr |g| / (eps + max |g|) to a few roundings, subtracted from u at u's own spacing
    assert float((dv.params.detach() - u_before).abs().max()) <= lr * (1 + 1e-6) + float(np.spacing(F32(u_before.abs().max().item())))
    stale = out["verts"]
    assert U.refresh_verts(out) is out["verts"] and out["verts"] is not stale
    fresh = dv.verts()
    assert torch.equal(out["verts"].detach().view(torch.int32), fresh.detach().view(torch.int32))
    moved = (out["verts"].detach() - before).abs()
    print(f"largest move of a vertex coordinate {float(moved.max()):.3e} of lr = {lr}")
    assert float(moved.max()) > 0 and float(moved.max()) <= lr * (1 + 4 * TOL)
    assert all(dv.last_info()["converged"]) and all(dv.last_info(backward=True)["converged"])


def test_the_regularisers_see_this_steps_vertices(LS, cases, dev):
    """verts() hands out a fresh tensor (version 0) every step, at an address the allocator recycles: the regularisers'
    per-tensor cache must not take it for the vertices of an earlier step"""
    from st3d import mesh_losses as ML
    from st3d import render as RD
    c = cases["cow"]
    dv = LS.DiffusedVertices(_t(c.v, dev), _t(c.f, dev), 19.0)
    faces = _t(c.f, dev)
    e = np.unique(np.sort(np.concatenate([c.f[:, [1, 2]], c.f[:, [2, 0]], c.f[:, [0, 1]]]), 1), axis=0)
    gen = torch.Generator().manual_seed(0)
    held = None
    for step in range(6):
        with torch.no_grad():
            dv.params.add_((0.5 * torch.randn(dv.params.shape, generator=gen)).to(dev))
        held = verts = dv.verts()                       # the previous step's tensor is released here, as in cli.Run
        got = float(ML.mesh_edge_loss(RD.Meshes([verts], [faces])))
        v64 = verts.detach().cpu().double().numpy()
        want = float((np.linalg.norm(v64[e[:, 0]] - v64[e[:, 1]], axis=1) ** 2).mean())
        assert abs(got - want) <= 1e-4 * want, (step, got, want)


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


def _losses(folder):
    return [line.split("Loss ")[1] for line in open(os.path.join(folder, "log.txt")).read().splitlines()[1:]]


def test_three_steps_a_checkpoint_and_three_more_equal_six_straight_steps(dev, cow, golden_dir, tmp_path, capsys):
    import losses as L
    import second_approach as SA
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0",
              "--optimization_target", "mesh", "--verts_lr", "0.002", "--save_every", "0", "--epochs", "6"]
    flag = ["--verts_diffusion", "19"]
    full, part = str(tmp_path / "full"), str(tmp_path / "part")
    SA.main(common + flag + ["--output_path", full])
    said = capsys.readouterr().out
    assert "Vertex diffusion: lambda 19, largest degree 8, at most 254 CG iterations" in said and "WARNING: the" not in said
    SA.main(common[:-2] + flag + ["--epochs", "3", "--output_path", part, "--checkpoint_every", "3"])
    ck3 = os.path.join(part, "checkpoint.pt")
    blob = torch.load(ck3, map_location="cpu", weights_only=True)
    assert blob["progress"] == 3 and blob["verts_diffusion_lambda"] == 19.0 and blob["verts_diffusion"].shape == (2930, 3)
    assert blob["optimizer"]["lrs"] == [0.002] and len(blob["optimizer"]["state"]) == 1
    resumed = str(tmp_path / "resumed")
    SA.main(common + flag + ["--output_path", resumed, "--resume", ck3])
    lf, lp, lr_ = _losses(full), _losses(part), _losses(resumed)
    print("losses", lf, "first three", lp, "resumed", lr_)
    assert len(lf) == 6 and len(lp) == 3 and len(lr_) == 3 and all(math.isfinite(float(v)) for v in lf)
    assert lp == lf[:3] and lr_ == lf[3:]
    assert open(os.path.join(full, "final.obj")).read() == open(os.path.join(resumed, "final.obj")).read()
    for bad in (["--verts_diffusion", "5"], []):
        with pytest.raises(ValueError, match="verts_diffusion"):
            SA.main(common + bad + ["--output_path", str(tmp_path / "bad"), "--resume", ck3])


def test_second_approach_on_both_targets_ends_finite_with_a_mesh(dev, cow, golden_dir, tmp_path):
    import losses as L
    import second_approach as SA
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    outp = str(tmp_path / "both")
    SA.main(["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0",
             "--optimization_target", "both", "--verts_diffusion", "19", "--epochs", "2", "--save_every", "0",
             "--output_path", outp])
    losses = _losses(outp)
    assert len(losses) == 2 and all(math.isfinite(float(v)) for v in losses)
    from st3d import io as stio
    verts, faces, _ = stio.load_obj(os.path.join(outp, "final.obj"))
    assert verts.shape == (2930, 3) and torch.isfinite(verts).all() and faces.verts_idx.shape == (5856, 3)
    assert float((verts - torch.from_numpy(cow["verts"])).abs().max()) > 0          # the vertices did move
    assert len(os.listdir(os.path.join(outp, "final_render"))) == 12


# ---------------------------------------------------------------------------- 5. between guard zones
@pytest.mark.parametrize("lds,regs", [("1", "1"), ("1", "0"), ("0", "1")], ids=["registers", "lds", "global"])
@pytest.mark.parametrize("name", ["tetrahedron", "grid33x32"])
def test_every_wrapper_between_guard_zones(LS, cases, dev, monkeypatch, name, lds, regs):
    """no guard byte changes, every output is the shim's or the caller's, A == B bit for bit (nothing -- the workspace and
    the partials included -- is read before it is written) and the plain run == A"""
    monkeypatch.setenv("ST3D_DIFFUSE_LDS", lds)
    monkeypatch.setenv("ST3D_DIFFUSE_REGS", regs)
    c = cases[name]
    rng = np.random.default_rng(9)
    b = _t(rng.standard_normal((c.V, 3)).astype(F32), dev)

    def apply():
        return {"y": LS.diffuse_apply(c.off, c.idx, b, 19.0)}

    def solve():
        x, info = LS.diffuse_solve(c.off, c.idx, b, 19.0, TOL, c.cap(19.0))
        return {"x": x, "info": info}

    def solve_capped():
        x, info = LS.diffuse_solve(c.off, c.idx, b, 100.0, TOL, 2)
        return {"x": x, "info": info}

    n = 3 * c.V
    g = _t(rng.standard_normal(n).astype(F32), dev)

    def adam():
        p, m, s = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        LS.adam_step_uniform(p, g, m, s, 1, 0.01)
        LS.adam_step_uniform(p, g * 0.5, m, s, 2, 0.01)
        return {"p": p, "m": m, "s": s}

    G.compare_ab(apply, modules=MODULES)
    out = G.compare_ab(solve, modules=MODULES)
    assert all(LS.read_info(out["info"])["converged"])
    G.compare_ab(solve_capped, modules=MODULES)
    G.compare_ab(adam, modules=MODULES, own=lambda o: [o["p"], o["m"], o["s"]])


def test_a_diffused_step_between_guard_zones(LS, cases, dev):
    """DiffusedVertices.verts() and its backward allocate through the same wrappers"""
    c = cases["grid33x32"]
    dv = LS.DiffusedVertices(_t(c.v, dev), _t(c.f, dev), 19.0)
    w = _t(np.random.default_rng(10).standard_normal((c.V, 3)).astype(F32), dev)

    def step():
        dv.params.grad = None
        v = dv.verts()
        (v * w).sum().backward()
        return {"verts": v, "grad": dv.params.grad}

    G.compare_ab(step, modules=MODULES, own=lambda o: [o["grad"]])          # .grad is autograd's: the solve's output or its copy
