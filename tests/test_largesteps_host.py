"""Host side of --verts_diffusion: the C ABI's refusals (which launch nothing), the Python wrappers' validation and their
refusal of CPU tensors, DiffusedVertices' set-up arithmetic, the "uniform" Adam group, setup_optimizations with the flag off
(today's dict) and on (the wiring, on a numpy solve), the flag on all three scripts and the checkpoint keys.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import _largesteps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_diffuse_apply", "st3d_diffuse_workspace_bytes", "st3d_diffuse_solve", "st3d_adam_step_uniform")
NAN, INF = float("nan"), float("inf")


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_bound_and_built_without_contraction():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    assert re.search(r'"diffuse\.hip":\s*\[[^\]]*"-ffp-contract=off"', build)


def test_workspace_size_is_pure_host_logic():
    from st3d import _lib
    lib = _lib.load()
    for V, padded in ((1, 4), (4, 4), (5, 8), (1056, 1056), (2930, 2932), (47000, 47000)):
        assert lib.st3d_diffuse_workspace_bytes(V) == 9 * padded * 4
    assert lib.st3d_diffuse_workspace_bytes(0) == 0 and lib.st3d_diffuse_workspace_bytes(-3) == 0


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, q, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4100)            # never dereferenced
    need = lib.st3d_diffuse_workspace_bytes(100)

    def variants(good, pointers, values):
        out = [good[:i] + [None] + good[i + 1:] for i in pointers]
        out += [good[:i] + [v] + good[i + 1:] for i, vs in values.items() for v in vs]
        return out
    lams, sizes = (-1.0, -1e-30, NAN, INF, -INF), (0, -1)
    cases = {
        #                    off idx V    lam   x  y  stream
        "st3d_diffuse_apply": variants([p, p, 100, 19.0, p, q, None], (0, 1, 4, 5), {2: sizes, 3: lams, 5: (p,)}),
        #                    off idx V    lam   b  x  tol   max_iter ws bytes info stream
        "st3d_diffuse_solve": variants([p, p, 100, 19.0, p, q, 1e-6, 50, p, need, p, None], (0, 1, 4, 5, 8, 10),
                                       {2: sizes, 3: lams, 5: (p,), 6: (0.0, -1e-6, NAN, INF), 7: (0, -1), 8: (odd,),
                                        9: (0, need - 1), 10: (ctypes.c_void_p(4098),)}),
        #                        p  g  m  v  n    step lr    b1   b2     eps   partials stream
        "st3d_adam_step_uniform": variants([p, p, p, p, 300, 1, 0.01, 0.9, 0.999, 1e-8, p, None], (0, 1, 2, 3, 10),
                                           {4: (0,), 5: (0, -1)}),
    }
    for name, bad in cases.items():
        assert len(bad) >= 7
        for args in bad:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 2. the Python wrappers
def _tetra():
    v, f = R.tetrahedron()
    off, idx = R.adjacency(f, 4)
    return torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(off).int(), torch.from_numpy(idx).int()


def test_the_wrappers_live_outside_ops_and_refuse_cpu_tensors():
    from st3d import largesteps as LS
    from st3d import ops
    for name in ("diffuse_apply", "diffuse_solve", "adam_step_uniform"):
        assert callable(getattr(LS, name)) and not hasattr(ops, name)
    v, f, off, idx = _tetra()
    for call in (lambda: LS.diffuse_apply(off, idx, v, 19.0), lambda: LS.diffuse_solve(off, idx, v, 19.0),
                 lambda: LS.adam_step_uniform(v.clone(), v, torch.zeros(4, 3), torch.zeros(4, 3), 1, 0.01)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_wrappers_validate_before_they_call():
    from st3d import largesteps as LS
    v, f, off, idx = _tetra()
    for lam in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match="lambda"):
            LS.diffuse_apply(off, idx, v, lam)
        with pytest.raises(ValueError, match="lambda"):
            LS.diffuse_solve(off, idx, v, lam)
    for tol in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="tol"):
            LS.diffuse_solve(off, idx, v, 19.0, tol=tol)
    for cap in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="max_iter"):
            LS.diffuse_solve(off, idx, v, 19.0, max_iter=cap)
    for bad in (torch.zeros(4), torch.zeros(4, 2), torch.zeros(0, 3), torch.zeros(5, 3)):
        with pytest.raises(ValueError):
            LS.diffuse_solve(off, idx, bad, 19.0)
    with pytest.raises(TypeError):
        LS.diffuse_apply(off, idx, [[0.0, 0.0, 0.0]], 19.0)


def test_diffused_vertices_sets_up_the_leaf_the_cap_and_the_topology():
    from st3d import largesteps as LS
    for name in ("cow", "teapot"):
        v, f = R.fixture(name)
        dv = LS.DiffusedVertices(torch.from_numpy(v), torch.from_numpy(f), 19.0)
        off, idx = R.adjacency(f, len(v))
        assert np.array_equal(dv.nbr_off.numpy(), off) and np.array_equal(dv.nbr_idx.numpy(), idx)
        want = (R.system(f, len(v), 19.0) @ v.astype(np.float64)).astype(np.float32)          # fp64 on the host, rounded once
        assert dv.params.is_leaf and dv.params.requires_grad and dv.params.dtype == torch.float32
        got = dv.params.detach().numpy()      # another fp64 summation order: 1e-12 where the terms cancel, else the same rounding
        assert (np.abs(got - want) <= np.spacing(np.abs(want)) + 1e-12).all() and (got == want).mean() > 0.999, name
        assert dv.max_degree == np.diff(off).max() and dv.max_iter == R.iteration_cap(19.0, dv.max_degree, 1e-6)
        assert dv.last_info() is None and dv.last_info(backward=True) is None
        assert dv.max_iter == {"cow": 254, "teapot": 439}[name]
    v, f = R.fixture("cow")
    assert LS.DiffusedVertices(torch.from_numpy(v), torch.from_numpy(f), 19.0, max_iter=7).max_iter == 7
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for kw in ({"lam": 0.0}, {"lam": -1.0}, {"lam": NAN}, {"lam": 19.0, "tol": 0.0}, {"lam": 19.0, "max_iter": 0}):
        with pytest.raises(ValueError):
            LS.DiffusedVertices(tv, tf, **kw)
    with pytest.raises(ValueError, match="outside"):
        LS.DiffusedVertices(tv[:100], tf, 19.0)
    with pytest.raises(ValueError):
        LS.DiffusedVertices(tv.reshape(-1), tf, 19.0)
    before = dv.params
    new = torch.rand(dv.params.shape)
    dv.load_params(new)
    assert dv.params is before and torch.equal(dv.params.detach(), new)
    with pytest.raises(ValueError):
        dv.load_params(torch.rand(3, 3))


# ---------------------------------------------------------------------------- 3. Adam and setup_optimizations
def test_the_uniform_group_selects_the_uniform_update(monkeypatch):
    from st3d import largesteps as LS
    from st3d import ops
    from st3d import optim as O
    calls = []
    monkeypatch.setattr(ops, "adam_step", lambda p, *a: calls.append(("plain", id(p))))
    monkeypatch.setattr(LS, "adam_step_uniform", lambda p, *a: calls.append(("uniform", id(p))))
    a, b, c = (torch.rand(3, 3).requires_grad_(True) for _ in range(3))
    opt = O.Adam([{"params": [a], "uniform": True, "lr": 0.5}, {"params": [b]}, {"params": [c], "uniform": False}], lr=0.01)
    assert [g.get("uniform", False) for g in opt.param_groups] == [True, False, False]
    assert "uniform" not in O.Adam([a], lr=0.01).param_groups[0] and "uniform" not in opt.param_groups[1]
    for t in (a, b, c):
        t.grad = torch.ones(3, 3)
    opt.step()
    assert [k for k, _ in calls] == ["uniform", "plain", "plain"]
    sd = opt.state_dict()
    assert sd["lrs"] == [0.5, 0.01, 0.01] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    O.Adam([{"params": [a], "uniform": True}, {"params": [b]}, {"params": [c]}], lr=0.01).load_state_dict(sd)


def _mesh(kind="uv"):
    import utils as U
    g = torch.Generator().manual_seed(0)
    verts = torch.rand(5, 3, generator=g)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4]])
    if kind == "vertex":
        return U.build_mesh_vertex(torch.rand(5, 3, generator=g), verts, faces), verts, faces
    if kind == "atlas":
        return U.build_mesh_atlas(torch.rand(2, 2, 2, 3, generator=g), verts, faces), verts, faces
    return U.build_mesh(torch.rand(1, 6, 2, generator=g), torch.tensor([[[0, 1, 2], [3, 4, 5]]]), torch.rand(1, 8, 8, 3, generator=g),
                        verts, faces), verts, faces


def test_setup_optimizations_without_diffusion_is_todays(monkeypatch):
    import utils as U
    from st3d import largesteps as LS
    monkeypatch.setattr(LS, "DiffusedVertices", lambda *a, **k: pytest.fail("verts_diffusion = 0 must make no object"))
    mesh, verts, faces = _mesh()
    for target, leaves in (("texture", ["texture_map"]), ("mesh", ["verts"]), ("both", ["verts", "texture_map"])):
        for out in (U.setup_optimizations(target, mesh, 0.01), U.setup_optimizations(target, mesh, 0.01, verts_diffusion=0),
                    U.setup_optimizations(target, mesh, 0.01, 1, 0.0)):
            assert sorted(out) == ["faces", "faces_uvs", "optimizable_mesh", "optimizer", "texture_map", "verts", "verts_uvs"]
            assert [id(p) for p in out["optimizer"].params] == [id(out[k]) for k in leaves]
            assert out["verts"].is_leaf and torch.equal(out["verts"].detach(), verts)
            assert len(out["optimizer"].param_groups) == 1 and "uniform" not in out["optimizer"].param_groups[0]
            assert U.refresh_verts(out) is out["verts"]
    for kind, keys in (("vertex", ["faces", "optimizable_mesh", "optimizer", "verts", "verts_features"]),
                       ("atlas", ["atlas", "faces", "optimizable_mesh", "optimizer", "verts"])):
        assert sorted(U.setup_optimizations("both", _mesh(kind)[0], 0.01, verts_diffusion=0.0)) == keys


def test_setup_optimizations_refuses_what_cannot_be_preconditioned():
    import utils as U
    for kind in ("uv", "vertex", "atlas"):
        mesh = _mesh(kind)[0]
        with pytest.raises(ValueError, match="verts_diffusion"):
            U.setup_optimizations("texture", mesh, 0.01, verts_diffusion=19.0)
        for bad in (-1.0, NAN, INF):
            for target in ("texture", "mesh", "both"):
                with pytest.raises(ValueError, match="verts_diffusion"):
                    U.setup_optimizations(target, mesh, 0.01, verts_diffusion=bad)
    with pytest.raises(UnboundLocalError):                  # the reference's own failure stays what it was
        U.setup_optimizations("nothing", _mesh()[0], 0.01, verts_diffusion=19.0)


def test_setup_optimizations_with_diffusion_swaps_the_vertex_leaf_only(monkeypatch):
    """the wiring, with the device solve replaced by the fp64 direct solve"""
    import utils as U
    from st3d import largesteps as LS

    def solve(off, idx, b, lam, tol, max_iter):
        f = torch.tensor([[0, 1, 2], [2, 3, 4]]).numpy()
        x = R.direct_solver(f, 5, lam)(b.double().numpy())
        return torch.from_numpy(x).float(), torch.tensor([[1, 1, 0]] * 3, dtype=torch.int32)
    monkeypatch.setattr(LS, "diffuse_solve", solve)
    for kind, colour in (("uv", "texture_map"), ("vertex", "verts_features"), ("atlas", "atlas")):
        mesh, verts, faces = _mesh(kind)
        for target in ("mesh", "both"):
            out = U.setup_optimizations(target, mesh, 0.01, verts_diffusion=19.0)
            dv = out["verts_diffusion"]
            assert isinstance(dv, LS.DiffusedVertices) and dv.lam == 19.0
            groups = out["optimizer"].param_groups
            assert groups[0]["params"][0] is dv.params and groups[0]["uniform"] is True and groups[0]["lr"] == 0.01
            want = [id(dv.params)] + ([id(out[colour])] if target == "both" else [])
            assert [id(p) for p in out["optimizer"].params] == want and len(groups) == len(want)
            assert all("uniform" not in g for g in groups[1:])
            assert out[colour].requires_grad == (target == "both")
            assert not out["verts"].is_leaf and out["verts"].requires_grad
            torch.testing.assert_close(out["verts"].detach(), verts, rtol=0, atol=1e-6)
            (out["verts"] * torch.arange(15.0).reshape(5, 3)).sum().backward()
            want_grad = R.direct_solver(faces.numpy(), 5, 19.0)(np.arange(15.0).reshape(5, 3))
            np.testing.assert_allclose(dv.params.grad.numpy(), want_grad, rtol=1e-5)
            old = out["verts"]
            assert U.refresh_verts(out) is out["verts"] and out["verts"] is not old
    both = U.setup_optimizations("both", _mesh()[0], 0.01, texture_pyramid_levels=2, verts_diffusion=19.0)
    assert [id(p) for p in both["optimizer"].params] == [id(both["verts_diffusion"].params), id(both["texture_pyramid"].params)]


# ---------------------------------------------------------------------------- 4. the flag and the checkpoint
def test_the_flag_parses_on_all_three_scripts_and_is_refused_three_ways(capsys):
    for mod in _scripts():
        assert mod.build_parser().parse_args([]).verts_diffusion == 0.0
        assert mod.build_parser().parse_args(["--verts_diffusion", "0", "--optimization_target", "texture"]).verts_diffusion == 0.0
        for target in ("mesh", "both"):
            a = mod.build_parser().parse_args(["--verts_diffusion", "19", "--optimization_target", target])
            assert a.verts_diffusion == 19.0
        for argv in (["--verts_diffusion", "19"],                                            # the default target is 'texture'
                     ["--verts_diffusion", "19", "--optimization_target", "texture"],
                     ["--verts_diffusion", "-1", "--optimization_target", "mesh"],
                     ["--verts_diffusion", "nan", "--optimization_target", "mesh"],
                     ["--verts_diffusion", "inf", "--optimization_target", "both"]):
            with pytest.raises(SystemExit):
                mod.build_parser().parse_args(argv)
            assert "verts_diffusion" in capsys.readouterr().err


def _fake_run(tmp_path, diffusion):
    from st3d import cli
    state = {"step": 3}
    optimizer = types.SimpleNamespace(state_dict=lambda: dict(state), load_state_dict=lambda d: state.update(d))
    run = types.SimpleNamespace(main=True, pyramid=None, atlas_r=0, vertex_colors=False, out_dir=str(tmp_path), device="cpu",
                                args=types.SimpleNamespace(optimization_target="both"), optimizer=optimizer,
                                opt={"texture_map": torch.rand(1, 4, 4, 3), "verts": torch.rand(4, 3)}, say=lambda msg: None,
                                progress=0, diffusion=diffusion)
    run.texture_key = cli.Run.texture_key.fget(run)
    return run


def _fake_diffusion(lam, seed):
    params = torch.rand(4, 3, generator=torch.Generator().manual_seed(seed)).requires_grad_(True)

    def load(t):
        with torch.no_grad():
            params.copy_(t)
    return types.SimpleNamespace(lam=lam, params=params, load_params=load)


def test_the_checkpoint_holds_u_and_lambda_and_a_mismatch_is_refused(tmp_path):
    from st3d import cli
    path = os.path.join(str(tmp_path), "checkpoint.pt")
    off = _fake_run(tmp_path, None)
    cli.Run.save_checkpoint(off, 1)
    plain = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(plain) == ["optimization_target", "optimizer", "progress", "texture_atlas", "texture_map", "texture_type", "verts"]
    with pytest.raises(ValueError, match="--verts_diffusion 0, this run has 19"):
        cli.Run.load_checkpoint(_fake_run(tmp_path, _fake_diffusion(19.0, 1)), path)
    on = _fake_run(tmp_path, _fake_diffusion(19.0, 2))
    cli.Run.save_checkpoint(on, 2)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(set(blob) - set(plain)) == ["verts_diffusion", "verts_diffusion_lambda"]
    assert blob["verts_diffusion_lambda"] == 19.0 and torch.equal(blob["verts_diffusion"], on.diffusion.params.detach())
    again = _fake_run(tmp_path, _fake_diffusion(19.0, 3))
    leaf, stale = again.diffusion.params, again.opt["verts"].clone()
    cli.Run.load_checkpoint(again, path)
    assert again.progress == 2 and again.diffusion.params is leaf and torch.equal(leaf.detach(), on.diffusion.params.detach())
    assert torch.equal(again.opt["verts"], stale)            # derived: solved for again, never copied from the file
    with pytest.raises(ValueError, match="--verts_diffusion 19, this run has 5"):
        cli.Run.load_checkpoint(_fake_run(tmp_path, _fake_diffusion(5.0, 4)), path)
    with pytest.raises(ValueError, match="--verts_diffusion 19, this run has 0"):
        cli.Run.load_checkpoint(off, path)
