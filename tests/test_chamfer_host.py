"""Host side of the Chamfer term: the C ABI's refusals (which launch nothing), argument validation in Python, the refusal of
CPU tensors, the CLI flags on all three scripts, that weight 0 calls nothing, and the checkpoint key.  No GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

import _cotref as COT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_knn1_geometry", "st3d_knn1_workspace_bytes", "st3d_knn1", "st3d_face_area_cdf_scratch_bytes", "st3d_face_area_cdf",
         "st3d_sample_points_fwd", "st3d_sample_points_bwd_scratch_bytes", "st3d_sample_points_bwd", "st3d_chamfer_sum",
         "st3d_chamfer_bwd")
BIG = (1 << 20) + 1


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def _cpu_mesh():
    from st3d import render as R
    v, f = COT.tetrahedron()
    return R.Meshes(v, f)


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_and_bound():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    assert "chamfer.hip" in open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()


def test_geometry_and_sizes_are_pure_host_logic():
    from st3d import _lib
    lib = _lib.load()
    tile, seg = ctypes.c_int(-1), ctypes.c_int(-1)
    for P1, P2 in ((1, 1), (63, 257), (1000, 1000), (5000, 5000), (20000, 20000), (8, 1 << 20), (1 << 20, 1 << 20)):
        assert lib.st3d_knn1_geometry(P1, P2, ctypes.byref(tile), ctypes.byref(seg)) == 0
        ntiles = -(-P2 // tile.value)
        assert tile.value >= 1 and 1 <= seg.value <= ntiles
        assert lib.st3d_knn1_workspace_bytes(P1, P2) == seg.value * P1 * 8
    assert lib.st3d_knn1_geometry(1, 1, ctypes.byref(tile), ctypes.byref(seg)) == 0 and seg.value == 1
    for bad in ((0, 5), (5, 0), (-1, 5), (BIG, 5), (5, BIG)):
        assert lib.st3d_knn1_geometry(*bad, ctypes.byref(tile), ctypes.byref(seg)) == -1
        assert lib.st3d_knn1_workspace_bytes(*bad) == 0
    assert lib.st3d_knn1_geometry(5, 5, None, ctypes.byref(seg)) == -1 and lib.st3d_knn1_geometry(5, 5, ctypes.byref(tile), None) == -1
    assert lib.st3d_face_area_cdf_scratch_bytes(0) == 0 and lib.st3d_face_area_cdf_scratch_bytes(5856) >= 8
    assert lib.st3d_sample_points_bwd_scratch_bytes(0) == 0 and lib.st3d_sample_points_bwd_scratch_bytes(10) == 720


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)            # never dereferenced
    big = 1 << 40

    def variants(good, pointers, sizes):
        out = [good[:i] + [None] + good[i + 1:] for i in pointers]
        out += [good[:i] + [v] + good[i + 1:] for i, values in sizes.items() for v in values]
        return out
    points = (0, -1, BIG)
    cases = {
        #            x  y  P1 P2 ws bytes idx dist stream
        "st3d_knn1": variants([p, p, 100, 300, p, big, p, p, None], (0, 1, 4, 6, 7),
                              {2: points, 3: points, 5: (0, 100 * 8 * 2 - 1), 4: (odd,)}),
        #                     verts faces F scratch bytes cdf stream
        "st3d_face_area_cdf": variants([p, p, 2000, p, big, p, None], (0, 1, 3, 5), {2: (0, -1), 4: (0, 15), 3: (odd,), 5: (odd,)}),
        #                         verts faces F cdf r N points face_idx stream
        "st3d_sample_points_fwd": variants([p, p, 10, p, p, 64, p, p, None], (0, 1, 3, 4, 6, 7), {2: (0, -1), 5: points, 3: (odd,)}),
        #                         grad r face_idx N F V inc_off inc_ref scratch bytes grad_verts stream
        "st3d_sample_points_bwd": variants([p, p, p, 64, 10, 8, p, p, p, big, p, None], (0, 1, 2, 6, 7, 8, 10),
                                           {3: points, 4: (0, -1), 5: (0, -1), 9: (0, 719), 8: (odd,)}),
        #                   dist P scale loss stream
        "st3d_chamfer_sum": variants([p, 64, 1.0, p, None], (0, 3), {1: points}),
        #                   x y P1 P2 nn order sorted c_self c_other grad stream
        "st3d_chamfer_bwd": variants([p, p, 64, 80, p, p, p, 1.0, 1.0, p, None], (0, 1, 9, 5, 6), {2: points, 3: points}),
    }
    cases["st3d_chamfer_bwd"].append([p, p, 64, 80, None, None, None, 1.0, 1.0, p, None])     # neither term
    for name, bad in cases.items():
        for args in bad:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 2. the Python surface
def test_unsupported_arguments_name_themselves():
    from st3d import mesh_losses as ML
    x, y = torch.rand(5, 3), torch.rand(1, 7, 3)
    one = torch.ones(1)
    for name, value in (("x_lengths", one.long()), ("y_lengths", one.long()), ("x_normals", x), ("y_normals", y), ("weights", one),
                        ("norm", 1), ("point_reduction", None), ("batch_reduction", None)):
        with pytest.raises(NotImplementedError, match=name):
            ML.chamfer_distance(x, y, **{name: value})
    with pytest.raises(NotImplementedError, match="K"):
        ML.knn_points(x, y, K=2)
    mesh = _cpu_mesh()
    with pytest.raises(NotImplementedError, match="return_normals"):
        ML.sample_points_from_meshes(mesh, 10, return_normals=True)
    with pytest.raises(NotImplementedError, match="return_textures"):
        ML.sample_points_from_meshes(mesh, 10, return_textures=True)


def test_bad_shapes_sizes_and_names_are_value_errors():
    from st3d import mesh_losses as ML, ops
    x = torch.rand(5, 3)
    for bad in (torch.rand(2, 5, 3), torch.rand(5, 2), torch.rand(0, 3), torch.rand(5), torch.rand(1, 1, 5, 3)):
        with pytest.raises(ValueError):
            ML.chamfer_distance(bad, x)
        with pytest.raises(ValueError):
            ML.chamfer_distance(x, bad)
        with pytest.raises(ValueError):
            ML.knn_points(x, bad)
    with pytest.raises(ValueError):
        ML.chamfer_distance(torch.empty((BIG, 3)), x)
    for kw in ({"norm": 3}, {"point_reduction": "max"}, {"batch_reduction": "median"}):
        with pytest.raises(ValueError):
            ML.chamfer_distance(x, x, **kw)
    mesh = _cpu_mesh()
    for n in (0, -3, BIG, 2.5, True, None):
        with pytest.raises(ValueError):
            ML.sample_points_from_meshes(mesh, n)
        with pytest.raises(ValueError):
            ops.check_num_points(n)
    with pytest.raises(TypeError):
        ML.sample_points_from_meshes(mesh, 10, True)                     # PyTorch3D's third positional is return_normals
    assert abs(ML.chamfer_floor(5.7095, 5000) - 7.2696e-4) < 1e-8


def test_cpu_tensors_are_refused():
    from st3d import mesh_losses as ML
    x, mesh = torch.rand(5, 3), _cpu_mesh()
    for call in (lambda: ML.chamfer_distance(x, x), lambda: ML.chamfer_distance(x, x, single_directional=True, point_reduction="sum"),
                 lambda: ML.knn_points(x, x[None]), lambda: ML.sample_points_from_meshes(mesh, 10),
                 lambda: ML.sample_points_from_meshes(mesh, 10, torch.Generator().manual_seed(0)), lambda: ML.surface_area(mesh)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_out_of_range_faces_never_reach_the_device(monkeypatch):
    from st3d import mesh_losses as ML, ops, render as R

    def boom(*a, **k):
        raise AssertionError("the faces reached the device")
    for name in ("face_area_cdf", "sample_points_fwd"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    v, _ = COT.tetrahedron()
    for f in (torch.tensor([[0, 1, 4]]), torch.tensor([[0, -1, 2]])):
        with pytest.raises(ValueError, match="outside"):
            ML.sample_points_from_meshes(R.Meshes(v, f), 10, torch.Generator().manual_seed(0))


# ---------------------------------------------------------------------------- 3. the CLI
def test_all_three_parsers_carry_the_flags_with_their_defaults():
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.chamfer_weight == 0.0 and a.chamfer_samples == 5000
        b = mod.build_parser().parse_args(["--chamfer_weight", "0.5", "--chamfer_samples", "1048576", "--optimization_target", "mesh"])
        assert b.chamfer_weight == 0.5 and b.chamfer_samples == 1 << 20


def test_bad_combinations_are_refused_before_any_gpu_work(monkeypatch, capsys):
    import st3d.cli as cli

    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    for mod in _scripts():
        monkeypatch.setattr(mod, "Run", no_gpu)
        for argv, word in ((["--chamfer_weight", "1"], "--chamfer_weight needs --optimization_target mesh or both"),
                           (["--chamfer_weight", "1", "--optimization_target", "texture"], "--chamfer_weight needs"),
                           (["--chamfer_weight", "-1", "--optimization_target", "mesh"], "--chamfer_weight must be"),
                           (["--chamfer_weight", "nan", "--optimization_target", "mesh"], "--chamfer_weight must be"),
                           (["--chamfer_samples", "0"], "--chamfer_samples must be"),
                           (["--chamfer_samples", "1048577", "--optimization_target", "both"], "--chamfer_samples must be")):
            with pytest.raises(SystemExit) as e:
                mod.main(argv)
            assert e.value.code == 2, argv
            assert word in capsys.readouterr().err
    ok = _scripts()[1].build_parser().parse_args(["--chamfer_weight", "0", "--chamfer_samples", "7"])
    assert ok.optimization_target == "texture" and cli.check_args(ok) is None          # the default, spelled out, is no refusal


def _recording_ops(monkeypatch, calls):
    """every wrapper of the new entry points replaced by a CPU stand-in that records its name"""
    from st3d import ops

    def rec(name, fn):
        def inner(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, inner)
    rec("face_area_cdf", lambda v, f: torch.ones(f.shape[0], dtype=torch.float64).cumsum(0))
    rec("sample_points_fwd", lambda v, f, cdf, r: (v[f[torch.zeros(r.shape[1], dtype=torch.int64), 0].long()].clone(),
                                                   torch.zeros(r.shape[1], dtype=torch.int32)))
    rec("sample_points_bwd", lambda g, r, fi, F, inc, out: out)
    rec("knn1", lambda x, y: (torch.zeros(x.shape[0], dtype=torch.int32), torch.ones(x.shape[0])))
    rec("chamfer_sum", lambda d, s, out: out.add_(float(s) * float(d.sum())))
    rec("chamfer_bwd", lambda x, y, nn, o, s, c1, c2, out: out)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def test_weight_zero_calls_nothing_and_the_term_is_these_calls_in_this_order(monkeypatch):
    import st3d.cli as cli
    calls = []
    _recording_ops(monkeypatch, calls)
    made = []
    run = cli.Run.__new__(cli.Run)
    run.args = _scripts()[1].build_parser().parse_args(["--optimization_target", "both"])
    run.world, run.chamfer_generator, run.chamfer_target = 1, None, None
    mesh = _cpu_mesh()
    assert run.chamfer_term(mesh) == 0 and calls == [] and run.chamfer_generator is None
    # and switched on, the term is these calls, in this order, at weight / world
    run.args = _scripts()[1].build_parser().parse_args(["--optimization_target", "both", "--chamfer_weight", "3", "--chamfer_samples",
                                                        "16", "--seed", "4"])
    run.device, run.content_mesh, run.say = torch.device("cpu"), mesh, lambda msg: made.append(msg)
    run.world = 2
    run.setup_chamfer()
    assert calls == ["face_area_cdf", "sample_points_fwd", "face_area_cdf"]          # the target cloud, then the area it prints
    assert len(made) == 1 and "16 points per cloud" in made[0] and "expected floor" in made[0]
    assert run.chamfer_generator.initial_seed() == 4 and run.chamfer_target.shape == (1, 16, 3)
    del calls[:]
    v = mesh.verts_packed().clone().requires_grad_(True)
    from st3d import render as R
    term = run.chamfer_term(R.Meshes(v, mesh.faces_packed()))
    assert calls == ["face_area_cdf", "sample_points_fwd", "knn1", "chamfer_sum", "knn1", "chamfer_sum"]
    assert float(term.detach()) == (3.0 / 2) * 2.0                                             # two directions of mean 1
    del calls[:]
    term.backward()
    assert calls == ["chamfer_bwd", "sample_points_bwd"] and v.grad is not None


def test_seed_unset_is_seed_zero(monkeypatch):
    import st3d.cli as cli
    _recording_ops(monkeypatch, [])
    run = cli.Run.__new__(cli.Run)
    run.args = _scripts()[0].build_parser().parse_args(["--optimization_target", "mesh", "--chamfer_weight", "1", "--chamfer_samples", "4"])
    run.device, run.content_mesh, run.say, run.world = torch.device("cpu"), _cpu_mesh(), lambda msg: None, 1
    run.setup_chamfer()
    assert run.args.seed is None and run.chamfer_generator.initial_seed() == 0


# ---------------------------------------------------------------------------- 4. checkpoints
def _fake_run(tmp_path, generator):
    from st3d import cli
    state = {"step": 3}
    optimizer = types.SimpleNamespace(state_dict=lambda: dict(state), load_state_dict=lambda d: state.update(d))
    run = types.SimpleNamespace(main=True, pyramid=None, atlas_r=0, vertex_colors=False, out_dir=str(tmp_path), device="cpu",
                                args=types.SimpleNamespace(optimization_target="both"), optimizer=optimizer,
                                opt={"texture_map": torch.rand(1, 4, 4, 3), "verts": torch.rand(4, 3)}, say=lambda msg: None,
                                progress=0, chamfer_generator=generator)
    run.texture_key = cli.Run.texture_key.fget(run)
    return run


def test_the_checkpoint_key_is_there_only_with_the_flag_and_resume_restores_the_draws(tmp_path):
    from st3d import cli
    path = os.path.join(str(tmp_path), "checkpoint.pt")
    off = _fake_run(tmp_path, None)
    cli.Run.save_checkpoint(off, 1)
    plain = torch.load(path, map_location="cpu", weights_only=True)
    assert "chamfer_generator_state" not in plain
    assert sorted(plain) == ["optimization_target", "optimizer", "progress", "texture_atlas", "texture_map", "texture_type", "verts"]
    with pytest.raises(ValueError, match="without --chamfer_weight"):
        cli.Run.load_checkpoint(_fake_run(tmp_path, torch.Generator().manual_seed(1)), path)
    gen = torch.Generator().manual_seed(7)
    torch.rand(5, generator=gen)
    on = _fake_run(tmp_path, gen)
    cli.Run.save_checkpoint(on, 2)
    want = torch.rand(6, generator=gen)                                   # what the uninterrupted run draws next
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert blob["chamfer_generator_state"].dtype == torch.uint8 and sorted(set(blob) - set(plain)) == ["chamfer_generator_state"]
    again = _fake_run(tmp_path, torch.Generator().manual_seed(99))
    cli.Run.load_checkpoint(again, path)
    assert again.progress == 2 and torch.equal(torch.rand(6, generator=again.chamfer_generator), want)
    with pytest.raises(ValueError, match="written with --chamfer_weight"):
        cli.Run.load_checkpoint(off, path)
