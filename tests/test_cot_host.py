"""Host side of the cotangent Laplacian / edge target length: the static lists of build_cot_topology on hand-checked meshes
(and, gathered in list order the way the kernels do, against the fp64 restatement), argument validation in Python, the C
ABI's refusals (which launch nothing), the CLI flags.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _cotref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(faces, V):
    from st3d import mesh_losses as ML
    topo = {k: t.numpy() for k, t in ML.build_topology(faces, V).items()}
    cot = {k: t.numpy() for k, t in ML.build_cot_topology(faces, V).items()}
    return topo, cot


# ---------------------------------------------------------------------------- 1. the lists
def test_lists_of_two_triangles_sharing_an_edge():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    topo, cot = _lists(faces, 5)                                        # vertex 4 is used by no face
    assert topo["edges"].tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    assert cot["faces"].tolist() == faces.tolist() and cot["faces"].dtype == np.int32
    # edge -> face * 3 + (corner opposite): (0,1) is opposite corner 2 of face 0, (0,2) corner 1; (1,2) is opposite corner 0 of
    # face 0 and corner 2 of face 1 = (2,1,3); (1,3) opposite its corner 0; (2,3) opposite its corner 1
    assert cot["edge_off"].tolist() == [0, 1, 2, 4, 5, 6]
    assert cot["edge_ref"].tolist() == [2, 1, 0, 5, 3, 4]
    # adjacency rows: 0: [1, 2]; 1: [0, 2, 3]; 2: [0, 1, 3]; 3: [1, 2]; 4: []
    assert topo["nbr_off"].tolist() == [0, 2, 5, 8, 10, 10]
    assert topo["nbr_idx"].tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]
    assert cot["nbr_edge"].tolist() == [0, 1, 0, 2, 3, 1, 2, 4, 3, 4]
    # vertex -> face * 3 + corner
    assert cot["inc_off"].tolist() == [0, 1, 3, 5, 6, 6]
    assert cot["inc_ref"].tolist() == [0, 1, 4, 2, 3, 5]


def test_lists_of_a_non_manifold_edge():
    _, faces = C.non_manifold()
    topo, cot = _lists(faces, 5)
    assert topo["edges"][0].tolist() == [0, 1]
    assert cot["edge_off"][:2].tolist() == [0, 3]                        # three faces on the edge (0, 1)
    assert cot["edge_ref"][:3].tolist() == [0 * 3 + 2, 1 * 3 + 2, 2 * 3 + 2]
    assert np.diff(cot["edge_off"])[1:].tolist() == [1] * 6              # the six other edges are boundary edges


@pytest.mark.parametrize("name", sorted(C.SMALL_MESHES) + ["cow"])
def test_lists_are_consistent_and_gathered_in_order_give_the_restatement(name, cow):
    v, faces = C.SMALL_MESHES[name]() if name != "cow" else C.cow_mesh(cow)[:2]
    V, F = v.shape[0], faces.shape[0]
    topo, cot = _lists(faces, V)
    edges, off, nbr = topo["edges"], topo["nbr_off"], topo["nbr_idx"]
    E = edges.shape[0]
    fl = faces.numpy()
    assert cot["nbr_edge"].shape == (2 * E,) and cot["edge_off"].shape == (E + 1,) and cot["edge_ref"].shape == (3 * F,)
    assert sorted(cot["edge_ref"].tolist()) == list(range(3 * F)) and sorted(cot["inc_ref"].tolist()) == list(range(3 * F))
    src = np.repeat(np.arange(V), np.diff(off))
    slot_edge = edges[cot["nbr_edge"]]
    assert (np.minimum(src, nbr) == slot_edge[:, 0]).all() and (np.maximum(src, nbr) == slot_edge[:, 1]).all()
    for e in range(E):
        refs = cot["edge_ref"][cot["edge_off"][e]:cot["edge_off"][e + 1]]
        assert (np.diff(refs) > 0).all() and refs.size >= 1
        for r in refs:
            rest = sorted(int(fl[r // 3, (r % 3 + k) % 3]) for k in (1, 2))
            assert rest == edges[e].tolist()
    for i in range(V):
        refs = cot["inc_ref"][cot["inc_off"][i]:cot["inc_off"][i + 1]]
        assert (np.diff(refs) > 0).all() and (fl.reshape(-1)[refs] == i).all()
    # the kernels' gathers, in list order, in fp64
    cotf, area = C.face_cot_area(v.double(), faces)
    fc = torch.cat([cotf, area[:, None]], 1).reshape(-1).numpy()
    wedge = np.array([sum(fc[r + r // 3] for r in cot["edge_ref"][cot["edge_off"][e]:cot["edge_off"][e + 1]]) for e in range(E)])
    wslot = wedge[cot["nbr_edge"]]
    vd = v.double().numpy()
    Lsum, Lv, Asum = np.zeros(V), np.zeros((V, 3)), np.zeros(V)
    np.add.at(Lsum, src, wslot)
    np.add.at(Lv, src, wslot[:, None] * vd[nbr])
    for i in range(V):
        Asum[i] = sum(fc[4 * (r // 3) + 3] for r in cot["inc_ref"][cot["inc_off"][i]:cot["inc_off"][i + 1]])
    c = C.constants(v.double(), faces)
    scale = float(c["Lsum"].abs().max())
    assert np.abs(Lsum - c["Lsum"].numpy()).max() <= 1e-12 * scale and np.abs(Asum - c["Asum"].numpy()).max() <= 1e-14
    nw = np.where(Lsum > 0, 1.0 / np.where(Lsum > 0, Lsum, 1.0), Lsum)
    r_cot = Lv * nw[:, None] - vd
    assert np.abs(r_cot - C.residuals(v.double(), c, "cot").numpy()).max() <= 1e-11


def test_out_of_range_and_malformed_faces_are_refused_on_the_host():
    from st3d import mesh_losses as ML
    for bad, V in ((torch.tensor([[0, 1, 3]]), 3), (torch.tensor([[0, -1, 2]]), 3), (torch.zeros((0, 3), dtype=torch.int64), 3),
                   (torch.tensor([[0, 1]]), 3)):
        with pytest.raises(ValueError):
            ML.build_cot_topology(bad, V)


# ---------------------------------------------------------------------------- 2. the Python surface
def _cpu_mesh():
    from st3d import render as R
    v, f = C.tetrahedron()
    return R.Meshes(v, f)


def test_method_and_target_length_are_validated_before_any_device_work():
    from st3d import mesh_losses as ML, ops
    mesh = _cpu_mesh()
    for bad in ("cotan", "", None, 1, "Uniform"):
        with pytest.raises(ValueError):
            ML.mesh_laplacian_smoothing(mesh, method=bad)
    for bad in (-1.0, float("nan"), float("inf"), "mean", None, True):
        with pytest.raises(ValueError):
            ML.mesh_edge_loss(mesh, target_length=bad)
    v = mesh.verts_packed()
    w = {'mesh_verts_weight': 1.0, 'mesh_edge_loss_weight': 1.0, 'mesh_laplacian_smoothing_weight': 1.0,
         'mesh_normal_consistency_weight': 1.0}
    with pytest.raises(ValueError):
        ML.mesh_terms(v, v, mesh, dict(w, mesh_laplacian_method="cotangent"))
    with pytest.raises(ValueError):
        ML.mesh_terms(v, v, mesh, dict(w, mesh_edge_target_length=-0.5))
    # valid settings get as far as the device check: there is no CPU path
    for call in (lambda: ML.mesh_laplacian_smoothing(mesh, method="cot"), lambda: ML.mesh_laplacian_smoothing(mesh, method="cotcurv"),
                 lambda: ML.mesh_edge_loss(mesh, target_length=0.5), lambda: ML.mesh_terms(v, v, mesh, dict(w, mesh_laplacian_method="cot"))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    topo = ML.build_topology(mesh.faces_packed(), 4)
    with pytest.raises(ValueError):
        ops.mesh_reg_ex(v, v, topo, None, [1, 1, 1, 1], "cot")          # the cotangent methods need their lists
    with pytest.raises(ValueError):
        ops.mesh_reg_ex(v, v, topo, None, [1, 1, 1, 1], "nope")
    with pytest.raises(ValueError):
        ops.mesh_reg_ex(v, v, topo, None, [1, 1, 1, 1], "uniform", -1.0)


def test_defaults_take_todays_call(monkeypatch):
    from st3d import mesh_losses as ML, ops
    calls = []

    def fake_reg(verts, target, topo, weights, want_grad=True):
        calls.append(("mesh_reg", list(weights)))
        return torch.arange(5.0), torch.zeros_like(verts)

    def fake_ex(verts, target, topo, cot, weights, method="uniform", t=0.0, want_grad=True):
        calls.append(("mesh_reg_ex", list(weights), method, t, cot is not None))
        return torch.arange(5.0), torch.zeros_like(verts)
    monkeypatch.setattr(ops, "mesh_reg", fake_reg)
    monkeypatch.setattr(ops, "mesh_reg_ex", fake_ex)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    mesh = _cpu_mesh()
    v = mesh.verts_packed()
    w = {'mesh_verts_weight': 0.5, 'mesh_edge_loss_weight': 1.5, 'mesh_laplacian_smoothing_weight': 2.0,
         'mesh_normal_consistency_weight': 3.0, 'main_loss_weight': 3.0}
    ML.mesh_terms(v, v, mesh, w)
    ML.mesh_terms(v, v, mesh, dict(w, mesh_laplacian_method="uniform", mesh_edge_target_length=0.0))
    assert calls == [("mesh_reg", [0.5, 1.5, 2.0, 3.0])] * 2
    del calls[:]
    ML.mesh_terms(v, v, mesh, dict(w, mesh_laplacian_method="cotcurv"))
    ML.mesh_terms(v, v, mesh, dict(w, mesh_edge_target_length=0.25))
    assert calls == [("mesh_reg_ex", [0.5, 1.5, 2.0, 3.0], "cotcurv", 0.0, True), ("mesh_reg_ex", [0.5, 1.5, 2.0, 3.0], "uniform", 0.25, False)]
    del calls[:]
    ML._REG_CACHE.clear()
    ML.mesh_edge_loss(mesh)
    ML.mesh_laplacian_smoothing(mesh)
    ML.mesh_laplacian_smoothing(mesh, method="uniform")                  # cached on the vertices' version
    assert calls == [("mesh_reg", [0.0, 1.0, 0.0, 0.0]), ("mesh_reg", [0.0, 0.0, 1.0, 0.0])]
    del calls[:]
    ML.mesh_laplacian_smoothing(mesh, method="cot")
    ML.mesh_edge_loss(mesh, target_length=0.3)
    assert calls == [("mesh_reg_ex", [0.0, 0.0, 1.0, 0.0], "cot", 0.0, True), ("mesh_reg_ex", [0.0, 1.0, 0.0, 0.0], "uniform", 0.3, False)]
    ML._REG_CACHE.clear()


# ---------------------------------------------------------------------------- 3. the C ABI
def test_symbols_are_declared_bound_and_validate_their_arguments():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in ("st3d_mesh_reg_ex", "st3d_mesh_reg_ex_scratch_floats"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.st3d_mesh_reg_ex_scratch_floats(0, 6, 4, 6) == 0 and lib.st3d_mesh_reg_ex_scratch_floats(4, 0, 4, 6) == 0
    n = lib.st3d_mesh_reg_ex_scratch_floats(4, 6, 4, 6)
    assert n >= lib.st3d_mesh_reg_scratch_floats(4, 6) + 2 * (4 * 4 + 2 * 6 + 6 * 4) and n % 2 == 0
    p = ctypes.c_void_p(4096)            # never dereferenced: validation comes before any launch
    w = (ctypes.c_float * 4)(1, 1, 1, 1)
    #         verts tgt V edges E off idx pairs P poff pref faces F nedge eoff eref ioff iref method t w scratch parts out grad stream
    good = [p, p, 4, p, 6, p, p, p, 6, p, p, p, 4, p, p, p, p, p, 1, 0.0, w, p, p, p, p, None]
    bad = []
    for i in (0, 1, 3, 5, 6, 20, 21, 22, 23):                             # pointers every call needs
        bad.append(good[:i] + [None] + good[i + 1:])
    for i in (7, 9, 10):                                                  # the pair lists when P > 0
        bad.append(good[:i] + [None] + good[i + 1:])
    for i in (11, 13, 14, 15, 16, 17):                                    # the cotangent lists when the method needs them
        for method in (1, 2):
            bad.append(good[:i] + [None] + good[i + 1:18] + [method] + good[19:])
    for i, value in ((2, 0), (2, -1), (4, 0), (8, -1), (12, 0), (18, 3), (18, -1), (19, -1.0), (19, float("nan")), (19, float("inf"))):
        bad.append(good[:i] + [value] + good[i + 1:])
    bad.append(good[:21] + [ctypes.c_void_p(4100)] + good[22:])           # scratch holds fp64: 8-byte aligned
    for args in bad:
        assert lib.st3d_mesh_reg_ex(*args) == -1, args
        assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 4. the CLI
def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_all_three_parsers_carry_the_flags_with_their_defaults():
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.laplacian_method == "uniform" and a.edge_target_length == 0.0
        b = mod.build_parser().parse_args(["--laplacian_method", "cotcurv", "--edge_target_length", "0.02",
                                           "--optimization_target", "both"])
        assert b.laplacian_method == "cotcurv" and b.edge_target_length == 0.02
        c = mod.build_parser().parse_args(["--edge_target_length", "mean", "--optimization_target", "mesh"])
        assert c.edge_target_length == "mean"


def test_non_default_values_with_the_texture_target_are_refused_before_any_gpu_work(monkeypatch, capsys):
    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    for mod in _scripts():
        monkeypatch.setattr(mod, "Run", no_gpu)
        for argv in (["--laplacian_method", "cot"], ["--laplacian_method", "cotcurv", "--optimization_target", "texture"],
                     ["--edge_target_length", "mean"], ["--edge_target_length", "0.1", "--optimization_target", "texture"],
                     ["--edge_target_length", "-1", "--optimization_target", "mesh"],
                     ["--edge_target_length", "nan", "--optimization_target", "mesh"],
                     ["--edge_target_length", "long", "--optimization_target", "mesh"],
                     ["--laplacian_method", "cotangent", "--optimization_target", "mesh"]):
            with pytest.raises(SystemExit) as e:
                mod.main(argv)
            assert e.value.code == 2, argv
            err = capsys.readouterr().err
            assert "laplacian_method" in err or "edge_target_length" in err
        ok = mod.build_parser().parse_args(["--laplacian_method", "uniform", "--edge_target_length", "0"])
        assert ok.optimization_target == "texture"                       # the defaults, spelled out, are no refusal


def test_flags_reach_the_weights_dict_and_mean_is_the_meshs_mean_edge_length(capsys):
    import st3d.cli as cli
    v, f = C.tetrahedron()
    parse = _scripts()[1].build_parser().parse_args
    assert cli.mesh_regulariser_keys(parse([]), v, f) == {}
    assert cli.mesh_regulariser_keys(parse(["--optimization_target", "both"]), v, f) == {}
    keys = cli.mesh_regulariser_keys(parse(["--optimization_target", "both", "--laplacian_method", "cot", "--edge_target_length",
                                            "0.5"]), v, f)
    assert keys == {"mesh_laplacian_method": "cot", "mesh_edge_target_length": 0.5}
    capsys.readouterr()
    keys = cli.mesh_regulariser_keys(parse(["--optimization_target", "mesh", "--edge_target_length", "mean"]), v, f)
    e = C.unique_edges(f)
    mean = float((v.double()[e[:, 0]] - v.double()[e[:, 1]]).norm(dim=1).mean())
    assert list(keys) == ["mesh_edge_target_length"] and abs(keys["mesh_edge_target_length"] - mean) <= 1e-15
    assert "%.6g" % mean in capsys.readouterr().out
