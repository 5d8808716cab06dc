"""csrc/chamfer.hip on the GPU against tests/_chamferref.py: the nearest-neighbour scan bit for bit (indices and distances, at
every size where the launch changes shape, with equal points on both sides of every tile and segment boundary), the sampled
points bit for bit, the loss and the three gradients against fp64 on the GPU's own indices, determinism, the sign of the
vertex gradient, the public functions, and one short second_approach run with a resume."""
import math
import os

import numpy as np
import pytest
import torch

import _chamferref as C

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _knn_both(ops, x, y, dev):
    idx, d = ops.knn1(_t(x, dev), _t(y, dev))
    return idx.cpu().numpy(), d.cpu().numpy()


def _seglen(ops, P1, P2):
    tile, segments = ops.knn1_geometry(P1, P2)
    ntiles = (P2 + tile - 1) // tile
    return tile, segments, (ntiles + segments - 1) // segments * tile


# ---------------------------------------------------------------------------- 1. knn1
def test_knn1_matches_the_scan_bit_for_bit_at_every_size(ops, dev):
    tile, segments = ops.knn1_geometry(1000, 1000)
    assert tile >= 1 and segments >= 1
    base = [1, 63, 64, 65, 257, 1000]
    extra = [tile - 1, tile + 1, segments * tile + 1]
    pairs = [(a, b) for a in base for b in base] + [(a, b) for a in extra for b in extra] + [(65, e) for e in extra] + \
            [(e, 65) for e in extra]
    rng = np.random.default_rng(0)
    pool_x, pool_y = rng.random((max(base + extra), 3), F32), rng.random((max(base + extra), 3), F32)
    for P1, P2 in pairs:
        x, y = pool_x[:P1], pool_y[:P2]
        want_idx, want_d = C.knn1(x, y)
        idx, d = _knn_both(ops, x, y, dev)
        assert idx.dtype == np.int32 and (idx == want_idx).all(), (P1, P2)
        assert (_bits(d) == _bits(want_d)).all(), (P1, P2)


@pytest.mark.parametrize("P1,P2,several_tiles", [(70, 1500, False), (16384, 40000, True), (8, 1 << 20, False)])
def test_knn1_equal_points_across_tile_and_segment_boundaries_give_the_lower_index(ops, dev, P1, P2, several_tiles):
    """the middle case has so many query blocks that a segment is several tiles long; the last is the largest cloud"""
    tile, segments, seglen = _seglen(ops, P1, P2)
    print("P1 %d P2 %d: tile %d, %d segments of %d points" % (P1, P2, tile, segments, seglen))
    assert segments > 1 and seglen % tile == 0 and seglen * segments >= P2 and 3 * seglen + tile < P2
    assert (seglen > tile) == several_tiles
    rng = np.random.default_rng(1)
    x, y = rng.random((P1, 3), F32), rng.random((P2, 3), F32)
    js = [3, tile - 1, seglen + 5][:P1 // 2]
    for q, j in enumerate(js):                                            # a tile apart
        y[j + tile] = y[j]
        x[2 * q] = y[j]
    for q, j in enumerate(js):                                            # a segment apart (and two)
        j2 = j + 17
        y[j2 + seglen] = y[j2]
        if j2 + 2 * seglen < P2:
            y[j2 + 2 * seglen] = y[j2]
        x[2 * q + 1] = y[j2]
    idx, d = _knn_both(ops, x, y, dev)
    rows = np.unique(np.r_[np.arange(min(P1, 8)), rng.integers(0, P1, 56)])          # the restatement on these queries
    want_idx, want_d = C.knn1(x[rows], y, chunk=4)
    for q, j in enumerate(js):
        assert idx[2 * q] == j and idx[2 * q + 1] == j + 17 and d[2 * q] == 0 and d[2 * q + 1] == 0
    assert (idx[rows] == want_idx).all() and (_bits(d[rows]) == _bits(want_d)).all()


def test_knn1_nan_query_gives_nan_and_a_nan_target_is_never_chosen(ops, dev):
    rng = np.random.default_rng(2)
    x, y = rng.random((130, 3), F32), rng.random((700, 3), F32)
    nearest = C.knn1(x, y)[0]
    y[nearest[:40], 1] = np.nan                                           # what would have been chosen
    y[0] = np.nan                                                         # and the start value's index
    x[5, 0] = np.nan
    x[64] = np.nan
    idx, d = _knn_both(ops, x, y, dev)
    want_idx, want_d = C.knn1(x, y)
    assert (idx == want_idx).all()
    ok = np.ones(130, bool)
    ok[[5, 64]] = False
    assert np.isnan(d[~ok]).all() and (idx[~ok] == 0).all()
    assert np.isfinite(d[ok]).all() and not np.isnan(y[idx[ok]]).any()
    assert (_bits(d[ok]) == _bits(want_d[ok])).all()


# ---------------------------------------------------------------------------- 2. sampling
@pytest.fixture(scope="module")
def cow_gpu(cow, dev):
    from st3d import render as R
    verts, faces = C.cow(cow)
    mesh = R.Meshes(_t(verts, dev), _t(faces, dev))
    return verts, faces, mesh


@pytest.mark.parametrize("N", [1, 64, 1000])
def test_sampled_points_match_the_restatement_bit_for_bit(ops, dev, cow_gpu, N):
    verts, faces, mesh = cow_gpu
    cdf = ops.face_area_cdf(mesh.verts_packed(), mesh.faces_i32())
    want_cdf = C.area_cdf(verts, faces)
    err = np.abs(cdf.cpu().numpy() - want_cdf).max() / want_cdf[-1]
    print("cdf: largest difference / total %.3g (bound %.3g)" % (err, len(faces) * 2.0 ** -52))
    assert cdf.dtype == torch.float64 and err <= len(faces) * 2.0 ** -52
    r = C.uniforms(N, 20 + N)
    points, face_idx = ops.sample_points_fwd(mesh.verts_packed(), mesh.faces_i32(), cdf, _t(r, dev))
    want_p, want_f, _ = C.sample(verts, faces, r)
    assert (face_idx.cpu().numpy() == want_f).all() and face_idx.dtype == torch.int32
    assert (_bits(points.cpu().numpy()) == _bits(want_p)).all()


# ---------------------------------------------------------------------------- 3. loss, gradients, determinism, sign
def _problem(cow_gpu, dev, N, M, scale=1.03):
    """current cloud: N points of the cow scaled by `scale` (with an autograd edge to its vertices); target: M points"""
    from st3d import mesh_losses as ML, render as R
    verts, faces, mesh = cow_gpu
    v = (mesh.verts_packed() * scale).detach().requires_grad_(True)
    moving = R.Meshes(v, mesh.faces_packed())
    g = torch.Generator(device=dev).manual_seed(3)
    with torch.no_grad():
        target = ML.sample_points_from_meshes(mesh, M, generator=g)
    return ML, moving, v, target, g


def _run_once(cow_gpu, dev, N, M, single=False, reduction="mean"):
    ML, moving, v, target, g = _problem(cow_gpu, dev, N, M)
    target = target.clone().requires_grad_(True)
    r_state = g.get_state()
    points, face_idx = ML.sample_points_from_meshes(moving, N, generator=g, return_face_idx=True)
    points.retain_grad()
    loss, none = ML.chamfer_distance(points, target, single_directional=single, point_reduction=reduction)
    assert none is None and loss.shape == ()
    loss.backward()
    return dict(loss=loss.detach(), points=points.detach()[0], gx=points.grad[0], gy=target.grad[0], gv=v.grad, target=target.detach()[0],
                face_idx=face_idx, r_state=r_state, v=v.detach())


@pytest.mark.parametrize("N,M,single,reduction", [(1000, 1300, False, "mean"), (257, 64, True, "mean"), (300, 1100, False, "sum")])
def test_loss_and_gradients_against_fp64_on_the_gpus_own_indices(ops, dev, cow_gpu, N, M, single, reduction):
    from st3d import mesh_losses as ML
    verts, faces, _ = cow_gpu
    out = _run_once(cow_gpu, dev, N, M, single, reduction)
    x, y = out["points"], out["target"]
    nn_x, d_x = ops.knn1(x, y)
    nn_y, d_y = ops.knn1(y, x)
    sx, sy = (1.0 / N, 1.0 / M) if reduction == "mean" else (1.0, 1.0)
    want = sx * d_x.double().sum().item() + (0.0 if single else sy * d_y.double().sum().item())
    err = abs(out["loss"].item() - want) / want
    print("loss %.6e, fp64 %.6e, relative difference %.3g" % (out["loss"].item(), want, err))
    assert err <= 2.0 ** -23
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    ix, iy = nn_x.cpu().numpy(), (None if single else nn_y.cpu().numpy())

    def check(name, got, g64, mag):
        got = got.cpu().numpy().astype(np.float64)
        slack = 2.0 ** -23 * np.abs(g64) + 1e-12 * mag
        worst = (np.abs(got - g64) / np.maximum(slack, 1e-300)).max()
        print("%s: largest |g - g64| / bound = %.3f, largest |g64| %.3e" % (name, worst, np.abs(g64).max()))
        assert np.abs(g64).max() > 0 and (np.abs(got - g64) <= slack).all()
    check("dx", out["gx"], *C.chamfer_grad64(xn, yn, ix, iy, sx, sy))
    check("dy", out["gy"], *C.chamfer_grad64(yn, xn, iy, ix, sy, sx))
    # the vertex gradient from the GPU's own dx, face choice and weights
    g = torch.Generator(device=dev)
    g.set_state(out["r_state"])
    r = ML.sample_uniforms(N, g, dev).cpu().numpy()
    check("dverts", out["gv"], *C.sample_grad64(out["gx"].cpu().numpy(), out["face_idx"].cpu().numpy(), C.bary(r), faces, len(verts)))
    # and those are the restatement's: the points reproduce from r
    want_p, want_f, _ = C.sample(out["v"].cpu().numpy(), faces, r, cdf=ops.face_area_cdf(out["v"], _t(faces, dev).int()).cpu().numpy())
    assert (want_f == out["face_idx"].cpu().numpy()).all() and (_bits(want_p) == _bits(xn)).all()


def test_two_runs_are_bit_equal(dev, cow_gpu):
    a, b = _run_once(cow_gpu, dev, 1000, 1300), _run_once(cow_gpu, dev, 1000, 1300)
    for k in ("loss", "points", "gx", "gy", "gv", "face_idx"):
        assert torch.equal(a[k], b[k]), k


def test_the_gradient_of_a_swollen_cow_points_outwards(dev, cow_gpu):
    from st3d import mesh_losses as ML, render as R
    _, _, mesh = cow_gpu
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        target = ML.sample_points_from_meshes(mesh, 2000, generator=g)
    centroid = mesh.verts_packed().mean(0)
    v = ((mesh.verts_packed() - centroid) * 1.05 + centroid).detach().requires_grad_(True)
    loss, _ = ML.chamfer_distance(ML.sample_points_from_meshes(R.Meshes(v, mesh.faces_packed()), 2000, generator=g), target)
    loss.backward()
    inner = float((v.grad.double() * (v.detach() - centroid).double()).sum())
    print("chamfer %.4e, <dverts, verts - centroid> = %.4e" % (loss.item(), inner))
    assert inner > 0                                                      # descending the loss shrinks the cow back


# ---------------------------------------------------------------------------- 4. the public functions
def test_public_functions_are_the_ops_composition_bit_for_bit(ops, dev, cow_gpu):
    import losses as L
    from st3d import mesh_losses as ML, render as R
    assert L.chamfer_distance is ML.chamfer_distance and L.knn_points is ML.knn_points
    assert L.sample_points_from_meshes is ML.sample_points_from_meshes
    _, _, mesh = cow_gpu
    N = 777
    g1, g2 = torch.Generator(device=dev).manual_seed(9), torch.Generator(device=dev).manual_seed(9)
    pts = L.sample_points_from_meshes(mesh, N, generator=g1)
    r = torch.rand((3, N), generator=g2, dtype=torch.float32, device=dev)
    r[0] = torch.sort(r[0]).values
    want, _ = ops.sample_points_fwd(mesh.verts_packed(), mesh.faces_i32(), ops.face_area_cdf(mesh.verts_packed(), mesh.faces_i32()), r)
    assert pts.shape == (1, N, 3) and torch.equal(pts[0], want)
    cpu_gen = torch.Generator().manual_seed(4)                            # a CPU generator: the restatement's uniforms
    pts_cpu = L.sample_points_from_meshes(mesh, 64, generator=cpu_gen)
    want_cpu, _ = ops.sample_points_fwd(mesh.verts_packed(), mesh.faces_i32(), ops.face_area_cdf(mesh.verts_packed(), mesh.faces_i32()),
                                        _t(C.uniforms(64, 4), dev))
    assert torch.equal(pts_cpu[0], want_cpu)
    torch.manual_seed(5)
    a = L.sample_points_from_meshes(mesh, 100)                            # the global generator
    torch.manual_seed(5)
    assert torch.equal(a, L.sample_points_from_meshes(mesh, 100))
    other = L.sample_points_from_meshes(mesh, 500, generator=g1)
    dists, idx = L.knn_points(pts, other)
    i2, d2 = ops.knn1(pts[0], other[0])
    assert dists.shape == (1, N, 1) and idx.shape == (1, N, 1) and idx.dtype == torch.int64
    assert torch.equal(dists[0, :, 0], d2) and torch.equal(idx[0, :, 0], i2.long())
    assert L.knn_points(pts[0], other[0])[0].shape == (N, 1)
    loss, _ = L.chamfer_distance(pts, other[0])
    out = torch.zeros(1, device=dev)
    ops.chamfer_sum(d2, 1.0 / N, out)
    ops.chamfer_sum(ops.knn1(other[0], pts[0])[1], 1.0 / 500, out)
    assert torch.equal(loss, out[0])
    assert torch.equal(L.chamfer_distance(pts, other, batch_reduction="sum")[0], loss)
    nan_pts = pts.clone()
    nan_pts[0, 3, 1] = float("nan")
    assert torch.isnan(L.chamfer_distance(nan_pts, other)[0]) and torch.isnan(L.chamfer_distance(other, nan_pts)[0])
    nan_v = mesh.verts_packed().clone()
    nan_v[7] = float("nan")                                               # a NaN vertex: NaN points and a NaN loss, nothing else
    bad = L.sample_points_from_meshes(R.Meshes(nan_v, mesh.faces_packed()), 400, generator=g1)
    assert torch.isnan(bad).all() and torch.isnan(L.chamfer_distance(bad, other)[0])
    floor = ML.chamfer_floor(ML.surface_area(mesh), 5000)
    assert abs(floor - C.floor(5.7095, 5000)) <= 1e-4 * floor


# ---------------------------------------------------------------------------- 5. end to end
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


def test_second_approach_with_the_chamfer_term_ends_finite_and_resumes_on_the_same_bits(dev, cow, golden_dir, tmp_path, capsys):
    import losses as L
    import second_approach as SA
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "2", "--batch_size", "2", "--seed", "0",
              "--optimization_target", "both", "--chamfer_weight", "1", "--chamfer_samples", "500", "--save_every", "0",
              "--epochs", "3"]
    full, part = str(tmp_path / "full"), str(tmp_path / "part")
    SA.main(common + ["--output_path", full, "--checkpoint_every", "2"])
    said = capsys.readouterr().out
    assert "Chamfer term: 500 points per cloud" in said and "expected floor 2A/(pi N) = 0.00726" in said
    ck = os.path.join(full, "checkpoint.pt")
    blob = torch.load(ck, map_location="cpu", weights_only=True)
    assert blob["progress"] == 2 and blob["chamfer_generator_state"].dtype == torch.uint8
    SA.main(common + ["--output_path", part, "--resume", ck])            # epoch 2 only
    log = lambda d: [line.split("Loss ")[1] for line in open(os.path.join(d, "log.txt")).read().splitlines()[1:]]
    lf, lp = log(full), log(part)
    print("losses", lf, "resumed", lp)
    assert len(lf) == 3 and len(lp) == 1 and all(math.isfinite(float(v)) for v in lf)
    assert lp[0] == lf[2]
    assert open(os.path.join(full, "final.obj")).read() == open(os.path.join(part, "final.obj")).read()
    with pytest.raises(ValueError, match="chamfer_weight"):
        SA.main(common[:-8] + ["--save_every", "0", "--epochs", "3", "--output_path", str(tmp_path / "bad"), "--resume", ck])
