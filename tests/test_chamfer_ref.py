"""The CPU restatement of the Chamfer contract (tests/_chamferref.py) checked against hand cases, an fp64 kd-tree, the geometry
of the sampled points, the 2A/(pi N) floor and fp64 autograd / central differences.  No GPU."""
import math

import numpy as np
import pytest
import torch

import _chamferref as C

F32 = np.float32


# ---------------------------------------------------------------------------- 1. hand cases
def test_two_point_clouds():
    x = np.array([[0, 0, 0], [1, 0, 0]], F32)
    y = np.array([[0, 0, 0.5], [1, 2, 0]], F32)
    loss, (ix, dx), (iy, dy) = C.chamfer(x, y)
    assert ix.tolist() == [0, 0] and dx.tolist() == [0.25, 1.25]
    assert iy.tolist() == [0, 1] and dy.tolist() == [0.25, 4.0]
    assert loss == F32(0.75 + 2.125)
    assert C.chamfer(x, y, single_directional=True)[0] == F32(0.75)
    assert C.chamfer(x, y, point_reduction="sum")[0] == F32(1.5 + 4.25)


def test_a_shifted_cloud_is_two_delta_squared_apart():
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(F32)   # spacing 1
    delta = np.array([0.25, -0.125, 0.375], F32)                          # below half the spacing, exact in fp32
    d2 = float((delta.astype(np.float64) ** 2).sum())
    loss, (ix, _), (iy, _) = C.chamfer(g, g + delta)
    assert (ix == np.arange(len(g))).all() and (iy == np.arange(len(g))).all()
    assert loss == F32(2 * d2)
    assert C.chamfer(g, g + delta, single_directional=True)[0] == F32(d2)


def test_duplicate_targets_choose_the_lower_index_and_nan_is_never_chosen():
    y = np.array([[5, 5, 5], [1, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]], F32)
    x = np.array([[1, 0, 0], [0.9, 0, 0], [0.5, 0.5, 0]], F32)
    idx, d = C.knn1(x, y)
    assert idx.tolist() == [1, 1, 1] and d[0] == 0
    y[1] = np.nan
    idx, d = C.knn1(x, y)
    assert idx.tolist() == [2, 2, 2] and np.isfinite(d).all()
    x[1, 2] = np.nan
    idx, d = C.knn1(x, y)
    assert idx.tolist() == [2, 0, 2] and np.isnan(d[1]) and np.isfinite(d[[0, 2]]).all()
    assert np.isnan(C.chamfer(x, y)[0])                                   # a NaN anywhere is a NaN loss


# ---------------------------------------------------------------------------- 2. against an fp64 kd-tree
@pytest.mark.parametrize("P1,P2,seed", [(2000, 2000, 0), (1000, 257, 1), (65, 1000, 2)])
def test_fp32_scan_against_an_fp64_kdtree(P1, P2, seed):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    x, y = rng.random((P1, 3), F32), rng.random((P2, 3), F32)
    idx, d = C.knn1(x, y)
    dd, ii = cKDTree(y.astype(np.float64)).query(x.astype(np.float64), k=2)
    gap = (dd[:, 1] ** 2 - dd[:, 0] ** 2) / dd[:, 1] ** 2
    keep = gap > 8 * 2.0 ** -24                                           # the two nearest differ by more than fp32 resolves
    print("left out: %d of %d" % ((~keep).sum(), P1))
    assert (~keep).sum() <= 0.005 * P1
    assert (idx[keep] == ii[keep, 0]).all()
    rel = np.abs(d.astype(np.float64) - dd[:, 0] ** 2) / dd[:, 0] ** 2
    print("mismatches %d, max relative error %.3g" % ((idx != ii[:, 0]).sum(), rel[keep].max()))
    assert rel[keep].max() <= 4 * 2.0 ** -24


# ---------------------------------------------------------------------------- 3. sampling
def test_points_reproduce_from_their_faces_and_lie_in_their_planes(cow):
    verts, faces = C.cow(cow)
    r = C.uniforms(3000, 3)
    p, f, w = C.sample(verts, faces, r)
    assert (np.diff(f) >= 0).all() and f.min() >= 0 and f.max() < len(faces)
    assert (np.diff(r[0]) >= 0).all() and r.min() >= 0 and r.max() < 1
    again = (w[:, 0:1] * verts[faces[f, 0]] + w[:, 1:2] * verts[faces[f, 1]]) + w[:, 2:3] * verts[faces[f, 2]]
    assert (again == p).all()
    assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -24 and w.min() >= 0
    v = verts.astype(np.float64)
    a, b, c = v[faces[f, 0]], v[faces[f, 1]], v[faces[f, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    size = np.linalg.norm(v.max(0) - v.min(0))
    off = np.abs(((p.astype(np.float64) - a) * n).sum(1))
    print("largest distance from the face's plane / size: %.3g" % (off.max() / size))
    assert off.max() <= 1e-6 * size


def test_a_zero_area_face_is_never_drawn_and_counts_follow_the_areas():
    # faces of area 1, 0 (degenerate), 3
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [0, 3, 1], [2, 0, 1]], F32)
    faces = np.array([[0, 1, 2], [0, 1, 1], [3, 5, 4]], np.int64)
    assert C.face_areas(verts, faces).tolist() == [1.0, 0.0, 3.0]
    N = 40000
    _, f, _ = C.sample(verts, faces, C.uniforms(N, 5))
    counts = np.bincount(f, minlength=3)
    assert counts[1] == 0 and counts.sum() == N
    sigma = math.sqrt(N * 0.25 * 0.75)
    print("face 0 drew %d of %d, expected %d, sigma %.1f" % (counts[0], N, N // 4, sigma))
    assert abs(counts[0] - 0.25 * N) <= 4 * sigma
    # r0 = 0 on a mesh whose FIRST face is degenerate: cdf_0 = 0 is not > 0
    faces2 = faces[[1, 0, 2]]
    r = C.uniforms(64, 6)
    r[0, 0] = 0.0
    assert C.sample(verts, faces2, r)[1].min() == 1
    # a NaN vertex: the total area is NaN, no face is drawn, every point is NaN
    verts[2, 1] = np.nan
    p, f, _ = C.sample(verts, faces, r)
    assert np.isnan(p).all() and (f == 2).all()


def test_icosphere_samples_lie_between_the_inscribed_radius_and_one():
    verts, faces = C.icosphere(2)
    v = verts.astype(np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    inscribed = np.abs((v[faces[:, 0]] * n).sum(1) / np.linalg.norm(n, axis=1)).min()
    p, _, _ = C.sample(verts, faces, C.uniforms(20000, 7))
    rad = np.linalg.norm(p.astype(np.float64), axis=1)
    print("radii in [%.6f, %.6f], inscribed %.6f" % (rad.min(), rad.max(), inscribed))
    assert rad.min() >= inscribed - 1e-6 and rad.max() <= 1 + 1e-6


# ---------------------------------------------------------------------------- 4. the floor and the response to scale
@pytest.fixture(scope="module")
def cow_clouds(cow):
    verts, faces = C.cow(cow)
    N = 5000
    target, _, _ = C.sample(verts, faces, C.uniforms(N, 0))
    out = {}
    for s in (1.0, 1.02, 1.05):
        cur, _, _ = C.sample((verts * F32(s)).astype(F32), faces, C.uniforms(N, 1))
        out[s] = float(C.chamfer(cur, target)[0])
    return out, float(C.area_cdf(verts, faces)[-1]), N


def test_two_samplings_of_the_cow_sit_on_the_floor(cow_clouds):
    values, area, N = cow_clouds
    want = C.floor(area, N)
    print("chamfer %.4e, 2A/(pi N) %.4e, gap %.1f %%" % (values[1.0], want, 100 * abs(values[1.0] - want) / want))
    assert abs(area - 5.7095) < 1e-3
    assert abs(values[1.0] - want) <= 0.15 * want


def test_chamfer_rises_with_the_scale(cow_clouds):
    values, _, _ = cow_clouds
    print({k: "%.3e" % v for k, v in values.items()})
    assert values[1.0] < values[1.02] < values[1.05]


# ---------------------------------------------------------------------------- 5. gradients
def _small_problem(cow, n=300):
    verts, faces = C.cow(cow)
    r = C.uniforms(n, 11)
    x, fi, w = C.sample((verts * F32(1.03)).astype(F32), faces, r)
    y, _, _ = C.sample(verts, faces, C.uniforms(n + 37, 12))
    return verts, faces, x, y, fi, w


@pytest.mark.parametrize("single", [False, True])
def test_gradients_against_fp64_autograd(cow, single):
    verts, faces, x, y, fi, w = _small_problem(cow)
    nn_x, _ = C.knn1(x, y)
    nn_y = None if single else C.knn1(y, x)[0]
    sx, sy = 1.0 / len(x), 1.0 / len(y)
    gx, _ = C.chamfer_grad64(x, y, nn_x, nn_y, sx, sy)
    gy, _ = C.chamfer_grad64(y, x, nn_y, nn_x, sy, sx)
    v64 = torch.from_numpy((verts * F32(1.03)).astype(F32)).double().requires_grad_(True)
    y64 = torch.from_numpy(y).double().requires_grad_(True)
    pts = C.sample_torch64(v64, faces, fi, w)
    pts.retain_grad()
    assert np.abs(pts.detach().numpy() - x).max() <= 4 * 2.0 ** -24 * np.abs(verts).max() * 1.03
    # the loss at the fp32 points, the vertex gradient through the (linear) sampling
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    C.chamfer_torch64(x64, y64, nn_x, nn_y, sx, sy).backward()
    pts.backward(x64.grad)
    gv, _ = C.sample_grad64(gx, fi, w, faces, len(verts))
    errs = [np.abs(got.numpy() - want).max() / np.abs(want).max() for got, want in ((x64.grad, gx), (y64.grad, gy), (v64.grad, gv))]
    print("relative to the largest entry: dx %.3g, dy %.3g, dverts %.3g" % tuple(errs))
    assert max(errs) <= 1e-12
    assert np.abs(gv).max() > 0


def test_gradients_against_central_differences(cow):
    _, _, x, y, _, _ = _small_problem(cow, 120)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)

    def full(a, b):                                                       # fp64, neighbours found afresh
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        return d.min(1).mean() + d.min(0).mean(), d.argmin(1), d.argmin(0)
    _, nn_x, nn_y = full(x64, y64)
    gx, _ = C.chamfer_grad64(x, y, nn_x, nn_y, 1.0 / len(x), 1.0 / len(y))
    gy, _ = C.chamfer_grad64(y, x, nn_y, nn_x, 1.0 / len(y), 1.0 / len(x))
    h, checked, worst = 1e-5, 0, 0.0
    for which, g in ((0, gx), (1, gy)):
        for i in range(0, g.shape[0], 7):
            for c in range(3):
                vals = []
                for sgn in (+1, -1):
                    a, b = x64.copy(), y64.copy()
                    (a if which == 0 else b)[i, c] += sgn * h
                    v, ia, ib = full(a, b)
                    vals.append(v if (ia == nn_x).all() and (ib == nn_y).all() else None)
                if None in vals:
                    continue                                              # an index switched inside the stencil
                checked += 1
                fd = (vals[0] - vals[1]) / (2 * h)
                worst = max(worst, abs(fd - g[i, c]) / max(np.abs(g).max(), abs(fd)))
                assert abs(fd - g[i, c]) <= 1e-6 * max(np.abs(g).max(), abs(fd)), (which, i, c, fd, g[i, c])
    print("%d entries checked, largest difference relative to the largest entry %.3g" % (checked, worst))
    assert checked > 60
