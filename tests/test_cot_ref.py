"""The fp64 restatement of the cotangent Laplacian regularisers and the edge target length (tests/_cotref.py) pinned to facts
that do not come from the restatement itself: planar patches, the equilateral fan, the sphere's mean curvature, hand-counted
weights on boundary / non-manifold / degenerate / unused cases, finite differences.  No GPU."""
import math

import pytest
import torch

import _cotref as C

D = torch.float64


def test_planar_patch_with_an_irregular_triangulation_has_no_cot_residual():
    v, f, interior = C.jittered_plane()
    c = C.constants(v, f)
    for method in ("cot", "cotcurv"):
        r = C.residuals(v, c, method)[interior].norm(dim=1)
        assert float(r.max()) <= 1e-13, (method, float(r.max()))
    uni = C.residuals(v, c, "uniform")[interior].norm(dim=1)
    assert float(uni.min()) > 1e-3 and float(uni.mean()) > 3e-2           # the uniform Laplacian drags a flat, uneven patch


def test_equilateral_fan_has_spoke_weights_two_over_root_three_and_cot_equals_uniform_at_the_centre():
    v, f = C.hex_fan()
    v = v.double()
    v[0] = torch.tensor([0.05, -0.02, 0.3], dtype=D)                      # lift the centre: its residual is not 0
    flat = v.clone()
    flat[0] = 0.0
    L = C.dense_L(flat, f)
    assert float((L[0, 1:] - 2.0 / math.sqrt(3.0)).abs().max()) <= 1e-14  # two 60-degree corners face every spoke
    assert float((L - L.t()).abs().max()) == 0.0
    assert float((L[1, 2] - 1.0 / math.sqrt(3.0)).abs()) <= 1e-14         # a rim (boundary) edge has one
    c = C.constants(flat, f)                                              # equal spoke weights: the weighted mean is the plain mean
    r_cot, r_uni = C.residuals(v, c, "cot")[0], C.residuals(v, c, "uniform")[0]
    assert float((r_cot - r_uni).abs().max()) <= 1e-15
    assert float((r_uni + v[0]).abs().max()) <= 1e-15                     # the rim's mean is the origin


def test_cotcurv_on_the_unit_icosphere_approaches_a_third_of_the_mean_curvature():
    """sum_j L_ij (v_j - v_i) = -4 A_bary H n with A_bary = Asum / 3, so |r_i| = H / 3 = 1 / (3 radius).  Measured in fp64:
    relative gap 2.2206e-3 at two refinements (162 vertices), 5.9001e-4 at three (642): it shrinks 3.76-fold, about h^2.
    Bars: 3e-3 and 8e-4 (1.35 x the measured gaps), and at least a 3-fold drop."""
    gaps = []
    for level, radius in ((2, 1.0), (3, 1.0), (2, 2.0)):
        v, f = C.icosphere(level, radius)
        loss = float(C.laplacian_loss(v.double(), f, "cotcurv"))
        gaps.append(abs(loss * 3.0 * radius - 1.0))
        print(f"icosphere level {level} radius {radius}: cotcurv loss {loss:.12g}, relative gap {gaps[-1]:.4e}")
    assert gaps[0] <= 3e-3 and gaps[1] <= 8e-4 and gaps[2] <= 3e-3
    assert gaps[1] * 3.0 <= gaps[0]


def test_boundary_non_manifold_degenerate_and_unused():
    # one right triangle: every edge is a boundary edge with the single cotangent of the corner opposite it
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=D)
    f = torch.tensor([[0, 1, 2]])
    L = C.dense_L(v, f)
    assert abs(float(L[1, 2])) <= 1e-15 and abs(float(L[0, 1]) - 1.0) <= 1e-15 and abs(float(L[0, 2]) - 1.0) <= 1e-15
    c = C.constants(v, f)
    assert float((c["Asum"] - 0.5).abs().max()) <= 1e-15
    # three right triangles around the edge (0, 1), apexes at distance 1 above vertex 0: the edge takes one cot(45 deg) each
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0]], dtype=D)
    f = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    L = C.dense_L(v, f)
    assert abs(float(L[0, 1]) - 3.0) <= 1e-14 and abs(float(L[1, 0]) - 3.0) <= 1e-14
    assert float((C.constants(v, f)["Asum"][:2] - 1.5).abs().max()) <= 1e-15
    # zero-area face: the 1e-12 clamp, area 1e-6, finite everything
    for make in (C.degenerate_face, C.zero_length_edge):
        v, f = make()
        cot, area = C.face_cot_area(v.double(), f)
        assert float(area[4]) == 1e-6 and torch.isfinite(cot).all()
        for method in ("cot", "cotcurv"):
            loss, grad = C.loss_and_grad(v.double(), f, lambda a, b: C.laplacian_loss(a, b, method))
            assert math.isfinite(float(loss)) and torch.isfinite(grad).all()
    cot, _ = C.face_cot_area(C.degenerate_face()[0].double(), C.degenerate_face()[1])
    assert float(cot[4, 0]) > 1e5 and float(cot[4, 1]) > 1e5 and float(cot[4, 2]) < -1e5      # 0, 0 and 180 degrees over area 1e-6
    v, f = C.zero_length_edge()
    cot, area = C.face_cot_area(v.double(), f)
    b2 = float((v[0].double() - v[3].double()).pow(2).sum())
    assert abs(float(cot[-1, 0]) - 2.0 * b2 / 4e-6) <= 1e-9 * b2 / 4e-6 and float(cot[-1, 1]) == 0.0 and float(cot[-1, 2]) == 0.0
    # unused vertex: r = -v under cot, 0 under cotcurv
    v, f = C.unused_vertex()
    c = C.constants(v.double(), f)
    assert float(c["Lsum"][4]) == 0.0 and float(c["nw"][4]) == 0.0 and float(c["inv"][4]) == 0.0
    assert torch.equal(C.residuals(v.double(), c, "cot")[4], -v[4].double())
    assert float(C.residuals(v.double(), c, "cotcurv")[4].abs().max()) == 0.0
    # nw is the reciprocal where the row sum is positive (cot_b + cot_c > 0 in every proper triangle, obtuse or not); a row sum
    # that is not -- 0 above -- keeps its own value (PyTorch3D's masked reciprocal)
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0.5, 0.05, 0]], dtype=D)         # corner 2 is obtuse: L[0,1] = cot_2 < 0
    L = C.dense_L(v, torch.tensor([[0, 1, 2]]))
    c = C.constants(v, torch.tensor([[0, 1, 2]]))
    assert float(L[0, 1]) < 0 and bool((c["Lsum"] > 0).all()) and torch.equal(c["nw"], 1.0 / c["Lsum"])


@pytest.mark.parametrize("name", ["tetrahedron", "fan", "strip", "non_manifold", "unused_vertex"])
@pytest.mark.parametrize("method", ["cot", "cotcurv"])
def test_gradient_is_the_finite_difference_of_the_constant_L_objective(name, method):
    v, f = C.SMALL_MESHES[name]()
    v = v.double()
    c = C.constants(v, f)
    _, grad = C.loss_and_grad(v, f, lambda a, b: C.laplacian_loss(a, b, method))
    h = 1e-6
    fd = torch.zeros_like(v)
    for i in range(v.shape[0]):
        for k in range(3):
            p, m = v.clone(), v.clone()
            p[i, k] += h
            m[i, k] -= h
            fd[i, k] = (C.laplacian_loss(p, f, method, c) - C.laplacian_loss(m, f, method, c)) / (2 * h)
    assert float((fd - grad).norm()) <= 1e-8 * float(grad.norm()), float((fd - grad).norm() / grad.norm())
    # and the contract's closed form
    r = C.residuals(v, c, method)
    n = r.norm(dim=1, keepdim=True)
    u = torch.where(n > 0, r / n.clamp(min=1e-300), torch.zeros_like(r))
    L = C.dense_L(v, f)
    V = v.shape[0]
    if method == "cot":
        closed = (L @ (c["nw"][:, None] * u) - u) / V
    else:
        q = 0.25 * c["inv"][:, None] * u
        closed = (L @ q - c["Lsum"][:, None] * q) / V
    assert float((closed - grad).norm()) <= 1e-14 * float(grad.norm())


def test_edge_loss_with_a_target_length():
    v, f = C.zero_length_edge()
    v = v.double()
    e = C.unique_edges(f)
    length = (v[e[:, 0]] - v[e[:, 1]]).norm(dim=1)
    assert int((length == 0).sum()) == 1
    for t in (0.0, 0.7, float(length[length > 0].mean())):
        loss, grad = C.loss_and_grad(v, f, lambda a, b: C.edge_loss(a, b, t))
        assert abs(float(loss) - float(((length - t) ** 2).mean())) <= 1e-15
        closed = torch.zeros_like(v)
        for (a, b), l in zip(e.tolist(), length.tolist()):
            if l > 0:
                d = (2.0 / e.shape[0]) * (l - t) * (v[a] - v[b]) / l
                closed[a] += d
                closed[b] -= d
        assert torch.isfinite(grad).all() and float((closed - grad).abs().max()) <= 1e-15
    # at t = 0 it is the reference's mean squared edge length
    v, f = C.tetrahedron()
    v, e = v.double(), C.unique_edges(f)
    assert e.shape[0] == 6
    assert abs(float(C.edge_loss(v, f, 0.0)) - float(((v[e[:, 0]] - v[e[:, 1]]) ** 2).sum(1).mean())) <= 1e-15
