"""Independent restatement, in plain torch, of the cotangent Laplacian regularisers and the edge loss with a target length
(DESIGN.md 7 holds the contract; PyTorch3D's cot_laplacian / mesh_laplacian_smoothing / mesh_edge_loss).  Everything takes
the dtype of `verts`: fp64 is the reference of the tests, fp32 is "what a PyTorch3D user gets" and sets the GPU test's bars.
L, nw, inv and Lsum are built under no_grad; the gradient is autograd's.  Also the small meshes the tests share."""
import math

import torch


# ---------------------------------------------------------------------------- the formulas
def face_cot_area(verts, faces):
    """-> cot (F,3), area (F,): Heron's formula as PyTorch3D writes it"""
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp(min=1e-12).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cot = torch.stack([B2 + C2 - A2, A2 + C2 - B2, A2 + B2 - C2], dim=1) / (4.0 * area[:, None])
    return cot, area


def half_edges(faces):
    """-> ii, jj (3F,), corner-major: corner c of face f weighs the edge opposite it, L[ii, jj] += cot[f, c] and transposed"""
    return (torch.cat([faces[:, 1], faces[:, 2], faces[:, 0]]), torch.cat([faces[:, 2], faces[:, 0], faces[:, 1]]))


def constants(verts, faces):
    """The constants of the backward -> dict(ii, jj, w (3F,), Lsum (V,), Asum (V,), nw (V,), inv (V,))"""
    with torch.no_grad():
        V = verts.shape[0]
        cot, area = face_cot_area(verts.detach(), faces)
        ii, jj = half_edges(faces)
        w = cot.t().reshape(-1)
        Lsum = torch.zeros(V, dtype=verts.dtype).index_add_(0, ii, w).index_add_(0, jj, w)
        Asum = torch.zeros(V, dtype=verts.dtype).index_add_(0, faces.reshape(-1), area[:, None].expand(-1, 3).reshape(-1))
        nw = torch.where(Lsum > 0, 1.0 / Lsum, Lsum)
        inv = torch.where(Asum > 0, 1.0 / Asum, torch.zeros_like(Asum))
    return {"ii": ii, "jj": jj, "w": w, "Lsum": Lsum, "Asum": Asum, "nw": nw, "inv": inv}


def dense_L(verts, faces):
    c = constants(verts, faces)
    V = verts.shape[0]
    L = torch.zeros(V, V, dtype=verts.dtype)
    L.index_put_((c["ii"], c["jj"]), c["w"], accumulate=True)
    L.index_put_((c["jj"], c["ii"]), c["w"], accumulate=True)
    return L


def residuals(verts, c, method):
    """r (V,3) of 'cot' / 'cotcurv' with the constants c held fixed; 'uniform' ignores the weights"""
    ii, jj, w = c["ii"], c["jj"], c["w"]
    if method == "uniform":
        e = torch.unique(torch.sort(torch.stack([ii, jj], 1), dim=1).values, dim=0)
        a, b = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
        deg = torch.zeros(verts.shape[0], dtype=verts.dtype).index_add_(0, a, torch.ones(a.shape[0], dtype=verts.dtype))
        s = torch.zeros_like(verts).index_add(0, a, verts[b])
        return torch.where(deg[:, None] > 0, s / deg.clamp(min=1)[:, None] - verts, torch.zeros_like(verts))
    Lv = torch.zeros_like(verts).index_add(0, ii, w[:, None] * verts[jj]).index_add(0, jj, w[:, None] * verts[ii])
    if method == "cot":
        return Lv * c["nw"][:, None] - verts
    if method == "cotcurv":
        return (Lv - c["Lsum"][:, None] * verts) * (0.25 * c["inv"])[:, None]
    raise ValueError(method)


def laplacian_loss(verts, faces, method, c=None):
    """(1/V) sum_i |r_i|; differentiable in verts with L constant (c: constants frozen elsewhere, e.g. for finite differences)"""
    c = constants(verts, faces) if c is None else c
    return residuals(verts, c, method).norm(dim=1).sum() / verts.shape[0]


def unique_edges(faces):
    ii, jj = half_edges(faces)
    return torch.unique(torch.sort(torch.stack([ii, jj], 1), dim=1).values, dim=0)


def edge_loss(verts, faces, t):
    """(1/E) sum_e (|a - b| - t)^2, plain autograd (the norm's subgradient at 0 is 0: the contract's direction term)"""
    e = unique_edges(faces)
    return (((verts[e[:, 0]] - verts[e[:, 1]]).norm(dim=1) - t) ** 2).mean()


def loss_and_grad(verts, faces, fn):
    v = verts.clone().requires_grad_(True)
    out = fn(v, faces)
    out.backward()
    return out.detach(), v.grad


# ---------------------------------------------------------------------------- meshes (fp32 vertices, int64 faces)
def _jitter(verts, seed, amount):
    g = torch.Generator().manual_seed(seed)
    return (verts + amount * (torch.rand(verts.shape, generator=g, dtype=torch.float64) - 0.5)).float()


def tetrahedron():
    v = torch.tensor([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=torch.float64)
    return _jitter(v, 1, 0.3), torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def hex_fan(jitter=0.0):
    """centre 0 and six rim vertices on the unit circle: equilateral (and fp64) when jitter = 0; the rim is a boundary"""
    ang = torch.arange(6, dtype=torch.float64) * (math.pi / 3)
    v = torch.cat([torch.zeros(1, 3, dtype=torch.float64), torch.stack([ang.cos(), ang.sin(), torch.zeros(6, dtype=torch.float64)], 1)])
    f = torch.tensor([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)])
    return (_jitter(v, 2, jitter) if jitter else v), f


def open_strip(n=5):
    """two rows of n vertices, 2 (n - 1) triangles, all vertices on the boundary"""
    x = torch.arange(n, dtype=torch.float64)
    v = torch.cat([torch.stack([x, torch.zeros_like(x), 0.1 * x * x], 1), torch.stack([x + 0.4, torch.ones_like(x), 0.05 * x], 1)])
    f = []
    for k in range(n - 1):
        f += [[k, k + 1, n + k], [k + 1, n + k + 1, n + k]]
    return _jitter(v, 3, 0.2), torch.tensor(f)


def non_manifold():
    """edge (0, 1) shared by three faces; every other edge is a boundary"""
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.6, 0.8], [0.4, -0.5, -0.9]], dtype=torch.float64)
    return _jitter(v, 4, 0.2), torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]])


def zero_length_edge():
    """the tetrahedron plus vertex 4 AT vertex 3 and the zero-area face (0, 3, 4): area clamp, an edge of length 0.  Vertex 4
    touches that face alone, so its Laplacian residual is exactly 0 and |r| has its kink there: u_4 is 0 by the contract, a
    rounding residue normalised to a unit vector (times weights of 1e6 and more) in any evaluation that does not cancel
    exactly -- fp32 torch is 0.49 (cot) / 0.07 (cotcurv) relative L2 away from fp64 torch on this mesh.  So it serves the edge
    loss and the finiteness checks, not the Laplacian's parity."""
    v, f = tetrahedron()
    return torch.cat([v, v[3:4]]), torch.cat([f, torch.tensor([[0, 3, 4]])])


def degenerate_face():
    """the tetrahedron plus vertex 4 at the (fp32) midpoint of the edge (0, 3), the zero-area face (0, 3, 4) -- its area^2 is
    rounding residue far below the 1e-12 clamp, its cotangents are of the order of +-1e6 -- and the proper face (4, 1, 2),
    which keeps vertex 4's residual away from 0"""
    v, f = tetrahedron()
    return torch.cat([v, 0.5 * (v[0:1] + v[3:4])]), torch.cat([f, torch.tensor([[0, 3, 4], [4, 1, 2]])])


def unused_vertex():
    v, f = tetrahedron()
    return torch.cat([v, torch.tensor([[0.3, -0.2, 0.7]])]), f


def icosphere(level, radius=1.0):
    """unit icosahedron subdivided `level` times (midpoints pushed to the sphere): 10 * 4^level + 2 vertices"""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [tuple(c / math.sqrt(1 + p * p) for c in q) for q in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                q = [(x + y) / 2 for x, y in zip(v[a], v[b])]
                n = math.sqrt(sum(c * c for c in q))
                v.append(tuple(c / n for c in q))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (radius * torch.tensor(v, dtype=torch.float64)).float(), torch.tensor(f)


def jittered_plane(n=7, seed=5):
    """an n x n grid in the plane z = 0.3 x - 0.2 y + 1 with every vertex moved inside the plane, split into triangles with
    alternating diagonals -> verts, faces, interior mask"""
    g = torch.Generator().manual_seed(seed)
    ij = torch.stack(torch.meshgrid(torch.arange(n, dtype=torch.float64), torch.arange(n, dtype=torch.float64), indexing="ij"), -1)
    xy = ij.reshape(-1, 2) + 0.6 * (torch.rand(n * n, 2, generator=g, dtype=torch.float64) - 0.5)
    v = torch.cat([xy, (0.3 * xy[:, :1] - 0.2 * xy[:, 1:] + 1.0)], 1)
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, i * n + j + 1, (i + 1) * n + j, (i + 1) * n + j + 1
            f += [[a, b, d], [a, d, c]] if (i + j) % 2 else [[a, b, c], [b, d, c]]
    i, j = ij.reshape(-1, 2)[:, 0], ij.reshape(-1, 2)[:, 1]
    interior = (i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)
    return v, torch.tensor(f), interior


def cow_mesh(cow, seed=0, amount=0.01):
    """the golden cow with its vertices perturbed like tests/test_gpu_kernels.py does -> verts fp32, faces, original verts"""
    import numpy as np
    target = torch.from_numpy(cow["verts"]).float()
    g = torch.Generator().manual_seed(seed)
    return target + amount * torch.randn(target.shape, generator=g), torch.from_numpy(cow["faces"].astype(np.int64)), target


SMALL_MESHES = {"tetrahedron": tetrahedron, "fan": lambda: hex_fan(0.3), "strip": open_strip, "non_manifold": non_manifold,
                "degenerate": degenerate_face, "unused_vertex": unused_vertex, "icosphere2": lambda: icosphere(2)}
