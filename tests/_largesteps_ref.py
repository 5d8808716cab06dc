"""References for csrc/diffuse.hip and st3d/largesteps.py (no GPU, no libst3d).

  * the matrix M = I + lambda L of a triangle mesh as a scipy sparse matrix and its fp64 direct solve (splu);
  * the solver restated in numpy: fp32 vectors, the row accumulated as differences in adjacency order, fp32 products added
    in fp64 -- the kernel's arithmetic except for the order in which a dot product's fp64 terms are added;
  * the iteration cap restated from its derivation;
  * the uniform-second-moment Adam restated in torch;
  * the test meshes that are not fixtures.
"""
import math
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------- meshes
def fixture(name):
    """(verts (V,3) fp32, faces (F,3) int64) of tests/golden/assets_<name>_mesh.npz"""
    d = np.load(os.path.join(GOLDEN, f"assets_{name}_mesh.npz"))
    return np.ascontiguousarray(d["verts"], F32), np.ascontiguousarray(d["faces"]).astype(np.int64)


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)


def grid(nx=33, ny=32):
    """an open nx x ny sheet (boundary vertices of degree 2..4, inner ones of degree 6), gently bent"""
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = np.stack([x / (nx - 1), y / (ny - 1), 0.1 * np.sin(3.0 * x / nx) * np.cos(2.0 * y / ny)], -1).reshape(-1, 3).astype(F32)
    i = (y[:-1, :-1] * nx + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)])
    return v, f.astype(np.int64)


def two_tetrahedra_sharing_an_edge():
    """vertices 0 and 1 are an edge of both solids: four faces meet there (non-manifold)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0.3], [0.5, 0.2, 1], [0.5, -1, -0.3], [0.5, -0.2, -1]], F32)
    f = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2], [0, 1, 4], [0, 5, 1], [1, 5, 4], [0, 4, 5]]
    return v, np.array(f, np.int64)


def with_a_loose_vertex(v, f):
    """one appended vertex that no face names: degree 0, its row of M is the identity"""
    return np.concatenate([v, np.array([[0.3, -0.2, 0.7]], F32)]), f


def meshes():
    """name -> (verts, faces): every mesh the GPU tests use"""
    cow = fixture("cow")
    return {"tetrahedron": tetrahedron(), "grid33x32": grid(), "teapot": fixture("teapot"), "cow": cow,
            "cow_loose_vertex": with_a_loose_vertex(*cow), "two_tetrahedra": two_tetrahedra_sharing_an_edge()}


# ---------------------------------------------------------------------------- the matrix
def adjacency(faces, V):
    """CSR (off (V+1), idx) of the unique undirected edges, both directions, neighbours ascending (the order of
    st3d.mesh_losses.build_topology)"""
    e = np.concatenate([faces[:, [1, 2]], faces[:, [2, 0]], faces[:, [0, 1]]])
    e = np.unique(np.sort(e, 1), axis=0)
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    order = np.argsort(src * V + dst, kind="stable")
    src, dst = src[order], dst[order]
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(src, minlength=V))
    return off, dst


def laplacian(faces, V):
    off, idx = adjacency(faces, V)
    deg = np.diff(off)
    A = sp.csr_matrix((np.ones(len(idx)), idx, off), shape=(V, V))
    return (sp.diags(deg.astype(F64)) - A).tocsr()


def system(faces, V, lam):
    """M = I + lam L, fp64 CSR"""
    return (sp.eye(V) + float(lam) * laplacian(faces, V)).tocsr()


def direct_solver(faces, V, lam):
    """b (V,) or (V,k) fp64 -> M^-1 b by sparse LU"""
    lu = spl.splu(system(faces, V, lam).tocsc())
    return lambda b: lu.solve(np.ascontiguousarray(b, F64))


# ---------------------------------------------------------------------------- the solver, restated
class Rows:
    """the adjacency as a (V, d_max) table so that a row's differences are added one neighbour at a time, in order"""

    def __init__(self, faces, V):
        self.off, self.idx = adjacency(faces, V)
        deg = np.diff(self.off)
        self.V, self.d_max = V, int(deg.max()) if V else 0
        self.nb = np.zeros((V, max(self.d_max, 1)), np.int64)
        self.valid = np.zeros((V, max(self.d_max, 1)), bool)
        for k in range(self.d_max):
            has = deg > k
            self.nb[has, k] = self.idx[self.off[:-1][has] + k]
            self.valid[has, k] = True

    def apply32(self, lam, x):
        """M x for one fp32 column, rounding for rounding what the kernel's row does"""
        x = np.ascontiguousarray(x, F32)
        l = np.zeros(self.V, F32)
        for k in range(self.d_max):
            l = np.where(self.valid[:, k], l + (x - x[self.nb[:, k]]), l).astype(F32)
        return (x + F32(lam) * l).astype(F32)


def dot64(a, b):
    """fp32 products, added in fp64"""
    return float(np.sum((a * b).astype(F64)))


def cg32(rows, lam, b, tol, max_iter):
    """one column: -> (x fp32, iterations, converged)"""
    b = np.ascontiguousarray(b, F32)
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    bb = dot64(b, b)
    if bb == 0.0:
        return x, 0, True
    rr, stop = bb, float(tol) * float(tol) * bb
    for it in range(1, max_iter + 1):
        Ap = rows.apply32(lam, p)
        alpha = F32(rr / dot64(p, Ap))
        x = (x + alpha * p).astype(F32)
        r = (r - alpha * Ap).astype(F32)
        rr_new = dot64(r, r)
        if rr_new <= stop:
            return x, it, True
        p = (r + F32(rr_new / rr) * p).astype(F32)
        rr = rr_new
    return x, max_iter, False


def cg32_columns(rows, lam, b, tol, max_iter):
    """b (V,3) -> (x (V,3) fp32, [iterations], [converged])"""
    out = [cg32(rows, lam, b[:, c], tol, max_iter) for c in range(b.shape[1])]
    return np.stack([o[0] for o in out], 1), [o[1] for o in out], [o[2] for o in out]


def relative_max_error(x, exact):
    """||x - x*||_inf / ||x*||_inf over the whole array"""
    exact = np.asarray(exact, F64)
    return float(np.abs(np.asarray(x, F64) - exact).max() / np.abs(exact).max())


def iteration_cap(lam, d_max, tol):
    """twice sqrt(kappa) / 2 * ln(2 / tol) with kappa <= 1 + 2 lam d_max (Gershgorin), at least 8"""
    return max(8, int(math.ceil(math.sqrt(1.0 + 2.0 * lam * d_max) * math.log(2.0 / tol))))


# ---------------------------------------------------------------------------- Adam with one denominator
def adam_uniform_step(p, g, m, s, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch tensors, in place: m <- b1 m + (1 - b1) g; s <- b2 s + (1 - b2) g^2;
    p <- p - lr (m / (1 - b1^t)) / (eps + max sqrt(s / (1 - b2^t)))"""
    m.mul_(b1).add_(g, alpha=1.0 - b1)
    s.mul_(b2).addcmul_(g, g, value=1.0 - b2)
    denom = eps + (s / (1.0 - b2 ** step)).sqrt().max()
    p.sub_(lr * (m / (1.0 - b1 ** step)) / denom)
    return denom
