"""Laplacian-preconditioned vertex steps (Nicolet, Jacobson and Jakob, "Large Steps in Inverse Rendering of
Geometry", SIGGRAPH Asia 2021).

The render gradient reaches a vertex only through the pixels its faces cover in the step's views: sparse, noisy and different
at every vertex.  Instead of penalising what that noise does to the mesh, the step itself is preconditioned: the optimised
leaf is u = M v with M = I + lambda L, L the combinatorial Laplacian of the (static) topology, and every step recovers
v = M^-1 u.  M is symmetric, so d loss / d u = M^-1 d loss / d v: every eigen-component of the gradient is scaled by
1 / (1 + lambda mu) <= 1 and the high frequencies are damped.  M^-1 is entrywise non-negative with unit row sums, so no
vertex moves further than the largest move of an entry of u.

    dv = DiffusedVertices(verts, faces, lam=19.0)
    Adam([{"params": [dv.params], "uniform": True}], lr)     # ONE (V,3) leaf; the paper's Adam with one denominator
    verts = dv.verts()                                         # (V,3), differentiable w.r.t. dv.params

The device wrappers of csrc/diffuse.hip live here as well: diffuse_apply, diffuse_solve, adam_step_uniform.
"""
import math

import torch

from . import _lib
from ._lib import call, dptr, stream_ptr

F32, I32 = torch.float32, torch.int32


def _check_lambda(lam):
    lam = float(lam)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"lambda must be finite and >= 0, got {lam!r}")
    return lam


def _check_system(nbr_off, nbr_idx, x, what):
    if not torch.is_tensor(x):
        raise TypeError(f"{what} must be a tensor (V,3)")
    if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError(f"{what} must be (V,3) with V >= 1, got {tuple(x.shape)}")
    V = int(x.shape[0])
    if nbr_off.dim() != 1 or nbr_off.numel() != V + 1 or nbr_idx.dim() != 1:
        raise ValueError(f"nbr_off must hold V + 1 = {V + 1} offsets and nbr_idx be flat, got {tuple(nbr_off.shape)} and "
                         f"{tuple(nbr_idx.shape)}")
    return V


def diffuse_apply(nbr_off, nbr_idx, x, lam):
    """y (V,3) = (I + lam L) x, (L x)_i = sum_{j in nbr(i)} (x_i - x_j) in adjacency order; nbr_off (V+1) / nbr_idx: the
    int32 CSR adjacency of st3d.mesh_losses.build_topology (the CALLER guarantees every index is in [0, V))."""
    V = _check_system(nbr_off, nbr_idx, x, "x")
    lam = _check_lambda(lam)
    x = x.detach().to(F32).contiguous()
    y = torch.empty((V, 3), dtype=F32, device=x.device)
    call("st3d_diffuse_apply", dptr(nbr_off, I32), dptr(nbr_idx, I32), V, lam, dptr(x), dptr(y), stream_ptr())
    return y


def diffuse_solve(nbr_off, nbr_idx, b, lam, tol=1e-6, max_iter=1000):
    """(x (V,3), info (3,3) int32) with (I + lam L) x = b, column by column by conjugate gradients from x = 0 until
    ||r|| <= tol ||b|| or max_iter iterations.  info[c] = (iterations, converged, the bits of the fp32 relative residual) of
    column c, written on the device: read_info(info) turns it into Python numbers (and synchronises)."""
    V = _check_system(nbr_off, nbr_idx, b, "b")
    lam = _check_lambda(lam)
    tol = float(tol)
    if not (math.isfinite(tol) and tol > 0.0):
        raise ValueError(f"tol must be finite and > 0, got {tol!r}")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
    b = b.detach().to(F32).contiguous()
    nbytes = _lib.load().st3d_diffuse_workspace_bytes(V)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=b.device)
    x = torch.empty((V, 3), dtype=F32, device=b.device)
    info = torch.empty((3, 3), dtype=I32, device=b.device)
    call("st3d_diffuse_solve", dptr(nbr_off, I32), dptr(nbr_idx, I32), V, lam, dptr(b), dptr(x), tol, int(max_iter), dptr(ws),
         nbytes, dptr(info), stream_ptr())
    return x, info


def read_info(info):
    """info (3,3) int32 of diffuse_solve -> {"iterations": [3 ints], "converged": [3 bools], "residual": [3 floats]}; one
    device-to-host copy."""
    host = info.detach().cpu()
    return {"iterations": [int(v) for v in host[:, 0]], "converged": [bool(v) for v in host[:, 1]],
            "residual": [float(v) for v in host[:, 2].contiguous().view(F32)]}


def adam_step_uniform(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """The Adam update with one denominator for the whole tensor, in place on p, m, v:
        m <- m + (g - m)(1 - b1);  v <- b2 v + (1 - b2) g^2;  p <- p - lr (m / (1 - b1^t)) / (eps + max sqrt(v / (1 - b2^t)))"""
    partials = torch.empty((_lib.load().st3d_reduce_partials(),), dtype=F32, device=p.device)
    call("st3d_adam_step_uniform", dptr(p, F32), dptr(g.contiguous(), F32), dptr(m, F32), dptr(v, F32), p.numel(), int(step),
         float(lr), float(b1), float(b2), float(eps), dptr(partials), stream_ptr())


def iteration_cap(lam, max_degree, tol):
    """The max_iter DiffusedVertices derives: kappa(M) <= 1 + 2 lam d_max (Gershgorin: the eigenvalues of L lie in
    [0, 2 d_max]); conjugate gradients reach a relative error tol in the M-norm after at most sqrt(kappa) / 2 * ln(2 / tol)
    iterations in exact arithmetic.  The cap is twice that, and at least 8."""
    kappa = 1.0 + 2.0 * float(lam) * float(max_degree)
    return max(8, int(math.ceil(2.0 * 0.5 * math.sqrt(kappa) * math.log(2.0 / float(tol)))))


class _Solve(torch.autograd.Function):
    """v = M^-1 u; M is symmetric, so the backward is the same solve applied to the incoming gradient."""

    @staticmethod
    def forward(ctx, params, owner):
        ctx.owner = owner
        x, owner._info = diffuse_solve(owner.nbr_off, owner.nbr_idx, params.detach(), owner.lam, owner.tol, owner.max_iter)
        return x

    @staticmethod
    def backward(ctx, grad_verts):
        owner = ctx.owner
        g, owner._info_backward = diffuse_solve(owner.nbr_off, owner.nbr_idx, grad_verts.contiguous(), owner.lam, owner.tol,
                                                owner.max_iter)
        return g, None


class DiffusedVertices:
    def __init__(self, verts, faces, lam, tol=1e-6, max_iter=None):
        from .mesh_losses import build_topology
        v = verts.detach()
        if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1:
            raise ValueError(f"verts must be (V,3) with V >= 1, got {tuple(verts.shape)}")
        f = faces.detach()
        if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f"faces must be (F,3) with F >= 1, got {tuple(faces.shape)}")
        V = int(v.shape[0])
        if int(f.min()) < 0 or int(f.max()) >= V:          # on the device an index outside the mesh would be a fault
            raise ValueError(f"faces name vertices outside [0, {V})")
        self.lam = _check_lambda(lam)
        if not self.lam > 0.0:
            raise ValueError("lambda must be > 0: with 0 the vertices are their own parameters")
        self.tol = float(tol)
        if not (math.isfinite(self.tol) and self.tol > 0.0):
            raise ValueError(f"tol must be finite and > 0, got {tol!r}")
        topo = build_topology(f.to(v.device), V)
        self.nbr_off, self.nbr_idx = topo["nbr_off"], topo["nbr_idx"]
        off = self.nbr_off.cpu().long()
        idx = self.nbr_idx.cpu().long()
        degree = off[1:] - off[:-1]
        self.max_degree = int(degree.max())
        self.max_iter = iteration_cap(self.lam, self.max_degree, self.tol) if max_iter is None else int(max_iter)
        if self.max_iter < 1:
            raise ValueError(f"max_iter must be >= 1, got {max_iter!r}")
        # u = M v once, on the host in fp64, rounded once
        v64 = v.cpu().double()
        row = torch.repeat_interleave(torch.arange(V), degree)
        lap = degree[:, None].double() * v64
        lap.index_add_(0, row, -v64[idx])
        self.params = (v64 + self.lam * lap).to(F32).to(v.device).contiguous().requires_grad_(True)
        self._info = self._info_backward = None

    def verts(self):
        """(V,3) = M^-1 params, with the same solve as its backward.  No host synchronisation."""
        return _Solve.apply(self.params, self)

    def load_params(self, t):
        """Overwrite the parameters in place (checkpoint resume): the leaf and Adam's moments keep their identity."""
        if tuple(t.shape) != tuple(self.params.shape):
            raise ValueError(f"the diffused vertices hold {tuple(self.params.shape)} parameters, got {tuple(t.shape)}")
        with torch.no_grad():
            self.params.copy_(t)

    def last_info(self, backward=False):
        """Iterations, convergence and relative residual per column of the latest forward (or backward) solve, None before
        the first; synchronises the host."""
        info = self._info_backward if backward else self._info
        return None if info is None else read_info(info)
