"""TEST INFRASTRUCTURE ONLY: torch restatement (any dtype; fp64 + autograd in the gradient tests) of PyTorch3D's
blending.sigmoid_alpha_blend alpha channel -- what SoftSilhouetteShader renders -- and of the silhouette loss, plus the
silhouette-fitting scene both the host and the GPU suite use.

PARITY UNPINNED: PyTorch3D is absent; formula per pytorch3d/renderer/blending.py:
    mask = pix_to_face >= 0;  prob = sigmoid(-dists / sigma) * mask;  alpha = 1 - prod_k (1 - prob_k)."""
import math

import numpy as np
import torch


def sigmoid_alpha_blend(dists, mask, sigma=1e-4):
    """dists (..., K), mask (..., K) bool -> alpha (...)."""
    prob = torch.sigmoid(-dists / sigma) * mask.to(dists.dtype)
    return 1.0 - torch.prod(1.0 - prob, dim=-1)


def alpha_grad_closed_form(dists, mask, sigma=1e-4):
    """d alpha / d dists_k = -prob_k * prod_j (1 - prob_j) / sigma: the full product, no division (csrc/silhouette.hip)."""
    prob = torch.sigmoid(-dists / sigma) * mask.to(dists.dtype)
    keep = torch.prod(1.0 - prob, dim=-1, keepdim=True)
    return -prob * keep / sigma


def silhouette_loss(alpha, target):
    """mean over views and pixels of (alpha - target)^2"""
    return ((alpha - target) ** 2).mean()


def blur_radius(sigma):
    """PyTorch3D's silhouette tutorial: np.log(1. / 1e-4 - 1.) * blend_params.sigma"""
    return math.log(1.0 / 1e-4 - 1.0) * sigma


# ------------------------------------------------------------------ the fitting scene (issue: "host test 5" / "GPU test 9")
FIT = dict(S=64, K=8, sigma=1e-4, dist=2.1, elev=20.0, azims=(0.0, 90.0, 180.0, 270.0), lr=0.005, steps=40, bound=0.45)
DISPLACEMENTS = {"shift": lambda v: v + np.array([0.06, 0.03, 0.0], v.dtype), "scale": lambda v: v * v.dtype.type(1.08)}


def fit_cameras():
    from oracle import render_ref as rr
    n = len(FIT["azims"])
    return rr.look_at_view_transform(FIT["dist"], [FIT["elev"]] * n, list(FIT["azims"]))


def fit_on_the_reference(cow, displacement, nthreads=8):
    """The silhouette fit on the CPU in fp64: C oracle rasteriser for the fragment assignment of every step,
    oracle.soft_ref.soft_geometry for the differentiable distances, this module's alpha and loss, torch.optim.Adam.
    -> list of the losses of all steps."""
    from oracle import render_ref as rr
    from oracle import soft_ref as SR
    S, K, sigma = FIT["S"], FIT["K"], FIT["sigma"]
    blur = blur_radius(sigma)
    R, T = fit_cameras()
    faces_np = cow["faces"]
    faces = torch.from_numpy(faces_np).long()
    targets = []
    for b in range(R.shape[0]):
        hard = rr.rasterize_k(rr.project_verts(cow["verts"], R[b], T[b]), faces_np, S, 1, 0.0, nthreads=nthreads)
        targets.append(torch.from_numpy((hard[0][..., 0] >= 0).astype(np.float64)))
    verts = torch.from_numpy(DISPLACEMENTS[displacement](cow["verts"])).double().requires_grad_(True)
    opt = torch.optim.Adam([verts], lr=FIT["lr"])
    losses = []
    for _ in range(FIT["steps"]):
        opt.zero_grad()
        total = 0.0
        v32 = verts.detach().numpy().astype(np.float32)
        for b in range(R.shape[0]):
            frag = rr.rasterize_k(rr.project_verts(v32, R[b], T[b]), faces_np, S, K, blur, True, nthreads=nthreads)
            p2f = torch.from_numpy(frag[0].astype(np.int64))
            ndc = SR.project(verts, torch.from_numpy(R[b]).double(), torch.from_numpy(T[b]).double())
            _, _, sd, mask = SR.soft_geometry(ndc, faces, p2f, S, True)
            total = total + silhouette_loss(sigmoid_alpha_blend(sd, mask, sigma), targets[b])
        loss = total / R.shape[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses
