"""GPU tests of the silhouette rasteriser (csrc/silraster.hip and everything above it): SoftSilhouetteShader's alpha, the
silhouette loss and its vertex gradient at faces_per_pixel K = 1..64 without fragments in memory.

Where K <= 8 the existing path (st3d_raster_soft_fwd's fragments + csrc/silhouette.hip) is the reference, bit for bit; beyond
it the C oracle (K <= 16, its lists hold 16 entries) and tests/_silraster_ref.py (any K; pinned to the oracle by
tests/test_silraster_ref.py), both evaluated on the fp32 projected vertices the kernels consumed.  Every test about K > 8
asserts with the CPU reference that its scene has pixels with more than 8 candidates.

Bounds are the project's existing ones (tests/test_gpu_silhouette.py): alpha 2e-5 absolute against fp64, a loss 2e-5 relative,
d/d verts 5e-5 relative L2 (1e-4 through clipped faces)."""
import os

import numpy as np
import pytest
import torch

import _silhouette_ref as SIL
import _silraster_ref as SRR
from test_gpu_silhouette import CASES, NEAR_CAMERA

pytestmark = pytest.mark.gpu

FAR = [dict(dist=2.1, elev=[20.0], azim=[30.0], at=(0, 0.10, 0.25)), dict(dist=2.1, elev=[-15.0], azim=[200.0], at=(0, 0.10, 0.25))]
# the cow from nearby: at sigma = 1e-4 with the tutorial's blur 92 % of the pixels with 0 < alpha < 1 have more than 8
# candidates, the largest count is 61 and ten pixels have more than 50 (tests/_silraster_ref.py on the CPU)
DENSE = dict(dist=1.3, elev=[35.0], azim=[65.0], at=(0, 0.10, 0.25))
NT = min(8, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


def _cameras(views):
    from oracle import render_ref as rr
    RT = [rr.look_at_view_transform(c["dist"], c["elev"], c["azim"], at=c["at"]) for c in views]
    return np.concatenate([r for r, _ in RT]), np.concatenate([t for _, t in RT])


def _ndc(ops, dev, cow, views, verts=None):
    R, T = _cameras(views)
    v = torch.from_numpy(cow["verts"] if verts is None else verts).to(dev)
    faces = torch.from_numpy(cow["faces"]).to(dev)
    return ops.project_verts(v, torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)), faces, R, T


def _disc(S, B, seed=5):
    """a 0/1 mask that is neither the coverage nor its complement: a disc per view"""
    ys, xs = np.mgrid[0:S, 0:S]
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 1, S, S), np.float32)
    for b in range(B):
        c, r = rng.uniform(0.35, 0.65, 2) * S, rng.uniform(0.25, 0.4) * S
        out[b, 0] = ((ys - c[0]) ** 2 + (xs - c[1]) ** 2 <= r * r)
    return torch.from_numpy(out)


def _candidates(ndc, cow, S, blur, clip=True):
    return [SRR.candidates(ndc[b].cpu().numpy(), cow["faces"], S, blur, clip, False, True, 0.5) for b in range(ndc.shape[0])]


# ---------------------------------------------------------------------------- 1. K <= 8: the existing path, bit for bit
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"K{c[0]}-blur{c[1]:g}-sigma{c[2]:g}")
def test_alpha_and_loss_equal_the_fragment_path_bit_for_bit(dev, ops, cow, case, near):
    """alpha == silhouette_fwd(raster_soft_fwd(...)) and the fused loss == ops.silhouette_loss on those fragments, bitwise,
    at K = 1, 4, 8 and the case's own K.  The one place allowed to differ is the documented corner (a pixel with more than K
    candidates of which one lies on a quadrilateral split by the near plane: 'halves first, then the K nearest' here, the
    K-list's memory in the fragment path); such pixels are held to the definition (tests/_silraster_ref.py, 2e-5) instead."""
    _, blur, sigma = case
    S = 64
    views = [NEAR_CAMERA] if near else FAR
    ndc, faces, _, _ = _ndc(ops, dev, cow, views)
    B = ndc.shape[0]
    target = _disc(S, B).to(dev)
    scale = 1.0 / (S * S * B)
    cands = _candidates(ndc, cow, S, blur, blur > 0)
    for K in sorted({1, 4, 8, case[0]}):
        frag = ops.raster_soft_fwd(ndc, faces, S, K, blur, blur > 0, z_clip=0.5 if near else None)
        old = ops.silhouette_fwd(frag[0], frag[3], sigma)
        alpha, state = ops.silraster_fwd(ndc, faces, S, K, blur, sigma, blur > 0)
        assert alpha.shape == (B, 1, S, S) and alpha.dtype == torch.float32 and state.shape == (3, B, S, S)
        differ = (alpha != old)[:, 0].cpu().numpy()
        corner = np.zeros((B, S, S), bool)
        for b, c in enumerate(cands):
            on_half = np.zeros(S * S, bool)
            on_half[c.pix[(c.code[c.slot] >= 2) & (c.code[c.slot] < 8)]] = True
            corner[b] = ((c.count > K) & on_half).reshape(S, S)
            ref = c.alpha(K, sigma)
            err = float(np.abs(alpha[b, 0].cpu().double().numpy() - ref).max())
            print(f"near={near} K={K} blur={blur} view {b}: max |alpha - ref| {err:.3e}")
            assert err <= 2e-5
        print(f"near={near} K={K} blur={blur}: {int(differ.sum())} pixels differ from the fragment path, "
              f"{int(corner.sum())} pixels in the corner")
        assert not (differ & ~corner).any()
        if not near:
            assert not corner.any() and torch.equal(alpha, old)
        assert bool((alpha > 0).any()) and bool((alpha == 0).any())
        loss, state4 = ops.silraster_loss(ndc, faces, target, K, blur, sigma, scale, blur > 0)
        assert state4.shape == (4, B, S, S) and torch.equal(state4[:3].view(torch.int32), state.view(torch.int32))
        assert torch.equal(state4[3], (alpha - target)[:, 0])
        if not differ.any():
            old_loss, _ = ops.silhouette_loss(frag[0], frag[3], target, sigma, scale)
            assert torch.equal(loss, old_loss)


# ---------------------------------------------------------------------------- 2. the deck: selection and exhaustion
@pytest.mark.parametrize("K", [1, 8, 12, 20, 50])
def test_deck_of_twenty_triangles_matches_the_closed_form(dev, ops, K):
    """20 copies of one triangle at depths 2.00, 2.05, ...: every covered pixel has exactly 20 candidates with the same d, so
    alpha = 1 - (1 - p)^min(K, 20): selection when K < 20, exhaustion when K > 20, a second and a third pass in between."""
    S, sigma, n = 64, 1e-4, 20
    blur = SIL.blur_radius(sigma)
    ndc_np, faces_np = SRR.deck(n)
    cand = SRR.candidates(ndc_np, faces_np, S, blur, True, False, True, 0.5)
    assert set(np.unique(cand.count).tolist()) == {0, n}
    ndc = torch.from_numpy(ndc_np)[None].to(dev)
    alpha, _ = ops.silraster_fwd(ndc, torch.from_numpy(faces_np).to(dev), S, K, blur, sigma)
    got = alpha[0, 0].cpu().double().numpy()
    covered = (cand.count > 0).reshape(S, S)
    p = np.zeros(S * S)
    p[cand.pix] = 1.0 / (1.0 + np.exp(cand.sd.astype(np.float64) / sigma))
    closed = (1.0 - (1.0 - p) ** min(K, n)).reshape(S, S)
    e_closed, e_ref = float(np.abs(got - closed).max()), float(np.abs(got - cand.alpha(K, sigma)).max())
    print(f"deck K={K}: max |alpha - closed form| {e_closed:.3e}, max |alpha - reference| {e_ref:.3e}")
    assert e_closed <= 2e-5 and e_ref <= 2e-5
    assert float(np.abs(got[~covered]).max()) == 0.0 and covered.sum() > 500
    partial = (closed > 1e-3) & (closed < 1 - 1e-3)
    assert partial.sum() > 20                                   # pixels where the exponent min(K, 20) is visible


# ---------------------------------------------------------------------------- 3. the dense scene
def _dense(ops, dev, cow, S=128):
    ndc, faces, R, T = _ndc(ops, dev, cow, [DENSE])
    blur = SIL.blur_radius(1e-4)
    cand = _candidates(ndc, cow, S, blur)[0]
    a64 = cand.alpha(64, 1e-4).reshape(-1)
    partial = (a64 > 0) & (a64 < 1)
    share = float((cand.count[partial] > 8).mean())
    print(f"dense scene at {S}^2: {int(partial.sum())} pixels with 0 < alpha < 1, {100 * share:.1f} % of them with more than 8 "
          f"candidates, largest count {int(cand.count.max())}, {int((cand.count > 50).sum())} pixels over 50")
    assert partial.sum() > 1000 and share >= 0.01 and cand.count.max() <= 64        # the precondition
    return ndc, faces, R, T, blur, cand


def test_dense_scene_matches_the_oracle_and_the_reference(dev, ops, cow):
    from oracle import render_ref as rr
    S, sigma = 128, 1e-4
    ndc, faces, _, _, blur, cand = _dense(ops, dev, cow, S)
    # K = 16: the C oracle's fragments + sigmoid_alpha_blend
    p2f, _, _, dists = rr.rasterize_k(ndc[0].cpu().numpy(), cow["faces"], S, 16, blur, True, NT, z_clip=0.5)
    ref16 = SIL.sigmoid_alpha_blend(torch.from_numpy(dists.astype(np.float64)), torch.from_numpy(p2f >= 0), sigma).numpy()
    alpha = {K: ops.silraster_fwd(ndc, faces, S, K, blur, sigma)[0][0, 0].cpu().double().numpy() for K in (8, 16, 50, 64)}
    e16 = float(np.abs(alpha[16] - ref16).max())
    print(f"dense K=16: max |alpha - oracle| {e16:.3e}")
    assert e16 <= 2e-5
    for K in (16, 50, 64):
        err = float(np.abs(alpha[K] - cand.alpha(K, sigma)).max())
        print(f"dense K={K}: max |alpha - reference| {err:.3e}")
        assert err <= 2e-5
    d50 = float(np.abs(alpha[50] - alpha[8]).max())
    d64 = float(np.abs(alpha[64] - alpha[50]).max())
    print(f"dense: max |alpha_50 - alpha_8| {d50:.4f}, max |alpha_64 - alpha_50| {d64:.3e}")
    assert d50 > 1e-3                                           # a ninth face matters: what K <= 8 cannot give
    assert (cand.count > 50).any() and d64 > 0.0


# ---------------------------------------------------------------------------- 4. the vertex gradient
def _public(dev, cow, S, R, T, verts_np=None):
    from st3d.render import FoVPerspectiveCameras, Meshes, MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    verts = torch.from_numpy(cow["verts"] if verts_np is None else verts_np).to(dev).requires_grad_(True)
    mesh = Meshes(verts=[verts], faces=[torch.from_numpy(cow["faces"].astype(np.int64)).to(dev)])
    renderer = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftPhongShader())
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(T), device=dev)
    return mesh, verts, renderer, cams


def _loss_and_grad(dev, cow, S, R, T, target, K, sigma=1e-4, batch_denom=None, verts_np=None):
    import losses as L
    mesh, verts, renderer, cams = _public(dev, cow, S, R, T, verts_np)
    loss = L.compute_silhouette_loss(renderer, mesh, cams, target, sigma=sigma, batch_denom=batch_denom, faces_per_pixel=K)
    loss.backward()
    return loss.detach(), verts.grad.detach().clone()


def _reference_loss_and_grad(ops, dev, cow, S, R, T, target, K, sigma, verts_np, near):
    """fp64 autograd of the restatement over oracle.soft_ref's geometry on the REFERENCE's fragment assignment
    (tests/_silraster_ref.py), as tests/test_gpu_silhouette.py::_reference_loss_and_grad does on the GPU's: the fp32 NDC the
    kernels consumed with the fp64 projection's graph attached.  -> (loss, d/d verts, fragments on clipped records, cands)"""
    from oracle import soft_ref as SR
    blur = SIL.blur_radius(sigma)
    ndc = ops.project_verts(torch.from_numpy(verts_np).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev))
    fc = torch.from_numpy(cow["faces"]).long()
    vt = torch.from_numpy(verts_np).double().requires_grad_(True)
    B = R.shape[0]
    total, clipped, cands = 0.0, 0, _candidates(ndc, cow, S, blur)
    for b in range(B):
        ndc_b = SR.project(vt, torch.from_numpy(R[b]).double(), torch.from_numpy(T[b]).double())
        ndc_b = ndc_b + (ndc[b].cpu().double() - ndc_b).detach()
        slots = torch.from_numpy(cands[b].fragments(K)[0])
        clipped += int((cands[b].code[slots[slots >= 0].numpy()] >= 2).sum())
        if near:
            _, _, sd, mask = SR.clipped_geometry(ndc_b, fc, slots, S, True, True, 0.5)
        else:
            _, _, sd, mask = SR.soft_geometry(ndc_b, fc, torch.where(slots >= 0, slots >> 1, slots), S, True)
        alpha = SIL.sigmoid_alpha_blend(sd, mask, sigma)
        total = total + ((alpha - target[b, 0].cpu().double()) ** 2).sum()
    loss = total / (S * S * B)
    loss.backward()
    return float(loss.detach()), vt.grad, clipped, cands


@pytest.mark.parametrize("K", [16, 50])
def test_vertex_gradient_on_the_dense_scene_matches_fp64_autograd(dev, ops, cow, K):
    S = 128
    _, _, R, T, _, cand = _dense(ops, dev, cow, S)
    target = _disc(S, 1, seed=4).to(dev)
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, K)
    ref_loss, ref_grad, clipped, _ = _reference_loss_and_grad(ops, dev, cow, S, R, T, target, K, 1e-4, cow["verts"], near=False)
    rel_l = abs(float(loss) - ref_loss) / ref_loss
    rel_v = float((grad.cpu().double() - ref_grad).norm() / ref_grad.norm())
    print(f"dense K={K}: loss {float(loss):.8f} ref {ref_loss:.8f} rel {rel_l:.3e}; d/d verts rel L2 {rel_v:.3e}")
    assert clipped == 0 and ref_loss > 1e-3 and float(ref_grad.norm()) > 0
    assert rel_l <= 2e-5
    assert rel_v <= 5e-5


def test_vertex_gradient_flows_through_clipped_faces_at_sixteen(dev, ops, cow):
    from oracle import render_ref as rr
    S, K = 48, 16
    R, T = rr.look_at_view_transform(NEAR_CAMERA["dist"], NEAR_CAMERA["elev"], NEAR_CAMERA["azim"], at=NEAR_CAMERA["at"])
    target = _disc(S, 1, seed=9).to(dev)
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, K)
    ref_loss, ref_grad, clipped, cands = _reference_loss_and_grad(ops, dev, cow, S, R, T, target, K, 1e-4, cow["verts"], near=True)
    rel_l = abs(float(loss) - ref_loss) / ref_loss
    rel_v = float((grad.cpu().double() - ref_grad).norm() / ref_grad.norm())
    print(f"near view K={K}: {clipped} fragments on clipped records, {int((cands[0].count > 8).sum())} pixels with more than 8 "
          f"candidates; loss rel {rel_l:.3e}; d/d verts rel L2 {rel_v:.3e}")
    assert clipped > 20 and (cands[0].count > 8).sum() > 20       # slot code >= 2, and a ninth face
    assert rel_l <= 2e-5
    assert rel_v <= 1e-4


def test_gradient_at_eight_is_the_existing_paths(dev, cow):
    """faces_per_pixel=8 asks for the new kernels at the old K: the same loss bit for bit, the gradient within 5e-5 (the same
    contributions summed in another order)"""
    import losses as L
    S = 64
    R, T = _cameras(FAR)
    target = _disc(S, 2).to(dev)
    v_np = SIL.DISPLACEMENTS["shift"](cow["verts"])
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, 8, verts_np=v_np)
    mesh, verts, renderer, cams = _public(dev, cow, S, R, T, v_np)
    old = L.compute_silhouette_loss(renderer, mesh, cams, target)
    old.backward()
    rel = float((grad - verts.grad).norm() / verts.grad.norm())
    print(f"K=8: d/d verts differs from the fragment path's by {rel:.3e} relative L2")
    assert torch.equal(loss, old.detach()) and float(verts.grad.norm()) > 0
    assert rel <= 5e-5


# ---------------------------------------------------------------------------- 5. the memory rule
def _kept_bytes(node, exclude_shapes):
    seen, total = set(), 0

    def walk(x):
        nonlocal total
        if torch.is_tensor(x):
            if x.data_ptr() not in seen and tuple(x.shape) not in exclude_shapes:
                seen.add(x.data_ptr())
                total += x.numel() * x.element_size()
        elif isinstance(x, (tuple, list)):
            for y in x:
                walk(y)
        elif isinstance(x, dict):
            for y in x.values():
                walk(y)
    walk(list(vars(node).values()))
    return total


def test_at_most_sixteen_bytes_per_pixel_are_kept_for_the_backward(dev, cow):
    """what the autograd node keeps besides vertices, faces and cameras: <= 16 bytes per pixel at K = 50 (the fragment path
    keeps p2f, grad_dists and the record slots: 12 K bytes per pixel, and its rasteriser writes 28 K)"""
    import losses as L
    S, B = 64, 2
    R, T = _cameras(FAR)
    target = _disc(S, B).to(dev)
    V, Fn = cow["verts"].shape[0], cow["faces"].shape[0]
    exclude = {(V, 3), (Fn, 3), (B, 3, 3), (B, 3), (B, V, 3)}
    mesh, verts, renderer, cams = _public(dev, cow, S, R, T)
    loss = L.compute_silhouette_loss(renderer, mesh, cams, target, faces_per_pixel=50)
    new = _kept_bytes(loss.grad_fn, exclude - {(B, V, 3)})
    old_loss = L.compute_silhouette_loss(renderer, mesh, cams, target)
    old = _kept_bytes(old_loss.grad_fn, exclude)
    print(f"kept per pixel: silhouette rasteriser at K=50 {new / (B * S * S):.1f} B, fragment path at K=8 {old / (B * S * S):.1f} B")
    assert 0 < new <= 16 * B * S * S
    assert old >= 12 * 8 * B * S * S
    from st3d.render import MeshRasterizer, MeshRenderer, SilhouetteRasterizationSettings, SoftSilhouetteShader
    sil = MeshRenderer(MeshRasterizer(None, SilhouetteRasterizationSettings(image_size=S, blur_radius=SIL.blur_radius(1e-4),
                                                                            faces_per_pixel=50)), SoftSilhouetteShader())
    _, alpha = sil.render(mesh, cams)
    assert 0 < _kept_bytes(alpha.grad_fn, exclude - {(B, V, 3)}) <= 16 * B * S * S


# ---------------------------------------------------------------------------- 6. determinism, NaN, sharding, the renderer
def test_loss_and_gradient_are_bitwise_reproducible(dev, cow):
    from st3d import ops as O
    assert O.is_deterministic()
    S = 64
    R, T = _cameras(FAR)
    target = _disc(S, 2).to(dev)
    v_np = SIL.DISPLACEMENTS["shift"](cow["verts"])
    a = _loss_and_grad(dev, cow, S, R, T, target, 50, verts_np=v_np)
    b = _loss_and_grad(dev, cow, S, R, T, target, 50, verts_np=v_np)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1].abs().sum()) > 0


def test_float_atomics_agree_with_the_fixed_point_gradient(dev, cow):
    from st3d import ops as O
    S = 64
    R, T = _cameras(FAR)
    target = _disc(S, 2).to(dev)
    det = _loss_and_grad(dev, cow, S, R, T, target, 50)
    O.set_deterministic(False)
    try:
        flt = _loss_and_grad(dev, cow, S, R, T, target, 50)
    finally:
        O.set_deterministic(True)
    assert torch.equal(det[0], flt[0])
    assert float((det[1] - flt[1]).norm()) <= 1e-5 * float(det[1].norm())


def test_a_nan_vertex_gives_a_nan_loss_and_gradient(dev, cow):
    S = 64
    R, T = _cameras(FAR)
    target = _disc(S, 2).to(dev)
    v_np = cow["verts"].copy()
    v_np[cow["faces"][100, 0], 1] = np.nan
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, 50, verts_np=v_np)
    assert bool(torch.isnan(loss)) and bool(torch.isnan(grad).all())
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, 50)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())


def test_two_halves_of_a_batch_sum_to_the_full_batch(dev, cow):
    S, K = 64, 50
    views = FAR + [dict(dist=2.1, elev=[40.0], azim=[100.0], at=(0, 0.10, 0.25)), DENSE]
    R, T = _cameras(views)
    target = _disc(S, 4).to(dev)
    v_np = SIL.DISPLACEMENTS["shift"](cow["verts"])
    full_l, full_g = _loss_and_grad(dev, cow, S, R, T, target, K, verts_np=v_np)
    parts = [_loss_and_grad(dev, cow, S, R[s], T[s], target[s].contiguous(), K, batch_denom=4, verts_np=v_np)
             for s in (slice(0, 2), slice(2, 4))]
    sum_l, sum_g = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert abs(float(sum_l) - float(full_l)) <= 1e-6 * float(full_l)
    assert float((sum_g - full_g).norm()) <= 1e-6 * float(full_g.norm())
    assert float(parts[0][0]) > 0 and float(parts[1][0]) > 0


def test_soft_silhouette_shader_with_silhouette_raster_settings(dev, ops, cow):
    """MeshRenderer(SilhouetteRasterizationSettings(faces_per_pixel=50), SoftSilhouetteShader): (n,S,S,4), RGB = 1, alpha and
    gradient bitwise the op chain's"""
    from st3d.render import (BlendParams, FoVPerspectiveCameras, Meshes, MeshRasterizer, MeshRenderer,
                             SilhouetteRasterizationSettings, SoftSilhouetteShader)
    S, K, sigma = 64, 50, 1e-4
    blur = SIL.blur_radius(sigma)
    R, T = _cameras(FAR)
    verts = torch.from_numpy(cow["verts"]).to(dev).requires_grad_(True)
    mesh = Meshes(verts=[verts], faces=[torch.from_numpy(cow["faces"].astype(np.int64)).to(dev)])
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(T), device=dev)
    renderer = MeshRenderer(MeshRasterizer(None, SilhouetteRasterizationSettings(image_size=S, blur_radius=blur, faces_per_pixel=K)),
                            SoftSilhouetteShader(blend_params=BlendParams(sigma=sigma)))
    rgba = renderer(meshes_world=mesh, cameras=cams)
    assert rgba.shape == (2, S, S, 4) and bool((rgba[..., :3] == 1).all())
    ndc = ops.project_verts(verts.detach(), cams.R, cams.T)
    alpha, state = ops.silraster_fwd(ndc, mesh.faces_i32(), S, K, blur, sigma)
    assert torch.equal(rgba[..., 3].detach(), alpha[:, 0])
    old, _ = ops.silraster_fwd(ndc, mesh.faces_i32(), S, 8, blur, sigma)
    assert float((alpha - old).abs().max()) > 1e-3
    ga = torch.from_numpy(np.random.default_rng(6).standard_normal((2, S, S)).astype(np.float32)).to(dev)
    (rgba[..., 3] * ga).sum().backward()
    gv = ops.project_verts_bwd(verts.detach(), cams.R, cams.T,
                               ops.silraster_bwd(state, ndc, mesh.faces_i32(), blur, sigma, ga[:, None].contiguous()))
    assert torch.equal(verts.grad, gv) and float(gv.abs().sum()) > 0


# ---------------------------------------------------------------------------- 7. the fit and the CLI
@pytest.mark.parametrize("displacement", ["shift", "scale"])
def test_silhouette_fit_at_fifty_faces_per_pixel(dev, cow, displacement):
    """the fit of tests/_silhouette_ref.py:FIT through the public API with faces_per_pixel=50, under its bar 0.45"""
    import losses as L
    from st3d import optim
    from st3d.render import Meshes
    from test_gpu_silhouette import _hard_coverage
    F = SIL.FIT
    R, T = SIL.fit_cameras()
    target = _hard_coverage(dev, cow, F["S"], R, T)
    mesh0, verts, renderer, cams = _public(dev, cow, F["S"], R, T, SIL.DISPLACEMENTS[displacement](cow["verts"]))
    opt = optim.Adam([verts], lr=F["lr"])
    losses = []
    for _ in range(F["steps"]):
        opt.zero_grad()
        mesh = Meshes(verts=[verts], faces=[mesh0.faces_packed()])
        loss = L.compute_silhouette_loss(renderer, mesh, cams, target, sigma=F["sigma"], faces_per_pixel=50)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"{displacement} K=50: first {losses[0]:.6f} last {losses[-1]:.6f} ratio {losses[-1] / losses[0]:.4f}")
    assert all(np.isfinite(losses))
    assert losses[-1] / losses[0] <= F["bound"], (losses[0], losses[-1])


def test_second_approach_with_silhouette_faces_per_pixel(dev, cow, golden_dir, tmp_path):
    import second_approach as SA
    from test_gpu_silhouette import _log_losses, _write_cow_assets
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "4", "--batch_size", "4", "--epochs", "2",
              "--seed", "0", "--optimization_target", "both", "--save_every", "0", "--silhouette_weight", "10"]
    k50, k8 = str(tmp_path / "k50"), str(tmp_path / "k8")
    SA.main(common + ["--output_path", k50, "--silhouette_faces_per_pixel", "50"])
    SA.main(common + ["--output_path", k8])
    l50, l8 = _log_losses(k50), _log_losses(k8)
    assert len(l50) == 2 and len(l8) == 2 and all(np.isfinite(l50)) and all(np.isfinite(l8))
    assert l50 != l8         # (the first losses can agree: at 2e6 an fp32 loss resolves 0.25, the two terms differ by less)
    assert os.path.exists(os.path.join(k50, "final.obj"))
