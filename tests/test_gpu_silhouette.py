"""GPU tests of the silhouette feature (csrc/silhouette.hip and everything above it): the three kernels against fp64
autograd of the restatement in tests/_silhouette_ref.py evaluated on the GPU's own fp32 fragments, the vertex gradient
through the public API (far views and a view from inside the mesh, where clipped faces carry gradient), the gradient
SoftPhongShader's alpha now has, determinism, NaN propagation, batch sharding, the silhouette fit, and the CLI.

Bounds are the project's existing ones (tests/test_gpu_kernels.py::test_soft_shade_forward_and_backward_match_oracle):
alpha 2e-5 absolute; d/d dists  ||err|| <= 5e-5 ||ref|| + 4e-7 ||upstream|| / (4 sigma)  (the absolute floor is fp32
rounding of alpha, ~1e-7, times the largest slope 1 / (4 sigma)); a loss value 2e-5 relative; d/d verts 5e-5 relative L2
(1e-4 through clipped faces)."""
import os

import numpy as np
import pytest
import torch

import _silhouette_ref as SIL

pytestmark = pytest.mark.gpu

CASES = [(1, 0.0, 1e-4), (4, 3e-4, 1e-4), (8, 9.21e-4, 1e-4), (3, 1e-3, 1e-3)]      # (K, blur_radius, sigma)
NEAR_CAMERA = dict(dist=0.75, elev=[10.0], azim=[35.0], at=(0, 0.10, 0.25))            # inside the cow's bounding sphere


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


def _cams(n, seed=7):
    from oracle import render_ref as rr
    g = torch.Generator().manual_seed(seed)
    elev, azim = rr.random_camera_angles(n, lambda k: torch.rand(k, generator=g).numpy())
    return rr.look_at_view_transform(2.10, elev, azim, at=(0, 0.10, 0.25))


def _fragments(ops, dev, cow, S, K, blur, B=2, verts=None):
    R, T = _cams(B)
    v = torch.from_numpy(cow["verts"] if verts is None else verts).to(dev)
    faces = torch.from_numpy(cow["faces"]).to(dev)
    Rd, Td = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    ndc = ops.project_verts(v, Rd, Td)
    frag = ops.raster_soft_fwd(ndc, faces, S, K, blur, blur > 0)
    return frag, ndc, (R, T, Rd, Td), faces


def _target(S, B, seed=5):
    """a 0/1 mask that is neither the coverage nor its complement: a disc per view"""
    ys, xs = np.mgrid[0:S, 0:S]
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 1, S, S), np.float32)
    for b in range(B):
        c, r = rng.uniform(0.35, 0.65, 2) * S, rng.uniform(0.25, 0.4) * S
        out[b, 0] = ((ys - c[0]) ** 2 + (xs - c[1]) ** 2 <= r * r)
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("K,blur,sigma", CASES)
def test_silhouette_fwd_is_the_alpha_of_the_soft_shader_bitwise(dev, ops, cow, K, blur, sigma):
    S, B, Tn = 64, 2, 24
    frag, _, _, _ = _fragments(ops, dev, cow, S, K, blur, B)
    tex = torch.from_numpy(np.random.default_rng(1).random((Tn, Tn, 3), dtype=np.float32)).to(dev)
    uvs, fuv = torch.from_numpy(cow["verts_uvs"]).to(dev), torch.from_numpy(cow["faces_uvs"]).to(dev)
    _, alpha_blend = ops.shade_soft_fwd(frag, uvs, fuv, tex, sigma, 1e-4, (0.2, 0.5, 0.9))
    alpha = ops.silhouette_fwd(frag[0], frag[3], sigma)
    assert alpha.shape == (B, 1, S, S) and alpha.dtype == torch.float32
    assert torch.equal(alpha, alpha_blend)
    ref = SIL.sigmoid_alpha_blend(frag[3].cpu().double(), frag[0].cpu() >= 0, sigma)
    err = float((alpha[:, 0].cpu().double() - ref).abs().max())
    print(f"K={K} sigma={sigma}: alpha max abs err {err:.3e}")
    assert err <= 2e-5
    covered = (frag[0] >= 0).any(dim=-1)
    assert float(alpha[:, 0][~covered].abs().max()) == 0.0 and bool(covered.any()) and bool((~covered).any())
    if K == 1 and blur == 0.0:
        a = alpha[:, 0][covered]
        assert float(a.min()) >= 0.5 and float(a.max()) <= 1.0      # sigmoid(-d / sigma), d <= 0 inside the face


# ---------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("K,blur,sigma", CASES)
def test_silhouette_bwd_matches_fp64_autograd_and_accumulates_exactly(dev, ops, cow, K, blur, sigma):
    S, B = 72, 2
    frag, _, _, _ = _fragments(ops, dev, cow, S, K, blur, B)
    p2f, dists = frag[0], frag[3]
    rng = np.random.default_rng(2)
    ga = torch.from_numpy(rng.standard_normal((B, 1, S, S)).astype(np.float32))
    gd = ops.silhouette_bwd(ga.to(dev), p2f, dists, sigma)
    mask = p2f.cpu() >= 0
    assert float(gd.cpu()[~mask].abs().max()) == 0.0             # empty layers get 0
    for b in range(B):
        dl = dists[b].cpu().double().requires_grad_(True)
        (SIL.sigmoid_alpha_blend(dl, mask[b], sigma) * ga[b, 0].double()).sum().backward()
        err = float((gd[b].cpu().double() - dl.grad).norm())
        bound = 5e-5 * float(dl.grad.norm()) + 4e-7 * float(ga[b].norm()) / (4 * sigma)
        print(f"K={K} sigma={sigma} view {b}: |err| {err:.3e} |ref| {float(dl.grad.norm()):.3e} bound {bound:.3e}")
        assert float(dl.grad.norm()) > 0 and err <= bound, (err, float(dl.grad.norm()), bound)
    # accumulate mode: exactly prefilled + gradient on the covered layers, the prefilled value elsewhere
    pre = torch.from_numpy(rng.standard_normal((B, S, S, K)).astype(np.float32)).to(dev)
    out = pre.clone()
    assert ops.silhouette_bwd(ga.to(dev), p2f, dists, sigma, out=out) is out
    assert torch.equal(out, torch.where(p2f >= 0, pre + gd, pre))


# ---------------------------------------------------------------------------- 3. fused loss
@pytest.mark.parametrize("K,blur,sigma", CASES)
def test_silhouette_loss_is_the_three_launch_composition(dev, ops, cow, K, blur, sigma):
    S, B = 64, 2
    frag, _, _, _ = _fragments(ops, dev, cow, S, K, blur, B)
    p2f, dists = frag[0], frag[3]
    target = _target(S, B).to(dev)
    scale = 1.0 / (S * S * B)
    loss, gd = ops.silhouette_loss(p2f, dists, target, sigma, scale)
    alpha64 = SIL.sigmoid_alpha_blend(dists.cpu().double(), p2f.cpu() >= 0, sigma)
    ref = float(SIL.silhouette_loss(alpha64, target[:, 0].cpu().double()))
    rel = abs(float(loss) - ref) / ref
    print(f"K={K} sigma={sigma}: loss {float(loss):.8f} ref {ref:.8f} rel {rel:.3e}")
    assert ref > 0 and rel <= 2e-5
    two_scale = torch.tensor(scale, dtype=torch.float32, device=dev) * 2
    composed = ops.silhouette_bwd((ops.silhouette_fwd(p2f, dists, sigma) - target) * two_scale, p2f, dists, sigma)
    assert torch.equal(gd, composed)
    loss2, gd2 = ops.silhouette_loss(p2f, dists, target, sigma, scale)
    assert torch.equal(loss, loss2) and torch.equal(gd, gd2)
    loss3, none = ops.silhouette_loss(p2f, dists, target, sigma, scale, want_grad=False)
    assert none is None and torch.equal(loss, loss3)


# ---------------------------------------------------------------------------- 4. vertex gradient through the public API
def _api_scene(dev, cow, S, R, T, verts_np=None):
    import utils as U
    from st3d.render import FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    U.device = dev
    verts = torch.from_numpy(cow["verts"] if verts_np is None else verts_np).to(dev).requires_grad_(True)
    tex = torch.from_numpy(np.random.default_rng(3).random((24, 24, 3), dtype=np.float32))[None].to(dev)
    mesh = U.build_mesh(torch.from_numpy(cow["verts_uvs"])[None].to(dev), torch.from_numpy(cow["faces_uvs"].astype(np.int64))[None].to(dev),
                        tex, verts, torch.from_numpy(cow["faces"].astype(np.int64)).to(dev))
    renderer = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftPhongShader())
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(T), device=dev)
    return mesh, verts, renderer, cams


def _shifted(cow):
    return SIL.DISPLACEMENTS["shift"](cow["verts"])


def _loss_and_grad(dev, cow, S, R, T, target, sigma=1e-4, batch_denom=None, verts_np=None):
    import losses as L
    mesh, verts, renderer, cams = _api_scene(dev, cow, S, R, T, verts_np)
    loss = L.compute_silhouette_loss(renderer, mesh, cams, target, sigma=sigma, batch_denom=batch_denom)
    loss.backward()
    return loss.detach(), verts.grad.detach().clone()


def _hard_coverage(dev, cow, S, R, T):
    """0/1 coverage (B,1,S,S) of the undisplaced cow through the renderer, as the CLIs get their targets"""
    import utils as U
    mesh, _, renderer, cams = _api_scene(dev, cow, S, R, T)
    with torch.no_grad():
        _, cov = U.render_meshes(renderer, mesh, cams)
    assert set(torch.unique(cov).tolist()) == {0.0, 1.0}
    return cov


def _reference_loss_and_grad(ops, dev, cow, S, R, T, target, sigma, verts_np, near):
    """fp64 autograd of the restatement over oracle.soft_ref's geometry at the GPU's fragment assignment; the fp32 NDC the
    kernels consumed with the fp64 projection's graph attached.  -> (loss, d/d verts, number of clipped fragments)"""
    import losses as L
    from oracle import soft_ref as SR
    K, blur = L.SILHOUETTE_FACES_PER_PIXEL, L.silhouette_blur_radius(sigma)
    faces = torch.from_numpy(cow["faces"]).to(dev)
    ndc = ops.project_verts(torch.from_numpy(verts_np).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev))
    p2f, _, _, _, slots = ops.raster_soft_fwd(ndc, faces, S, K, blur, True, z_clip=0.5)
    fc = torch.from_numpy(cow["faces"]).long()
    vt = torch.from_numpy(verts_np).double().requires_grad_(True)
    B = R.shape[0]
    total, clipped = 0.0, 0
    for b in range(B):
        ndc_b = SR.project(vt, torch.from_numpy(R[b]).double(), torch.from_numpy(T[b]).double())
        ndc_b = ndc_b + (ndc[b].cpu().double() - ndc_b).detach()
        pf = p2f[b].cpu().long()
        behind = (ndc[b].cpu()[:, 2] < 0.5)[fc[pf.clamp_min(0)]].any(dim=-1) & (pf >= 0)
        clipped += int(behind.sum())
        if near:
            _, _, sd, mask = SR.clipped_geometry(ndc_b, fc, slots[b].cpu().long(), S, True, True, 0.5)
        else:
            assert not bool(behind.any())
            _, _, sd, mask = SR.soft_geometry(ndc_b, fc, pf, S, True)
        alpha = SIL.sigmoid_alpha_blend(sd, mask, sigma)
        total = total + ((alpha - target[b, 0].cpu().double()) ** 2).sum()
    loss = total / (S * S * B)
    loss.backward()
    return float(loss.detach()), vt.grad, clipped


def test_vertex_gradient_of_the_silhouette_loss_matches_fp64_autograd(dev, ops, cow):
    S, B = 64, 2
    R, T = _cams(B)
    target = _hard_coverage(dev, cow, S, R, T)
    v_np = _shifted(cow)
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, verts_np=v_np)
    ref_loss, ref_grad, _ = _reference_loss_and_grad(ops, dev, cow, S, R, T, target, 1e-4, v_np, near=False)
    rel_l = abs(float(loss) - ref_loss) / ref_loss
    rel_v = float((grad.cpu().double() - ref_grad).norm() / ref_grad.norm())
    print(f"far views: loss {float(loss):.8f} ref {ref_loss:.8f} rel {rel_l:.3e}; d/d verts rel L2 {rel_v:.3e}")
    assert ref_loss > 1e-3 and float(ref_grad.norm()) > 0
    assert rel_l <= 2e-5
    assert rel_v <= 5e-5


def test_vertex_gradient_flows_through_clipped_faces(dev, ops, cow):
    """The camera inside the cow's bounding sphere: fragments live on clipped sub-triangles whose cut points depend on the
    vertices; reference = oracle.soft_ref.clipped_geometry on the GPU's frag_slot."""
    from oracle import render_ref as rr
    S = 64
    R, T = rr.look_at_view_transform(NEAR_CAMERA["dist"], NEAR_CAMERA["elev"], NEAR_CAMERA["azim"], at=NEAR_CAMERA["at"])
    target = _target(S, 1, seed=9).to(dev)
    v_np = cow["verts"]
    loss, grad = _loss_and_grad(dev, cow, S, R, T, target, verts_np=v_np)
    ref_loss, ref_grad, clipped = _reference_loss_and_grad(ops, dev, cow, S, R, T, target, 1e-4, v_np, near=True)
    rel_l = abs(float(loss) - ref_loss) / ref_loss
    rel_v = float((grad.cpu().double() - ref_grad).norm() / ref_grad.norm())
    print(f"near view: {clipped} clipped fragments; loss rel {rel_l:.3e}; d/d verts rel L2 {rel_v:.3e}")
    assert clipped > 20
    assert rel_l <= 2e-5
    assert rel_v <= 1e-4


# ---------------------------------------------------------------------------- 5. SoftPhongShader's alpha
def _phong_scene(dev, cow, S, K, blur, sigma, gamma, bg, lights=None):
    import utils as U
    from st3d.render import (BlendParams, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings,
                             SoftPhongShader)
    U.device = dev
    B = 2
    R, T = _cams(B, seed=11)
    tex_np = np.random.default_rng(3).random((24, 24, 3), dtype=np.float32)
    verts = torch.from_numpy(cow["verts"]).to(dev).requires_grad_(True)
    tex = torch.from_numpy(tex_np)[None].to(dev).requires_grad_(True)
    mesh = U.build_mesh(torch.from_numpy(cow["verts_uvs"])[None].to(dev), torch.from_numpy(cow["faces_uvs"].astype(np.int64))[None].to(dev),
                        tex, verts, torch.from_numpy(cow["faces"].astype(np.int64)).to(dev))
    rs = RasterizationSettings(image_size=S, blur_radius=blur, faces_per_pixel=K)
    renderer = MeshRenderer(MeshRasterizer(None, rs), SoftPhongShader(device=dev, lights=lights,
                                                                      blend_params=BlendParams(sigma, gamma, bg)))
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(T), device=dev)
    return mesh, verts, tex, tex_np, renderer, cams, R, T


def _direct_chain(ops, dev, cow, mesh, verts, tex, cams, S, K, blur, sigma, gamma, bg, g, ga=None, lights=None):
    """the op chain of the render backward called directly: shade_soft(_lit)_bwd [-> silhouette_bwd accumulating into its
    grad_dists] -> raster_soft_bwd -> project_verts_bwd [-> the lighting's vertex terms]"""
    from st3d import render as RM
    v = verts.detach()
    ndc = ops.project_verts(v, cams.R, cams.T)
    frag = ops.raster_soft_fwd(ndc, mesh.faces_i32(), S, K, blur, True, z_clip=0.5)
    slots, frag = frag[4], frag[:4]
    uvs = torch.from_numpy(cow["verts_uvs"]).to(dev)
    fuv = mesh.textures.faces_uvs_i32()
    t = tex.detach()[0].contiguous()
    lit = RM._lit_setup(RM.lighting_of(lights, None, dev), verts, v, mesh.faces_i32(), cams.R, cams.T)
    gnp = None
    if lit is None:
        gt, geo = ops.shade_soft_bwd(g, frag, uvs, fuv, t, sigma, gamma, bg)
    else:
        gt, geo, gnp = ops.shade_soft_lit_bwd(g, frag, uvs, fuv, t, lit, sigma, gamma, bg)
    if ga is not None:
        ops.silhouette_bwd(ga, frag[0], frag[3], sigma, out=geo[2])
    gv = ops.project_verts_bwd(v, cams.R, cams.T, ops.raster_soft_bwd(geo, frag[0], ndc, mesh.faces_i32(), True, True, slots, 0.5))
    if lit is not None:
        gv = RM._lit_vertex_grad(lit, gv, gnp, frag[0], frag[2])
    return gv, gt, frag, ndc, geo, slots


def test_soft_phong_alpha_is_differentiable(dev, ops, cow):
    """K = 4 soft settings, loss (rgb g).sum() + (alpha ga).sum().  As test_soft_shade_forward_and_backward_match_oracle
    does, fp64 autograd is evaluated stage by stage on the GPU's fp32 fragments: softmax_rgb_blend (which returns both
    outputs) gives the reference for the combined d/d (bary, depth, dists) under that test's bounds -- the dists floor now
    carries both upstream norms --, and soft_geometry / project with the GPU's own upstream gives the reference for d/d verts
    at 5e-5.  Without ga the gradients are bitwise those of today's op chain; the same with a point light."""
    from oracle import soft_ref as SR
    from st3d.render import PointLights
    S, K, blur, sigma, gamma, bg = 64, 4, 3e-4, 1e-4, 1e-4, (0.2, 0.5, 0.9)
    rng = np.random.default_rng(4)
    g_np = rng.standard_normal((2, 3, S, S)).astype(np.float32)
    ga_np = rng.standard_normal((2, 1, S, S)).astype(np.float32)
    g, ga = torch.from_numpy(g_np).to(dev), torch.from_numpy(ga_np).to(dev)
    for lights in (None, PointLights(location=((0.5, 1.5, 2.0),), device=dev)):
        # without ga: exactly today's launches and bits
        mesh, verts, tex, tex_np, renderer, cams, R, T = _phong_scene(dev, cow, S, K, blur, sigma, gamma, bg, lights)
        rgb, alpha = renderer.render(mesh, cams)
        assert alpha.requires_grad
        (rgb * g).sum().backward()
        gv0, gt0, frag, ndc, _, slots = _direct_chain(ops, dev, cow, mesh, verts, tex, cams, S, K, blur, sigma, gamma, bg, g, None, lights)
        assert torch.equal(verts.grad, gv0) and torch.equal(tex.grad[0], gt0)
        # with ga: the alpha gradient joins grad_dists before the one raster backward
        mesh, verts, tex, tex_np, renderer, cams, R, T = _phong_scene(dev, cow, S, K, blur, sigma, gamma, bg, lights)
        rgb, alpha = renderer.render(mesh, cams)
        ((rgb * g).sum() + (alpha * ga).sum()).backward()
        gv1, gt1, frag, ndc, geo, slots = _direct_chain(ops, dev, cow, mesh, verts, tex, cams, S, K, blur, sigma, gamma, bg, g, ga, lights)
        assert torch.equal(verts.grad, gv1) and torch.equal(tex.grad[0], gt1) and torch.equal(gt1, gt0)
        assert not torch.equal(gv1, gv0)
        grad_both = verts.grad.clone()
        # only alpha: the RGB backward is skipped, the texture gets no gradient
        mesh, verts, tex, tex_np, renderer, cams, R, T = _phong_scene(dev, cow, S, K, blur, sigma, gamma, bg, lights)
        rgb, alpha = renderer.render(mesh, cams)
        (alpha * ga).sum().backward()
        assert tex.grad is None
        gd = ops.silhouette_bwd(ga, frag[0], frag[3], sigma)
        only = ops.project_verts_bwd(verts.detach(), cams.R, cams.T,
                                     ops.raster_soft_bwd((None, None, gd), frag[0], ndc, mesh.faces_i32(), True, True, slots, 0.5))
        assert torch.equal(verts.grad, only)
        if lights is not None:
            continue
        # fp64, unlit
        fc = torch.from_numpy(cow["faces"]).long()
        uv64, fuv64 = torch.from_numpy(cow["verts_uvs"]).double(), torch.from_numpy(cow["faces_uvs"]).long()
        tt = torch.from_numpy(tex_np).double()
        vt = torch.from_numpy(cow["verts"]).double().requires_grad_(True)
        gtol = max(5e-5, 2e-7 / gamma)
        for b in range(2):
            p2f = frag[0][b].cpu().long()
            mask = p2f >= 0
            bl, zl, dl = (frag[i][b].cpu().double().requires_grad_(True) for i in (2, 1, 3))
            r, a_ = SR.softmax_rgb_blend(SR.sample_texture(bl, p2f, uv64, fuv64, tt), zl, dl, mask, sigma, gamma, bg)
            ((r.permute(2, 0, 1) * torch.from_numpy(g_np[b]).double()).sum() + (a_ * torch.from_numpy(ga_np[b, 0]).double()).sum()).backward()
            gnorm, ganorm = float(np.linalg.norm(g_np[b])), float(np.linalg.norm(ga_np[b]))
            for name, ref_g, got_g, floor in (("bary", bl.grad, geo[0][b], 0.0), ("zbuf", zl.grad, geo[1][b], 4e-7 * gnorm / (99 * gamma)),
                                              ("dists", dl.grad, geo[2][b], 4e-7 * (gnorm + ganorm) / (4 * sigma))):
                m = mask.double() if ref_g.dim() == 3 else mask.double().unsqueeze(-1)
                err = float(((got_g.cpu().double() - ref_g) * m).norm())
                print(f"view {b} d/d {name}: |err| {err:.3e} |ref| {float((ref_g * m).norm()):.3e} floor {floor:.3e}")
                assert err <= gtol * float((ref_g * m).norm()) + floor, (name, err, float((ref_g * m).norm()), floor)
            ndc_b = SR.project(vt, torch.from_numpy(R[b]).double(), torch.from_numpy(T[b]).double())
            ndc_b = ndc_b + (ndc[b].cpu().double() - ndc_b).detach()
            bary64, pz64, sd64, m64 = SR.soft_geometry(ndc_b, fc, p2f, S, True)
            md = m64.double()
            ((bary64 * geo[0][b].cpu().double() * md.unsqueeze(-1)).sum() + (pz64 * geo[1][b].cpu().double() * md).sum()
             + (sd64 * geo[2][b].cpu().double() * md).sum()).backward()
        rel_v = float((grad_both.cpu().double() - vt.grad).norm() / vt.grad.norm())
        print(f"SoftPhongShader rgb + alpha: d/d verts rel L2 {rel_v:.3e}")
        assert rel_v <= 5e-5, rel_v


def test_hard_settings_keep_the_detached_mask(dev, cow):
    """the hard path and the near-plane reroute of hard settings hand out the 0/1 mask without a gradient, as before"""
    from oracle import render_ref as rr
    S = 64
    R, T = _cams(1)
    mesh, verts, renderer, cams = _api_scene(dev, cow, S, R, T)
    _, cov = renderer.render(mesh, cams)
    assert not cov.requires_grad and set(torch.unique(cov).tolist()) == {0.0, 1.0}
    Rn, Tn = rr.look_at_view_transform(NEAR_CAMERA["dist"], NEAR_CAMERA["elev"], NEAR_CAMERA["azim"], at=NEAR_CAMERA["at"])
    mesh, verts, renderer, cams = _api_scene(dev, cow, S, Rn, Tn)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, cov = renderer.render(mesh, cams)
    assert not cov.requires_grad and set(torch.unique(cov).tolist()) <= {0.0, 1.0}


def test_soft_silhouette_shader_through_the_renderer(dev, ops, cow):
    """(n,S,S,4) with RGB = 1 and alpha in channel 3; a mesh WITHOUT textures; the gradient is the op chain's, bitwise"""
    from st3d.render import (BlendParams, FoVPerspectiveCameras, Meshes, MeshRasterizer, MeshRenderer, RasterizationSettings,
                             SoftSilhouetteShader)
    S, K, sigma = 64, 8, 1e-4
    blur = SIL.blur_radius(sigma)
    R, T = _cams(2)
    verts = torch.from_numpy(cow["verts"]).to(dev).requires_grad_(True)
    mesh = Meshes(verts=[verts], faces=[torch.from_numpy(cow["faces"].astype(np.int64)).to(dev)])
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(T), device=dev)
    renderer = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S, blur_radius=blur, faces_per_pixel=K)),
                            SoftSilhouetteShader(blend_params=BlendParams(sigma=sigma)))
    rgba = renderer(meshes_world=mesh, cameras=cams)
    assert rgba.shape == (2, S, S, 4) and bool((rgba[..., :3] == 1).all())
    ndc = ops.project_verts(verts.detach(), cams.R, cams.T)
    p2f, _, _, dists, slots = ops.raster_soft_fwd(ndc, mesh.faces_i32(), S, K, blur, True, z_clip=0.5)
    assert torch.equal(rgba[..., 3].detach(), ops.silhouette_fwd(p2f, dists, sigma)[:, 0])
    ga = torch.from_numpy(np.random.default_rng(6).standard_normal((2, S, S)).astype(np.float32)).to(dev)
    (rgba[..., 3] * ga).sum().backward()
    gd = ops.silhouette_bwd(ga[:, None].contiguous(), p2f, dists, sigma)
    gv = ops.project_verts_bwd(verts.detach(), cams.R, cams.T,
                               ops.raster_soft_bwd((None, None, gd), p2f, ndc, mesh.faces_i32(), True, True, slots, 0.5))
    assert torch.equal(verts.grad, gv) and float(gv.abs().sum()) > 0
    # hard raster settings still render on the general rasteriser: alpha = sigmoid(-d / sigma) in [0.5, 1) where covered
    hard = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftSilhouetteShader())
    with torch.no_grad():
        _, a = hard.render(mesh, cams)
    assert float(a[a > 0].min()) >= 0.5 and float(a.max()) <= 1.0 and bool((a == 0).any())


# ---------------------------------------------------------------------------- 6. determinism
def test_silhouette_loss_and_gradient_are_bitwise_reproducible(dev, cow):
    from st3d import ops as O
    assert O.is_deterministic()
    S, B = 64, 2
    R, T = _cams(B)
    target = _hard_coverage(dev, cow, S, R, T)
    a = _loss_and_grad(dev, cow, S, R, T, target, verts_np=_shifted(cow))
    b = _loss_and_grad(dev, cow, S, R, T, target, verts_np=_shifted(cow))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------- 7. NaN
def test_nan_distance_poisons_its_pixel_only(dev, ops, cow):
    S, B, K, sigma = 64, 2, 8, 1e-4
    frag, _, _, _ = _fragments(ops, dev, cow, S, K, SIL.blur_radius(sigma), B)
    p2f, dists = frag[0], frag[3]
    target = _target(S, B).to(dev)
    scale = 1.0 / (S * S * B)
    loss, gd = ops.silhouette_loss(p2f, dists, target, sigma, scale)
    full = torch.nonzero((p2f >= 0).all(dim=-1))           # a pixel with all K layers covered
    assert len(full) > 0
    b, y, x = full[len(full) // 2].tolist()
    bad = dists.clone()
    bad[b, y, x, 3] = float("nan")
    loss_n, gd_n = ops.silhouette_loss(p2f, bad, target, sigma, scale)
    assert bool(torch.isnan(loss_n).all()) and bool(torch.isfinite(loss).all())
    assert bool(torch.isnan(gd_n[b, y, x]).all())           # every layer's gradient carries the full product
    assert bool(torch.isnan(ops.silhouette_fwd(p2f, bad, sigma)[b, 0, y, x]))
    other = torch.ones_like(p2f, dtype=torch.bool)
    other[b, y, x] = False
    assert torch.equal(gd_n[other], gd[other]) and bool(torch.isfinite(gd_n[other]).all())


# ---------------------------------------------------------------------------- 8. batch sharding
def test_two_halves_of_a_batch_sum_to_the_full_batch(dev, cow):
    S, B = 64, 4
    R, T = _cams(B, seed=3)
    target = _hard_coverage(dev, cow, S, R, T)
    v_np = _shifted(cow)
    full_l, full_g = _loss_and_grad(dev, cow, S, R, T, target, verts_np=v_np)
    parts = [_loss_and_grad(dev, cow, S, R[s], T[s], target[s].contiguous(), batch_denom=4, verts_np=v_np)
             for s in (slice(0, 2), slice(2, 4))]
    sum_l, sum_g = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert abs(float(sum_l) - float(full_l)) <= 1e-6 * float(full_l)
    assert float((sum_g - full_g).norm()) <= 1e-6 * float(full_g.norm())
    assert float(parts[0][0]) > 0 and float(parts[1][0]) > 0


# ---------------------------------------------------------------------------- 9. the fit
@pytest.mark.parametrize("displacement", ["shift", "scale"])
def test_silhouette_fit_recovers_the_outline(dev, cow, displacement):
    """The fit of tests/test_silhouette_host.py through the public API: MeshRenderer, compute_silhouette_loss,
    st3d.optim.Adam; the fp64 reference reaches 0.338 (shift) and 0.321 (scale) of the first loss."""
    import losses as L
    import utils as U
    from st3d import optim
    from st3d.render import FoVPerspectiveCameras
    F = SIL.FIT
    R, T = SIL.fit_cameras()
    target = _hard_coverage(dev, cow, F["S"], R, T)
    mesh0, verts, renderer, cams = _api_scene(dev, cow, F["S"], R, T, SIL.DISPLACEMENTS[displacement](cow["verts"]))
    tx = mesh0.textures
    opt = optim.Adam([verts], lr=F["lr"])
    losses = []
    for _ in range(F["steps"]):
        opt.zero_grad()
        mesh = U.build_mesh(tx.verts_uvs_padded(), tx.faces_uvs_padded(), tx.maps_padded(), verts, mesh0.faces_packed())
        loss = L.compute_silhouette_loss(renderer, mesh, cams, target, sigma=F["sigma"])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"{displacement}: first {losses[0]:.6f} last {losses[-1]:.6f} ratio {losses[-1] / losses[0]:.4f}")
    assert all(np.isfinite(losses))
    assert losses[-1] / losses[0] <= F["bound"], (losses[0], losses[-1])


# ---------------------------------------------------------------------------- 10. the CLI
def _write_cow_assets(tmp, cow, golden_dir, tex_size=64):
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


def _log_losses(path):
    lines = open(os.path.join(path, "log.txt")).read().splitlines()
    return [float(line.split("Loss ")[1]) for line in lines[1:]]


def test_second_approach_with_silhouette_weight(dev, cow, golden_dir, tmp_path):
    import second_approach as SA
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "4", "--batch_size", "4", "--epochs", "2",
              "--seed", "0", "--optimization_target", "both", "--save_every", "0"]
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    SA.main(common + ["--output_path", on, "--silhouette_weight", "10"])
    SA.main(common + ["--output_path", off])
    l_on, l_off = _log_losses(on), _log_losses(off)
    assert len(l_on) == 2 and len(l_off) == 2 and all(np.isfinite(l_on)) and all(np.isfinite(l_off))
    assert l_on != l_off and all(a != b for a, b in zip(l_on, l_off))
    assert os.path.exists(os.path.join(on, "final.obj"))


def test_first_approach_with_silhouette_weight(dev, cow, golden_dir, tmp_path):
    """phase B gains the term: the masked MSE is masked by the current render's own coverage and cannot see the outline"""
    import first_approach as FA
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0",
              "--n_style_transfer_steps", "2", "--n_mse_steps", "3", "--optimization_target", "mesh"]
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    FA.main(common + ["--output_path", on, "--silhouette_weight", "10"])
    FA.main(common + ["--output_path", off])
    l_on, l_off = _log_losses(on), _log_losses(off)
    assert len(l_on) == 3 and all(np.isfinite(l_on)) and all(np.isfinite(l_off))
    assert l_on[0] > l_off[0]              # the first step differs by exactly the (positive) silhouette term
    assert os.path.exists(os.path.join(on, "final.obj"))
