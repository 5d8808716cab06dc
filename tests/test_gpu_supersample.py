"""Supersampled rendering on the GPU (csrc/shade.hip: shade_ss_fwd_kernel, shade_bwd_kernel<.., A>, box_down_*): the fused
kernels against the oracle restatement (tests/_ssref.py) and, bit for bit, against the composition they replace (the plain
kernels at a * S and the box filter); the renderer's keyword; the general path; the tags a loss relies on.

Shapes: cow, B = 2, S in {16, 17, 20, 24} (a * S a multiple of the 16-pixel tile or not, S % 4 == 0 -- the box filter's
16-byte path -- or not), a in {2, 3, 4}, T in {32, 37}.  Tolerances are the ones test_gpu_kernels.py holds the same outputs
to at a = 1; averaging does not widen them."""
import numpy as np
import pytest
import torch

import _ssref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


def _scale_close(got, ref, rtol, name=""):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = (torch.tensor(ref) if isinstance(ref, np.ndarray) else ref).detach().double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    print(f"{name}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e} (bound {rtol:.1e})")
    assert err <= rtol * scale, f"{name}: max err {err:.3e} > {rtol:.1e} * scale {scale:.3e}"


def _rel_l2(got, ref, name=""):
    got, ref = np.asarray(torch.as_tensor(got).detach().cpu(), np.float64), np.asarray(ref, np.float64)
    rel = np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30)
    print(f"{name}: relative L2 {rel:.3e}")
    return rel


def _device_scene(c, dev, ops, S, a, lit=False):
    """the case's mesh as the kernels take it, its fragments at side a * S and (lit) a point light's LitSetup"""
    from st3d import render as R
    m = c["mesh"]
    verts = torch.from_numpy(m["verts"]).to(dev)
    faces = torch.from_numpy(m["faces"]).to(dev).to(torch.int32).contiguous()
    uvs = torch.from_numpy(m["verts_uvs"]).to(dev)
    fuv = torch.from_numpy(m["faces_uvs"]).to(dev).to(torch.int32).contiguous()
    tex = torch.tensor(c["tex"]).to(dev)
    Rd, Td = torch.tensor(c["R"]).to(dev), torch.tensor(c["T"]).to(dev)
    ndc = ops.project_verts(verts, Rd, Td)
    frag = ops.raster_fwd(ndc, faces, a * S)
    setup = None
    if lit:
        lighting = R.lighting_of(R.PointLights(location=((0.5, 1.0, 2.0),), device=dev), None, dev)
        setup = R._lit_setup(lighting, verts, verts, faces, Rd, Td)
    return dict(verts=verts, faces=faces, uvs=uvs, fuv=fuv, tex=tex, R=Rd, T=Td, ndc=ndc, frag=frag, lit=setup)


def _ordered_box_torch(x, a):
    s = x[..., 0::a, 0::a].clone()
    for j in range(a):
        for i in range(a):
            if j or i:
                s = s + x[..., j::a, i::a]
    return s / float(a * a)


def _within_one_ulp(got, ref):
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    return bool((np.abs(got - ref) <= np.spacing(np.abs(ref))).all())


# ------------------------------------------------------------------ 1. fused forward against the oracle
@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_fused_forward_matches_the_oracle(dev, ops, S, T, a):
    """rgb within 2e-6 abs (test_shade_fwd_bwd_match_oracle's bound); coverage and what the need tag is made of exactly"""
    c = _ssref.case(S, T, a)
    d = _device_scene(c, dev, ops, S, a)
    for b in range(_ssref.B):       # the fragments themselves are the oracle's, bit for bit
        np.testing.assert_array_equal(d["frag"][0][b].cpu().numpy(), c["frags"][b][0])
    rgb, cov = ops.shade_ss_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"], a)
    assert rgb.shape == (_ssref.B, 3, S, S) and cov.shape == (_ssref.B, 1, S, S)
    err = np.abs(rgb.cpu().numpy() - c["rgb"]).max()
    print(f"rgb max abs err {err:.3e} (bound 2e-6)")
    assert err <= 2e-6
    np.testing.assert_array_equal(cov.cpu().numpy(), c["cov"])
    np.testing.assert_array_equal((cov > 0).cpu().numpy(), c["cov"] > 0)
    assert (rgb.permute(0, 2, 3, 1)[cov[:, 0] == 0] == 1.0).all()        # no fragment: exactly white


# ------------------------------------------------------------------ 2. fused forward against the composition, the box kernel
@pytest.mark.parametrize("lit", [False, True], ids=["unlit", "point"])
@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_fused_forward_is_bitwise_the_plain_kernel_and_the_box_filter(dev, ops, S, T, a, lit):
    c = _ssref.case(S, T, a)
    d = _device_scene(c, dev, ops, S, a, lit)
    if lit:
        rgb, cov = ops.shade_ss_lit_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"], d["lit"], a)
        hi, mask = ops.shade_lit_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"], d["lit"])
    else:
        rgb, cov = ops.shade_ss_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"], a)
        hi, mask = ops.shade_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"])
    assert torch.equal(rgb, ops.box_down_fwd(hi, a)) and torch.equal(cov, ops.box_down_fwd(mask, a))
    if lit:
        assert not torch.equal(rgb, ops.shade_ss_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"], a)[0])     # the light is on
    # the box kernel itself against ordered torch additions (torch divides by 9 its own way: one ulp there)
    for x in (hi, torch.randn(3, 2, a * S, a * S, device=dev), torch.randn(1, 1, a * S, a * S, device=dev)):
        got, ref = ops.box_down_fwd(x, a), _ordered_box_torch(x, a)
        assert torch.equal(got, ref) if a in (2, 4) else _within_one_ulp(got, ref)
    # a view whose storage is not 16-byte aligned takes the scalar kernels: same bits
    flat = torch.randn(2 * (a * S) ** 2 + 1, device=dev)
    x = flat[1:].view(1, 2, a * S, a * S)
    assert torch.equal(ops.box_down_fwd(x, a), ops.box_down_fwd(x.clone(), a))
    g = torch.randn(_ssref.B, 3, S, S, device=dev)
    up = ops.box_down_bwd(g, a)
    assert up.shape == (_ssref.B, 3, a * S, a * S)
    assert torch.equal(up, torch.from_numpy(_ssref.box_down_t(g.cpu().numpy(), a)).to(dev))


# ------------------------------------------------------------------ 3. fused backward, float atomics
@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_fused_backward_float_atomics(dev, ops, monkeypatch, S, T, a):
    """against the composition (box transpose, then the plain backward at a * S): per-pixel outputs bitwise, the texture
    scatter within 1e-5 of its max (atomics, any order); against the oracle at test_gpu_kernels.py's bounds"""
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    c = _ssref.case(S, T, a)
    d = _device_scene(c, dev, ops, S, a)
    g = torch.tensor(c["g"]).to(dev)
    gt, guv, gbary = ops.shade_ss_bwd(g, d["frag"], d["uvs"], d["fuv"], d["tex"], a, want_uv=True, want_bary=True)
    g_hi = ops.box_down_bwd(g, a)
    gt2, guv2, gbary2 = ops.shade_bwd(g_hi, d["frag"], d["uvs"], d["fuv"], d["tex"], want_uv=True, want_bary=True)
    assert torch.equal(guv, guv2) and torch.equal(gbary, gbary2)
    _scale_close(gt, gt2, 1e-5, "grad_texture vs composition")
    _scale_close(gt, c["gtex"], 1e-5, "grad_texture vs oracle")
    _scale_close(gbary, c["gbary"], 1e-4, "grad_bary vs oracle")
    gndc = ops.raster_bwd(gbary, d["frag"][0], d["ndc"], d["faces"])
    gverts = ops.project_verts_bwd(d["verts"], d["R"], d["T"], gndc)
    assert _rel_l2(gverts, c["gverts"], "grad_verts vs oracle") <= 2e-4
    # vertices only
    only = ops.shade_ss_bwd(g, d["frag"], d["uvs"], d["fuv"], d["tex"], a, want_bary=True, want_texture=False)
    assert only[0] is None and torch.equal(only[1], gbary)


@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_fused_lit_backward_float_atomics(dev, ops, monkeypatch, S, T, a):
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    c = _ssref.case(S, T, a)
    d = _device_scene(c, dev, ops, S, a, lit=True)
    g = torch.tensor(c["g"]).to(dev)
    gt, gbary, gnp = ops.shade_ss_lit_bwd(g, d["frag"], d["uvs"], d["fuv"], d["tex"], d["lit"], a, want_geometry=True)
    gt2, gbary2, gnp2 = ops.shade_lit_bwd(ops.box_down_bwd(g, a), d["frag"], d["uvs"], d["fuv"], d["tex"], d["lit"],
                                          want_geometry=True)
    hit = d["frag"][0] >= 0          # grad_np is written where there is a face (st3d_phong_scatter reads it only there)
    assert torch.equal(gbary, gbary2) and torch.equal(gnp[hit], gnp2[hit]) and float(gnp[hit].abs().sum()) > 0
    _scale_close(gt, gt2, 1e-5, "lit grad_texture vs composition")


# ------------------------------------------------------------------ 4. fixed point
@pytest.mark.parametrize("lit", [False, True], ids=["unlit", "point"])
@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_fixed_point_backward_is_reproducible_and_loud(dev, ops, monkeypatch, S, T, a, lit):
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    c = _ssref.case(S, T, a)
    d = _device_scene(c, dev, ops, S, a, lit)
    g = torch.tensor(c["g"]).to(dev)

    def run(grad):
        if lit:
            return ops.shade_ss_lit_bwd(grad, d["frag"], d["uvs"], d["fuv"], d["tex"], d["lit"], a, want_geometry=True)[:2]
        return ops.shade_ss_bwd(grad, d["frag"], d["uvs"], d["fuv"], d["tex"], a, want_bary=True)
    gt, gbary = run(g)
    gt_again, gbary_again = run(g)
    assert torch.equal(gt, gt_again) and torch.equal(gbary, gbary_again)
    if not lit:
        _scale_close(gt, c["gtex"], 1e-5, "fixed-point grad_texture vs oracle")
        _scale_close(gbary, c["gbary"], 1e-4, "grad_bary vs oracle")
        gverts = ops.project_verts_bwd(d["verts"], d["R"], d["T"], ops.raster_bwd(gbary, d["frag"][0], d["ndc"], d["faces"]))
        assert _rel_l2(gverts, c["gverts"], "grad_verts vs oracle") <= 2e-4
    else:
        monkeypatch.setattr(ops, "_DETERMINISTIC", False)
        _scale_close(gt, run(g)[0], 1e-5, "lit fixed point vs float atomics")
        monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    # what a loss writes on pixels no sub-pixel covers changes no bit (they deposit nothing and leave the bound alone) ...
    off = (torch.tensor(c["cov"]).to(dev) == 0).expand(-1, 3, -1, -1)
    noisy = torch.where(off, 1e3 * torch.randn(g.shape, generator=torch.Generator().manual_seed(S)).to(dev), g)
    gt_noisy, gbary_noisy = run(noisy)
    assert torch.equal(gt_noisy, gt) and torch.equal(gbary_noisy, gbary)
    # ... but a NaN comes out as NaN wherever it sits: on the mesh and off it
    for y, x in ((int(i) for i in (~off[1, 0]).nonzero()[0]), (int(i) for i in off[1, 0].nonzero()[0])):
        bad = g.clone()
        bad[1, 2, y, x] = float("nan")
        assert torch.isnan(run(bad)[0]).all()


# ------------------------------------------------------------------ 5. the public API
def _renderer(S, **kw):
    from st3d.render import MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    return MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S, **kw)), SoftPhongShader())


def _mesh(c, dev, texture=None):
    import utils as U
    U.device = dev
    m = c["mesh"]
    tex = torch.tensor(c["tex"])[None].to(dev).requires_grad_(True) if texture is None else texture
    verts = torch.from_numpy(m["verts"]).to(dev).requires_grad_(True)
    mesh = U.build_mesh(torch.from_numpy(m["verts_uvs"])[None].to(dev), torch.from_numpy(m["faces_uvs"].astype(np.int64))[None].to(dev),
                        tex, verts, torch.from_numpy(m["faces"].astype(np.int64)).to(dev))
    return mesh, verts, tex


def _cams(c, dev):
    from st3d.render import FoVPerspectiveCameras
    return FoVPerspectiveCameras(R=torch.tensor(c["R"]), T=torch.tensor(c["T"]), device=dev)


def _step(renderer, c, dev):
    """render, a seeded weighted-sum loss, backward -> rgb, coverage, need tag, d/dtexture, d/dverts"""
    from st3d.render import need_of
    mesh, verts, tex = _mesh(c, dev)
    rgb, cov = renderer.render(mesh, _cams(c, dev))
    need = need_of(rgb)
    (rgb * torch.tensor(c["g"]).to(dev)).sum().backward()
    return rgb.detach(), cov.detach(), need, tex.grad[0], verts.grad


@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_renderer_keyword_matches_the_oracle(dev, ops, monkeypatch, S, T, a):
    monkeypatch.delenv("ST3D_SS_FUSED", raising=False)
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)         # (the default: the vertex scatter is then bitwise reproducible)
    c = _ssref.case(S, T, a)
    rgb, cov, need, gtex, gverts = _step(_renderer(S, supersample=a), c, dev)
    assert np.abs(rgb.cpu().numpy() - c["rgb"]).max() <= 2e-6
    np.testing.assert_array_equal(cov.cpu().numpy(), c["cov"])
    assert need is not None and need.dtype == torch.uint8 and need.shape == (_ssref.B, S, S)
    np.testing.assert_array_equal(need.cpu().numpy(), (c["cov"][:, 0] > 0).astype(np.uint8))
    _scale_close(gtex, c["gtex"], 1e-5, "renderer grad_texture vs oracle")
    assert _rel_l2(gverts, c["gverts"], "renderer grad_verts vs oracle") <= 2e-4
    # the A/B switch: the composition on the same rasteriser -- same bits wherever nothing is summed in another order
    monkeypatch.setenv("ST3D_SS_FUSED", "0")
    rgb0, cov0, need0, gtex0, gverts0 = _step(_renderer(S, supersample=a), c, dev)
    assert torch.equal(rgb, rgb0) and torch.equal(cov, cov0) and torch.equal(need, need0) and torch.equal(gverts, gverts0)
    _scale_close(gtex0, gtex, 1e-5, "composition grad_texture vs fused")


@pytest.mark.parametrize("S", [17, 24])
def test_supersample_one_is_the_renderer_without_the_keyword(dev, ops, monkeypatch, S):
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    c = _ssref.case(S, 32 if S == 24 else 37, 2)
    got, ref = _step(_renderer(S, supersample=1), c, dev), _step(_renderer(S), c, dev)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    assert set(np.unique(got[1].cpu().numpy()).tolist()) <= {0.0, 1.0}


def test_lit_renderer_and_texture_pyramid(dev, ops):
    """a point light through the keyword: bitwise the composition's pixels; with a TexturePyramid the gradient reaches every level"""
    from st3d.render import PointLights
    from st3d.texpyr import TexturePyramid
    S, T, a = 24, 32, 3
    c = _ssref.case(S, T, a)
    r = _renderer(S, supersample=a)
    lights = PointLights(location=((0.5, 1.0, 2.0),), device=dev)
    pyr = TexturePyramid(torch.tensor(c["tex"])[None].to(dev), 3)
    mesh, verts, _ = _mesh(c, dev, pyr.texture())
    rgb, cov = r.render(mesh, _cams(c, dev), lights=lights)
    np.testing.assert_array_equal(cov.detach().cpu().numpy(), c["cov"])
    d = _device_scene(c, dev, ops, S, a, lit=True)
    hi, _ = ops.shade_lit_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"], d["lit"])
    assert torch.equal(rgb.detach(), ops.box_down_fwd(hi, a))
    (rgb * torch.tensor(c["g"]).to(dev)).sum().backward()
    assert torch.isfinite(verts.grad).all() and float(verts.grad.abs().sum()) > 0
    for l in range(pyr.levels):
        gl = pyr.params.grad[pyr.offsets[l]:pyr.offsets[l + 1]]
        assert torch.isfinite(gl).all() and float(gl.abs().sum()) > 0, l


# ------------------------------------------------------------------ 6. the general path
@pytest.mark.parametrize("S,a", [(17, 2), (20, 3), (16, 4)])
def test_general_path_is_the_hand_composition(dev, ops, S, a):
    """K = 4 with blur: _SoftRenderFn at a * S, then the box filter over rgb and alpha, bit for bit; coverage in [0, 1];
    a gradient for alpha reaches the vertices through the filter's transpose"""
    from st3d import render as R
    T = 37
    c = _ssref.case(20, T, 3)        # (only its mesh, cameras and texture are used)
    K, blur = 4, 2e-4
    r = _renderer(S, supersample=a, faces_per_pixel=K, blur_radius=blur)
    assert not r.is_hard
    mesh, verts, tex = _mesh(c, dev)
    cams = _cams(c, dev)
    rgb, alpha = r.render(mesh, cams)
    rs, bp = r.rasterizer.raster_settings, R.BlendParams()
    with torch.no_grad():
        hi, ahi = R._SoftRenderFn.apply(mesh.verts_packed(), mesh.textures.maps_padded(), mesh.faces_i32(),
                                        mesh.textures.verts_uvs_padded(), mesh.textures.faces_uvs_i32(), cams.R, cams.T, a * S, K,
                                        blur, rs.clip_barycentric_coords, bp.sigma, bp.gamma, bp.background_color,
                                        rs.cull_backfaces, rs.perspective_correct, rs.z_clip, None)
    assert torch.equal(rgb.detach(), ops.box_down_fwd(hi, a)) and torch.equal(alpha.detach(), ops.box_down_fwd(ahi, a))
    assert float(alpha.detach().min()) >= 0.0 and 0.5 < float(alpha.detach().max()) <= 1.0
    need = R.need_of(rgb)
    assert need is not None and need.shape == (2, S, S) and bool((need.bool() | (alpha.detach()[:, 0] == 0)).all())
    w = torch.randn(alpha.shape, generator=torch.Generator().manual_seed(S)).to(dev)
    (alpha * w).sum().backward()
    assert tex.grad is None and torch.isfinite(verts.grad).all() and float(verts.grad.abs().sum()) > 0
    ga = verts.grad.clone()
    # rgb and alpha together: the texture gets its gradient, the vertices both
    mesh, verts, tex = _mesh(c, dev)
    rgb, alpha = r.render(mesh, cams)
    ((rgb * torch.randn(rgb.shape, generator=torch.Generator().manual_seed(1)).to(dev)).sum() + (alpha * w).sum()).backward()
    assert torch.isfinite(tex.grad).all() and float(tex.grad.abs().sum()) > 0 and not torch.equal(verts.grad, ga)


def test_near_plane_reroute_hands_out_fractional_coverage(dev, ops):
    """hard settings, camera inside the near plane: the clipping kernels at a * S, alpha thresholded there, then filtered"""
    import warnings
    from oracle import render_ref as rr
    from st3d import render as R
    S, a = 20, 2
    c = _ssref.case(20, 37, 3)
    Rn, Tn = rr.look_at_view_transform(0.75, [10.0], [35.0], at=(0, 0.10, 0.25))
    near = R.FoVPerspectiveCameras(R=torch.from_numpy(Rn), T=torch.from_numpy(Tn), device=dev)
    mesh, verts, tex = _mesh(c, dev)
    r = _renderer(S, supersample=a)
    assert r.is_hard
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rgb, cov = r.render(mesh, near)
            hi, ahi = _renderer(a * S, z_clip_value=0.5).render(mesh, near)
        assert torch.equal(rgb.detach(), ops.box_down_fwd(hi.detach(), a))
        assert torch.equal(cov, ops.box_down_fwd((ahi.detach() > 0).float(), a))
        vals = set(np.unique(cov.cpu().numpy()).tolist())
        assert vals <= {0.0, 0.25, 0.5, 0.75, 1.0} and len(vals) > 2
        rgb.sum().backward()
        assert torch.isfinite(verts.grad).all() and float(verts.grad.abs().sum()) > 0 and float(tex.grad.abs().sum()) > 0
    finally:
        ops.reset_near_plane()


# ------------------------------------------------------------------ 7. the tags a loss relies on
def test_perceptual_loss_on_a_supersampled_render(dev, ops, monkeypatch):
    """S = 64, a = 2: the need and flat tags of a supersampled render are true -- a loss that relies on them gives the
    bits of one that does not; a NaN texel still fails loudly"""
    import losses as L
    import style_transfer as ST
    import utils as U
    import _scenes
    U.device = ST.device = L.device = dev
    S, T, a = 64, 32, 2
    c = dict(_ssref.case(16, T, a))
    r = _renderer(S, supersample=a)
    cams = _cams(c, dev)
    vgg = U.get_vgg(seed=0)
    style = _scenes.style_at(1, S).to(dev).expand(_ssref.B, -1, -1, -1)
    with torch.no_grad():
        content, _ = U.render_meshes(r, _mesh(c, dev)[0], cams)

    def run(texture_np):
        cc = dict(c, tex=texture_np)
        mesh, _, tex = _mesh(cc, dev)
        cur, mask = U.render_meshes(r, mesh, cams)
        assert set(np.unique(mask.cpu().numpy()).tolist()) <= {0.0, 1.0}          # render_meshes keeps mask = (alpha > 0)
        loss = L.compute_perceptual_loss(cur, content, style, vgg)
        loss.backward()
        return loss.detach().clone(), tex.grad.clone()
    for k in ("ST3D_NEED_MASK", "ST3D_FLAT"):
        monkeypatch.delenv(k, raising=False)
    loss, gtex = run(c["tex"])
    assert torch.isfinite(loss) and float(gtex.abs().sum()) > 0
    for k in ("ST3D_NEED_MASK", "ST3D_FLAT"):
        monkeypatch.setenv(k, "0")
        loss0, gtex0 = run(c["tex"])
        monkeypatch.delenv(k)
        assert torch.equal(loss, loss0) and torch.equal(gtex, gtex0), k
    bad = c["tex"].copy()
    ty, tx = np.unravel_index(int(gtex[0].abs().sum(-1).argmax()), (T, T))        # a texel the views do touch
    bad[ty, tx, 1] = np.nan
    assert torch.isnan(run(bad)[0])
