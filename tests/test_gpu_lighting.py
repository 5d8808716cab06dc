"""Phong lighting on the GPU: vertex normals, the lit specialised (K = 1) and general kernels, forward and backward, against
the fp64 restatement of tests/_phong_ref.py composed with oracle/soft_ref.py -- evaluated stage by stage on the GPU's own
fp32 fragments, as test_soft_shade_forward_and_backward_match_oracle does: the shading stage (texels, lighting, blend) is
differentiated in fp64 with the fragments (barycentrics, depth, distance) as leaves, and its fragment gradients are then
carried through the fp64 geometry (soft_geometry / clipped_geometry) to the vertices.

Fragments whose fp64 n.l or e.r lies within KINK of 0 (the relu / [cos > 0] kinks, where fp32 and fp64 can land on
different sides) are excluded: their upstream gradient is zeroed and their pixels are not compared; the tests count them."""
import os
import warnings

import numpy as np
import pytest
import torch

import _phong_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINK = 1e-4
ATOL, TEX_RTOL, VERT_RTOL = 2e-5, 2e-5, 5e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bob():
    d = np.load(os.path.join(ROOT, "tests", "golden", "assets_bob_mesh.npz"))
    return {k: d[k] for k in d.files}


def _cams(n, seed=0, dist=2.10):
    from oracle import render_ref as rr
    g = torch.Generator().manual_seed(seed)
    elev, azim = rr.random_camera_angles(n, lambda k: torch.rand(k, generator=g).numpy())
    return rr.look_at_view_transform(dist, elev, azim, at=(0, 0.10, 0.25))


def _scene(cow, dev, Tn=32, seed=1):
    from st3d import render as R
    rng = np.random.default_rng(seed)
    tex = rng.random((Tn, Tn, 3), dtype=np.float32)
    verts = torch.from_numpy(cow["verts"]).to(dev).requires_grad_(True)
    texd = torch.from_numpy(tex).to(dev)[None].requires_grad_(True)
    faces = torch.from_numpy(cow["faces"].astype(np.int64)).to(dev)
    uvs = torch.from_numpy(cow["verts_uvs"]).to(dev)
    fuv = torch.from_numpy(cow["faces_uvs"].astype(np.int64)).to(dev)
    mesh = R.Meshes(verts, faces, R.TexturesUV(maps=texd, faces_uvs=fuv[None], verts_uvs=uvs[None]))
    return mesh, verts, texd, tex


def _light_dict(lights, mats, b, C):
    from st3d import render as R
    ent = lambda t: t[min(b, t.shape[0] - 1)].detach().cpu().double()       # noqa: E731
    m = mats if mats is not None else R.Materials()
    mat = dict(ambient=ent(m.ambient_color), diffuse=ent(m.diffuse_color), specular=ent(m.specular_color),
               shininess=float(m.shininess[min(b, m.shininess.shape[0] - 1)]))
    d = dict(ambient=ent(lights.ambient_color), diffuse=ent(lights.diffuse_color), specular=ent(lights.specular_color))
    if isinstance(lights, R.AmbientLights):
        d["kind"] = "ambient"
    elif isinstance(lights, R.DirectionalLights):
        d.update(kind="directional", direction=ent(lights.direction))
    elif isinstance(lights, R.HeadLights):
        d.update(kind="point", location=C)
    else:
        d.update(kind="point", location=ent(lights.location))
    return d, mat


def _reference(cow, tex, R_, T_, frags, g, lights, mats, S, geometry, sigma=1e-4, gamma=1e-4, bg=(1.0, 1.0, 1.0)):
    """fp64 restatement per view on the GPU's fragments -> (rgb (B,3,S,S), d/dtexture, d/dverts, covered-pixel mask, number
    of fragments excluded at the kinks).  frags: (p2f, zbuf, bary, dists[, slots]) as the kernels saw them."""
    from oracle import soft_ref as SR
    fc = torch.from_numpy(cow["faces"]).long()
    uv64, fuv64 = torch.from_numpy(cow["verts_uvs"]).double(), torch.from_numpy(cow["faces_uvs"]).long()
    tt = torch.from_numpy(tex).double().requires_grad_(True)
    vt = torch.from_numpy(cow["verts"]).double().requires_grad_(True)
    B = R_.shape[0]
    rgbs, keep, excluded = [], [], 0
    for b in range(B):
        Rb, Tb = torch.from_numpy(R_[b]).double(), torch.from_numpy(T_[b]).double()
        C = PR.camera_centre(Rb, Tb)
        light, mat = _light_dict(lights, mats, b, C)
        p2f = frags[0][b].cpu().long()
        if p2f.dim() == 2:
            p2f = p2f[..., None]
        K = p2f.shape[-1]
        mask = p2f >= 0
        bl = frags[2][b].cpu().double().reshape(S, S, K, 3).requires_grad_(True)
        zl = frags[1][b].cpu().double().reshape(S, S, K).requires_grad_(True)
        dl = frags[3][b].cpu().double().reshape(S, S, K).requires_grad_(True)
        normals = PR.vertex_normals(vt, fc)
        texels = SR.sample_texture(bl, p2f, uv64, fuv64, tt)
        colors = PR.lit_colors(texels, bl, p2f, vt, normals, fc, C, light, mat)
        r, _ = SR.softmax_rgb_blend(colors, zl, dl, mask, sigma, gamma, bg)
        with torch.no_grad():
            kink = (PR.kink_margin(bl, p2f, vt, normals, fc, C, light) < KINK) & mask
        excluded += int(kink.sum())
        ok = ~kink.any(-1)
        keep.append(ok)
        rgbs.append(r.detach().permute(2, 0, 1))
        (r.permute(2, 0, 1) * torch.from_numpy(g[b]).double() * ok.double()).sum().backward()
        # geometry stage with the fp64 fragment gradients
        ndc_b = SR.project(vt, Rb, Tb)
        ndc32 = SR.project(vt.detach().float(), Rb.float(), Tb.float()).double()
        ndc_b = ndc_b + (ndc32 - ndc_b).detach()
        bary64, pz64, sd64, m64 = geometry(ndc_b, fc, b, p2f)
        md = m64.double()
        ((bary64 * bl.grad * md.unsqueeze(-1)).sum() + (pz64 * zl.grad * md).sum() + (sd64 * dl.grad * md).sum()).backward()
    return torch.stack(rgbs), tt.grad, vt.grad, torch.stack(keep), excluded


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / (b.norm() + 1e-30))


def _hard_geometry(S):
    from oracle import soft_ref as SR
    return lambda ndc_b, fc, b, p2f: SR.soft_geometry(ndc_b, fc, p2f, S, False)


def _render(mesh, R_, T_, S, lights, mats, rs=None, bp=None, g=None):
    from st3d import render as R
    rgb, cov = R.render_views(mesh, torch.from_numpy(R_), torch.from_numpy(T_), S, rs, bp, lights, mats)
    if g is not None:
        (rgb * torch.from_numpy(g).to(rgb.device)).sum().backward()
    return rgb, cov


def _frags_hard(mesh, R_, T_, S, dev):
    from st3d import ops
    ndc = ops.project_verts(mesh.verts_packed().detach(), torch.from_numpy(R_).to(dev), torch.from_numpy(T_).to(dev))
    return ops.raster_fwd(ndc, mesh.faces_i32(), S)


# ------------------------------------------------------------------------------------------------ vertex normals
@pytest.mark.parametrize("name", ["cow", "bob"])
def test_vertex_normals_forward_backward_match_fp64(dev, cow, bob, name):
    from st3d import ops, render as R
    m = cow if name == "cow" else bob
    v = torch.from_numpy(m["verts"]).float().to(dev)
    f = torch.from_numpy(m["faces"].astype(np.int64)).to(dev)
    f32 = f.to(torch.int32).contiguous()
    inc = R.vertex_incidence(f32, v.shape[0])
    n, mm = ops.vertex_normals(v, f32, inc)
    n2, _ = ops.vertex_normals(v, f32, inc)
    assert torch.equal(n, n2)
    vt = torch.from_numpy(m["verts"]).double().requires_grad_(True)
    ref = PR.vertex_normals(vt, f.cpu())
    np.testing.assert_allclose(n.cpu().numpy(), ref.detach().numpy(), atol=2e-6)
    gn = torch.randn(v.shape, generator=torch.Generator().manual_seed(3))
    gp = torch.randn(v.shape, generator=torch.Generator().manual_seed(4))
    (ref * gn.double()).sum().backward()
    out = torch.zeros_like(v)
    ops.vertex_normals_bwd(v, f32, inc, mm, gn.to(dev), gp.to(dev), out)
    out2 = torch.zeros_like(v)
    ops.vertex_normals_bwd(v, f32, inc, mm, gn.to(dev), gp.to(dev), out2)
    assert torch.equal(out, out2)
    assert _rel(out - gp.to(dev), vt.grad) <= VERT_RTOL


# ------------------------------------------------------------------------------------------------ specialised K = 1 path
def _cases():
    from st3d import render as R
    return {
        "point": (R.PointLights(location=((2.0, 2.0, 2.0),)), None),
        "directional_from_below": (R.DirectionalLights(direction=((0.3, -1.0, 0.2),)), None),
        "ambient_colour": (R.AmbientLights(ambient_color=((0.3, 0.6, 0.9),)), None),
        "materials_shininess_1": (R.PointLights(location=((0.0, 2.0, 3.0),), diffuse_color=((0.6, 0.5, 0.4),),
                                                specular_color=((0.5, 0.6, 0.7),)),
                                  R.Materials(ambient_color=((0.2, 0.3, 0.4),), diffuse_color=((0.9, 0.7, 0.5),),
                                              specular_color=((0.8, 0.8, 0.8),), shininess=1)),
        "per_view_shininess_64": (R.PointLights(location=((2.0, 1.0, 0.0), (-1.0, 2.0, 2.0), (0.0, -2.0, 1.0)),
                                                specular_color=((1.0, 1.0, 1.0),)),
                                  R.Materials(specular_color=((1.0, 0.5, 0.25),), shininess=64)),
        "headlight": (R.HeadLights(diffuse_color=((0.6, 0.6, 0.6),)), None),
    }


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("case", ["point", "directional_from_below", "ambient_colour", "materials_shininess_1",
                                  "per_view_shininess_64", "headlight"])
def test_hard_lit_forward_backward_match_fp64(dev, cow, case, det):
    from st3d import ops
    lights, mats = _cases()[case]
    S, B = 64, 3
    R_, T_ = _cams(B, seed=5)
    mesh, verts, texd, tex = _scene(cow, dev)
    g = np.random.default_rng(2).standard_normal((B, 3, S, S)).astype(np.float32)
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        rgb, cov = _render(mesh, R_, T_, S, lights, mats)
        frags = _frags_hard(mesh, R_, T_, S, dev)
        ref, gt_ref, gv_ref, keep, excluded = _reference(cow, tex, R_, T_, frags, g, lights, mats, S, _hard_geometry(S))
        gk = (torch.from_numpy(g) * keep[:, None].float()).numpy()
        (rgb * torch.from_numpy(gk).to(dev)).sum().backward()
        gtex, gverts = texd.grad[0].clone(), verts.grad.clone()
        if det:             # bitwise reproducible
            texd.grad, verts.grad = None, None
            rgb2, _ = _render(mesh, R_, T_, S, lights, mats, g=gk)
            assert torch.equal(rgb, rgb2) and torch.equal(texd.grad[0], gtex) and torch.equal(verts.grad, gverts)
            # one target at a time takes the same backward: its own gradient bit for bit, none for the other
            for need_v in (True, False):
                texd.grad, verts.grad = None, None
                verts.requires_grad_(need_v), texd.requires_grad_(not need_v)
                try:
                    _render(mesh, R_, T_, S, lights, mats, g=gk)
                finally:
                    verts.requires_grad_(True), texd.requires_grad_(True)
                if need_v:
                    assert texd.grad is None and torch.equal(verts.grad, gverts)
                else:
                    assert verts.grad is None and torch.equal(texd.grad[0], gtex)
    finally:
        ops.set_deterministic(was)
    covered = frags[0].cpu() >= 0
    assert excluded < 0.02 * int(covered.sum()), excluded
    sel = keep[:, None].expand(-1, 3, -1, -1)
    err = float((rgb.cpu().double() - ref)[sel].abs().max())
    assert err <= ATOL, err
    assert _rel(gtex, gt_ref) <= TEX_RTOL, _rel(gtex, gt_ref)
    assert _rel(gverts, gv_ref) <= VERT_RTOL, _rel(gverts, gv_ref)
    if case != "ambient_colour":            # the light actually shapes the image
        rgb0, _ = _render(mesh, R_, T_, S, None, None)
        assert float((rgb0 - rgb).abs().max()) > 0.05


def test_headlight_is_a_point_light_at_each_camera(dev, cow):
    from st3d import render as R
    S, B = 48, 3
    R_, T_ = _cams(B, seed=9)
    mesh, *_ = _scene(cow, dev)
    C = [PR.camera_centre(torch.from_numpy(R_[b]).double(), torch.from_numpy(T_[b]).double()).tolist() for b in range(B)]
    a, _ = _render(mesh, R_, T_, S, R.HeadLights(), None)
    b, _ = _render(mesh, R_, T_, S, R.PointLights(location=C), None)
    assert float((a - b).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ general path
@pytest.mark.parametrize("case", ["point", "per_view_shininess_64"])
def test_soft_lit_k4_blur_match_fp64(dev, cow, case):
    from oracle import soft_ref as SR
    from st3d import ops, render as R
    lights, mats = _cases()[case]
    S, B, K = 48, 3, 4
    sigma, gamma, bg = 1e-4, 1e-2, (0.2, 0.5, 0.9)
    R_, T_ = _cams(B, seed=6)
    mesh, verts, texd, tex = _scene(cow, dev)
    rs = R.RasterizationSettings(image_size=S, blur_radius=2e-4, faces_per_pixel=K)
    bp = R.BlendParams(sigma, gamma, bg)
    g = np.random.default_rng(3).standard_normal((B, 3, S, S)).astype(np.float32)
    rgb, _ = _render(mesh, R_, T_, S, lights, mats, rs, bp)
    ndc = ops.project_verts(verts.detach(), torch.from_numpy(R_).to(dev), torch.from_numpy(T_).to(dev))
    frags = ops.raster_soft_fwd(ndc, mesh.faces_i32(), S, K, 2e-4, True, z_clip=0.5)[:4]     # as the renderer rasterises
    geom = lambda ndc_b, fc, b, p2f: SR.soft_geometry(ndc_b, fc, p2f, S, True)      # noqa: E731
    ref, gt_ref, gv_ref, keep, excluded = _reference(cow, tex, R_, T_, frags, g, lights, mats, S, geom, sigma, gamma, bg)
    gk = (torch.from_numpy(g) * keep[:, None].float()).to(dev)
    (rgb * gk).sum().backward()
    assert excluded < 0.02 * int((frags[0] >= 0).sum()), excluded
    sel = keep[:, None].expand(-1, 3, -1, -1)
    # K > 1: the fp32 depth term's ~6e-8 of rounding is divided by gamma in the softmax (as in test_gpu_kernels)
    atol, vtol = max(ATOL, 3e-8 / gamma), max(VERT_RTOL, 2e-7 / gamma)
    err = float((rgb.detach().cpu().double() - ref)[sel].abs().max())
    assert err <= atol, err
    assert _rel(texd.grad[0], gt_ref) <= max(TEX_RTOL, 3e-8 / gamma), _rel(texd.grad[0], gt_ref)
    assert _rel(verts.grad, gv_ref) <= vtol, _rel(verts.grad, gv_ref)


def test_near_plane_reroute_keeps_the_lighting(dev, cow):
    """Cameras inside the cow's bounding sphere: render_views sends the hard configuration to the clipping kernels, lit."""
    from oracle import soft_ref as SR
    from st3d import ops, render as R
    lights, mats = _cases()["point"]
    S, B = 48, 2
    R_, T_ = _cams(B, seed=4, dist=0.9)
    mesh, verts, texd, tex = _scene(cow, dev)
    ndc = ops.project_verts(verts.detach(), torch.from_numpy(R_).to(dev), torch.from_numpy(T_).to(dev))
    assert float(ndc[..., 2].min()) < 0.5, "the scene must reach the near plane"
    g = np.random.default_rng(4).standard_normal((B, 3, S, S)).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (the one-per-process note that rendering moved to the clipping kernels)
        rgb, _ = _render(mesh, R_, T_, S, lights, mats)
    frags = ops.raster_soft_fwd(ndc, mesh.faces_i32(), S, 1, 0.0, False, z_clip=0.5)
    slots = frags[4].cpu().long()
    geom = lambda ndc_b, fc, b, p2f: SR.clipped_geometry(ndc_b, fc, slots[b], S, False, True, 0.5)     # noqa: E731
    ref, gt_ref, gv_ref, keep, excluded = _reference(cow, tex, R_, T_, frags[:4], g, lights, mats, S, geom)
    (rgb * (torch.from_numpy(g) * keep[:, None].float()).to(dev)).sum().backward()
    sel = keep[:, None].expand(-1, 3, -1, -1)
    err = float((rgb.detach().cpu().double() - ref)[sel].abs().max())
    assert err <= ATOL, err
    assert _rel(texd.grad[0], gt_ref) <= TEX_RTOL, _rel(texd.grad[0], gt_ref)
    assert _rel(verts.grad, gv_ref) <= VERT_RTOL, _rel(verts.grad, gv_ref)


# ------------------------------------------------------------------------------------------------ API
def test_default_shading_is_unchanged(dev, cow):
    from st3d import render as R
    S, B = 64, 2
    R_, T_ = _cams(B, seed=2)
    g = np.random.default_rng(5).standard_normal((B, 3, S, S)).astype(np.float32)
    outs = []
    for lights, mats in ((None, None), (R.AmbientLights(), None), (R.AmbientLights(), R.Materials())):
        mesh, verts, texd, _ = _scene(cow, dev)
        rgb, cov = _render(mesh, R_, T_, S, lights, mats, g=g)
        outs.append((rgb.detach(), cov, texd.grad.clone(), verts.grad.clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))
    # one target at a time takes the same (unlit) backward: its own gradient bit for bit, none for the other
    for need_v in (True, False):
        mesh, verts, texd, _ = _scene(cow, dev)
        verts.requires_grad_(need_v), texd.requires_grad_(not need_v)
        _render(mesh, R_, T_, S, None, None, g=g)
        if need_v:
            assert texd.grad is None and torch.equal(verts.grad, outs[0][3])
        else:
            assert verts.grad is None and torch.equal(texd.grad, outs[0][2])


def test_per_call_lights_override_the_shader(dev, cow):
    from st3d import render as R
    S = 48
    R_, T_ = _cams(2, seed=3)
    mesh, *_ = _scene(cow, dev)
    cams = R.FoVPerspectiveCameras(R=torch.from_numpy(R_), T=torch.from_numpy(T_), device=dev)
    rast = R.MeshRasterizer(cams, R.RasterizationSettings(image_size=S))
    lights = R.DirectionalLights(direction=((0.2, 0.8, 0.4),), device=dev)
    plain = R.MeshRenderer(rast, R.SoftPhongShader(device=dev))
    lit = R.MeshRenderer(rast, R.SoftPhongShader(device=dev, lights=lights))
    a = plain(mesh, cameras=cams, lights=lights)
    b = lit(mesh, cameras=cams)
    assert torch.equal(a, b)
    assert not torch.equal(plain(mesh, cameras=cams), b)


def test_nan_propagates_through_the_lighting(dev, cow):
    from oracle import soft_ref as SR
    from st3d import ops, render as R
    S, B = 48, 2
    R_, T_ = _cams(B, seed=8)
    mesh, verts, texd, tex = _scene(cow, dev)
    lights = R.PointLights(location=((2.0, 2.0, 2.0),))
    # a NaN texel: exactly the covered pixels whose footprint touches it go NaN (the restatement decides which)
    with torch.no_grad():
        texd[0, 10, 12, 1] = float("nan")
    tex_nan = texd[0].detach().cpu().numpy()
    rgb, _ = _render(mesh, R_, T_, S, lights, None)
    frags = _frags_hard(mesh, R_, T_, S, dev)
    uv64, fuv64 = torch.from_numpy(cow["verts_uvs"]).double(), torch.from_numpy(cow["faces_uvs"]).long()
    want = torch.zeros(B, S, S, dtype=torch.bool)
    for b in range(B):
        p2f = frags[0][b].cpu().long()[..., None]
        t = SR.sample_texture(frags[2][b].cpu().double()[:, :, None], p2f, uv64, fuv64, torch.from_numpy(tex_nan).double())
        want[b] = torch.isnan(t).any(-1)[..., 0] & (p2f[..., 0] >= 0)
    got = torch.isnan(rgb.detach().cpu()).any(1)
    assert int(want.sum()) > 0 and torch.equal(got, want)
    # a NaN light location: every covered pixel NaN, the background finite
    mesh, verts, texd, tex = _scene(cow, dev)
    rgb, cov = _render(mesh, R_, T_, S, R.PointLights(location=((float("nan"), 1.0, 0.0),)), None)
    covered = cov.detach().cpu()[:, 0] > 0
    isn = torch.isnan(rgb.detach().cpu()).any(1)
    assert torch.equal(isn, covered) and bool(torch.isfinite(rgb.detach().cpu()[~covered[:, None].expand(-1, 3, -1, -1)]).all())
    # a NaN upstream gradient: NaN texture gradient in the deterministic mode
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        mesh, verts, texd, tex = _scene(cow, dev)
        rgb, _ = _render(mesh, R_, T_, S, lights, None)
        gr = torch.zeros_like(rgb)
        gr[0, 1, S // 2, S // 2] = float("nan")
        rgb.backward(gr)
        assert bool(torch.isnan(texd.grad).all())
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ end to end
def _write_cow_assets(tmp, cow, tex_size=64):
    from PIL import Image
    from st3d import io as stio
    tex = torch.from_numpy(cow["texture_u8"][::1024 // tex_size, ::1024 // tex_size].copy()).float() / 255
    obj = os.path.join(tmp, "cow.obj")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    sty = np.load(os.path.join(ROOT, "tests", "golden", "assets_style1_512.npz"))["rgb_u8"]
    style = os.path.join(tmp, "style.png")
    Image.fromarray(sty).save(style)
    return obj, style


@pytest.mark.parametrize("target", ["texture", "both"])
def test_second_approach_lit_end_to_end(dev, cow, tmp_path, target):
    import losses as L
    import second_approach as SA
    import style_transfer as ST
    import utils as U
    from PIL import Image
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow)
    runs = {}
    for lights in ("point", "ambient"):
        outp = str(tmp_path / f"out_{lights}")
        SA.main(["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "3", "--batch_size", "2",
                 "--epochs", "4", "--output_path", outp, "--seed", "0", "--lr", "0.02", "--optimization_target", target,
                 "--lights", lights])
        log = open(os.path.join(outp, "log.txt")).read().splitlines()
        losses = [float(line.split("Loss ")[1]) for line in log[1:]]
        assert len(losses) == 4 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        assert sorted(os.listdir(os.path.join(outp, "current_images"))) == ["view_0.png", "view_1.png", "view_2.png"]
        assert len(os.listdir(os.path.join(outp, "final_render"))) == 12
        runs[lights] = outp
    for sub in ("current_images/view_0.png", "final_render/view_0.png"):
        a = np.asarray(Image.open(os.path.join(runs["point"], sub)), dtype=np.float32)
        b = np.asarray(Image.open(os.path.join(runs["ambient"], sub)), dtype=np.float32)
        assert np.abs(a - b).max() > 10, sub
