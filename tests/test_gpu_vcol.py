"""Per-vertex colours on the GPU (csrc/vcolor.hip) against their numpy restatement (tests/_vcolref.py) on the GPU's own
fragments, at the bars test_gpu_kernels.py, the supersample and the mip files hold the UV kernels to: the forward, the
colour / barycentric / vertex gradients in both scatter modes, adjointness, the fixed-point scatter, the public API and one
CLI run.

Scenes: 'cow' -- B = 2, S in {16, 17, 24} (17: partial tiles, 24: 2 x 2 tiles; 64..166 covered pixels a view, at most 233
distinct vertices in a tile on the GPU's fragments); 'sub' -- the cow subdivided twice (93 696 faces), S = 24: nearly every
pixel has its own three vertices, the fullest the LDS table gets (255 distinct vertices in a tile); 'quad' -- two triangles
over the whole image, S = 16: every lane of the tile deposits into the same entries."""
import os

import numpy as np
import pytest
import torch

import _vcolref as VC

pytestmark = pytest.mark.gpu

CASES = [("cow", 16), ("cow", 17), ("cow", 24), ("sub", 24), ("quad", 16)]


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


_SCENES, _REFS = {}, {}


def _scene(dev, ops, name, S):
    """the scene on the device: mesh, colours, upstream gradient, projected vertices and the GPU's own fragments"""
    if (name, S) not in _SCENES:
        if name == "quad":
            verts, faces, Rn, Tn = VC.two_triangles()
        else:
            verts, faces = (VC.cow()["verts"], VC.cow()["faces"]) if name == "cow" else VC.cow_subdivided(2)
            Rn, Tn = VC.cameras()
        nb = Rn.shape[0]
        d = dict(verts_np=np.asarray(verts, np.float32), faces_np=np.asarray(faces, np.int32), R_np=Rn, T_np=Tn, B=nb,
                 col_np=VC.colours(verts.shape[0], S), g_np=VC.upstream(S, nb))
        d["verts"] = torch.from_numpy(d["verts_np"]).to(dev)
        d["faces"] = torch.from_numpy(d["faces_np"]).to(dev).contiguous()
        d["col"], d["g"] = torch.from_numpy(d["col_np"]).to(dev), torch.from_numpy(d["g_np"]).to(dev)
        d["R"], d["T"] = torch.tensor(Rn).to(dev), torch.tensor(Tn).to(dev)
        d["ndc"] = ops.project_verts(d["verts"], d["R"], d["T"])
        d["frag"] = ops.raster_fwd(d["ndc"], d["faces"], S)
        d["frag_np"] = [tuple(x[b].cpu().numpy() for x in d["frag"]) for b in range(nb)]
        d["ndc_np"] = d["ndc"].cpu().numpy()
        _SCENES[(name, S)] = d
    return _SCENES[(name, S)]


def _reference(dev, ops, name, S):
    """the restatement on the GPU's fragments, computed once per scene and left unchanged: rgb and mask with every operation
    rounded to fp32 in the kernels' order, the gradients in fp64, the vertex gradient by the CPU oracle's raster and
    projection backward from the fp32-rounded barycentric gradient (the chain the UV path is checked with)"""
    if (name, S) not in _REFS:
        from oracle import render_ref as rr
        d = _scene(dev, ops, name, S)
        rgb, mask, gbary = [], [], []
        gcol = np.zeros(d["col_np"].shape, np.float64)
        gverts = np.zeros(d["verts_np"].shape, np.float64)
        for b in range(d["B"]):
            fr = d["frag_np"][b]
            c, k = VC.shade_fwd(fr, d["faces_np"], d["col_np"], np.float32)
            rgb.append(c)
            mask.append(k)
            _, gb = VC.shade_bwd(d["g_np"][b], fr, d["faces_np"], d["col_np"], np.float64, gcol)
            gbary.append(gb)
            gndc = rr.raster_bwd(gb.astype(np.float32), fr[0], d["ndc_np"][b], d["faces_np"])
            rr.project_verts_bwd(d["verts_np"], d["R_np"][b], d["T_np"][b], gndc, gverts)
        ref = dict(rgb=np.stack(rgb), mask=np.stack(mask), gcol=gcol, gbary=np.stack(gbary), gverts=gverts)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[(name, S)] = ref
    return _REFS[(name, S)]


def _tile_vertices(d, S):
    """the largest number of distinct vertices a 16 x 16 tile deposits into"""
    worst = 0
    for fr in d["frag_np"]:
        for y in range(0, S, 16):
            for x in range(0, S, 16):
                f = fr[0][y:y + 16, x:x + 16]
                worst = max(worst, np.unique(d["faces_np"][f[f >= 0]]).size)
    return worst


def test_the_scenes_are_what_they_are_for(dev, ops):
    most = {}
    for name, S in CASES:
        d = _scene(dev, ops, name, S)
        cov = [int((fr[0] >= 0).sum()) for fr in d["frag_np"]]
        tv = _tile_vertices(d, S)
        print(f"{name} S={S}: covered {cov}, most distinct vertices in a tile {tv}")
        assert tv <= 768
        most[(name, S)] = tv
        if name == "quad":
            assert cov == [256] and tv == 4                  # asserted on the GPU's own pix_to_face: every lane deposits
        else:
            assert all(40 <= c < S * S for c in cov)
        if name == "sub":
            assert d["faces_np"].shape[0] == 93696
    assert most[("sub", 24)] > most[("cow", 24)]             # the fullest the table gets


# ------------------------------------------------------------------ 8. forward
@pytest.mark.parametrize("name,S", CASES)
def test_forward_is_the_restatement(dev, ops, name, S):
    d, ref = _scene(dev, ops, name, S), _reference(dev, ops, name, S)
    rgb, mask = ops.shade_vc_fwd(d["frag"], d["faces"], d["col"])
    assert rgb.shape == (d["B"], 3, S, S) and mask.shape == (d["B"], 1, S, S)
    err = float((rgb.double().cpu() - torch.tensor(ref["rgb"]).double()).abs().max())
    print(f"rgb: max err {err:.3e} (bar 2e-6)")
    assert err <= 2e-6
    assert np.array_equal(mask.cpu().numpy(), ref["mask"])
    off = (d["frag"][0] < 0)[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(rgb[off].view(torch.int32), torch.ones_like(rgb[off]).view(torch.int32))      # bitwise 1.0
    assert not mask[d["frag"][0][:, None] < 0].any()
    # the blend and the mask are the UV kernel's: a constant colour is what a constant texture renders, bit for bit
    const = torch.tensor([0.25, 0.5, 0.8125], device=dev)
    one, mask1 = ops.shade_vc_fwd(d["frag"], d["faces"], const.expand(d["col"].shape[0], 3).contiguous())
    uvs = torch.zeros(d["col"].shape[0], 2, device=dev)
    want, mask0 = ops.shade_fwd(d["frag"], uvs, d["faces"], const.expand(4, 4, 3).contiguous())
    assert torch.equal(mask1, mask0) and torch.equal(mask, mask0)
    assert float((one - want).abs().max()) <= 1e-6


# ------------------------------------------------------------------ 9. backward, both scatter modes
@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("name,S", CASES)
def test_backward_is_the_fp64_restatement(dev, ops, monkeypatch, name, S, det):
    monkeypatch.setattr(ops, "_DETERMINISTIC", det)
    d, ref = _scene(dev, ops, name, S), _reference(dev, ops, name, S)
    gcol, gbary = ops.shade_vc_bwd(d["g"], d["frag"], d["faces"], d["col"], want_bary=True)
    assert gcol.shape == d["col"].shape and gbary.shape == (d["B"], S, S, 3)
    _scale_close(gcol, ref["gcol"], 1e-5, "grad colours")
    _scale_close(gbary, ref["gbary"], 1e-4, "grad bary")
    assert not gbary[d["frag"][0] < 0].any()
    gverts = ops.project_verts_bwd(d["verts"], d["R"], d["T"], ops.raster_bwd(gbary, d["frag"][0], d["ndc"], d["faces"]))
    rel = np.linalg.norm(gverts.double().cpu().numpy() - ref["gverts"]) / (np.linalg.norm(ref["gverts"]) + 1e-30)
    print(f"grad verts: relative L2 {rel:.3e} (bar 2e-4)")
    assert rel <= 2e-4
    # the outputs do not depend on which of them is asked for; grad_colours given is accumulated into
    only_c = ops.shade_vc_bwd(d["g"], d["frag"], d["faces"], d["col"])
    only_b = ops.shade_vc_bwd(d["g"], d["frag"], d["faces"], d["col"], want_colours=False, want_bary=True)
    assert torch.equal(only_b, gbary)
    if det:
        assert torch.equal(only_c, gcol)
        base = torch.ones_like(gcol)
        acc = ops.shade_vc_bwd(d["g"], d["frag"], d["faces"], d["col"], grad_colours=base)
        assert acc is base and torch.equal(acc, 1.0 + gcol)
    else:
        _scale_close(only_c, ref["gcol"], 1e-5, "grad colours alone")


# ------------------------------------------------------------------ 10. adjointness
@pytest.mark.parametrize("name,S", CASES)
def test_backward_is_the_adjoint_of_the_forward(dev, ops, monkeypatch, name, S):
    """the forward is affine in C: <g, F(C + dC) - F(C)> = <dL/dC, dC>, host dot products in fp64"""
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, name, S)
    dC = torch.from_numpy(np.random.default_rng(7 + S).uniform(-1, 1, d["col_np"].shape).astype(np.float32)).to(dev)
    f0, _ = ops.shade_vc_fwd(d["frag"], d["faces"], d["col"])
    f1, _ = ops.shade_vc_fwd(d["frag"], d["faces"], d["col"] + dC)
    gcol = ops.shade_vc_bwd(d["g"], d["frag"], d["faces"], d["col"])
    lhs = float((d["g"].double().cpu() * (f1.double().cpu() - f0.double().cpu())).sum())
    rhs = float((gcol.double().cpu() * dC.double().cpu()).sum())
    print(f"<g, dF> = {lhs:.9e}, <dC*, dC> = {rhs:.9e}, relative {abs(lhs - rhs) / abs(rhs):.3e}")
    assert abs(rhs) > 1e-3 and abs(lhs - rhs) <= 1e-5 * abs(rhs)


# ------------------------------------------------------------------ 11. fixed point
@pytest.mark.parametrize("name,S", CASES)
def test_fixed_point_backward_is_reproducible_and_loud(dev, ops, monkeypatch, name, S):
    """Uncovered pixels deposit nothing: what a loss writes there enters the bound with weight 0, so finite values change
    no bit of the result; a NaN there (x * 0) poisons the bound like a NaN on a covered pixel poisons the sums"""
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, name, S)

    def run(grad):
        return ops.shade_vc_bwd(grad, d["frag"], d["faces"], d["col"], want_bary=True)
    gc, gbary = run(d["g"])
    gc_again, gbary_again = run(d["g"])
    assert torch.equal(gc, gc_again) and torch.equal(gbary, gbary_again) and float(gc.abs().sum()) > 0
    off = (d["frag"][0] < 0)[:, None].expand(-1, 3, -1, -1)
    on = ~off
    y, x = (int(i) for i in on[-1, 0].nonzero()[0])
    bad = d["g"].clone()
    bad[-1, 2, y, x] = float("nan")
    assert torch.isnan(run(bad)[0]).all()
    if name == "quad":
        assert not off.any()
        return
    noisy = torch.where(off, torch.randn(d["g"].shape, generator=torch.Generator().manual_seed(S)).to(dev), d["g"])
    assert not torch.equal(noisy, d["g"])
    gc_noisy, gbary_noisy = run(noisy)
    assert torch.equal(gc_noisy, gc) and torch.equal(gbary_noisy, gbary)
    y, x = (int(i) for i in off[0, 0].nonzero()[0])
    bad = d["g"].clone()
    bad[0, 1, y, x] = float("nan")
    out = run(bad)
    assert torch.isnan(out[0]).all() and torch.equal(out[1], gbary)        # through the bound pass; gbary is per pixel


# ------------------------------------------------------------------ 12. the public API
def _renderer(S, **kw):
    from st3d.render import MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    return MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S, **kw)), SoftPhongShader())


def _cams(d, dev):
    from st3d.render import FoVPerspectiveCameras
    return FoVPerspectiveCameras(R=d["R"], T=d["T"], device=dev)


def _vertex_mesh(d, dev, colours=None):
    import utils as U
    U.device = dev
    col = d["col"].clone().requires_grad_(True) if colours is None else colours
    verts = d["verts"].clone().requires_grad_(True)
    return U.build_mesh_vertex(col, verts, d["faces"].to(torch.int64)), verts, col


@pytest.mark.parametrize("name,S", [("cow", 17), ("cow", 24), ("quad", 16)])
def test_renderer_is_the_stagewise_composition(dev, ops, monkeypatch, name, S):
    from st3d.render import flat_of, need_of
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, name, S)
    mesh, verts, col = _vertex_mesh(d, dev)
    rgb, cov = _renderer(S).render(mesh, _cams(d, dev))
    need, flat = need_of(rgb), flat_of(rgb)
    (rgb * d["g"]).sum().backward()
    rgb0, mask0 = ops.shade_vc_fwd(d["frag"], d["faces"], d["col"])
    gc0, gbary0 = ops.shade_vc_bwd(d["g"], d["frag"], d["faces"], d["col"], want_bary=True)
    gv0 = ops.project_verts_bwd(d["verts"], d["R"], d["T"], ops.raster_bwd(gbary0, d["frag"][0], d["ndc"], d["faces"]))
    assert torch.equal(rgb.detach(), rgb0) and torch.equal(cov, mask0)
    assert torch.equal(col.grad, gc0) and torch.equal(verts.grad, gv0)
    assert float(gc0.abs().sum()) > 0 and float(gv0.abs().sum()) > 0
    assert need is not None and torch.equal(need, (d["frag"][0] >= 0).view(torch.uint8)) and flat == (1.0, 1.0, 1.0)
    # the vertices alone: the same vertex gradient, no colour gradient; the colours alone: the same colour gradient
    mesh, verts, col = _vertex_mesh(d, dev, d["col"].clone())
    (_renderer(S).render(mesh, _cams(d, dev))[0] * d["g"]).sum().backward()
    assert torch.equal(verts.grad, gv0) and col.grad is None
    # the RGBA call and a silhouette of the same mesh
    rgba = _renderer(S)(mesh.detach(), _cams(d, dev))
    assert rgba.shape == (d["B"], S, S, 4) and torch.equal(rgba[..., :3].permute(0, 3, 1, 2), rgb0)
    from st3d.render import MeshRasterizer, MeshRenderer, RasterizationSettings, SoftSilhouetteShader
    sil = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftSilhouetteShader())
    _, alpha = sil.render(mesh.detach(), _cams(d, dev))
    assert torch.equal(alpha > 0, mask0 > 0)


def test_a_uv_mesh_takes_the_launches_it_took(dev, ops, monkeypatch):
    """the same renderer on a TexturesUV mesh: _RenderFn's output bit for bit, through the same library calls"""
    import utils as U
    from st3d import render as R
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    S, T = 24, 32
    d = _scene(dev, ops, "cow", S)
    m = VC.cow()
    U.device = dev
    tex_np = np.random.default_rng(3).random((T, T, 3), dtype=np.float32)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def parts():
        tex = torch.from_numpy(tex_np)[None].to(dev).requires_grad_(True)
        verts = d["verts"].clone().requires_grad_(True)
        mesh = U.build_mesh(torch.from_numpy(m["verts_uvs"])[None].to(dev), torch.from_numpy(m["faces_uvs"].astype(np.int64))[None].to(dev),
                            tex, verts, d["faces"].to(torch.int64))
        return mesh, verts, tex
    mesh, verts, tex = parts()
    rgb, cov = _renderer(S).render(mesh, _cams(d, dev))
    (rgb * d["g"]).sum().backward()
    through_renderer = list(names)
    names.clear()
    mesh2, verts2, tex2 = parts()
    t = mesh2.textures
    rgb2, cov2 = R._RenderFn.apply(verts2, t.maps_padded(), mesh2.faces_i32(), t.verts_uvs_padded(), t.faces_uvs_i32(), d["R"],
                                   d["T"], S, None)
    (rgb2 * d["g"]).sum().backward()
    assert through_renderer == names and not any("_vc_" in n for n in names)
    assert names == ["st3d_project_verts", "st3d_raster_fwd", "st3d_shade_fwd", "st3d_shade_bwd_det", "st3d_raster_bwd_det",
                     "st3d_project_verts_bwd"]
    assert torch.equal(rgb.detach(), rgb2.detach()) and torch.equal(cov, cov2)
    assert torch.equal(tex.grad, tex2.grad) and torch.equal(verts.grad, verts2.grad)
    # and a vertex-colour render is its own three launches forward, colour scatter + the unchanged vertex chain backward
    names.clear()
    vmesh, vverts, vcol = _vertex_mesh(d, dev)
    (_renderer(S).render(vmesh, _cams(d, dev))[0] * d["g"]).sum().backward()
    assert names == ["st3d_project_verts", "st3d_raster_fwd", "st3d_shade_vc_fwd", "st3d_shade_vc_bwd_det", "st3d_raster_bwd_det",
                     "st3d_project_verts_bwd"]


def test_perceptual_loss_on_a_vertex_colour_render(dev, ops, monkeypatch):
    """S = 64: the need and flat tags of a vertex-colour render are true -- a loss that relies on them gives the bits of one
    that does not (fixed-point scatter); a NaN colour still fails loudly"""
    import losses as L
    import style_transfer as ST
    import utils as U
    import _scenes
    from st3d.render import flat_of, need_of
    U.device = ST.device = L.device = dev
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    S = 64
    d = _scene(dev, ops, "cow", S)
    r, cams = _renderer(S), _cams(d, dev)
    vgg = U.get_vgg(seed=0)
    style = _scenes.style_at(1, S).to(dev).expand(d["B"], -1, -1, -1)
    with torch.no_grad():
        content, _ = U.render_meshes(r, _vertex_mesh(d, dev)[0], cams)

    def run(col_t):
        mesh, _, col = _vertex_mesh(d, dev, col_t.clone().requires_grad_(True))
        cur, mask = U.render_meshes(r, mesh, cams)
        assert need_of(cur) is not None and flat_of(cur) == (1.0, 1.0, 1.0)
        assert set(np.unique(mask.cpu().numpy()).tolist()) <= {0.0, 1.0}
        loss = L.compute_perceptual_loss(cur, content, style, vgg)
        loss.backward()
        return loss.detach().clone(), col.grad.clone()
    start = (d["col"] * 0.5 + 0.25)
    for k in ("ST3D_NEED_MASK", "ST3D_FLAT"):
        monkeypatch.delenv(k, raising=False)
    loss, gcol = run(start)
    assert torch.isfinite(loss) and float(gcol.abs().sum()) > 0
    for k in ("ST3D_NEED_MASK", "ST3D_FLAT"):
        monkeypatch.setenv(k, "0")
        loss0, gcol0 = run(start)
        monkeypatch.delenv(k)
        assert torch.equal(loss, loss0) and torch.equal(gcol, gcol0), k
    bad = start.clone()
    bad[int(gcol.abs().sum(-1).argmax()), 1] = float("nan")                     # a vertex the views do see
    assert torch.isnan(run(bad)[0])


# ------------------------------------------------------------------ 13. the CLI
@pytest.mark.parametrize("target", ["texture", "both"])
def test_second_approach_on_a_mesh_without_uvs(dev, golden_dir, tmp_path, target):
    import second_approach as SA
    from PIL import Image
    from st3d import io as stio
    tmp = str(tmp_path)
    tea = np.load(os.path.join(golden_dir, "assets_teapot_mesh.npz"))
    assert tea["verts"].shape == (1292, 3)
    obj, style = os.path.join(tmp, "teapot.obj"), os.path.join(tmp, "style.png")
    stio.save_obj(obj, torch.from_numpy(tea["verts"]), torch.from_numpy(tea["faces"].astype(np.int64)))
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    out = os.path.join(tmp, "out")
    SA.main(["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "2", "--batch_size", "2", "--epochs", "3",
             "--seed", "0", "--save_every", "0", "--texture_type", "vertex", "--optimization_target", target,
             "--output_path", out])
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    losses = [float(line.split("Loss ")[1]) for line in lines[1:]]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    if target == "texture":
        assert losses[-1] < losses[0]
    final = os.path.join(out, "final.obj")
    vlines = [ln.split() for ln in open(final) if ln.startswith("v ")]
    assert len(vlines) == 1292 and all(len(t) == 7 for t in vlines)
    col = stio.load_vertex_colors(final)
    assert col.shape == (1292, 3) and float(col.min()) >= 0.0 and float(col.max()) <= 1.0
    assert not os.path.exists(os.path.join(out, "final.mtl")) and not os.path.exists(os.path.join(out, "final.png"))
    assert os.path.exists(os.path.join(out, "final_render", "view_11.png"))
