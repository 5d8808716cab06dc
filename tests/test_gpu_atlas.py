"""The per-face texel atlas on the GPU (csrc/atlas.hip) against its numpy restatement (tests/_atlasref.py) on the GPU's own
fragments, at the bars tests/test_gpu_vcol.py holds the vertex-colour kernels to for the same quantities: the forward (rgb
within 2e-6 of the fp32 restatement, its test_forward_is_the_restatement), the scatter gradient in both modes (1e-5 of its
max against fp64, its test_backward_is_the_fp64_restatement), adjointness (1e-5 relative, its
test_backward_is_the_adjoint_of_the_forward); then the fixed-point scatter, the public API, supersampling, the launches of the
other texture classes, the perceptual loss and one CLI run.

Scenes: 'cow' -- B = 2, S in {16, 17, 24} (17: partial tiles, 24: 2 x 2 tiles; 64..166 covered pixels a view) at R in
{1, 3, 8}; 'quad' -- two triangles over the whole image, S = 16: at R = 1 all 256 lanes of the tile deposit into two texels,
at R = 64 nearly every lane has a texel of its own (the fullest the 256-entry table gets)."""
import os

import numpy as np
import pytest
import torch

import _atlasref as AR

pytestmark = pytest.mark.gpu

CASES = [("cow", S, R) for S in AR.SIDES for R in (1, 3, 8)] + [("quad", 16, 1), ("quad", 16, 64)]


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


_GEOM, _SCENES, _REFS = {}, {}, {}


def _geometry(dev, ops, name, S):
    """mesh, cameras, upstream gradient and the GPU's own fragments: shared by every R"""
    if (name, S) not in _GEOM:
        if name == "quad":
            verts, faces, Rn, Tn = AR.two_triangles()
        else:
            verts, faces = AR.cow()["verts"], AR.cow()["faces"]
            Rn, Tn = AR.cameras()
        nb = Rn.shape[0]
        d = dict(verts_np=np.asarray(verts, np.float32), faces_np=np.asarray(faces, np.int32), B=nb, g_np=AR.upstream(S, nb))
        d["F"] = d["faces_np"].shape[0]
        d["verts"] = torch.from_numpy(d["verts_np"]).to(dev)
        d["faces"] = torch.from_numpy(d["faces_np"]).to(dev).contiguous()
        d["g"] = torch.from_numpy(d["g_np"]).to(dev)
        d["R"], d["T"] = torch.tensor(Rn).to(dev), torch.tensor(Tn).to(dev)
        d["frag"] = ops.raster_fwd(ops.project_verts(d["verts"], d["R"], d["T"]), d["faces"], S)
        d["frag_np"] = [tuple(x[b].cpu().numpy() for x in d["frag"]) for b in range(nb)]
        _GEOM[(name, S)] = d
    return _GEOM[(name, S)]


def _scene(dev, ops, name, S, R):
    if (name, S, R) not in _SCENES:
        d = dict(_geometry(dev, ops, name, S))
        d["atlas_np"] = AR.atlas(d["F"], R, S)
        d["atlas"] = torch.from_numpy(d["atlas_np"]).to(dev)
        d["Rr"] = R
        _SCENES[(name, S, R)] = d
    return _SCENES[(name, S, R)]


def _reference(dev, ops, name, S, R):
    """the restatement on the GPU's fragments, computed once per scene and left unchanged: rgb and mask with every operation
    rounded to fp32 in the kernels' order, the atlas gradient in fp64, and the set of texels grad_rgb = 1 reaches"""
    if (name, S, R) not in _REFS:
        d = _scene(dev, ops, name, S, R)
        rgb, mask = [], []
        gat = np.zeros(d["atlas_np"].shape, np.float64)
        hit = np.zeros(d["atlas_np"].shape, np.float64)
        for b in range(d["B"]):
            fr = d["frag_np"][b]
            c, k = AR.shade_fwd(fr, d["atlas_np"], np.float32)
            rgb.append(c)
            mask.append(k)
            AR.shade_bwd(d["g_np"][b], fr, R, d["F"], np.float64, gat)
            AR.shade_bwd(np.ones_like(d["g_np"][b]), fr, R, d["F"], np.float64, hit)
        ref = dict(rgb=np.stack(rgb), mask=np.stack(mask), gatlas=gat, hit=hit)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[(name, S, R)] = ref
    return _REFS[(name, S, R)]


def _tile_texels(d, S, R):
    """the largest number of distinct texels a 16 x 16 tile deposits into"""
    worst = 0
    for fr in d["frag_np"]:
        for y in range(0, S, 16):
            for x in range(0, S, 16):
                f, b = fr[0][y:y + 16, x:x + 16], fr[2][y:y + 16, x:x + 16]
                wy, wx = AR.texel_index(b[f >= 0][:, 0], b[f >= 0][:, 1], R)
                worst = max(worst, np.unique((f[f >= 0].astype(np.int64) * R + wy) * R + wx).size)
    return worst


def test_the_scenes_are_what_they_are_for(dev, ops):
    for name, S, R in CASES:
        d = _scene(dev, ops, name, S, R)
        cov = [int((fr[0] >= 0).sum()) for fr in d["frag_np"]]
        tt = _tile_texels(d, S, R)
        print(f"{name} S={S} R={R}: covered {cov}, most distinct texels in a tile {tt}")
        assert tt <= 256
        if name == "quad":
            assert cov == [256]                                      # on the GPU's own pix_to_face: every lane deposits
            assert tt == 2 if R == 1 else tt >= 200                  # two keys for 256 lanes / (nearly) a key a lane
        else:
            assert all(40 <= c < S * S for c in cov)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,S,R", CASES)
def test_forward_is_the_restatement(dev, ops, name, S, R):
    d, ref = _scene(dev, ops, name, S, R), _reference(dev, ops, name, S, R)
    rgb, mask = ops.shade_atlas_fwd(d["frag"], d["atlas"])
    assert rgb.shape == (d["B"], 3, S, S) and mask.shape == (d["B"], 1, S, S)
    err = float((rgb.double().cpu() - torch.tensor(ref["rgb"]).double()).abs().max())
    print(f"rgb: max err {err:.3e} (bar 2e-6)")
    assert err <= 2e-6
    assert np.array_equal(mask.cpu().numpy(), ref["mask"])
    off = (d["frag"][0] < 0)[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(rgb[off].view(torch.int32), torch.ones_like(rgb[off]).view(torch.int32))      # bitwise 1.0
    assert not mask[d["frag"][0][:, None] < 0].any()
    # the blend and the mask are the UV kernel's: an atlas of one colour is what a constant texture renders
    const = torch.tensor([0.25, 0.5, 0.8125], device=dev)
    one, mask1 = ops.shade_atlas_fwd(d["frag"], const.expand(d["F"], R, R, 3).contiguous())
    uvs = torch.zeros(d["verts"].shape[0], 2, device=dev)
    want, mask0 = ops.shade_fwd(d["frag"], uvs, d["faces"], const.expand(4, 4, 3).contiguous())
    assert torch.equal(mask1, mask0) and torch.equal(mask, mask0)
    assert float((one - want).abs().max()) <= 1e-6


# ------------------------------------------------------------------ backward, both scatter modes
@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("name,S,R", CASES)
def test_backward_is_the_fp64_restatement(dev, ops, monkeypatch, name, S, R, det):
    monkeypatch.setattr(ops, "_DETERMINISTIC", det)
    d, ref = _scene(dev, ops, name, S, R), _reference(dev, ops, name, S, R)
    gat = ops.shade_atlas_bwd(d["g"], d["frag"], R, d["F"])
    assert gat.shape == d["atlas"].shape
    _scale_close(gat, ref["gatlas"], 1e-5, "grad atlas")
    # with grad_rgb = 1 every deposit is positive: the texels reached are the restatement's, exactly
    ones = ops.shade_atlas_bwd(torch.ones_like(d["g"]), d["frag"], R, d["F"])
    assert np.array_equal(ones.cpu().numpy() != 0, ref["hit"] != 0) and (ref["hit"] != 0).any()
    _scale_close(ones, ref["hit"], 1e-5, "texel hits")
    if det:
        base = torch.ones_like(gat)
        acc = ops.shade_atlas_bwd(d["g"], d["frag"], R, d["F"], grad_atlas=base)
        assert acc is base and torch.equal(acc, 1.0 + gat)


# ------------------------------------------------------------------ adjointness
@pytest.mark.parametrize("name,S,R", CASES)
def test_backward_is_the_adjoint_of_the_forward(dev, ops, monkeypatch, name, S, R):
    """the forward is affine in the atlas: <g, F(A + dA) - F(A)> = <dL/dA, dA>, host dot products in fp64"""
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, name, S, R)
    dA = torch.from_numpy(np.random.default_rng(7 + S + R).uniform(-1, 1, d["atlas_np"].shape).astype(np.float32)).to(dev)
    f0, _ = ops.shade_atlas_fwd(d["frag"], d["atlas"])
    f1, _ = ops.shade_atlas_fwd(d["frag"], d["atlas"] + dA)
    gat = ops.shade_atlas_bwd(d["g"], d["frag"], R, d["F"])
    lhs = float((d["g"].double().cpu() * (f1.double().cpu() - f0.double().cpu())).sum())
    rhs = float((gat.double().cpu() * dA.double().cpu()).sum())
    print(f"<g, dF> = {lhs:.9e}, <dA*, dA> = {rhs:.9e}, relative {abs(lhs - rhs) / abs(rhs):.3e}")
    assert abs(rhs) > 1e-3 and abs(lhs - rhs) <= 1e-5 * abs(rhs)


# ------------------------------------------------------------------ fixed point
@pytest.mark.parametrize("name,S,R", CASES)
def test_fixed_point_backward_is_reproducible_and_loud(dev, ops, monkeypatch, name, S, R):
    """Uncovered pixels deposit nothing: what a loss writes there enters the bound with weight 0, so finite values change
    no bit of the result; a NaN there (x * 0) poisons the bound like a NaN on a covered pixel poisons the sums"""
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, name, S, R)

    def run(grad):
        return ops.shade_atlas_bwd(grad, d["frag"], R, d["F"])
    ga = run(d["g"])
    assert torch.equal(ga, run(d["g"])) and float(ga.abs().sum()) > 0
    off = (d["frag"][0] < 0)[:, None].expand(-1, 3, -1, -1)
    on = ~off
    y, x = (int(i) for i in on[-1, 0].nonzero()[0])
    bad = d["g"].clone()
    bad[-1, 2, y, x] = float("nan")
    assert torch.isnan(run(bad)).all()
    if name == "quad":
        assert not off.any()
        return
    noisy = torch.where(off, torch.randn(d["g"].shape, generator=torch.Generator().manual_seed(S)).to(dev), d["g"])
    assert not torch.equal(noisy, d["g"])
    assert torch.equal(run(noisy), ga)
    y, x = (int(i) for i in off[0, 0].nonzero()[0])
    bad = d["g"].clone()
    bad[0, 1, y, x] = float("nan")
    assert torch.isnan(run(bad)).all()                               # through the bound pass


# ------------------------------------------------------------------ the public API
def _renderer(S, **kw):
    from st3d.render import MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    return MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S, **kw)), SoftPhongShader())


def _cams(d, dev):
    from st3d.render import FoVPerspectiveCameras
    return FoVPerspectiveCameras(R=d["R"], T=d["T"], device=dev)


def _atlas_mesh(d, dev, atlas=None, verts_grad=True):
    import utils as U
    U.device = dev
    at = d["atlas"].clone().requires_grad_(True) if atlas is None else atlas
    verts = d["verts"].clone().requires_grad_(verts_grad)
    return U.build_mesh_atlas(at, verts, d["faces"].to(torch.int64)), verts, at


@pytest.mark.parametrize("name,S,R", [("cow", 17, 3), ("cow", 24, 8), ("quad", 16, 64)])
def test_renderer_is_the_stagewise_composition(dev, ops, monkeypatch, name, S, R):
    from st3d.render import flat_of, need_of
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, name, S, R)
    mesh, verts, at = _atlas_mesh(d, dev)
    rgb, cov = _renderer(S).render(mesh, _cams(d, dev))
    need, flat = need_of(rgb), flat_of(rgb)
    (rgb * d["g"]).sum().backward()
    rgb0, mask0 = ops.shade_atlas_fwd(d["frag"], d["atlas"])
    ga0 = ops.shade_atlas_bwd(d["g"], d["frag"], R, d["F"])
    assert torch.equal(rgb.detach(), rgb0) and torch.equal(cov, mask0)
    assert torch.equal(at.grad, ga0) and float(ga0.abs().sum()) > 0
    assert verts.requires_grad and verts.grad is None                # the nearest-texel colour moves no vertex
    assert need is not None and torch.equal(need, (d["frag"][0] >= 0).view(torch.uint8)) and flat == (1.0, 1.0, 1.0)
    # the RGBA call and a silhouette of the same mesh
    rgba = _renderer(S)(mesh.detach(), _cams(d, dev))
    assert rgba.shape == (d["B"], S, S, 4) and torch.equal(rgba[..., :3].permute(0, 3, 1, 2), rgb0)
    from st3d.render import MeshRasterizer, MeshRenderer, RasterizationSettings, SoftSilhouetteShader
    sil = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftSilhouetteShader())
    _, alpha = sil.render(mesh.detach(), _cams(d, dev))
    assert torch.equal(alpha > 0, mask0 > 0)


@pytest.mark.parametrize("R", [3, 8])
def test_supersample_is_the_render_at_twice_the_side_then_the_box_filter(dev, ops, monkeypatch, R):
    """supersample = 2 at S = 12 is _AtlasRenderFn at 24 followed by box_down, bit for bit: rgb, coverage and -- in fixed
    point -- the atlas gradient through the filter's transpose"""
    from st3d import render as RR
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    S, a = 12, 2
    d = _scene(dev, ops, "cow", a * S, R)
    g = torch.from_numpy(AR.upstream(S, d["B"])).to(dev)
    mesh, verts, at = _atlas_mesh(d, dev)
    rgb, cov = _renderer(S, supersample=a).render(mesh, _cams(d, dev))
    need = RR.need_of(rgb)
    (rgb * g).sum().backward()
    at2 = d["atlas"].clone().requires_grad_(True)
    rgb_hi, mask_hi = RR._AtlasRenderFn.apply(d["verts"], at2, d["faces"], d["R"], d["T"], a * S)
    assert torch.equal(rgb_hi.detach(), ops.shade_atlas_fwd(d["frag"], d["atlas"])[0])
    rgb2, cov2 = ops.box_down_fwd(rgb_hi.detach(), a), ops.box_down_fwd(mask_hi, a)
    ga2 = ops.shade_atlas_bwd(ops.box_down_bwd(g, a), d["frag"], R, d["F"])
    assert rgb.shape == (d["B"], 3, S, S) and torch.equal(rgb.detach(), rgb2) and torch.equal(cov, cov2)
    assert torch.equal(at.grad, ga2) and float(ga2.abs().sum()) > 0 and verts.grad is None
    frac = cov[(cov > 0) & (cov < 1)]
    assert frac.numel() > 0 and set(np.unique(cov.cpu().numpy()).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert need is not None and torch.equal(need.bool(), cov[:, 0] > 0) and RR.flat_of(rgb) == (1.0, 1.0, 1.0)


def test_uv_and_vertex_meshes_take_the_launches_they_took(dev, ops, monkeypatch):
    """the same renderer on a TexturesUV and on a TexturesVertex mesh: the library calls of the parent commit, in their
    order (the lists tests/test_gpu_vcol.py pins); an atlas render is its own three launches forward, one scatter backward"""
    import utils as U
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    S, T = 24, 32
    d = _scene(dev, ops, "cow", S, 3)
    m = AR.cow()
    U.device = dev
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    tex = torch.from_numpy(np.random.default_rng(3).random((T, T, 3), dtype=np.float32))[None].to(dev).requires_grad_(True)
    verts = d["verts"].clone().requires_grad_(True)
    mesh = U.build_mesh(torch.from_numpy(m["verts_uvs"])[None].to(dev), torch.from_numpy(m["faces_uvs"].astype(np.int64))[None].to(dev),
                        tex, verts, d["faces"].to(torch.int64))
    (_renderer(S).render(mesh, _cams(d, dev))[0] * d["g"]).sum().backward()
    assert names == ["st3d_project_verts", "st3d_raster_fwd", "st3d_shade_fwd", "st3d_shade_bwd_det", "st3d_raster_bwd_det",
                     "st3d_project_verts_bwd"]
    names.clear()
    col = torch.rand(d["verts"].shape[0], 3, device=dev).requires_grad_(True)
    vverts = d["verts"].clone().requires_grad_(True)
    (_renderer(S).render(U.build_mesh_vertex(col, vverts, d["faces"].to(torch.int64)), _cams(d, dev))[0] * d["g"]).sum().backward()
    assert names == ["st3d_project_verts", "st3d_raster_fwd", "st3d_shade_vc_fwd", "st3d_shade_vc_bwd_det", "st3d_raster_bwd_det",
                     "st3d_project_verts_bwd"]
    names.clear()
    amesh, averts, at = _atlas_mesh(d, dev)
    (_renderer(S).render(amesh, _cams(d, dev))[0] * d["g"]).sum().backward()
    assert names == ["st3d_project_verts", "st3d_raster_fwd", "st3d_shade_atlas_fwd", "st3d_shade_atlas_bwd_det"]
    names.clear()
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    amesh, averts, at = _atlas_mesh(d, dev)
    (_renderer(S).render(amesh, _cams(d, dev))[0] * d["g"]).sum().backward()
    assert names == ["st3d_project_verts", "st3d_raster_fwd", "st3d_shade_atlas_fwd", "st3d_shade_atlas_bwd"]


def test_perceptual_loss_on_an_atlas_render(dev, ops, monkeypatch):
    """S = 64: the need and flat tags of an atlas render are true -- a loss that relies on them gives the bits of one that
    does not (fixed-point scatter)"""
    import losses as L
    import style_transfer as ST
    import utils as U
    import _scenes
    from st3d.render import flat_of, need_of
    U.device = ST.device = L.device = dev
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    S, R = 64, 3
    d = _scene(dev, ops, "cow", S, R)
    r, cams = _renderer(S), _cams(d, dev)
    vgg = U.get_vgg(seed=0)
    style = _scenes.style_at(1, S).to(dev).expand(d["B"], -1, -1, -1)
    with torch.no_grad():
        content, _ = U.render_meshes(r, _atlas_mesh(d, dev)[0], cams)

    def run(at_t):
        mesh, _, at = _atlas_mesh(d, dev, at_t.clone().requires_grad_(True), verts_grad=False)
        cur, mask = U.render_meshes(r, mesh, cams)
        assert need_of(cur) is not None and flat_of(cur) == (1.0, 1.0, 1.0)
        assert set(np.unique(mask.cpu().numpy()).tolist()) <= {0.0, 1.0}
        loss = L.compute_perceptual_loss(cur, content, style, vgg)
        loss.backward()
        return loss.detach().clone(), at.grad.clone()
    start = (d["atlas"] * 0.5 + 0.25)
    for k in ("ST3D_NEED_MASK", "ST3D_FLAT"):
        monkeypatch.delenv(k, raising=False)
    loss, gat = run(start)
    assert torch.isfinite(loss) and float(gat.abs().sum()) > 0
    for k in ("ST3D_NEED_MASK", "ST3D_FLAT"):
        monkeypatch.setenv(k, "0")
        loss0, gat0 = run(start)
        monkeypatch.delenv(k)
        assert torch.equal(loss, loss0) and torch.equal(gat, gat0), k


# ------------------------------------------------------------------ the CLI
@pytest.mark.parametrize("supersample", [1, 2])
def test_second_approach_on_a_mesh_without_uvs(dev, golden_dir, tmp_path, supersample):
    import second_approach as SA
    from PIL import Image
    from st3d import io as stio
    tmp = str(tmp_path)
    tea = np.load(os.path.join(golden_dir, "assets_teapot_mesh.npz"))
    assert tea["faces"].shape == (2464, 3)
    obj, style = os.path.join(tmp, "teapot.obj"), os.path.join(tmp, "style.png")
    stio.save_obj(obj, torch.from_numpy(tea["verts"]), torch.from_numpy(tea["faces"].astype(np.int64)))
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    out = os.path.join(tmp, "out")
    SA.main(["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "2", "--batch_size", "2", "--epochs", "3",
             "--seed", "0", "--save_every", "0", "--texture_atlas", "4", "--supersample", str(supersample), "--output_path", out])
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    losses = [float(line.split("Loss ")[1]) for line in lines[1:]]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    if supersample == 1:
        assert losses[-1] < losses[0]
    atlas = stio.load_atlas(os.path.join(out, "final_atlas.npy"))
    assert atlas.shape == (2464, 4, 4, 3) and float(atlas.min()) >= 0.0 and float(atlas.max()) <= 1.0
    vlines = [ln.split() for ln in open(os.path.join(out, "final.obj")) if ln.startswith("v ")]
    assert len(vlines) == 1292 and all(len(t) == 4 for t in vlines)              # geometry only
    clines = [ln.split() for ln in open(os.path.join(out, "final_colored.obj")) if ln.startswith("v ")]
    assert len(clines) == 3 * 2464 * 16 and all(len(t) == 7 for t in clines)     # x y z r g b: six numbers
    assert not os.path.exists(os.path.join(out, "final.mtl")) and not os.path.exists(os.path.join(out, "final.png"))
    assert os.path.exists(os.path.join(out, "final_render", "view_11.png"))
