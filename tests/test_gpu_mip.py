"""Mip-mapped trilinear texture sampling on the GPU (csrc/mipmap.hip) against its numpy restatement (tests/_mipref.py):
the chain and its adjoint bit for bit, the level of detail against the fp64 formula on the GPU's own fragments, the sample
and its backward stage-wise (the restatement gets the GPU's fragments and lambda plane) at the bars test_gpu_kernels.py
holds the plain kernels to, lambda == 0 against the plain kernels bit for bit, the fixed-point scatter, the renderer's
keyword and one CLI run.

Shapes: cow, B = 2, the five (S, T, L) of _mipref.CASES -- S a multiple of the 16-pixel tile or not, T a multiple of the
32-texel build tile or not, L from 2 to the full chain; every case holds pixels at lambda = 0 (one level read), between two
levels, and -- for L <= 3 -- clamped at the coarsest level (asserted on the GPU's own plane)."""
import os

import numpy as np
import pytest
import torch

import _mipref as M

pytestmark = pytest.mark.gpu

# the largest |lambda_gpu - lambda_fp64| over the five cases (bias 0, +0.75 and -0.75) measured on MI355X: the kernel
# evaluates the formula in fp64 and stores fp32, half an ulp of a lambda in [2, 4) is 1.2e-7.  The bar is 4 x the measured
# value
LOD_MEASURED = 1.4282e-7
LOD_BAR = 4 * LOD_MEASURED


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


def _scene(dev, ops, S, T):
    """the shared scene on the device: mesh, texture, upstream gradient, projected vertices and the GPU's fragments"""
    if (S, T) not in _SCENES:
        import _scenes
        m = _scenes.load_asset("cow")
        Rn, Tn = M.cameras()
        d = dict(mesh=m, tex_np=M.texture(T), g_np=M.upstream(S), R_np=Rn, T_np=Tn)
        d["verts"] = torch.from_numpy(m["verts"]).to(dev)
        d["faces"] = torch.from_numpy(m["faces"]).to(dev).to(torch.int32).contiguous()
        d["uvs"] = torch.from_numpy(m["verts_uvs"]).to(dev)
        d["fuv"] = torch.from_numpy(m["faces_uvs"]).to(dev).to(torch.int32).contiguous()
        d["tex"], d["g"] = torch.tensor(d["tex_np"]).to(dev), torch.tensor(d["g_np"]).to(dev)
        d["R"], d["T"] = torch.tensor(Rn).to(dev), torch.tensor(Tn).to(dev)
        d["ndc"] = ops.project_verts(d["verts"], d["R"], d["T"])
        d["frag"] = ops.raster_fwd(d["ndc"], d["faces"], S)
        d["frag_np"] = [tuple(x[b].cpu().numpy() for x in d["frag"]) for b in range(M.B)]
        d["ndc_np"] = d["ndc"].cpu().numpy()
        _SCENES[(S, T)] = d
    return _SCENES[(S, T)]


def _lod(dev, ops, S, T, L, bias=0.0):
    d = _scene(dev, ops, S, T)
    return ops.mip_lod(d["frag"], d["ndc"], d["faces"], d["uvs"], d["fuv"], T, L, bias)


def _reference(dev, ops, S, T, L):
    """the restatement on the GPU's fragments and the GPU's lambda plane, computed once per case and left unchanged.  It is
    evaluated as the CPU oracle the bars come from is: every operation the kernels do in fp32 rounded to fp32 in the same
    order, the scatter and the uv gradient accumulated in fp64 (at lambda == 0 it IS that oracle, tests/test_mip_ref.py).
    The all-fp64 evaluation differs from any fp32 evaluation of uv_footprint by ulp(ix) times the texel slope -- 3.5e-6 on
    rgb at T = 40 (ulp 3.8e-6 above ix = 32, random texels), the plain kernel included -- and is printed for the record."""
    if (S, T, L) not in _REFS:
        from oracle import render_ref as rr
        d = _scene(dev, ops, S, T)
        m = d["mesh"]
        lam = _lod(dev, ops, S, T, L).cpu().numpy()
        pyr = M.pack(M.build(d["tex_np"], L, np.float32))
        rgb, rgb64, mask, gbary = [], [], [], []
        gpyr = np.zeros(M.numel(T, L), np.float64)
        gverts = np.zeros(m["verts"].shape, np.float64)
        for b in range(M.B):
            fr = d["frag_np"][b]
            c, k = M.shade_fwd(fr, m["verts_uvs"], m["faces_uvs"], pyr, T, L, lam[b], np.float32)
            rgb.append(c)
            mask.append(k)
            rgb64.append(M.shade_fwd(fr, m["verts_uvs"], m["faces_uvs"], pyr.astype(np.float64), T, L, lam[b])[0])
            _, guv = M.shade_bwd(d["g_np"][b], fr, m["verts_uvs"], m["faces_uvs"], pyr, T, L, lam[b], np.float32, gpyr=gpyr)
            gb = rr.uv_to_bary_grad(guv.astype(np.float32), fr[0], m["verts_uvs"], m["faces_uvs"])
            gbary.append(gb)
            gndc = rr.raster_bwd(gb, fr[0], d["ndc_np"][b], m["faces"])
            rr.project_verts_bwd(m["verts"], d["R_np"][b], d["T_np"][b], gndc, gverts)
        ref = dict(lam=lam, rgb=np.stack(rgb), rgb64=np.stack(rgb64), mask=np.stack(mask), gpyr=gpyr, gtex=M.fold(gpyr, T, L), gbary=np.stack(gbary),
                   gverts=gverts)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[(S, T, L)] = ref
    return _REFS[(S, T, L)]


def _assert_classes(d, lam, L):
    """the case is not degenerate: pixels reading one level, pixels between two, and (L <= 3) pixels clamped at the coarsest"""
    cov = np.stack([f[0] >= 0 for f in d["frag_np"]])
    n, zero, frac, top = M.classes(lam, cov, L)
    print(f"covered {n}: lambda = 0 on {zero}, fractional on {frac}, clamped on {top}")
    assert zero >= 10 and frac >= 80
    if L <= 3:
        assert top >= 10
    assert not np.asarray(lam)[~cov].any()


# ------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("T,L", [(6, 2), (32, 2), (32, 5), (40, 4), (48, 3), (48, 5), (64, 2), (64, 6), (256, 8)])
def test_build_and_adjoint_are_bitwise_the_ordered_fp32_restatement(dev, ops, T, L):
    """(256, 8): the one-workgroup tail of the build takes levels 6 and 7; every other shape is the tile kernel alone"""
    rng = np.random.default_rng(1000 * T + L)
    tex = rng.standard_normal((T, T, 3)).astype(np.float32)
    pyr = ops.mip_build(torch.from_numpy(tex).to(dev), L)
    assert pyr.shape == (M.numel(T, L),) == (ops.mip_numel(T, L),)
    np.testing.assert_array_equal(pyr.cpu().numpy(), M.pack(M.build(tex, L)))
    g = rng.standard_normal(M.numel(T, L)).astype(np.float32)
    want = M.adjoint(M.unpack(g, T, L))
    got = ops.mip_adjoint(torch.from_numpy(g).to(dev), T, L)
    assert got.shape == (T, T, 3)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    base = rng.standard_normal((T, T, 3)).astype(np.float32)
    acc = ops.mip_adjoint(torch.from_numpy(g).to(dev), T, L, out=torch.from_numpy(base).to(dev))
    np.testing.assert_array_equal(acc.cpu().numpy(), base + want)
    # a NaN texel stays inside the blocks above it
    tex[T // 2, 1, 2] = np.nan
    bad = M.unpack(ops.mip_build(torch.from_numpy(tex).to(dev), L).cpu().numpy(), T, L)
    for l, lv in enumerate(bad):
        hit = np.argwhere(np.isnan(lv))
        assert hit.tolist() == [[(T // 2) >> l, 1 >> l, 2]], l


# ------------------------------------------------------------------ 2. the level of detail
def test_lod_against_the_fp64_formula_on_the_gpus_fragments(dev, ops):
    worst = 0.0
    for S, T, L in M.CASES:
        d = _scene(dev, ops, S, T)
        lam = _lod(dev, ops, S, T, L).cpu().numpy()
        assert lam.shape == (M.B, S, S) and lam.min() >= 0 and lam.max() <= L - 1
        _assert_classes(d, lam, L)
        m = d["mesh"]
        for b in range(M.B):
            ref = M.lod(d["frag_np"][b], d["ndc_np"][b], m["faces"], m["verts_uvs"], m["faces_uvs"], T, L)
            err = float(np.abs(lam[b] - ref).max())
            worst = max(worst, err)
            # a pixel is in the same class on both sides unless the formula sits within the error of a class boundary
            flip = (lam[b] == 0) != (ref == 0)
            assert not (flip & (np.abs(ref) > LOD_BAR)).any()
        for bias in (0.75, -0.75):
            lb = _lod(dev, ops, S, T, L, bias).cpu().numpy()
            ref = np.stack([M.lod(d["frag_np"][b], d["ndc_np"][b], m["faces"], m["verts_uvs"], m["faces_uvs"], T, L, bias)
                            for b in range(M.B)])
            worst = max(worst, float(np.abs(lb - ref).max()))
            assert ((lb == 0) | (lam > 0)).all()           # a bias lifts no pixel whose rho is <= 1
    print(f"lambda: largest |gpu - fp64| over the five cases {worst:.3e} (measured {LOD_MEASURED:.1e}, bar {LOD_BAR:.1e})")
    assert LOD_BAR <= 1e-3 and LOD_BAR <= 4 * LOD_MEASURED * (1 + 1e-9)
    assert worst <= LOD_BAR


# ------------------------------------------------------------------ 3. the sample and its backward, stage-wise
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "fixed"])
@pytest.mark.parametrize("S,T,L", M.CASES)
def test_sampling_stagewise(dev, ops, monkeypatch, S, T, L, det):
    monkeypatch.setattr(ops, "_DETERMINISTIC", det)
    d, ref = _scene(dev, ops, S, T), _reference(dev, ops, S, T, L)
    _assert_classes(d, ref["lam"], L)
    lod = torch.tensor(ref["lam"]).to(dev)
    pyr = ops.mip_build(d["tex"], L)
    rgb, mask = ops.shade_mip_fwd(d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L)
    err = np.abs(rgb.cpu().numpy() - ref["rgb"]).max()
    print(f"rgb max abs err {err:.3e} (bound 2e-6); against the all-fp64 evaluation {np.abs(rgb.cpu().numpy() - ref['rgb64']).max():.3e}")
    assert err <= 2e-6
    np.testing.assert_array_equal(mask.cpu().numpy(), ref["mask"])
    assert (rgb.permute(0, 2, 3, 1)[mask[:, 0] == 0] == 1.0).all()
    gt, guv, gbary, glev = ops.shade_mip_bwd(d["g"], d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L, want_uv=True, want_bary=True,
                                             want_levels=True)
    assert gt.shape == (T, T, 3) and guv.shape == (M.B, S, S, 2) and gbary.shape == (M.B, S, S, 3)
    _scale_close(gt, ref["gtex"], 1e-5, "grad_texture")
    _scale_close(glev, ref["gpyr"], 1e-5, "per-level gradient")
    off = M.texel_offsets(T, L) * 3
    for l in range(L):                                      # (L = 6 at T = 64: lambda stays below 5, the last block is empty)
        assert bool(glev[off[l]:off[l + 1]].any()) == bool(ref["gpyr"][off[l]:off[l + 1]].any()), l
    _scale_close(gbary, ref["gbary"], 1e-4, "grad_bary")
    gverts = ops.project_verts_bwd(d["verts"], d["R"], d["T"], ops.raster_bwd(gbary, d["frag"][0], d["ndc"], d["faces"]))
    rel = np.linalg.norm(gverts.double().cpu().numpy() - ref["gverts"]) / np.linalg.norm(ref["gverts"])
    print(f"grad_verts relative L2 {rel:.3e} (bound 2e-4)")
    assert rel <= 2e-4
    # accumulation into an existing gradient; vertices only
    base = torch.full((T, T, 3), 0.5, device=dev)
    acc = ops.shade_mip_bwd(d["g"], d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L, grad_texture=base.clone())
    _scale_close(acc - base, ref["gtex"], 1e-5, "accumulated grad_texture")
    only = ops.shade_mip_bwd(d["g"], d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L, want_bary=True, want_texture=False)
    assert only[0] is None and torch.equal(only[1], gbary)


# ------------------------------------------------------------------ 4. lambda == 0 is the plain kernel
@pytest.mark.parametrize("S,T,L", M.CASES)
def test_bias_minus_32_is_the_plain_kernels_bit_for_bit(dev, ops, monkeypatch, S, T, L):
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, S, T)
    lod = _lod(dev, ops, S, T, L, -32.0)
    assert not lod.any()
    pyr = ops.mip_build(d["tex"], L)
    rgb, mask = ops.shade_mip_fwd(d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L)
    rgb0, mask0 = ops.shade_fwd(d["frag"], d["uvs"], d["fuv"], d["tex"])
    assert torch.equal(rgb, rgb0) and torch.equal(mask, mask0)
    gt = ops.shade_mip_bwd(d["g"], d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L)
    gt0 = ops.shade_bwd(d["g"], d["frag"], d["uvs"], d["fuv"], d["tex"])
    assert torch.equal(gt, gt0) and float(gt.abs().sum()) > 0


@pytest.mark.parametrize("S,T,L", M.CASES)
def test_a_constant_texture_renders_as_the_plain_kernel_at_every_lambda(dev, ops, S, T, L):
    d = _scene(dev, ops, S, T)
    const = torch.tensor([0.25, 0.5, 0.8125], device=dev).expand(T, T, 3).contiguous()
    pyr = ops.mip_build(const, L)
    assert torch.equal(pyr.view(-1, 3), const[0, 0].expand(pyr.numel() // 3, 3))       # (the 2 x 2 mean of equal values is exact)
    want, mask0 = ops.shade_fwd(d["frag"], d["uvs"], d["fuv"], const)
    planes = [_lod(dev, ops, S, T, L), _lod(dev, ops, S, T, L, 1.5)]
    planes += [torch.full((M.B, S, S), v, device=dev) for v in (0.0, 0.5, 1.0, L - 1.5, float(L - 1))]
    for lod in planes:
        rgb, mask = ops.shade_mip_fwd(d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L)
        assert float((rgb - want).abs().max()) <= 1e-6 and torch.equal(mask, mask0)


# ------------------------------------------------------------------ 5. fixed point
@pytest.mark.parametrize("S,T,L", M.CASES)
def test_fixed_point_backward_is_reproducible_and_loud(dev, ops, monkeypatch, S, T, L):
    """Uncovered pixels deposit nothing: what a loss writes there reaches the result only through the bound, the sum of
    |grad_rgb|, that is through the power-of-two scale 2^(60 - e).  A deposit is an fp32 number: its product with the scale
    is an integer, at either scale, unless it lies below 2^-36 of the bound, so finite values of the gradient's own size on
    the background change no bit."""
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, S, T)
    lod, pyr = _lod(dev, ops, S, T, L), ops.mip_build(d["tex"], L)

    def run(grad):
        return ops.shade_mip_bwd(grad, d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L, want_bary=True)
    gt, gbary = run(d["g"])
    gt_again, gbary_again = run(d["g"])
    assert torch.equal(gt, gt_again) and torch.equal(gbary, gbary_again) and float(gt.abs().sum()) > 0
    off = (d["frag"][0] < 0)[:, None].expand(-1, 3, -1, -1)
    noisy = torch.where(off, torch.randn(d["g"].shape, generator=torch.Generator().manual_seed(S)).to(dev), d["g"])
    assert not torch.equal(noisy, d["g"])
    gt_noisy, gbary_noisy = run(noisy)
    assert torch.equal(gt_noisy, gt) and torch.equal(gbary_noisy, gbary)
    y, x = (int(i) for i in (~off[1, 0]).nonzero()[0])
    bad = d["g"].clone()
    bad[1, 2, y, x] = float("nan")
    assert torch.isnan(run(bad)[0]).all()


# ------------------------------------------------------------------ 6. the public API
def _renderer(S, **kw):
    from st3d.render import MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    return MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S, **kw)), SoftPhongShader())


def _mesh(d, dev, texture=None):
    import utils as U
    U.device = dev
    m = d["mesh"]
    tex = d["tex"].clone()[None].requires_grad_(True) if texture is None else texture
    verts = torch.from_numpy(m["verts"]).to(dev).requires_grad_(True)
    mesh = U.build_mesh(torch.from_numpy(m["verts_uvs"])[None].to(dev), torch.from_numpy(m["faces_uvs"].astype(np.int64))[None].to(dev),
                        tex, verts, torch.from_numpy(m["faces"].astype(np.int64)).to(dev))
    return mesh, verts, tex


def _step(renderer, d, dev):
    from st3d.render import FoVPerspectiveCameras, need_of
    mesh, verts, tex = _mesh(d, dev)
    rgb, cov = renderer.render(mesh, FoVPerspectiveCameras(R=d["R"], T=d["T"], device=dev))
    need = need_of(rgb)
    (rgb * d["g"]).sum().backward()
    return rgb.detach(), cov.detach(), need, tex.grad[0], verts.grad


@pytest.mark.parametrize("S,T", [(24, 64), (17, 48)])
def test_renderer_keyword_is_the_stagewise_composition(dev, ops, monkeypatch, S, T):
    """texture_mip_levels = 0 (the full chain: L = 6 under 64, 5 under 48): one texture-and-vertex backward through
    MeshRenderer against the ops calls it is made of -- fixed point, so bit for bit"""
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, S, T)
    L = ops.check_mip(0, T)
    assert L == M.max_levels(T)
    rgb, cov, need, gtex, gverts = _step(_renderer(S, texture_mip_levels=0, texture_lod_bias=0.25), d, dev)
    lod, pyr = _lod(dev, ops, S, T, L, 0.25), ops.mip_build(d["tex"], L)
    rgb0, mask0 = ops.shade_mip_fwd(d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L)
    gt0, gbary0 = ops.shade_mip_bwd(d["g"], d["frag"], d["uvs"], d["fuv"], pyr, lod, T, L, want_bary=True)
    gv0 = ops.project_verts_bwd(d["verts"], d["R"], d["T"], ops.raster_bwd(gbary0, d["frag"][0], d["ndc"], d["faces"]))
    assert torch.equal(rgb, rgb0) and torch.equal(cov, mask0) and torch.equal(gtex, gt0) and torch.equal(gverts, gv0)
    assert gtex.shape == (T, T, 3) and float(gtex.abs().sum()) > 0 and float(gverts.abs().sum()) > 0
    assert need is not None and torch.equal(need, (d["frag"][0] >= 0).view(torch.uint8))
    plain = _step(_renderer(S), d, dev)
    assert not torch.equal(rgb, plain[0]) and torch.equal(cov, plain[1])
    # more texels carry gradient than under the plain sampling
    assert int((gtex.abs().sum(-1) > 0).sum()) > int((plain[3].abs().sum(-1) > 0).sum())


@pytest.mark.parametrize("S,T", [(17, 48), (24, 64)])
def test_mip_levels_one_is_the_renderer_without_the_keyword(dev, ops, monkeypatch, S, T):
    monkeypatch.setattr(ops, "_DETERMINISTIC", True)
    d = _scene(dev, ops, S, T)
    got, ref = _step(_renderer(S, texture_mip_levels=1, texture_lod_bias=0.0), d, dev), _step(_renderer(S), d, dev)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def test_texture_pyramid_and_an_odd_side(dev, ops):
    """the pyramid parametrisation gets its gradient on every level through the mip-mapped render; texture_mip_levels = 0
    under an odd side is the plain render"""
    from st3d.render import FoVPerspectiveCameras
    from st3d.texpyr import TexturePyramid
    S, T = 24, 64
    d = _scene(dev, ops, S, T)
    cams = FoVPerspectiveCameras(R=d["R"], T=d["T"], device=dev)
    par = TexturePyramid(d["tex"].clone()[None], 3)
    mesh, verts, _ = _mesh(d, dev, par.texture())
    rgb, cov = _renderer(S, texture_mip_levels=0).render(mesh, cams)
    assert set(np.unique(cov.cpu().numpy()).tolist()) == {0.0, 1.0}
    (rgb * d["g"]).sum().backward()
    for l in range(par.levels):
        gl = par.params.grad[par.offsets[l]:par.offsets[l + 1]]
        assert torch.isfinite(gl).all() and float(gl.abs().sum()) > 0, l
    assert torch.isfinite(verts.grad).all()
    odd = dict(_scene(dev, ops, S, T), tex=torch.tensor(M.texture(37)).to(dev))
    got, ref = _step(_renderer(S, texture_mip_levels=0), odd, dev), _step(_renderer(S), odd, dev)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 7. the CLI
def test_second_approach_with_the_full_chain(dev, cow, golden_dir, tmp_path):
    import second_approach as SA
    from PIL import Image
    from st3d import io as stio
    tmp = str(tmp_path)
    tex = torch.from_numpy(cow["texture_u8"][::16, ::16].copy()).float() / 255
    obj, style = os.path.join(tmp, "cow.obj"), os.path.join(tmp, "style.png")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    out = os.path.join(tmp, "out")
    SA.main(["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "2", "--batch_size", "2", "--epochs", "3",
             "--seed", "0", "--save_every", "0", "--texture_mip_levels", "0", "--output_path", out])
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    losses = [float(line.split("Loss ")[1]) for line in lines[1:]]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert os.path.exists(os.path.join(out, "final.obj"))
