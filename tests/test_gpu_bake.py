"""csrc/bake.hip and st3d/bake.py on the GPU against tests/_bakeref.py (fp64): the texel -> surface map, the bake fed the
device's own fragments, exact colours, the round trip on the cow against 30 steps of the existing fitting loop, and both
scripts end to end.

What is compared, and how closely.  A decision the restatement took without margin (the constants at the top of _bakeref.py)
is left out; the share left out is capped (1 % of the texels, 2 % of the texel-views).  The bounds are derived from the fp32
operation chain of bake_views_kernel, u = 2^-24, for scenes with |vertex coordinate| <= M = 1.05, |T| <= 3 and view depth
zv >= 1 (asserted per scene):
  P = sum b_i v_i                      3 products, 2 sums of magnitude <= M              |dP| <= 5 u M per component
  xv = P . R[:,0] + T_0 (yv, zv alike) inherited sqrt(3) |dP|, 3 products <= M, 3 sums <= V = sqrt(3) M + 3 = 4.82
                                       |dxv| <= (8.7 M + 3 M + 3 V) u                    <= 32 u
  x_ndc = (s xv) / zv                  s = 1.74, |x_ndc| <= 1.1 on screen, zv >= 1       |dx_ndc| <= (s + 1.1) 32 u + 2.2 u <= 96 u
  ix = ((1 - x_ndc) S - 1) / 2         three roundings of values <= 2.1 S                |dix| <= (96 + 2.1 + 4.2) u S / 2 <= 52 u S
so the pixel position is off by at most DELTA = 2 x 52 u S (both axes, 1-norm): 4e-4 pixel at S = 64, inside the 1e-3 margin
of rint / floor, hence the same pixels are read.  The colour then differs by at most 4 DELTA G, G the largest difference
between adjacent pixels of the images (a bilinear blend moves by G per pixel, renormalising over covered taps divides by a
sum >= 1/4).
  n = unit normal                      cross of two edge vectors: cancellation by kappa = |e1| |e2| / |e1 x e2| >= 1
  d = unit(C - P), C = -T R^T          |dC| <= 15 u, |d| >= 1
  c = |n . d|                          |dc| <= (58 + 5.2 kappa) u   (below the 1e-4 margin of min_cos up to kappa = 100)
  w = powf(c, power)                   |dw| <= power c^(power-1) |dc| + 4 ulp of w
"""
import os
import re

import numpy as np
import pytest
import torch

import _bakeref as BR
import _scenes

pytestmark = pytest.mark.gpu
I32, F32 = torch.int32, torch.float32
U_ = 2.0 ** -24
M_MAX, T_MAX, ZV_MIN = 1.05, 3.0, 1.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bake():
    from st3d import bake
    return bake


def _np(t):
    return t.detach().cpu().numpy()


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------- scenes
def _look_at(dist, elev, azim):
    from oracle import render_ref as RR
    return RR.look_at_view_transform(dist, np.asarray(elev, np.float64), np.asarray(azim, np.float64))


def _geometry(name):
    """-> verts (V,3) f32, faces (F,3) i32, verts_uvs (VT,2) f32, faces_uvs (F,3) i32, R (3,3,3), T (3,3)"""
    if name == "cow":
        cow = _scenes.load_asset("cow")
        R, T = _scenes.random_cameras(3, 0)
        return cow["verts"], cow["faces"].astype(np.int32), cow["verts_uvs"].astype(np.float32), cow["faces_uvs"].astype(np.int32), R, T
    uvs, fuv = BR.quad_chart()
    R, T = _look_at(2.5, [0.0, 25.0, -15.0], [0.0, 30.0, -40.0])
    if name == "facing":
        verts, faces = BR.facing_quad(0.0, 0.6)
        return verts, faces, uvs, fuv, R, T
    assert name == "occluded"                   # a near quad in front of a far one, a chart each
    near_v, faces = BR.facing_quad(0.0, 0.5)
    far_v, _ = BR.facing_quad(-1.0, 1.0)
    return (np.concatenate([near_v, far_v]), np.concatenate([faces, faces + 4]).astype(np.int32),
            np.concatenate([uvs * 0.45, uvs * 0.45 + 0.5]).astype(np.float32), np.concatenate([fuv, fuv + 4]).astype(np.int32), R, T)


SCENES = {"facing": (16, 16), "occluded": (32, 16), "cow": (64, 64)}        # name -> (S, T)
_CACHE = {}


def _scene(name, dev, bake):
    """the scene on the device with the device's own surface map and fragments, computed and downloaded once"""
    if name not in _CACHE:
        from st3d import ops
        S, T = SCENES[name]
        verts, faces, uvs, fuv, R, Tr = _geometry(name)
        assert np.abs(verts).max() <= M_MAX and np.abs(Tr).max() <= T_MAX
        d = dict(S=S, T=T, verts=_t(verts, dev), faces=_t(faces, dev), uvs=_t(uvs, dev), fuv=_t(fuv, dev), R=_t(R, dev), Tr=_t(Tr, dev))
        d["t2f"], d["tbary"] = bake.texel_surface(d["uvs"], d["fuv"], T)
        ndc = ops.project_verts(d["verts"], d["R"], d["Tr"])
        assert float(ndc[..., 2].min()) >= ZV_MIN
        p2f, zbuf, _, _ = ops.raster_fwd(ndc, d["faces"], S)
        d["p2f"], d["zbuf"] = p2f, zbuf
        d["host"] = dict(verts=verts, faces=faces, R=R, Tr=Tr, t2f=_np(d["t2f"]), tbary=_np(d["tbary"]), p2f=_np(p2f), zbuf=_np(zbuf))
        ramps, g = BR.ramp_images(3, S)
        noise = np.random.default_rng(7).random((3, 3, S, S)).astype(np.float32)
        d["images"] = {"ramp": (ramps, g), "noise": (noise, 1.0)}
        assert BR.adjacent_difference(noise) <= 1.0
        _CACHE[name] = d
    return _CACHE[name]


_REF = {}


def _reference(name, kind, B, mode, d):
    key = (name, kind, B, mode)
    if key not in _REF:
        h = d["host"]
        imgs = d["images"][kind][0]
        _REF[key] = BR.bake(h["verts"], h["faces"], h["t2f"], h["tbary"], h["R"][:B], h["Tr"][:B], imgs[:B], h["p2f"][:B],
                            h["zbuf"][:B], mode=mode)
    return _REF[key]


def _kappa(h):
    """per texel: |e1| |e2| / |e1 x e2| of its face (1 where t2f < 0)"""
    f = np.where(h["t2f"].reshape(-1) >= 0, h["t2f"].reshape(-1), 0)
    v = h["verts"].astype(np.float64)[h["faces"][f]]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.linalg.norm(np.cross(e1, e2), axis=-1)
    return np.linalg.norm(e1, axis=-1) * np.linalg.norm(e2, axis=-1) / np.maximum(n, 1e-300)


def _tolerances(detail, h, S, G_img, power):
    """-> per view and texel: the bound on |colour error| (scalar) and on |weight error| (B,N), from the module docstring"""
    delta = 2 * 52 * U_ * S
    tol_c = 4 * delta * G_img
    dc = (58 + 5.2 * _kappa(h))[None] * U_
    c, w = detail["c"], detail["w"]
    dw = 1.01 * power * np.power(np.maximum(c, 1e-30), power - 1) * dc + 8 * U_ * w
    return tol_c, np.where(detail["used"], dw, 0.0)


# ---------------------------------------------------------------------------- 1. the surface map
@pytest.mark.parametrize("pad", [0.0, 1.5, 3.0])
@pytest.mark.parametrize("chart,T", [("quad", 8), ("quad", 17), ("cow", 64)])
def test_surface_equals_the_restatement_where_it_decided_with_margin(bake, dev, chart, T, pad):
    if chart == "quad":
        uvs, fuv = BR.quad_chart()
    else:
        cow = _scenes.load_asset("cow")
        uvs, fuv = cow["verts_uvs"].astype(np.float32), cow["faces_uvs"].astype(np.int32)
    want_f, want_b, unsure = BR.surface(uvs, fuv, T, pad)
    d_uvs, d_fuv = _t(uvs, dev), _t(fuv, dev)
    t2f, tbary = bake.texel_surface(d_uvs, d_fuv, T, pad)
    assert t2f.dtype == I32 and tuple(t2f.shape) == (T, T) and tbary.dtype == F32 and tuple(tbary.shape) == (T, T, 3)
    got_f, got_b = _np(t2f), _np(tbary)
    share = unsure.mean()
    print(f"{chart} T={T} pad={pad}: {share:.5f} of the texels without margin, {np.mean(want_f >= 0):.3f} owned, "
          f"{np.sum(got_f != want_f)} faces differ in all, max |tbary diff| {np.abs(got_b - want_b).max():.3g}")
    assert share <= 0.01
    ok = ~unsure
    assert (want_f >= 0).sum() >= 8 and np.array_equal(got_f[ok], want_f[ok])
    both = ok & (want_f >= 0)
    assert np.abs(got_b - want_b)[both].max() <= 1e-5
    assert np.all(got_b[got_f < 0] == 0) and got_f.max() < fuv.shape[0] and got_f.min() >= -1
    again = bake.texel_surface(d_uvs, d_fuv, T, pad)
    assert torch.equal(again[0], t2f) and torch.equal(again[1].view(I32), tbary.view(I32))       # two runs, the same bits


def test_surface_skips_dead_faces_and_takes_mirrored_ones(bake, dev):
    T = 9
    uvs = np.array([[1, 1], [3, 3], [5, 5], [1, 4], [6, 2]], np.float32) / 8
    fuv = np.array([[0, 1, 2], [0, 3, 2], [0, 4, 2]], np.int32)               # collinear (dead); mirrored; not mirrored
    want_f, want_b, unsure = BR.surface(uvs, fuv, T, 1.5)
    t2f, tbary = bake.texel_surface(_t(uvs, dev), _t(fuv, dev), T, 1.5)
    assert set(np.unique(want_f)) == {-1, 1, 2}
    assert np.array_equal(_np(t2f), want_f)                                    # exact coordinates: ties and edges included
    assert np.abs(_np(tbary) - want_b).max() <= 1e-6


# ---------------------------------------------------------------------------- 2. the bake
def _run_bake(bake, d, kind, B, mode, acc=None, lo=0):
    imgs = _t(d["images"][kind][0][lo:B], d["verts"].device)
    return bake.bake_views(d["verts"], d["faces"], d["t2f"], d["tbary"], d["R"][lo:B].contiguous(), d["Tr"][lo:B].contiguous(), imgs,
                           d["p2f"][lo:B].contiguous(), d["zbuf"][lo:B].contiguous(), mode=mode, acc=acc)


@pytest.mark.parametrize("mode", ["mean", "best"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,kind", [("facing", "ramp"), ("occluded", "ramp"), ("cow", "ramp"), ("cow", "noise")])
def test_bake_equals_the_restatement_on_the_devices_own_fragments(bake, dev, name, kind, B, mode):
    d = _scene(name, dev, bake)
    S, T = d["S"], d["T"]
    want, unsure, detail = _reference(name, kind, B, mode, d)
    acc = _run_bake(bake, d, kind, B, mode)
    assert acc.dtype == F32 and tuple(acc.shape) == (T, T, 4)
    got = _np(acc).astype(np.float64).reshape(-1, 4)
    want, unsure = want.reshape(-1, 4), unsure.reshape(-1)
    valid = detail["valid"]
    share = detail["unsure"].sum() / max(B * valid.sum(), 1)
    tol_c, dw = _tolerances(detail, d["host"], S, d["images"][kind][1], 2.0)
    used, w, col = detail["used"], detail["w"], detail["colour"]
    if mode == "mean":
        tol_w = dw.sum(0) + B * U_ * want[:, 3]
        tol_rgb = ((w * tol_c)[..., None] + dw[..., None] * col + 2 * U_ * w[..., None] * col).sum(0) + B * U_ * want[:, :3]
    else:
        pick = np.where(used, w, -1.0).argmax(0)
        n = np.arange(w.shape[1])
        tol_w = dw[pick, n] + U_ * want[:, 3]
        tol_rgb = (w[pick, n] * tol_c)[:, None] + dw[pick, n][:, None] * col[pick, n] + 2 * U_ * want[:, :3]
    ok = ~unsure & valid
    err_w, err_rgb = np.abs(got[:, 3] - want[:, 3]), np.abs(got[:, :3] - want[:, :3])
    print(f"{name}/{kind} B={B} {mode}: {share:.4f} of the texel-views without margin, {used.sum()} used, {int((want[:, 3] > 0).sum())} "
          f"texels written; max weight error / bound {np.max(err_w[ok] / np.maximum(tol_w[ok], 1e-300)):.3g}, max colour error / "
          f"bound {np.max(err_rgb[ok] / np.maximum(tol_rgb[ok], 1e-300)):.3g}")
    assert share <= 0.02 and used.sum() >= 20
    assert np.array_equal(got[ok, 3] > 0, want[ok, 3] > 0)                     # the same texels written
    assert np.all(got[~valid] == 0)                                            # texels without a face are never touched
    assert np.all(err_w[ok] <= tol_w[ok]) and np.all(err_rgb[ok] <= tol_rgb[ok])


def test_the_far_quads_hidden_texels_stay_unwritten(bake, dev):
    d = _scene("occluded", dev, bake)
    h = d["host"]
    acc = _np(_run_bake(bake, d, "ramp", 1, "mean"))
    P = (h["tbary"][..., None].astype(np.float64) * h["verts"][h["faces"][np.where(h["t2f"] >= 0, h["t2f"], 0)]]).sum(-2)
    on_far, on_near = h["t2f"] >= 2, (h["t2f"] >= 0) & (h["t2f"] < 2)
    shadow = 0.5 * 3.5 / 2.5                    # the near quad's outline on the far plane, seen from (0, 0, 2.5)
    hidden = on_far & (np.abs(P[..., 0]) < shadow - 0.1) & (np.abs(P[..., 1]) < shadow - 0.1)
    seen = on_far & ((np.abs(P[..., 0]) > shadow + 0.1) | (np.abs(P[..., 1]) > shadow + 0.1))
    seen &= (np.abs(P[..., 0]) < 0.9) & (np.abs(P[..., 1]) < 0.9)      # (not on the far quad's own outline: a pixel is 0.13 wide there)
    inside = on_near & (np.abs(P[..., 0]) < 0.4) & (np.abs(P[..., 1]) < 0.4)
    assert hidden.sum() > 3 and seen.sum() > 3 and inside.sum() >= 6
    assert np.all(acc[hidden] == 0) and np.all(acc[seen][:, 3] > 0) and np.all(acc[inside][:, 3] > 0)


@pytest.mark.parametrize("mode", ["mean", "best"])
def test_a_continued_acc_equals_one_call_over_all_views(bake, dev, mode):
    d = _scene("cow", dev, bake)
    whole = _run_bake(bake, d, "noise", 3, mode)
    first = _run_bake(bake, d, "noise", 1, mode)
    kept = first.clone()
    out = _run_bake(bake, d, "noise", 3, mode, acc=first, lo=1)
    assert out is first and not torch.equal(out, kept)
    assert torch.equal(out.view(I32), whole.view(I32))                         # the views are walked in index order: the same bits
    assert torch.equal(_run_bake(bake, d, "noise", 3, mode).view(I32), whole.view(I32))


# ---------------------------------------------------------------------------- 3. exactness
@pytest.mark.parametrize("name", ["facing", "cow"])
def test_constant_images_bake_to_their_colour(bake, dev, name):
    d = _scene(name, dev, bake)
    S, T = d["S"], d["T"]
    colour = torch.tensor([0.9, 0.1, 0.3], device=dev)
    imgs = colour[None, :, None, None].expand(3, 3, S, S).contiguous()
    fallback = torch.full((T, T, 3), 0.5, device=dev)
    for mode in ("mean", "best"):
        acc = bake.bake_views(d["verts"], d["faces"], d["t2f"], d["tbary"], d["R"], d["Tr"], imgs, d["p2f"], d["zbuf"], mode=mode)
        tex = bake.baked_texture(acc, fallback)
        written = acc[..., 3] > 0
        assert int(written.sum()) >= 20
        assert float((tex[written] - colour).abs().max()) <= 1e-6
        assert torch.equal(tex[~written], fallback[~written])


def test_views_of_different_constants_blend_with_the_restatements_weights(bake, dev):
    d = _scene("cow", dev, bake)
    S, T, h = d["S"], d["T"], d["host"]
    colours = np.array([[0.9, 0.1, 0.3], [0.2, 0.8, 0.4], [0.5, 0.5, 0.7]], np.float32)
    imgs = np.broadcast_to(colours[:, :, None, None], (3, 3, S, S)).copy()
    want, unsure, detail = BR.bake(h["verts"], h["faces"], h["t2f"], h["tbary"], h["R"], h["Tr"], imgs, h["p2f"], h["zbuf"])
    acc = bake.bake_views(d["verts"], d["faces"], d["t2f"], d["tbary"], d["R"], d["Tr"], _t(imgs, dev), d["p2f"], d["zbuf"])
    tex = _np(bake.baked_texture(acc, torch.zeros((T, T, 3), device=dev))).astype(np.float64).reshape(-1, 3)
    w = detail["w"]
    total = w.sum(0)
    ok = ~unsure.reshape(-1) & (total > 0)
    blend = np.einsum("bn,bc->nc", w, colours.astype(np.float64)) / np.where(total > 0, total, 1.0)[:, None]
    _, dw = _tolerances(detail, h, S, 0.0, 2.0)
    # d(sum w c / sum w) <= sum |dw_b| |c_b - blend| / sum w, |c_b - blend| <= 0.7 here; + the roundings of 3 products, 2 sums, 1 division
    tol = dw.sum(0) / np.where(total > 0, total, 1.0) * 0.7 + 8 * U_
    err = np.abs(tex - blend).max(-1)
    print(f"different constants: {ok.sum()} texels compared, {int((w > 0).sum(0).max())} views at most, max error / bound "
          f"{np.max(err[ok] / tol[ok]):.3g}")
    assert ok.sum() >= 500 and int(((w > 0).sum(0) >= 2).sum()) >= 50 and np.all(err[ok] <= tol[ok])


# ---------------------------------------------------------------------------- 4. the round trip on the cow
def test_round_trip_on_the_cow_beats_thirty_fitting_steps(bake, dev):
    """render 8 views of the cow with its own map, bake them into a grey map and re-render: the masked MSE against the
    original renders is below what 30 steps of the existing phase-B loop (Adam, lr 0.01) reach from the same grey map.
    (A CPU prototype of the rule had 0.0035 against 0.020.)"""
    import losses as L
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    S = T = 64
    cow = _scenes.load_asset("cow")
    R, Tr = _scenes.random_cameras(8, 0)
    mesh, renderer, cams = _scenes.device_scene(U, dev, cow["verts"], cow["faces"], cow["verts_uvs"], cow["faces_uvs"],
                                                _scenes.texture_at(cow, T), R, Tr, S)
    with torch.no_grad():
        targets, _ = U.render_meshes(renderer, mesh, cams)
    tex = mesh.textures
    grey = torch.full((1, T, T, 3), 0.5, device=dev)
    grey_mesh = U.build_mesh(tex.verts_uvs_padded(), tex.faces_uvs_padded(), grey, mesh.verts_packed(), mesh.faces_packed())

    def error(texture_map):
        with torch.no_grad():
            m = U.build_mesh(tex.verts_uvs_padded(), tex.faces_uvs_padded(), texture_map, mesh.verts_packed(), mesh.faces_packed())
            img, cov = U.render_meshes(renderer, m, cams)
            return float(L.compute_first_approach_loss(rendered=img, masks=cov, target_rendered=targets, verts=None,
                                                       target_verts=None, mesh=m, weights={}, opt_type='texture'))
    baked, acc = U.bake_texture(grey_mesh, targets, cams, S)
    assert tuple(baked.shape) == (T, T, 3) and tuple(acc.shape) == (T, T, 4)
    unwritten = acc[..., 3] == 0
    assert int(unwritten.sum()) > 0 and torch.equal(baked[unwritten], grey[0][unwritten])       # the fallback, bit for bit
    assert torch.equal(grey, torch.full_like(grey, 0.5))                                        # the mesh's own map is not written
    e_grey, e_bake = error(grey), error(baked[None])
    opt = U.setup_optimizations("texture", grey_mesh, 0.01)
    for _ in range(30):
        opt["optimizer"].zero_grad()
        m = U.build_mesh(opt["verts_uvs"], opt["faces_uvs"], opt["texture_map"], opt["verts"], opt["faces"])
        img, cov = U.render_meshes(renderer, m, cams)
        loss = L.compute_first_approach_loss(rendered=img, masks=cov, target_rendered=targets, verts=opt["verts"],
                                             target_verts=mesh.verts_packed(), mesh=m, weights={}, opt_type='texture')
        loss.backward()
        opt["optimizer"].step()
    e_adam = error(opt["texture_map"].detach())
    print(f"round trip: grey {e_grey:.5f}, baked {e_bake:.5f}, 30 Adam steps {e_adam:.5f}, {int((~unwritten).sum())} texels written")
    assert e_bake < e_adam < e_grey


# ---------------------------------------------------------------------------- 5. the scripts
def _write_cow_assets(tmp, cow, golden_dir, tex_size=64):
    from PIL import Image
    from st3d import io as stio
    tex = torch.from_numpy(cow["texture_u8"][::1024 // tex_size, ::1024 // tex_size].copy()).float() / 255
    obj = os.path.join(tmp, "cow.obj")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    style = os.path.join(tmp, "style.png")
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    return obj, style


def _final_map(folder):
    from st3d import io as stio
    _, _, aux = stio.load_obj(os.path.join(folder, "final.obj"))
    return next(iter(aux.texture_images.values()))


@pytest.mark.parametrize("script", ["first_approach", "third_approach"])
def test_script_bakes_end_to_end_and_is_unchanged_with_the_flag_off(script, bake, dev, cow, golden_dir, tmp_path, capsys, monkeypatch):
    import importlib
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import cli
    U.device = ST.device = L.device = dev
    mod = importlib.import_module(script)
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2",
              "--n_style_transfer_steps", "2", "--seed", "0"] + (["--n_rounds", "1"] if script == "third_approach" else [])
    accs = []
    real = bake.bake_views

    def spy(*a, **k):
        out = real(*a, **k)
        accs.append(out.clone())
        return out
    monkeypatch.setattr(bake, "bake_views", spy)
    on = str(tmp_path / "on")
    capsys.readouterr()
    mod.main(common + ["--bake_texture", "mean", "--n_mse_steps", "0", "--output_path", on])
    said = capsys.readouterr().out
    line = re.search(r"Bake \((?:round 0, )?batch 0\): (\d+) of 4096 texels written from 2 views \(--bake_texture mean\)", said)
    assert line and len(accs) == 1, said
    written = _np(accs[0][..., 3] > 0)
    assert int(line.group(1)) == written.sum() > 200
    loaded = cli.load_scene(obj, 64, True, dev)[4]
    want = bake.baked_texture(accs[0], loaded[0].contiguous())
    final = _final_map(on)
    as_saved = lambda t: (t.detach().cpu().clamp(0, 1) * 255.0).round().to(torch.uint8).numpy()
    assert np.array_equal(as_saved(final), as_saved(want))                     # a pure bake: the exported map is the baked one
    changed = (as_saved(final) != as_saved(loaded[0])).any(-1)
    # ... and differs from the loaded one on written texels only (two phase-A steps leave the views close to the content
    # renders, so a written texel may well round to the byte it had)
    assert not changed[~written].any() and changed[written].sum() > 0
    assert open(os.path.join(on, "log.txt")).read() == "Logger:\n" or script == "third_approach"
    monkeypatch.setattr(bake, "bake_views", real)
    off, plain = str(tmp_path / "off"), str(tmp_path / "plain")
    mod.main(common + ["--bake_texture", "off", "--n_mse_steps", "2", "--output_path", off])
    mod.main(common + ["--n_mse_steps", "2", "--output_path", plain])
    assert "Bake (" not in capsys.readouterr().out and len(accs) == 1
    assert open(os.path.join(off, "log.txt"), "rb").read() == open(os.path.join(plain, "log.txt"), "rb").read()
    assert len(open(os.path.join(off, "log.txt")).read().splitlines()) >= 2
    assert np.array_equal(as_saved(_final_map(off)), as_saved(_final_map(plain)))
