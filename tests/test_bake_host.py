"""Host side of --bake_texture: the fp64 restatement (tests/_bakeref.py) on cases with a known answer, that it leaves out few
enough decisions on the scenes the GPU tests use (rasterised by the CPU oracle), the C ABI's refusals (which launch nothing),
the wrappers' validation and their refusal of CPU tensors, the flags on first_approach / third_approach and what check_args
rules out.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _bakeref as BR
import _scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_bake_workspace_bytes", "st3d_bake_surface", "st3d_bake_views", "st3d_bake_resolve")


# ---------------------------------------------------------------------------- 1. the restatement on analytic cases
def _rect_chart(T, x0, y0, x1, y1):
    """an axis-parallel rectangle [x0, x1] x [y0, y1] in texel units as two triangles split along the (x0,y0)-(x1,y1) diagonal"""
    s = float(T - 1)
    uvs = np.array([[x0 / s, y0 / s], [x1 / s, y0 / s], [x1 / s, y1 / s], [x0 / s, y1 / s]], np.float64).astype(np.float32)
    return uvs, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


@pytest.mark.parametrize("pad", [0.0, 1.5, 3.0])
def test_one_quad_chart_at_8_is_the_clamp_onto_the_rectangle(pad):
    T = 8
    uvs, fuv = _rect_chart(T, 1.25, 2.4, 4.75, 5.3)                   # no texel at exactly pad from it, for any of the pads
    t2f, tbary, unsure = BR.surface(uvs, fuv, T, pad)
    pos = BR.texel_uv_units(T)
    near = np.stack([np.clip(pos[..., 0], 1.25, 4.75), np.clip(pos[..., 1], 2.4, 5.3)], -1)
    d2 = ((pos - near) ** 2).sum(-1)
    want = d2 <= pad * pad
    assert np.array_equal(t2f >= 0, want) and (want.sum() == 9 if pad == 0 else 9 < want.sum() <= 64)  # x in 2..4, y in 3..5
    corners = (uvs.astype(np.float64) * (T - 1))[fuv[np.where(want, t2f, 0)]]             # (T,T,3,2)
    point = (tbary[..., None] * corners).sum(-2)
    assert np.abs(point - near)[want].max() <= 1e-6                    # the barycentrics name the closest point (fp32 UVs)
    assert np.abs(tbary.sum(-1) - 1)[want].max() <= 1e-12 and tbary.min() >= 0 and np.all(tbary[~want] == 0)
    assert not unsure[d2 > (pad + 1) ** 2].any()                       # far from every triangle nothing is in doubt


def test_a_mirrored_triangle_counts_like_its_twin():
    T = 8
    uvs = np.array([[1.5, 1.5], [5.5, 2.0], [3.0, 5.5]], np.float64).astype(np.float32) / 7
    a, ba, _ = BR.surface(uvs, np.array([[0, 1, 2]]), T, 1.5)
    b, bb, _ = BR.surface(uvs, np.array([[0, 2, 1]]), T, 1.5)          # negative UV area
    assert (a >= 0).sum() > 10 and np.array_equal(a, b)
    assert np.abs(ba - bb[..., [0, 2, 1]]).max() <= 1e-12
    inside = np.zeros((T, T), bool)
    inside[T - 1 - 3, 3] = inside[T - 1 - 2, 3] = inside[T - 1 - 4, 3] = True            # (3,3), (3,2), (3,4) lie inside
    assert np.all(a[inside] == 0) and np.all(ba[inside] > 0)


def test_a_zero_area_triangle_is_skipped():
    T = 8
    uvs = np.array([[1, 1], [3, 3], [5, 5], [1, 4], [1, 4]], np.float32) / 7
    t2f, tbary, _ = BR.surface(uvs, np.array([[0, 1, 2], [0, 3, 4]]), T, 1.5)      # collinear; two corners coincide
    assert np.all(t2f == -1) and np.all(tbary == 0)
    t2f, _, _ = BR.surface(uvs, np.array([[0, 1, 2], [0, 2, 3]]), T, 0.0)
    assert set(np.unique(t2f)) == {-1, 1}                              # the live face is found behind the dead one


def test_the_lowest_face_wins_on_a_shared_edge():
    T = 9                                                              # UV x 8: integer texel coordinates are exact in fp32
    uvs, fuv = _rect_chart(T, 1, 1, 5, 5)                              # integer corners: the diagonal passes through texel centres
    t2f, tbary, unsure = BR.surface(uvs, fuv, T, 0.0)
    pos = BR.texel_uv_units(T)
    x, y = pos[..., 0], pos[..., 1]
    box = (x >= 1) & (x <= 5) & (y >= 1) & (y <= 5)
    assert np.array_equal(t2f >= 0, box)
    assert np.all(t2f[box & (y <= x)] == 0) and np.all(t2f[box & (y > x)] == 1)      # on the diagonal y == x: face 0
    assert np.all(unsure[box & (y == x)])                              # ... and the restatement says it had no margin
    swapped, _, _ = BR.surface(uvs, fuv[::-1], T, 0.0)
    assert np.all(swapped[box & (y < x)] == 1) and np.all(swapped[box & (y >= x)] == 0)


def test_bake_of_a_facing_quad_known_weights_and_occlusion():
    """a quad facing the camera at distance 2.5: every texel of the chart sees the camera at cos = z / |C - P|, weight cos^2;
    a second quad behind it is hidden wherever the near one covers its pixel"""
    from oracle import render_ref as RR
    S, T = 32, 16
    uvs, fuv = BR.quad_chart()
    near_v, faces = BR.facing_quad(0.0, 0.5)
    far_v, _ = BR.facing_quad(-1.0, 1.0)
    verts = np.concatenate([near_v, far_v])
    faces2 = np.concatenate([faces, faces + 4]).astype(np.int32)
    uvs2 = np.concatenate([uvs * 0.45, uvs * 0.45 + 0.5]).astype(np.float32)          # two charts, lower left and upper right
    fuv2 = np.concatenate([fuv, fuv + 4]).astype(np.int32)
    R, Tr = BR.front_camera(2.5)
    t2f, tbary, _ = BR.surface(uvs2, fuv2, T, 1.5)
    p2f, zbuf = BR.cpu_fragments(verts, faces2, R, Tr, S)
    imgs, _ = BR.ramp_images(1, S)
    acc, _, detail = BR.bake(verts, faces2, t2f, tbary, R, Tr, imgs, p2f, zbuf)
    used = detail["used"][0].reshape(T, T)
    on_near, on_far = (t2f >= 0) & (t2f < 2), t2f >= 2
    P = (tbary[..., None] * verts[faces2[np.where(t2f >= 0, t2f, 0)]]).sum(-2)
    # (a texel on the quad's outline may round to a pixel beside it: a pixel is 0.09 wide on the near plane)
    well_inside = on_near & (np.abs(P[..., 0]) < 0.4) & (np.abs(P[..., 1]) < 0.4)
    assert on_near.sum() > 20 and on_far.sum() > 20 and well_inside.sum() >= 6 and used[well_inside].all()
    cos = (2.5 - P[..., 2]) / np.linalg.norm(np.array([0, 0, 2.5]) - P, axis=-1)
    assert np.abs(acc[..., 3] - cos ** 2)[used].max() <= 1e-12
    # the far quad's surface points that project inside the near quad's outline are hidden; those outside it are seen
    s = BR.INV_TAN_HALF_FOV
    shadow = 0.5 * 3.5 / 2.5                                            # the near quad's outline on the far plane
    hidden = on_far & (np.abs(P[..., 0]) < shadow - 0.1) & (np.abs(P[..., 1]) < shadow - 0.1)
    seen = on_far & ((np.abs(P[..., 0]) > shadow + 0.1) | (np.abs(P[..., 1]) > shadow + 0.1))
    seen &= (np.abs(P[..., 0]) < 0.9) & (np.abs(P[..., 1]) < 0.9)      # (not on the far quad's own outline: a pixel is 0.13 wide there)
    assert hidden.sum() > 3 and seen.sum() > 3 and not used[hidden].any() and used[seen].all()
    assert np.all(acc[~used] == 0)
    tex = BR.resolve(acc, np.full((T, T, 3), 0.25))
    assert np.all(tex[~used] == 0.25) and np.all(tex[used] != 0.25)
    assert s > 1.7


def test_constant_images_bake_to_their_colour_and_best_keeps_the_squarest_view():
    from oracle import render_ref as RR
    S, T = 16, 8
    uvs, fuv = BR.quad_chart()
    verts, faces = BR.facing_quad(0.0, 0.6)
    R0, T0 = BR.front_camera(2.5)
    Rs, Ts = RR.look_at_view_transform(2.5, np.array([0.0, 30.0, 10.0]), np.array([0.0, 20.0, -50.0]))
    assert np.allclose(Rs[0], R0[0], atol=1e-6) and np.allclose(Ts[0], T0[0], atol=1e-6)       # front_camera is look_at(2.5, 0, 0)
    t2f, tbary, _ = BR.surface(uvs, fuv, T, 1.5)
    p2f, zbuf = BR.cpu_fragments(verts, faces, Rs, Ts, S)
    colours = np.array([[0.9, 0.1, 0.3], [0.2, 0.8, 0.4], [0.5, 0.5, 0.7]], np.float32)
    imgs = np.broadcast_to(colours[:, :, None, None], (3, 3, S, S)).copy()
    same = np.broadcast_to(colours[0][None, :, None, None], (3, 3, S, S)).copy()
    acc, _, detail = BR.bake(verts, faces, t2f, tbary, Rs, Ts, same, p2f, zbuf)
    written = acc[..., 3] > 0
    assert written.sum() >= 30 and np.abs(BR.resolve(acc, np.zeros((T, T, 3))) - colours[0])[written].max() <= 3e-8
    acc, _, detail = BR.bake(verts, faces, t2f, tbary, Rs, Ts, imgs, p2f, zbuf)
    w = detail["w"].reshape(3, T, T)
    want = np.einsum("btx,bc->txc", w, colours.astype(np.float64)) / np.where(written, w.sum(0), 1)[..., None]
    assert np.abs(BR.resolve(acc, np.zeros((T, T, 3))) - want)[written].max() <= 1e-12
    best, _, _ = BR.bake(verts, faces, t2f, tbary, Rs, Ts, imgs, p2f, zbuf, mode="best")
    squarest = colours.astype(np.float64)[w.argmax(0)]                 # argmax: the earliest view among equals
    assert np.abs(BR.resolve(best, np.zeros((T, T, 3))) - squarest)[written].max() <= 1e-12
    assert len(np.unique(w.argmax(0)[written])) >= 2 and np.all(w.argmax(0)[T // 2, T // 2] == 0)    # head-on at the centre
    a1, _, _ = BR.bake(verts, faces, t2f, tbary, Rs[:1], Ts[:1], imgs[:1], p2f[:1], zbuf[:1])
    a2, _, _ = BR.bake(verts, faces, t2f, tbary, Rs[1:], Ts[1:], imgs[1:], p2f[1:], zbuf[1:], acc=a1)
    assert np.array_equal(a2, acc)                                     # continued over two calls = one call over all views


def test_the_restatement_alone_stays_under_the_caps_on_the_cow():
    """the GPU tests may leave out 1 % of the texels (surface) and 2 % of the texel-views (bake): what the restatement marks
    as decided without margin on the cow stays under both, on the CPU oracle's fragments"""
    from oracle import render_ref as RR
    cow = _scenes.load_asset("cow")
    S = T = 64
    shares = {}
    for pad in (0.0, 1.5, 3.0):
        t2f, tbary, unsure = BR.surface(cow["verts_uvs"], cow["faces_uvs"], T, pad)
        shares[pad] = (float(unsure.mean()), float((t2f >= 0).mean()))
        assert unsure.mean() <= 0.01, shares
        if pad == 1.5:
            keep = (t2f, tbary)
    print("surface: (share without margin, share of texels owned) per pad", shares)
    assert 0.40 <= shares[0.0][1] <= 0.55 and 0.55 <= shares[1.5][1] <= 0.75
    t2f, tbary = keep
    R, Tr = _scenes.random_cameras(3, 0)
    p2f, zbuf = BR.cpu_fragments(cow["verts"], cow["faces"], R, Tr, S)
    imgs, _ = BR.ramp_images(3, S)
    _, _, detail = BR.bake(cow["verts"], cow["faces"], t2f, tbary, R, Tr, imgs, p2f, zbuf)
    share = detail["unsure"].sum() / (3 * detail["valid"].sum())
    print("bake: share of texel-views without margin", share, "used", detail["used"].mean())
    assert share <= 0.02 and detail["used"].sum() > 1000


# ---------------------------------------------------------------------------- 2. the C ABI
def test_symbols_are_declared_bound_and_built_like_cover():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    flags = lambda src: re.search(r'"%s":\s*\[([^\]]*)\]' % re.escape(src), build).group(1)
    assert flags("bake.hip") == flags("cover.hip")
    source = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "csrc", "bake.hip")).read()
    assert "atomicMin(" in source and "atomicAdd" not in source          # integer claims only, no float atomics


def test_workspace_size_is_pure_host_logic():
    from st3d import _lib
    lib = _lib.load()
    for T in (2, 8, 17, 512, 16384):
        assert lib.st3d_bake_workspace_bytes(T) == 8 * T * T            # one 64-bit key per texel
    for T in (1, 0, -1, 16385):
        assert lib.st3d_bake_workspace_bytes(T) == 0                    # a map needs two texels a side: UV x (T-1)


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, q, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4100)           # never dereferenced
    f = ctypes.c_float

    def variants(good, pointers, values):
        out = [good[:i] + [None] + good[i + 1:] for i in pointers]
        out += [good[:i] + [v] + good[i + 1:] for i, vs in values.items() for v in vs]
        return out
    cases = {
        #                    uvs fuv VT F  T  pad     ws  bytes     t2f tbary stream
        "st3d_bake_surface": variants([p, p, 4, 2, 8, f(1.5), q, 8 * 64, p, p, None], (0, 1, 6, 8, 9),
                                      {2: (0, -1), 3: (0, -1), 4: (1, 0, -1, 16385), 5: (f(-0.5), f(8.5), f(float("nan"))),
                                       6: (odd,), 7: (8 * 64 - 1, 0)}),
        #                  verts faces V F t2f tbary Tt R T imgs p2f zbuf B S   s       mode power  min_cos depth    acc stream
        "st3d_bake_views": variants([p, p, 4, 2, p, p, 8, p, p, p, p, p, 3, 16, f(1.7), 0, f(2.0), f(0.1), f(0.01), q, None],
                                    (0, 1, 4, 5, 7, 8, 9, 10, 11, 19),
                                    {2: (0, -1), 3: (0, -1), 6: (1, 0, 16385), 12: (0, -1), 13: (0, -1, 4097), 14: (f(0.0), f(-1.0)),
                                     15: (-1, 2), 16: (f(-1.0), f(float("nan"))), 17: (f(-0.1), f(1.5)), 18: (f(-0.01),)}),
        #                    acc fallback Tt out stream
        "st3d_bake_resolve": variants([p, p, 8, q, None], (0, 1, 3), {2: (1, 0, -1, 16385), 3: (p,)}),
    }
    for name, bad in cases.items():
        assert len(bad) >= 8
        for args in bad:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 3. the Python layer
def _stand_ins(T=8, B=2, S=16):
    return dict(verts=torch.zeros(4, 3), faces=torch.zeros(2, 3, dtype=torch.int32), t2f=torch.zeros(T, T, dtype=torch.int32),
                tbary=torch.zeros(T, T, 3), R=torch.eye(3).expand(B, 3, 3).contiguous(), T=torch.zeros(B, 3),
                images=torch.zeros(B, 3, S, S), p2f=torch.zeros(B, S, S, dtype=torch.int32), zbuf=torch.zeros(B, S, S))


def _bake_views(bake, **over):
    a = {**_stand_ins(), **over}
    extra = {k: a.pop(k) for k in list(a) if k in ("mode", "power", "min_cos", "depth_tol", "acc")}
    return bake.bake_views(a["verts"], a["faces"], a["t2f"], a["tbary"], a["R"], a["T"], a["images"], a["p2f"], a["zbuf"], **extra)


def test_the_wrappers_live_outside_ops_and_refuse_cpu_tensors():
    from st3d import bake, ops
    import utils as U
    for name in ("texel_surface", "bake_views", "baked_texture", "bake_texture"):
        assert callable(getattr(bake, name)) and not hasattr(ops, name)
    assert callable(U.bake_texture)
    for call in (lambda: bake.texel_surface(torch.zeros(4, 2), torch.zeros(2, 3, dtype=torch.int32), 8),
                 lambda: _bake_views(bake),
                 lambda: bake.baked_texture(torch.zeros(8, 8, 4), torch.zeros(8, 8, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_wrappers_validate_shapes_and_dtypes_before_they_call():
    from st3d import bake
    from st3d.render import Meshes, TexturesAtlas, TexturesVertex
    uvs, fuv = torch.zeros(4, 2), torch.zeros(2, 3, dtype=torch.int32)
    for T in (1, 0, 16385, 2.5, True):
        with pytest.raises(ValueError, match="texture side"):
            bake.texel_surface(uvs, fuv, T)
    for pad in (-0.1, 8.5, float("nan")):
        with pytest.raises(ValueError, match="pad must be in 0...8"):
            bake.texel_surface(uvs, fuv, 8, pad)
    with pytest.raises(ValueError, match="verts_uvs"):
        bake.texel_surface(torch.zeros(4, 3), fuv, 8)
    with pytest.raises(ValueError, match="faces_uvs_i32"):
        bake.texel_surface(uvs, torch.zeros(2, 4, dtype=torch.int32), 8)
    for over, word in ((dict(t2f=torch.zeros(8, 8)), "t2f"), (dict(t2f=torch.zeros(8, 9, dtype=torch.int32)), "t2f"),
                       (dict(tbary=torch.zeros(8, 8, 4)), "tbary"), (dict(mode="median"), "mode"),
                       (dict(power=-1.0), "power"), (dict(min_cos=1.5), "min_cos"), (dict(depth_tol=-1.0), "depth_tol"),
                       (dict(images=torch.zeros(2, 3, 16, 15)), "images"), (dict(images=torch.zeros(2, 4, 16, 16)), "images"),
                       (dict(p2f=torch.zeros(2, 15, 16, dtype=torch.int32)), "p2f"), (dict(zbuf=torch.zeros(3, 16, 16)), "zbuf"),
                       (dict(R=torch.zeros(3, 3, 3)), "R and T"), (dict(T=torch.zeros(2, 4)), "R and T"),
                       (dict(verts=torch.zeros(4, 2)), "verts"), (dict(acc=torch.zeros(8, 8, 3)), "acc"),
                       (dict(acc=torch.zeros(8, 8, 4, dtype=torch.float64)), "acc")):
        with pytest.raises(ValueError, match=word):
            _bake_views(bake, **over)
    with pytest.raises(ValueError, match="acc"):
        bake.baked_texture(torch.zeros(8, 8, 3), torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match="fallback"):
        bake.baked_texture(torch.zeros(8, 8, 4), torch.zeros(8, 8, 4))
    verts, faces = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    R, T = torch.eye(3)[None], torch.tensor([[0.0, 0.0, 3.0]])
    from st3d.render import FoVPerspectiveCameras
    cams = FoVPerspectiveCameras(R=R, T=T)
    for textures in (TexturesVertex(torch.rand(4, 3)), TexturesAtlas(torch.rand(2, 2, 2, 3))):
        with pytest.raises(NotImplementedError, match="TexturesUV"):
            bake.bake_texture(Meshes([verts], [faces], textures), torch.zeros(1, 3, 16, 16), cams, 16)
    import utils as U
    uv_mesh = U.build_mesh(torch.rand(1, 4, 2), faces[None], torch.rand(1, 8, 6, 3), verts, faces)
    with pytest.raises(NotImplementedError, match="square texture maps only"):
        bake.bake_texture(uv_mesh, torch.zeros(1, 3, 16, 16), cams, 16)
    square = U.build_mesh(torch.rand(1, 4, 2), faces[None], torch.rand(1, 8, 8, 3), verts, faces)
    with pytest.raises(ValueError, match="one per camera"):
        bake.bake_texture(square, torch.zeros(2, 3, 16, 16), cams, 16)
    with pytest.raises(ValueError, match="mode"):
        bake.bake_texture(square, torch.zeros(1, 3, 16, 16), cams, 16, mode="max")
    near = FoVPerspectiveCameras(R=R, T=torch.tensor([[0.0, 0.0, -5.0]]))
    with pytest.raises(NotImplementedError, match="near clipping plane"):
        bake.bake_texture(square, torch.zeros(1, 3, 16, 16), near, 16)


# ---------------------------------------------------------------------------- 4. the flags
def _scripts():
    import first_approach as FA
    import third_approach as TA
    return FA, TA


def test_flag_defaults_are_the_untouched_path_and_second_approach_has_none():
    import second_approach as SA
    from st3d import cli
    names = {f.name: (f.type, f.default, f.choices) for f in cli.BAKE_FLAGS}
    assert names == {"bake_texture": (str, "off", ["off", "mean", "best"]), "bake_power": (float, 2.0, None),
                     "bake_min_cos": (float, 0.1, None)}
    assert not {f.name for f in cli.SHARED_FLAGS} & set(names)
    help_text = next(f.help for f in cli.BAKE_FLAGS if f.name == "bake_texture")
    assert "--supersample" in help_text and "--texture_mip_levels" in help_text and "--n_mse_steps 0" in help_text
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.bake_texture == "off" and a.bake_power == 2.0 and a.bake_min_cos == 0.1
        assert {f.name for f in mod.FLAGS} >= set(names)
    a = SA.build_parser().parse_args([])
    assert not any(hasattr(a, n) for n in names)
    with pytest.raises(SystemExit):
        SA.build_parser().parse_args(["--bake_texture", "mean"])


def test_the_flags_parse_and_check_args_refuses(capsys):
    for mod in _scripts():
        parse = mod.build_parser().parse_args
        a = parse(["--bake_texture", "mean", "--n_mse_steps", "0"])
        assert a.bake_texture == "mean" and a.n_mse_steps == 0
        a = parse(["--bake_texture", "best", "--bake_power", "4", "--bake_min_cos", "0.3", "--optimization_target", "both"])
        assert (a.bake_texture, a.bake_power, a.bake_min_cos) == ("best", 4.0, 0.3)
        # allowed and ignored by the bake
        assert parse(["--bake_texture", "mean", "--supersample", "2"]).supersample == 2
        assert parse(["--bake_texture", "mean", "--texture_mip_levels", "0"]).texture_mip_levels == 0
        assert parse(["--bake_texture", "off"]).bake_texture == "off"
        for argv, word in ((["--bake_texture", "mean", "--optimization_target", "mesh"], "optimization_target texture or both"),
                           (["--bake_texture", "best", "--texture_type", "vertex"], "texture_type uv"),
                           (["--bake_texture", "mean", "--texture_atlas", "4"], "texture_atlas 0"),
                           (["--bake_texture", "mean", "--texture_pyramid_levels", "3"], "texture_pyramid_levels 1"),
                           (["--bake_texture", "mean", "--texture_pyramid_levels", "0"], "texture_pyramid_levels 1"),
                           (["--bake_texture", "mean", "--lights", "point"], "lights ambient"),
                           (["--bake_texture", "mean", "--lights", "headlight"], "lights ambient"),
                           (["--bake_texture", "mean", "--bake_power", "-1"], "bake_power"),
                           (["--bake_texture", "mean", "--bake_min_cos", "1.5"], "bake_min_cos"),
                           (["--bake_power", "3"], "need --bake_texture"),
                           (["--bake_texture", "off", "--bake_min_cos", "0.2"], "need --bake_texture"),
                           (["--bake_texture", "median"], "bake_texture")):
            with pytest.raises(SystemExit):
                parse(argv)
            assert word in capsys.readouterr().err, argv


def test_a_sharded_run_is_refused_before_any_gpu_work(monkeypatch):
    import first_approach as FA
    from st3d import cli, optim
    monkeypatch.setattr(optim, "init_distributed", lambda: (0, 2, 0))
    args = FA.build_parser().parse_args(["--bake_texture", "mean"])
    with pytest.raises(RuntimeError, match="torch.distributed"):
        cli.Run(args, lr=0.01, image_dir="x")
