"""Host side of the per-face texel atlas: the TexturesAtlas container, the face-count check, setup_optimizations /
finalize_mesh / the texture regularisers on such a mesh, what the renderer refuses before any launch, routing and the
supersample composition, --texture_atlas on the three scripts and the atlas it starts from, the .npy round trip, and the C
ABI's argument checks.  No GPU: CPU tensors and stubbed launches (anything that reached a kernel would raise
St3dError('no CPU fallback'))."""
import os
import types

import numpy as np
import pytest
import torch


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def _cpu_mesh(z=3.0, atlas=None, R=2):
    from st3d import render as R_
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    faces = torch.tensor([[0, 1, 2], [1, 3, 2]])
    tex = R_.TexturesAtlas(torch.rand(2, R, R, 3) if atlas is None else atlas)
    return R_.Meshes(verts, faces, tex), R_.FoVPerspectiveCameras(T=torch.tensor([[0.0, 0, z]]))


def _renderer(shader=None, **kw):
    from st3d import render as R
    return R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=8, **kw)), shader or R.SoftPhongShader())


# ------------------------------------------------------------------ the container
def test_textures_atlas_shapes_clone_detach():
    from st3d import render as R
    import utils as U
    assert U.TexturesAtlas is R.TexturesAtlas
    c = torch.rand(5, 3, 3, 3)
    for given in (c, c[None], [c], (c,)):
        t = R.TexturesAtlas(given)
        assert t.atlas_packed().shape == (5, 3, 3, 3) and t.atlas_padded().shape == (1, 5, 3, 3, 3)
        assert t.atlas_packed().data_ptr() == c.data_ptr() and t.atlas_padded().data_ptr() == c.data_ptr()      # views, no copy
    t = R.TexturesAtlas(atlas=c)
    k = t.clone()
    assert torch.equal(k.atlas_packed(), c) and k.atlas_packed().data_ptr() != c.data_ptr()
    leaf = c.clone().requires_grad_(True)
    t = R.TexturesAtlas(leaf)
    assert t.atlas_packed() is leaf and t.clone().atlas_packed().requires_grad
    d = t.detach().atlas_packed()
    assert not d.requires_grad and d.data_ptr() == leaf.data_ptr()
    for R_ in (1, 64):
        assert R.TexturesAtlas(torch.zeros(2, R_, R_, 3)).atlas_packed().shape[1] == R_
    for bad in (torch.rand(5, 3, 3), torch.rand(5, 3, 3, 4), torch.rand(5, 3, 2, 3), torch.rand(5, 2, 3, 3), torch.rand(2, 5, 3, 3, 3),
                torch.rand(1, 1, 5, 3, 3, 3), torch.zeros(5, 0, 0, 3), torch.zeros(2, 65, 65, 3), [c, c], []):
        with pytest.raises(ValueError):
            R.TexturesAtlas(bad)


def test_wrong_face_count_is_a_value_error():
    from st3d import render as R
    import utils as U
    verts, faces = torch.rand(4, 3), torch.tensor([[0, 1, 2], [1, 3, 2]])
    for n in (1, 3):
        with pytest.raises(ValueError, match="block per face"):
            R.Meshes(verts, faces, R.TexturesAtlas(torch.rand(n, 2, 2, 3)))
        with pytest.raises(ValueError, match="block per face"):
            U.build_mesh_atlas(torch.rand(n, 2, 2, 3), verts, faces)
    mesh, cams = _cpu_mesh()
    mesh.textures = R.TexturesAtlas(torch.rand(1, 2, 2, 3))     # swapped behind the constructor's back: render time refuses too
    with pytest.raises(ValueError, match="block per face"):
        _renderer().render(mesh, cams)
    with pytest.raises(ValueError, match="block per face"):
        _renderer(supersample=2).render(mesh, cams)
    m = U.build_mesh_atlas(torch.rand(1, 2, 4, 4, 3), verts, faces)
    assert isinstance(m.textures, R.TexturesAtlas) and m.clone().textures.atlas_packed().shape == (2, 4, 4, 3)
    assert isinstance(m.detach().textures, R.TexturesAtlas)


# ------------------------------------------------------------------ setup_optimizations, finalize_mesh, regularisers
def test_setup_optimizations_leaves_per_target():
    import utils as U
    at = torch.rand(2, 3, 3, 3)
    mesh, _ = _cpu_mesh(atlas=at)
    for target, leaves in (("texture", ["atlas"]), ("mesh", ["verts"]), ("both", ["verts", "atlas"])):
        for out in (U.setup_optimizations(target, mesh, 0.01), U.setup_optimizations(target, mesh, 0.01, 1)):
            assert sorted(out) == ["atlas", "faces", "optimizable_mesh", "optimizer", "verts"]
            assert [id(p) for p in out["optimizer"].params] == [id(out[k]) for k in leaves]
            assert out["atlas"].requires_grad == ("atlas" in leaves) and out["verts"].requires_grad == ("verts" in leaves)
            assert torch.equal(out["atlas"].detach(), at) and out["atlas"].shape == (2, 3, 3, 3)
            assert out["atlas"].data_ptr() != at.data_ptr()           # a clone: the content mesh stays as it is
            assert out["optimizer"].lr == 0.01 and len(out["optimizer"].param_groups) == 1
            assert U.build_mesh_atlas(out["atlas"], out["verts"], out["faces"]).textures.atlas_packed() is out["atlas"]
    for levels in (0, 2, 3):
        for target in ("texture", "both", "mesh"):
            with pytest.raises(ValueError, match="texture_pyramid_levels"):
                U.setup_optimizations(target, mesh, 0.01, texture_pyramid_levels=levels)
    with pytest.raises(UnboundLocalError):
        U.setup_optimizations("nothing", mesh, 0.01)


def test_finalize_mesh_clamps_the_atlas():
    import utils as U
    from st3d import render as R
    at = (torch.rand(2, 2, 2, 3) * 3 - 1).requires_grad_(True)
    mesh, _ = _cpu_mesh(atlas=at)
    final = U.finalize_mesh(mesh)
    assert isinstance(final.textures, R.TexturesAtlas)
    got = final.textures.atlas_packed()
    assert not got.requires_grad and torch.equal(got, at.detach().clamp(0, 1)) and float(at.detach().min()) < 0 and float(at.detach().max()) > 1
    assert torch.equal(final.verts_packed(), mesh.verts_packed()) and torch.equal(final.faces_packed(), mesh.faces_packed())


def test_texture_regularisers_read_the_atlas(monkeypatch):
    import losses as L
    seen = []
    monkeypatch.setattr(L, "_on_gpu", lambda t: t.to(torch.float32))

    def fake_apply(x, op, *extra):
        seen.append((x, op, extra))
        return x.sum()
    monkeypatch.setattr(L, "_FusedLossFn", types.SimpleNamespace(apply=fake_apply))
    at = torch.rand(2, 2, 2, 3)
    mesh, _ = _cpu_mesh(atlas=at)
    L.rgb_range_loss(mesh)
    L.texture_l2_loss(mesh, at.clone())
    assert seen[0][0] is at and seen[0][1] is L._ops.range_loss
    assert seen[1][0] is at and seen[1][1] is L._l2_to and seen[1][2][0].shape == (2, 2, 2, 3)
    with pytest.raises(ValueError, match="no pixel grid"):
        L.compute_tv_loss(mesh, torch.ones(1, 1, 8, 8))


# ------------------------------------------------------------------ refusals before any launch
def test_every_limitation_is_refused_before_a_launch():
    from st3d import render as R
    mesh, cams = _cpu_mesh()
    assert sorted(R.ATLAS_REFUSALS) == ["lights", "mip", "silhouette", "soft"]
    assert all("TexturesAtlas" in m for m in R.ATLAS_REFUSALS.values())
    for lights in (R.PointLights(), R.DirectionalLights(), R.HeadLights(), R.AmbientLights(ambient_color=((0.5, 0.5, 0.5),))):
        with pytest.raises(NotImplementedError, match="TexturesAtlas.*unlit"):
            _renderer().render(mesh, cams, lights=lights)
        with pytest.raises(NotImplementedError, match="TexturesAtlas.*unlit"):
            _renderer(supersample=2).render(mesh, cams, lights=lights)
    with pytest.raises(NotImplementedError, match="TexturesAtlas.*unlit"):
        _renderer(R.SoftPhongShader(lights=R.PointLights())).render(mesh, cams)
    with pytest.raises(NotImplementedError, match="TexturesAtlas.*unlit"):
        _renderer().render(mesh, cams, lights=R.AmbientLights(), materials=R.Materials(ambient_color=((0.5, 0.5, 0.5),)))
    for kw in (dict(texture_mip_levels=0), dict(texture_mip_levels=2), dict(texture_mip_levels=0, texture_lod_bias=0.5)):
        with pytest.raises(NotImplementedError, match="TexturesAtlas.*texture_mip_levels"):
            _renderer(**kw).render(mesh, cams)
    for kw in (dict(faces_per_pixel=2), dict(blur_radius=1e-4), dict(clip_barycentric_coords=True), dict(cull_backfaces=True),
               dict(z_clip_value=0.5), dict(perspective_correct=False), dict(faces_per_pixel=2, supersample=2)):
        with pytest.raises(NotImplementedError, match="TexturesAtlas.*hard settings"):
            _renderer(**kw).render(mesh, cams)
    for bp in (R.BlendParams(sigma=1e-3), R.BlendParams(gamma=1e-3), R.BlendParams(background_color=(0.0, 0.0, 0.0))):
        with pytest.raises(NotImplementedError, match="TexturesAtlas.*hard settings"):
            _renderer(R.SoftPhongShader(blend_params=bp)).render(mesh, cams)
    srs = R.SilhouetteRasterizationSettings(image_size=8, faces_per_pixel=50)
    with pytest.raises(NotImplementedError, match="SoftSilhouetteShader"):
        R.MeshRenderer(R.MeshRasterizer(None, srs), R.SoftPhongShader())
    with pytest.raises(NotImplementedError, match="TexturesAtlas"):
        R.render_views(mesh, cams.R, cams.T, 8, srs)
    # white ambient light is the unlit route, and supersample 1...4 is covered: they get as far as the kernels
    for lights in (None, R.AmbientLights()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _renderer().render(mesh, cams, lights=lights)
    for a in (1, 2, 3, 4):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _renderer(supersample=a).render(mesh, cams)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.render_views(mesh, cams.R, cams.T, 8)


def test_a_silhouette_render_needs_no_atlas(monkeypatch):
    from st3d import render as R
    calls = []

    def fake(name):
        def apply(*a):
            calls.append((name, a))
            return torch.zeros(1, 1, a[4], a[4])
        return types.SimpleNamespace(apply=apply)
    monkeypatch.setattr(R, "_SilhouetteFn", fake("general"))
    monkeypatch.setattr(R, "_SilhouetteRasterFn", fake("silraster"))
    mesh, cams = _cpu_mesh()
    rgb, alpha = _renderer(R.SoftSilhouetteShader()).render(mesh, cams)
    assert rgb.shape == (1, 3, 8, 8) and alpha.shape == (1, 1, 8, 8)
    srs = R.SilhouetteRasterizationSettings(image_size=8, faces_per_pixel=50)
    R.MeshRenderer(R.MeshRasterizer(None, srs), R.SoftSilhouetteShader()).render(mesh, cams)
    assert [c[0] for c in calls] == ["general", "silraster"]
    for _, a in calls:
        assert a[0] is mesh.verts_packed() and a[1].dtype == torch.int32 and len(a) == 12


def test_near_plane_is_an_error_whatever_the_policy(monkeypatch):
    from st3d import ops
    mesh, cams = _cpu_mesh(z=0.3)
    for policy in ("clip", "raise"):
        monkeypatch.setattr(ops, "NEAR_PLANE_POLICY", policy)
        for a in (1, 2):
            try:
                with pytest.raises(RuntimeError, match="near clipping plane.*TexturesAtlas"):
                    _renderer(supersample=a).render(mesh, cams)
                assert not ops.near_plane_triggered()
            finally:
                ops.reset_near_plane()


# ------------------------------------------------------------------ routing and the supersample composition
def _fake_fn(calls, name, s_at, grad=False):
    def apply(*a):
        calls.append((name, a))
        rgb = torch.zeros(1, 3, a[s_at], a[s_at], requires_grad=grad) + 0.0
        return rgb, torch.ones(1, 1, a[s_at], a[s_at])
    return types.SimpleNamespace(apply=apply)


def test_routing(monkeypatch):
    """a TexturesAtlas mesh is _AtlasRenderFn and nothing else; UV and vertex-colour meshes still reach their own functions
    with their old arguments"""
    from st3d import render as R
    calls = []
    monkeypatch.setattr(R, "_RenderFn", _fake_fn(calls, "uv", 7))
    monkeypatch.setattr(R, "_VertexColourRenderFn", _fake_fn(calls, "vertex", 5))
    monkeypatch.setattr(R, "_AtlasRenderFn", _fake_fn(calls, "atlas", 5))
    mesh, cams = _cpu_mesh()
    rgb, mask = _renderer().render(mesh, cams)
    _renderer().render(mesh, cams, lights=R.AmbientLights())
    assert [c[0] for c in calls] == ["atlas", "atlas"]
    a = calls[0][1]
    assert len(a) == 6 and a[0] is mesh.verts_packed() and a[1] is mesh.textures.atlas_packed()
    assert a[2].dtype == torch.int32 and a[2].tolist() == [[0, 1, 2], [1, 3, 2]] and a[5] == 8
    assert R.flat_of(rgb) == (1.0, 1.0, 1.0)
    calls.clear()
    uv = R.Meshes(mesh.verts_packed(), mesh.faces_packed(),
                  R.TexturesUV(maps=torch.rand(1, 8, 8, 3), faces_uvs=mesh.faces_packed()[None], verts_uvs=torch.rand(1, 4, 2)))
    _renderer().render(uv, cams)
    assert [c[0] for c in calls] == ["uv"] and len(calls[0][1]) == 9 and calls[0][1][8] is None
    calls.clear()
    vc = R.Meshes(mesh.verts_packed(), mesh.faces_packed(), R.TexturesVertex(torch.rand(4, 3)))
    _renderer().render(vc, cams)
    assert [c[0] for c in calls] == ["vertex"] and len(calls[0][1]) == 6 and calls[0][1][1] is vc.textures.verts_features_packed()


def test_supersample_is_atlas_at_a_s_then_the_box_filter(monkeypatch):
    """the order of the composition: _AtlasRenderFn at side a S, _BoxDownFn on rgb, ops.box_down_fwd on the mask, the
    coverage tag from the filtered mask"""
    from st3d import ops
    from st3d import render as R
    calls = []
    monkeypatch.setattr(R, "_AtlasRenderFn", _fake_fn(calls, "atlas", 5, grad=True))

    def box_fn(x, a):
        calls.append(("boxfn", (x, a)))
        return x[:, :, ::a, ::a] * 1.0
    monkeypatch.setattr(R, "_BoxDownFn", types.SimpleNamespace(apply=box_fn))

    def box_fwd(x, a):
        calls.append(("box_down_fwd", (x, a)))
        out = x[:, :, ::a, ::a] * 0.25
        out[0, 0, 0, 0] = 0.0
        return out
    monkeypatch.setattr(ops, "box_down_fwd", box_fwd)
    mesh, cams = _cpu_mesh()
    for a in (2, 3, 4):
        calls.clear()
        rgb, cov = _renderer(supersample=a).render(mesh, cams)
        assert [c[0] for c in calls] == ["atlas", "boxfn", "box_down_fwd"]
        assert calls[0][1][5] == 8 * a and calls[0][1][1] is mesh.textures.atlas_packed()
        assert calls[1][1][0].shape == (1, 3, 8 * a, 8 * a) and calls[1][1][1] == a
        assert calls[2][1][0].shape == (1, 1, 8 * a, 8 * a) and calls[2][1][1] == a
        assert rgb.shape == (1, 3, 8, 8) and cov.shape == (1, 1, 8, 8) and float(cov.max()) == 0.25       # fractional
        need = getattr(rgb, R.NEED_TAG)
        assert need.dtype == torch.uint8 and torch.equal(need.bool(), cov[:, 0] > 0) and not need[0, 0, 0]
        assert R.flat_of(rgb) == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="supersample"):
        _renderer(supersample=5).render(mesh, cams)


def test_atlas_render_fn_hands_the_vertices_no_gradient(monkeypatch):
    """_AtlasRenderFn on stubbed ops: the atlas gets shade_atlas_bwd's result, the vertices None"""
    from st3d import ops
    from st3d import render as R
    S = 4
    frag = (torch.zeros(1, S, S, dtype=torch.int32), torch.zeros(1, S, S), torch.zeros(1, S, S, 3), torch.zeros(1, S, S))
    seen = {}
    monkeypatch.setattr(ops, "project_verts", lambda v, R_, T: v[None])
    monkeypatch.setattr(ops, "raster_fwd", lambda ndc, f, S_: frag)
    monkeypatch.setattr(ops, "shade_atlas_fwd", lambda fr, at: (at[0, 0, 0].reshape(1, 3, 1, 1).expand(1, 3, S, S).clone(),
                                                                torch.ones(1, 1, S, S)))

    def bwd(g, fr, R_, F):
        seen["args"] = (tuple(g.shape), fr is frag, R_, F)
        return torch.full((F, R_, R_, 3), 2.0)
    monkeypatch.setattr(ops, "shade_atlas_bwd", bwd)
    verts = torch.rand(4, 3, requires_grad=True)
    atlas = torch.rand(1, 2, 3, 3, 3, requires_grad=True)                     # padded: the gradient comes back in this shape
    rgb, mask = R._AtlasRenderFn.apply(verts, atlas, torch.zeros(2, 3, dtype=torch.int32), torch.eye(3)[None], torch.zeros(1, 3), S)
    assert rgb.requires_grad and not mask.requires_grad
    rgb.sum().backward()
    assert verts.grad is None and atlas.grad.shape == (1, 2, 3, 3, 3) and float(atlas.grad.min()) == 2.0
    assert seen["args"] == ((1, 3, S, S), True, 3, 2)


def test_ops_wrappers_check_before_the_library():
    from st3d import _lib, ops
    frag = (torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8))
    at = torch.rand(2, 2, 2, 3)
    for bad in (torch.rand(2, 2, 2), torch.rand(2, 2, 3, 3), torch.rand(2, 2, 2, 4)):
        with pytest.raises(ValueError, match=r"\(F, R, R, 3\)"):
            ops.shade_atlas_fwd(frag, bad)
    with pytest.raises(ValueError, match="R must be"):
        ops.shade_atlas_fwd(frag, torch.zeros(1, 65, 65, 3))
    with pytest.raises(ValueError, match="R must be"):
        ops.shade_atlas_bwd(torch.rand(1, 3, 8, 8), frag, 0, 2)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.shade_atlas_bwd(torch.rand(1, 3, 8, 8), frag, 64, 1 << 20)
    with pytest.raises(ValueError, match="grad_rgb"):
        ops.shade_atlas_bwd(torch.rand(1, 3, 4, 4), frag, 2, 2)
    with pytest.raises(ValueError, match="grad_atlas"):
        ops.shade_atlas_bwd(torch.rand(1, 3, 8, 8), frag, 2, 2, grad_atlas=torch.zeros(2, 2, 2))
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_atlas_fwd(frag, at)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_atlas_bwd(torch.rand(1, 3, 8, 8), frag, 2, 2)


def test_c_abi_validates_before_any_launch():
    from st3d import _lib
    lib = _lib.load()
    one = 16        # any non-NULL value: the checks below fail before a pointer is followed
    p = [one] * 5   # pix_to_face, bary, zbuf, dists, atlas
    assert lib.st3d_shade_atlas_fwd(*p, 1, 8, 2, 4, one, None, None) == -1 and b"invalid argument" in lib.st3d_last_error()
    assert lib.st3d_shade_atlas_fwd(*p, 1, 8, 2, 4, None, one, None) == -1
    for k in range(5):
        q = list(p)
        q[k] = None
        assert lib.st3d_shade_atlas_fwd(*q, 1, 8, 2, 4, one, one, None) == -1
        assert lib.st3d_shade_atlas_bwd(*q, 1, 8, 2, 4, one, None) == -1
        assert lib.st3d_shade_atlas_bwd_det(*q, 1, 8, 2, 4, one, 16, 1 << 20, None) == -1
    big_f = (2 ** 31 - 1) // (64 * 64) + 1          # F R^2 one block past the key range at R = 64
    for B, S, F, R in ((0, 8, 2, 4), (1, 0, 2, 4), (1, 8, 0, 4), (1, 8, 2, 0), (-1, 8, 2, 4), (1, 8, 2, -3), (1, 4097, 2, 4),
                       (1, 8, 2, 65), (1, 8, big_f, 64), (1, 8, 2 ** 31 - 1, 2)):
        assert lib.st3d_shade_atlas_fwd(*p, B, S, F, R, one, one, None) == -1
        assert lib.st3d_shade_atlas_bwd(*p, B, S, F, R, one, None) == -1
        assert lib.st3d_shade_atlas_bwd_det(*p, B, S, F, R, one, one, 1 << 30, None) == -1
        if B == 1 and S == 8:
            assert lib.st3d_shade_atlas_bwd_det_workspace_bytes(F, R) == 0
    assert lib.st3d_shade_atlas_bwd(*p, 1, 8, 2, 4, None, None) == -1                      # no output
    need = lib.st3d_shade_atlas_bwd_det_workspace_bytes(2, 4)
    assert need >= 16 + 4 * 1024 + 8 * 2 * 16 * 3
    assert lib.st3d_shade_atlas_bwd_det_workspace_bytes(big_f - 1, 64) > 0                  # the last size within the key range
    assert lib.st3d_shade_atlas_bwd_det(*p, 1, 8, 2, 4, None, 16, need, None) == -1        # no output
    assert lib.st3d_shade_atlas_bwd_det(*p, 1, 8, 2, 4, one, None, need, None) == -1       # no workspace
    assert lib.st3d_shade_atlas_bwd_det(*p, 1, 8, 2, 4, one, 16, need - 1, None) == -1     # workspace too small
    assert lib.st3d_shade_atlas_bwd_det(*p, 1, 8, 2, 4, one, 24, need, None) == -1         # misaligned


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("k", [0, 1, 2])
def test_flag_reaches_all_three_scripts(k):
    p = _scripts()[k].build_parser()
    assert p.parse_args([]).texture_atlas == 0
    assert p.parse_args(["--texture_atlas", "0", "--texture_type", "vertex"]).texture_atlas == 0
    assert p.parse_args(["--texture_atlas", "8"]).texture_atlas == 8
    for a in ("1", "2", "3", "4"):
        assert p.parse_args(["--texture_atlas", "64", "--supersample", a]).supersample == int(a)
    refused = [["--texture_atlas", "-1"], ["--texture_atlas", "65"], ["--texture_atlas", "x"],
               ["--texture_atlas", "4", "--texture_type", "vertex"], ["--texture_atlas", "4", "--texture_pyramid_levels", "0"],
               ["--texture_atlas", "4", "--texture_pyramid_levels", "3", "--size", "64"],
               ["--texture_atlas", "4", "--texture_mip_levels", "0"], ["--texture_atlas", "4", "--texture_mip_levels", "2"],
               ["--texture_atlas", "4", "--lights", "point"], ["--texture_atlas", "4", "--lights", "directional"],
               ["--texture_atlas", "4", "--lights", "headlight"], ["--texture_atlas", "4", "--optimization_target", "mesh"],
               ["--texture_atlas", "4", "--optimization_target", "both"], ["--texture_atlas", "4", "--supersample", "5"]]
    if k == 1:          # the regulariser flags exist on second_approach.py alone
        refused.append(["--texture_atlas", "4", "--tv_weight", "0.5"])
        assert p.parse_args(["--texture_atlas", "4", "--texture_l2_weight", "0.5", "--rgb_range_weight", "1"]).texture_atlas == 4
    for argv in refused:
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_check_args_names_the_conflict():
    from st3d import cli
    base = dict(silhouette_weight=0.0, optimization_target="texture", silhouette_sigma=1e-4, silhouette_faces_per_pixel=None,
                texture_pyramid_levels=1, size=768, supersample=1, texture_mip_levels=1, texture_lod_bias=0.0, lights="ambient",
                resize_texture=True, texture_type="uv", tv_weight=0.0, texture_atlas=8)
    ns = lambda **kw: types.SimpleNamespace(**dict(base, **kw))      # noqa: E731
    assert cli.check_args(ns()) is None and cli.check_args(ns(supersample=4)) is None
    for kw, word in ((dict(texture_type="vertex"), "texture_type"), (dict(texture_pyramid_levels=0), "texture_pyramid_levels"),
                     (dict(texture_mip_levels=0), "texture_mip_levels"), (dict(lights="point"), "lights"),
                     (dict(tv_weight=0.1), "tv_weight"), (dict(optimization_target="mesh"), "optimization_target"),
                     (dict(optimization_target="both"), "optimization_target")):
        msg = cli.check_args(ns(**kw))
        assert msg and "--texture_atlas" in msg and word in msg, (kw, msg)
        if kw != dict(texture_type="vertex"):
            assert cli.check_args(ns(texture_atlas=0, **kw)) is None
    for r in (-1, 65):
        assert "--texture_atlas" in cli.check_args(ns(texture_atlas=r))
    # a namespace without the attribute (older callers): today's behaviour
    old = dict(base)
    del old["texture_atlas"]
    assert cli.check_args(types.SimpleNamespace(**old)) is None
    names = {f.name: (f.type, f.default, f.choices) for f in cli.SHARED_FLAGS}
    assert names["texture_atlas"] == (int, 0, None) and names["texture_type"][1:] == ("uv", ["uv", "vertex"])


def _two_triangle_obj(tmp_path, with_uvs):
    from PIL import Image
    path = tmp_path / "quad.obj"
    lines = []
    if with_uvs:
        # 4 x 4 map: channel 0 = column / 3, channel 1 = row / 3 (row 0 = the TOP of the image = v = 1), channel 2 = 1
        img = np.zeros((4, 4, 3), np.uint8)
        img[..., 0] = (np.arange(4)[None, :] * 85)
        img[..., 1] = (np.arange(4)[:, None] * 85)
        img[..., 2] = 255
        Image.fromarray(img).save(tmp_path / "quad.png")
        (tmp_path / "quad.mtl").write_text("newmtl m\nmap_Kd quad.png\n")
        lines += ["mtllib quad.mtl", "usemtl m"]
    lines += ["v 0 0 0", "v 1 0 0", "v 1 1 0", "v 0 1 0"]
    if with_uvs:
        lines += ["vt 0 0", "vt 1 0", "vt 1 1", "vt 0 1", "f 1/1 2/2 3/3", "f 1/1 3/3 4/4"]
    else:
        lines += ["f 1 2 3", "f 1 3 4"]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_initial_atlas_from_a_map(tmp_path):
    """by hand: the map's colour at (u, v) is (u, 1 - v, 1) (column = 3 u; v = 1 is row 0, whose green is 0; bilinear
    reproduces the ramp), so texel (y, x) of a face holds (u, 1 - v, 1) at the UV of its centre"""
    from st3d import cli
    verts, faces, atlas = cli.load_scene_atlas(_two_triangle_obj(tmp_path, True), 2, "cpu")
    assert verts.shape == (4, 3) and faces.tolist() == [[0, 1, 2], [0, 2, 3]] and atlas.shape == (2, 2, 2, 3)
    assert atlas.dtype == torch.float32
    # R = 2 centres (b0, b1), [y][x]: (1/6, 1/6) (4/6, 1/6) / (1/6, 4/6) (1/3, 1/3) -- the last is the flipped texel (1,1)
    cen = {(0, 0): (1 / 6, 1 / 6), (0, 1): (4 / 6, 1 / 6), (1, 0): (1 / 6, 4 / 6), (1, 1): (1 / 3, 1 / 3)}
    corners = [[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]]
    want = torch.zeros(2, 2, 2, 3)
    for f in range(2):
        for (y, x), (b0, b1) in cen.items():
            b = (b0, b1, 1 - b0 - b1)
            u = sum(b[i] * corners[f][i][0] for i in range(3))
            v = sum(b[i] * corners[f][i][1] for i in range(3))
            want[f, y, x] = torch.tensor([u, 1 - v, 1.0])
    assert (atlas - want).abs().max() <= 1e-6, atlas
    # face 0, texel (0,0): b = (1/6, 1/6, 2/3) -> uv = (1/6 + 2/3, 2/3) -> (5/6, 1/3, 1)
    assert (atlas[0, 0, 0] - torch.tensor([5 / 6, 1 / 3, 1.0])).abs().max() <= 1e-6
    b0, b1 = cli.atlas_texel_centres(3)
    assert b0.shape == (3, 3) and abs(float(b0[0, 2]) - (2 + 1 / 3) / 3) < 1e-15 and abs(float(b1[2, 2]) - (2 / 3) / 3) < 1e-15


def test_initial_atlas_without_uvs_is_seeded_noise(tmp_path, capsys):
    from st3d import cli
    verts, faces, atlas = cli.load_scene_atlas(_two_triangle_obj(tmp_path, False), 3, "cpu")
    want = (0.5 + 0.1 * torch.randn((2, 3, 3, 3), generator=torch.Generator().manual_seed(0))).clamp(0, 1)
    assert torch.equal(atlas, want) and faces.shape == (2, 3)
    assert "WARNING" not in capsys.readouterr().out


# ------------------------------------------------------------------ I/O
def test_npy_round_trip(tmp_path):
    from st3d import io
    at = torch.rand(5, 3, 3, 3)
    path = str(tmp_path / "a.npy")
    io.save_atlas(path, at)
    assert os.path.exists(path) and np.load(path).shape == (5, 3, 3, 3) and np.load(path).dtype == np.float32
    got = io.load_atlas(path)
    assert got.dtype == torch.float32 and torch.equal(got, at)
    io.save_atlas(path, at.double().requires_grad_(True))
    assert torch.equal(io.load_atlas(path), at)
    for n, bad in enumerate((np.zeros((5, 3, 3)), np.zeros((5, 3, 2, 3)), np.zeros((5, 3, 3, 4)), np.zeros((5, 65, 65, 3)),
                             np.zeros((5, 2, 2, 3), np.int32))):
        q = str(tmp_path / f"bad{n}.npy")
        np.save(q, bad)
        with pytest.raises(ValueError):
            io.load_atlas(q)
    with pytest.raises(ValueError):
        io.save_atlas(path, torch.rand(5, 3, 2, 3))


def test_final_export_writes_geometry_texels_and_the_soup(tmp_path, monkeypatch):
    from st3d import cli, io
    mesh, _ = _cpu_mesh(atlas=torch.rand(2, 3, 3, 3))
    out = str(tmp_path)
    said = cli.export_atlas_mesh(out, mesh)
    assert "18 faces" in said
    vlines = [ln.split() for ln in open(os.path.join(out, "final.obj")) if ln.startswith("v ")]
    assert len(vlines) == 4 and all(len(t) == 4 for t in vlines) and not os.path.exists(os.path.join(out, "final.mtl"))
    assert torch.equal(io.load_atlas(os.path.join(out, "final_atlas.npy")), mesh.textures.atlas_packed())
    clines = [ln.split() for ln in open(os.path.join(out, "final_colored.obj")) if ln.startswith("v ")]
    assert len(clines) == 3 * 18 and all(len(t) == 7 for t in clines)
    assert len([ln for ln in open(os.path.join(out, "final_colored.obj")) if ln.startswith("f ")]) == 18
    col = io.load_vertex_colors(os.path.join(out, "final_colored.obj"))
    assert (col.reshape(2, 3, 3, 3, 3)[:, :, :, 0] - mesh.textures.atlas_packed()).abs().max() <= 5e-7 + 2.0 ** -24
    # (six decimal places: half a step, and the fp32 rounding of the value read back)
    # past the limit the soup is skipped, and the export says so
    assert io.ATLAS_SOUP_MAX_FACES == 2 ** 20
    monkeypatch.setattr(io, "ATLAS_SOUP_MAX_FACES", 17)
    os.remove(os.path.join(out, "final_colored.obj"))
    said = cli.export_atlas_mesh(out, mesh)
    assert "skipped" in said and "18" in said and not os.path.exists(os.path.join(out, "final_colored.obj"))
    assert os.path.exists(os.path.join(out, "final_atlas.npy"))


def _fake_run(tmp_path, atlas_r, atlas):
    """the part of cli.Run that save_checkpoint / load_checkpoint / current_mesh touch, on the CPU"""
    import utils as U
    from st3d import cli
    verts = torch.rand(4, 3)
    state = {"step": 3}
    optimizer = types.SimpleNamespace(state_dict=lambda: dict(state), load_state_dict=lambda d: state.update(d))
    run = types.SimpleNamespace(main=True, pyramid=None, atlas_r=atlas_r, vertex_colors=False, out_dir=str(tmp_path), device="cpu",
                                args=types.SimpleNamespace(optimization_target="texture"), optimizer=optimizer, _utils=U,
                                opt={"atlas": atlas, "verts": verts, "faces": torch.tensor([[0, 1, 2], [1, 3, 2]])},
                                say=lambda msg: None, progress=0)
    run.texture_key = cli.Run.texture_key.fget(run)
    return run


def test_checkpoint_records_the_atlas_and_resume_checks_it(tmp_path):
    from st3d import cli
    from st3d import render as R
    at = torch.rand(2, 4, 4, 3)
    run = _fake_run(tmp_path, 4, at.clone())
    assert run.texture_key == "atlas"
    mesh = cli.Run.current_mesh(run)
    assert isinstance(mesh.textures, R.TexturesAtlas) and mesh.textures.atlas_packed() is run.opt["atlas"]
    cli.Run.save_checkpoint(run, 7)
    path = os.path.join(str(tmp_path), "checkpoint.pt")
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert blob["texture_atlas"] == 4 and torch.equal(blob["atlas"], at) and blob["texture_type"] == "uv" and "texture_map" not in blob
    again = _fake_run(tmp_path, 4, torch.zeros(2, 4, 4, 3))
    cli.Run.load_checkpoint(again, path)
    assert torch.equal(again.opt["atlas"], at) and again.progress == 7
    for other, key in ((0, "texture_map"), (2, "atlas")):
        wrong = _fake_run(tmp_path, other, torch.zeros(2, 2, 2, 3))
        wrong.texture_key = key
        with pytest.raises(ValueError, match="--texture_atlas 4, this run has %d" % other):
            cli.Run.load_checkpoint(wrong, path)
    # a checkpoint from before the flag counts as --texture_atlas 0
    del blob["texture_atlas"]
    torch.save(blob, path)
    with pytest.raises(ValueError, match="--texture_atlas 0, this run has 4"):
        cli.Run.load_checkpoint(again, path)
