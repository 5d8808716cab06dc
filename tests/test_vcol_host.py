"""Host side of per-vertex colours: the TexturesVertex container, setup_optimizations / finalize_mesh / the texture
regularisers on such a mesh, what the renderer refuses before any launch, --texture_type on the three scripts and the
initial colours it starts from, the OBJ round trip, and the C ABI's argument checks.  No GPU: CPU tensors and stubbed
launches (anything that reached a kernel would raise St3dError('no CPU fallback'))."""
import types

import pytest
import torch


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def _cpu_mesh(z=3.0, colours=None):
    from st3d import render as R
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    faces = torch.tensor([[0, 1, 2], [1, 3, 2]])
    tex = R.TexturesVertex(torch.rand(4, 3) if colours is None else colours)
    return R.Meshes(verts, faces, tex), R.FoVPerspectiveCameras(T=torch.tensor([[0.0, 0, z]]))


def _renderer(shader=None, **kw):
    from st3d import render as R
    return R.MeshRenderer(R.MeshRasterizer(None, R.RasterizationSettings(image_size=8, **kw)), shader or R.SoftPhongShader())


# ------------------------------------------------------------------ 3. the container
def test_textures_vertex_shapes_clone_detach():
    from st3d import render as R
    import utils as U
    assert U.TexturesVertex is R.TexturesVertex
    c = torch.rand(5, 3)
    for given in (c, c[None], [c], (c,)):
        t = R.TexturesVertex(given)
        assert t.verts_features_packed().shape == (5, 3) and t.verts_features_padded().shape == (1, 5, 3)
        assert t.verts_features_packed().data_ptr() == c.data_ptr()                 # views, no copy
        assert t.verts_features_padded().data_ptr() == c.data_ptr()
    t = R.TexturesVertex(verts_features=c)
    k = t.clone()
    assert torch.equal(k.verts_features_packed(), c) and k.verts_features_packed().data_ptr() != c.data_ptr()
    leaf = c.clone().requires_grad_(True)
    t = R.TexturesVertex(leaf)
    assert t.verts_features_packed() is leaf and t.clone().verts_features_packed().requires_grad
    d = t.detach().verts_features_packed()
    assert not d.requires_grad and d.data_ptr() == leaf.data_ptr()
    for bad in (torch.rand(5), torch.rand(5, 4), torch.rand(2, 5, 3), torch.rand(1, 1, 5, 3), [c, c], []):
        with pytest.raises(ValueError):
            R.TexturesVertex(bad)


def test_wrong_vertex_count_is_a_value_error():
    from st3d import render as R
    import utils as U
    verts, faces = torch.rand(4, 3), torch.tensor([[0, 1, 2], [1, 3, 2]])
    for n in (3, 5):
        with pytest.raises(ValueError, match="one row per vertex"):
            R.Meshes(verts, faces, R.TexturesVertex(torch.rand(n, 3)))
        with pytest.raises(ValueError, match="one row per vertex"):
            U.build_mesh_vertex(torch.rand(n, 3), verts, faces)
    mesh, cams = _cpu_mesh()
    mesh.textures = R.TexturesVertex(torch.rand(3, 3))          # swapped behind the constructor's back: render time refuses too
    with pytest.raises(ValueError, match="one row per vertex"):
        _renderer().render(mesh, cams)
    # an out-of-range face index is caught by Meshes.faces_i32 before any launch
    bad = R.Meshes(verts, torch.tensor([[0, 1, 4]]), R.TexturesVertex(torch.rand(4, 3)))
    with pytest.raises(ValueError, match="faces holds indices outside"):
        _renderer().render(bad, cams)
    m = U.build_mesh_vertex(torch.rand(1, 4, 3), verts, faces)
    assert isinstance(m.textures, R.TexturesVertex) and m.clone().textures.verts_features_packed().shape == (4, 3)
    assert isinstance(m.detach().textures, R.TexturesVertex)


# ------------------------------------------------------------------ 4. setup_optimizations, finalize_mesh, regularisers
def test_setup_optimizations_leaves_per_target():
    import utils as U
    col = torch.rand(4, 3)
    mesh, _ = _cpu_mesh(colours=col)
    for target, leaves in (("texture", ["verts_features"]), ("mesh", ["verts"]), ("both", ["verts", "verts_features"])):
        for out in (U.setup_optimizations(target, mesh, 0.01), U.setup_optimizations(target, mesh, 0.01, 1)):
            assert sorted(out) == ["faces", "optimizable_mesh", "optimizer", "verts", "verts_features"]
            assert [id(p) for p in out["optimizer"].params] == [id(out[k]) for k in leaves]
            assert out["verts_features"].requires_grad == ("verts_features" in leaves)
            assert out["verts"].requires_grad == ("verts" in leaves)
            assert torch.equal(out["verts_features"].detach(), col) and out["verts_features"].shape == (4, 3)
            assert out["verts_features"].data_ptr() != col.data_ptr()           # a clone: the content mesh stays as it is
            assert out["optimizer"].lr == 0.01 and len(out["optimizer"].param_groups) == 1
            again = U.build_mesh_vertex(out["verts_features"], out["verts"], out["faces"])
            assert again.textures.verts_features_packed() is out["verts_features"]
    for levels in (0, 2, 3):
        for target in ("texture", "both", "mesh"):
            with pytest.raises(ValueError, match="texture_pyramid_levels"):
                U.setup_optimizations(target, mesh, 0.01, texture_pyramid_levels=levels)
    with pytest.raises(UnboundLocalError):
        U.setup_optimizations("nothing", mesh, 0.01)


def test_finalize_mesh_clamps_the_colours():
    import utils as U
    from st3d import render as R
    col = torch.tensor([[-0.5, 0.25, 1.5], [0.0, 1.0, 2.0], [0.5, 0.5, 0.5], [-1.0, 3.0, 0.75]], requires_grad=True)
    mesh, _ = _cpu_mesh(colours=col)
    final = U.finalize_mesh(mesh)
    assert isinstance(final.textures, R.TexturesVertex)
    got = final.textures.verts_features_packed()
    assert not got.requires_grad and torch.equal(got, col.detach().clamp(0, 1))
    assert torch.equal(final.verts_packed(), mesh.verts_packed()) and torch.equal(final.faces_packed(), mesh.faces_packed())


def test_texture_regularisers_read_the_colours(monkeypatch):
    import losses as L
    seen = []
    monkeypatch.setattr(L, "_on_gpu", lambda t: t.to(torch.float32))

    def fake_apply(x, op, *extra):
        seen.append((x, op, extra))
        return x.sum()
    monkeypatch.setattr(L, "_FusedLossFn", types.SimpleNamespace(apply=fake_apply))
    col = torch.rand(4, 3)
    mesh, _ = _cpu_mesh(colours=col)
    L.rgb_range_loss(mesh)
    L.texture_l2_loss(mesh, col.clone())
    assert seen[0][0] is col and seen[0][1] is L._ops.range_loss
    assert seen[1][0] is col and seen[1][1] is L._l2_to and seen[1][2][0].shape == (4, 3)
    with pytest.raises(ValueError, match="no pixel grid"):
        L.compute_tv_loss(mesh, torch.ones(1, 1, 8, 8))


# ------------------------------------------------------------------ 5. refusals before any launch
def test_every_limitation_is_refused_before_a_launch():
    from st3d import render as R
    mesh, cams = _cpu_mesh()
    for lights in (R.PointLights(), R.DirectionalLights(), R.HeadLights(), R.AmbientLights(ambient_color=((0.5, 0.5, 0.5),))):
        with pytest.raises(NotImplementedError, match="TexturesVertex.*unlit"):
            _renderer().render(mesh, cams, lights=lights)
    with pytest.raises(NotImplementedError, match="TexturesVertex.*unlit"):
        _renderer(R.SoftPhongShader(lights=R.PointLights())).render(mesh, cams)
    with pytest.raises(NotImplementedError, match="TexturesVertex.*unlit"):
        _renderer().render(mesh, cams, lights=R.AmbientLights(), materials=R.Materials(ambient_color=((0.5, 0.5, 0.5),)))
    for a in (2, 3, 4):
        with pytest.raises(NotImplementedError, match="TexturesVertex.*supersample"):
            _renderer(supersample=a).render(mesh, cams)
    for kw in (dict(texture_mip_levels=0), dict(texture_mip_levels=2), dict(texture_mip_levels=0, texture_lod_bias=0.5)):
        with pytest.raises(NotImplementedError, match="TexturesVertex.*texture_mip_levels"):
            _renderer(**kw).render(mesh, cams)
    for kw in (dict(faces_per_pixel=2), dict(blur_radius=1e-4), dict(clip_barycentric_coords=True), dict(cull_backfaces=True),
               dict(z_clip_value=0.5), dict(perspective_correct=False)):
        with pytest.raises(NotImplementedError, match="TexturesVertex.*hard settings"):
            _renderer(**kw).render(mesh, cams)
    for bp in (R.BlendParams(sigma=1e-3), R.BlendParams(gamma=1e-3), R.BlendParams(background_color=(0.0, 0.0, 0.0))):
        with pytest.raises(NotImplementedError, match="TexturesVertex.*hard settings"):
            _renderer(R.SoftPhongShader(blend_params=bp)).render(mesh, cams)
    # colours through the silhouette rasteriser: refused at construction (any mesh) and, handed to render_views, by name
    srs = R.SilhouetteRasterizationSettings(image_size=8, faces_per_pixel=50)
    with pytest.raises(NotImplementedError, match="SoftSilhouetteShader"):
        R.MeshRenderer(R.MeshRasterizer(None, srs), R.SoftPhongShader())
    with pytest.raises(NotImplementedError, match="TexturesVertex"):
        R.render_views(mesh, cams.R, cams.T, 8, srs)
    # white ambient light is the unlit route: it gets as far as the kernels
    for lights in (None, R.AmbientLights()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _renderer().render(mesh, cams, lights=lights)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.render_views(mesh, cams.R, cams.T, 8)


def test_a_silhouette_render_needs_no_colours(monkeypatch):
    """SoftSilhouetteShader on a TexturesVertex mesh goes where it goes for any mesh: the silhouette functions, with the
    mesh's vertices and faces and nothing of its textures"""
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
    from st3d import render as R
    mesh, cams = _cpu_mesh(z=0.3)
    for policy in ("clip", "raise"):
        monkeypatch.setattr(ops, "NEAR_PLANE_POLICY", policy)
        try:
            with pytest.raises(RuntimeError, match="near clipping plane.*TexturesVertex"):
                _renderer().render(mesh, cams)
            assert not ops.near_plane_triggered()
        finally:
            ops.reset_near_plane()


def test_routing(monkeypatch):
    """a TexturesVertex mesh is _VertexColourRenderFn and nothing else; a TexturesUV mesh is _RenderFn with its old arguments"""
    from st3d import render as R
    calls = []

    def fake(name, s_at):
        def apply(*a):
            calls.append((name, a))
            return torch.zeros(1, 3, a[s_at], a[s_at]), torch.zeros(1, 1, a[s_at], a[s_at])
        return types.SimpleNamespace(apply=apply)
    monkeypatch.setattr(R, "_RenderFn", fake("uv", 7))
    monkeypatch.setattr(R, "_VertexColourRenderFn", fake("vertex", 5))
    mesh, cams = _cpu_mesh()
    rgb, mask = _renderer().render(mesh, cams)
    _renderer().render(mesh, cams, lights=R.AmbientLights())
    assert [c[0] for c in calls] == ["vertex", "vertex"]
    a = calls[0][1]
    assert len(a) == 6 and a[0] is mesh.verts_packed() and a[1] is mesh.textures.verts_features_packed()
    assert a[2].dtype == torch.int32 and a[2].tolist() == [[0, 1, 2], [1, 3, 2]] and a[5] == 8
    assert R.flat_of(rgb) == (1.0, 1.0, 1.0)
    calls.clear()
    uv = R.Meshes(mesh.verts_packed(), mesh.faces_packed(),
                  R.TexturesUV(maps=torch.rand(1, 8, 8, 3), faces_uvs=mesh.faces_packed()[None], verts_uvs=torch.rand(1, 4, 2)))
    _renderer().render(uv, cams)
    assert [c[0] for c in calls] == ["uv"] and len(calls[0][1]) == 9 and calls[0][1][8] is None


def test_ops_wrappers_check_before_the_library():
    from st3d import _lib, ops
    frag = (torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8))
    faces, col = torch.zeros(2, 3, dtype=torch.int32), torch.rand(4, 3)
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        ops.shade_vc_fwd(frag, faces, torch.rand(4, 2))
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        ops.shade_vc_fwd(frag, torch.zeros(2, 4, dtype=torch.int32), col)
    with pytest.raises(ValueError, match="grad_rgb"):
        ops.shade_vc_bwd(torch.rand(1, 3, 4, 4), frag, faces, col)
    with pytest.raises(ValueError, match="nothing asked for"):
        ops.shade_vc_bwd(torch.rand(1, 3, 8, 8), frag, faces, col, want_colours=False, want_bary=False)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_vc_fwd(frag, faces, col)
    with pytest.raises(_lib.St3dError, match="no CPU fallback"):
        ops.shade_vc_bwd(torch.rand(1, 3, 8, 8), frag, faces, col, want_bary=True)


def test_c_abi_validates_before_any_launch():
    from st3d import _lib
    lib = _lib.load()
    one = 16        # any non-NULL value: the checks below fail before a pointer is followed
    p = [one] * 6
    assert lib.st3d_shade_vc_fwd(*p, 1, 8, 2, 4, one, None, None) == -1 and b"invalid argument" in lib.st3d_last_error()
    assert lib.st3d_shade_vc_fwd(*p, 1, 8, 2, 4, None, one, None) == -1
    for k in range(6):
        q = list(p)
        q[k] = None
        assert lib.st3d_shade_vc_fwd(*q, 1, 8, 2, 4, one, one, None) == -1
    for B, S, F, V in ((0, 8, 2, 4), (1, 0, 2, 4), (1, 8, 0, 4), (1, 8, 2, 0), (-1, 8, 2, 4), (1, 8, 2, -3), (1, 4097, 2, 4)):
        assert lib.st3d_shade_vc_fwd(*p, B, S, F, V, one, one, None) == -1
        assert lib.st3d_shade_vc_bwd(one, *p, B, S, F, V, one, one, None) == -1
        assert lib.st3d_shade_vc_bwd_det(one, *p, B, S, F, V, one, one, one, 1 << 30, None) == -1
    g = [one] * 7
    assert lib.st3d_shade_vc_bwd(*g, 1, 8, 2, 4, None, None, None) == -1                  # nothing wanted
    for k in range(7):
        q = list(g)
        q[k] = None
        assert lib.st3d_shade_vc_bwd(*q, 1, 8, 2, 4, one, one, None) == -1
        assert lib.st3d_shade_vc_bwd_det(*q, 1, 8, 2, 4, one, one, 16, 1 << 20, None) == -1
    need = lib.st3d_shade_vc_bwd_det_workspace_bytes(4)
    assert need >= 16 + 4 * 1024 + 8 * 12 and lib.st3d_shade_vc_bwd_det_workspace_bytes(0) == 0
    assert lib.st3d_shade_vc_bwd_det_workspace_bytes(-5) == 0
    assert lib.st3d_shade_vc_bwd_det(*g, 1, 8, 2, 4, None, one, 16, need, None) == -1      # fixed point of nothing
    assert lib.st3d_shade_vc_bwd_det(*g, 1, 8, 2, 4, one, one, None, need, None) == -1     # no workspace
    assert lib.st3d_shade_vc_bwd_det(*g, 1, 8, 2, 4, one, one, 16, need - 1, None) == -1   # workspace too small
    assert lib.st3d_shade_vc_bwd_det(*g, 1, 8, 2, 4, one, one, 24, need, None) == -1       # misaligned


# ------------------------------------------------------------------ 6. CLI
@pytest.mark.parametrize("k", [0, 1, 2])
def test_flag_reaches_all_three_scripts(k):
    p = _scripts()[k].build_parser()
    assert p.parse_args([]).texture_type == "uv"
    assert p.parse_args(["--texture_type", "uv"]).texture_type == "uv"
    a = p.parse_args(["--texture_type", "vertex", "--optimization_target", "both", "--verts_lr", "0.001"])
    assert a.texture_type == "vertex"
    refused = [["--texture_type", "atlas"], ["--texture_type", "vertex", "--texture_pyramid_levels", "0"],
               ["--texture_type", "vertex", "--texture_pyramid_levels", "3", "--size", "64"],
               ["--texture_type", "vertex", "--texture_mip_levels", "0"], ["--texture_type", "vertex", "--texture_mip_levels", "2"],
               ["--texture_type", "vertex", "--supersample", "2"], ["--texture_type", "vertex", "--lights", "point"],
               ["--texture_type", "vertex", "--lights", "directional"], ["--texture_type", "vertex", "--lights", "headlight"]]
    if k == 1:          # the regulariser flags exist on second_approach.py alone
        refused.append(["--texture_type", "vertex", "--tv_weight", "0.5"])
        assert p.parse_args(["--texture_type", "vertex", "--texture_l2_weight", "0.5", "--rgb_range_weight", "1"]).texture_type == "vertex"
        assert p.parse_args(["--texture_type", "uv", "--tv_weight", "0.5"]).tv_weight == 0.5
    for argv in refused:
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_check_args_names_the_conflict():
    from st3d import cli
    base = dict(silhouette_weight=0.0, optimization_target="texture", silhouette_sigma=1e-4, silhouette_faces_per_pixel=None,
                texture_pyramid_levels=1, size=768, supersample=1, texture_mip_levels=1, texture_lod_bias=0.0, lights="ambient",
                resize_texture=True, texture_type="vertex", tv_weight=0.0)
    ns = lambda **kw: types.SimpleNamespace(**dict(base, **kw))      # noqa: E731
    assert cli.check_args(ns()) is None and cli.check_args(ns(optimization_target="both")) is None
    assert cli.check_args(ns(silhouette_weight=1.0, optimization_target="mesh")) is None
    for kw, word in ((dict(texture_pyramid_levels=0), "texture_pyramid_levels"), (dict(texture_mip_levels=0), "texture_mip_levels"),
                     (dict(supersample=2), "supersample"), (dict(lights="point"), "lights"), (dict(tv_weight=0.1), "tv_weight")):
        msg = cli.check_args(ns(**kw))
        assert msg and "texture_type vertex" in msg and word in msg, (kw, msg)
        assert cli.check_args(ns(texture_type="uv", **kw)) is None
    names = {f.name: (f.default, f.choices) for f in cli.SHARED_FLAGS}
    assert names["texture_type"] == ("uv", ["uv", "vertex"])


def _two_triangle_obj(tmp_path, with_uvs):
    from PIL import Image
    import numpy as np
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
    lines += ["v 0 0 0", "v 1 0 0", "v 1 1 0", "v 0 1 0", "v 5 5 5"]          # vertex 5: used by no face
    if with_uvs:
        # vt 1..5; vertex 2's first corner (face 1, corner 2) has vt 2, its second (face 2) vt 5 -- the first one counts
        lines += ["vt 0 0", "vt 1 0", "vt 1 1", "vt 0.5 0.5", "vt 0.25 0.75"]
        lines += ["f 1/1 2/2 3/3", "f 1/4 3/3 4/5"]
    else:
        lines += ["f 1 2 3", "f 1 3 4"]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_initial_colours_from_a_map(tmp_path):
    from st3d import cli
    verts, faces, col = cli.load_scene_vertex(_two_triangle_obj(tmp_path, True), "cpu")
    assert verts.shape == (5, 3) and faces.tolist() == [[0, 1, 2], [0, 2, 3]] and col.shape == (5, 3) and col.dtype == torch.float32
    # by hand: colour(u, v) = (u, 1 - v, 1) -- column = 3 u, and v = 1 is row 0 (rows flipped), whose green is 0
    want = torch.tensor([[0.0, 1.0, 1.0],         # vertex 1: vt (0, 0), its first corner -- not vt 4 of the second face
                         [1.0, 1.0, 1.0],         # vertex 2: vt (1, 0)
                         [1.0, 0.0, 1.0],         # vertex 3: vt (1, 1)
                         [0.25, 0.25, 1.0],       # vertex 4: vt (0.25, 0.75): between columns 0 and 1, rows 0 and 1
                         [0.5, 0.5, 0.5]])        # used by no face
    assert (col - want).abs().max() <= 1e-6, col
    # outside [0,1] clamps to the border
    c = cli.vertex_colors_from_map(3, torch.tensor([[0, 1, 2]]), torch.tensor([[-1.0, 2.0], [2.0, -1.0], [0.5, 0.5]]),
                                   torch.tensor([[0, 1, 2]]), torch.tensor([[[0.0, 0, 0], [1, 0, 0]], [[0, 1, 0], [1, 1, 1]]]))
    assert torch.allclose(c, torch.tensor([[0.0, 0, 0], [1.0, 1, 1], [0.5, 0.5, 0.25]]), atol=1e-6)


def test_initial_colours_without_uvs_are_seeded_noise(tmp_path, capsys):
    from st3d import cli
    verts, faces, col = cli.load_scene_vertex(_two_triangle_obj(tmp_path, False), "cpu")
    want = (0.5 + 0.1 * torch.randn((5, 3), generator=torch.Generator().manual_seed(0))).clamp(0, 1)
    assert torch.equal(col, want) and faces.shape == (2, 3)
    assert "WARNING" not in capsys.readouterr().out


# ------------------------------------------------------------------ 7. I/O
def test_obj_round_trip_with_colours(tmp_path):
    from st3d import io
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0.5], [0, 1, -2]])
    faces = torch.tensor([[0, 1, 2]])
    col = torch.tensor([[0.123456, 0.5, 1.0], [-0.25, 1.75, 0.0], [0.333333, 0.666667, 0.999999]])
    path = str(tmp_path / "c.obj")
    io.save_obj(path, verts, faces, verts_colors=col)
    assert not (tmp_path / "c.mtl").exists() and not (tmp_path / "c.png").exists()
    vlines = [ln.split() for ln in open(path) if ln.startswith("v ")]
    assert len(vlines) == 3 and all(len(t) == 7 for t in vlines) and vlines[0][4] == "0.123456" and vlines[1][4] == "0.000000"
    got = io.load_vertex_colors(path)
    assert got.shape == (3, 3) and got.dtype == torch.float32 and (got - col.clamp(0, 1)).abs().max() <= 5e-7
    v2, f2, aux = io.load_obj(path)                         # load_obj stays as it is: positions and faces, no colours
    assert torch.allclose(v2, verts) and f2.verts_idx.tolist() == [[0, 1, 2]] and aux.verts_uvs is None
    assert len(aux) == 5 and aux._fields == ("normals", "verts_uvs", "material_colors", "texture_images", "texture_atlas")
    io.save_obj(path, verts, faces, decimal_places=3, verts_colors=col)
    assert open(path).read().splitlines()[0] == "v 0.000 0.000 0.000 0.123 0.500 1.000"
    plain = str(tmp_path / "p.obj")
    io.save_obj(plain, verts, faces)
    assert io.load_vertex_colors(plain) is None
    with pytest.raises(ValueError):
        io.save_obj(path, verts, faces, verts_colors=col[:2])
