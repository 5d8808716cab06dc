"""Host-side lighting: PyTorch3D defaults and validation of the light / material objects, the routing between the unlit
and the lit kernels, the vertex incidence list, the CLI flags, and the fp64 restatement (tests/_phong_ref.py) pinned to
analytic cases.  No GPU."""
import math

import pytest
import torch

import _phong_ref as PR
from st3d import render as R


def _close(a, b):
    return torch.allclose(torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32))


def test_constructor_defaults_are_pytorch3ds():
    p = R.PointLights()
    assert _close(p.ambient_color, [[0.5] * 3]) and _close(p.diffuse_color, [[0.3] * 3])
    assert _close(p.specular_color, [[0.2] * 3]) and _close(p.location, [[0, 1, 0]])
    d = R.DirectionalLights()
    assert _close(d.ambient_color, [[0.5] * 3]) and _close(d.diffuse_color, [[0.3] * 3])
    assert _close(d.specular_color, [[0.2] * 3]) and _close(d.direction, [[0, 1, 0]])
    a = R.AmbientLights()
    assert _close(a.ambient_color, [[1] * 3]) and _close(a.diffuse_color, [[0] * 3]) and _close(a.specular_color, [[0] * 3])
    m = R.Materials()
    assert _close(m.ambient_color, [[1] * 3]) and _close(m.diffuse_color, [[1] * 3]) and _close(m.specular_color, [[1] * 3])
    assert float(m.shininess) == 64.0


def test_ambient_lights_accept_any_colour():
    assert _close(R.AmbientLights(ambient_color=((0.2, 0.4, 0.6),)).ambient_color, [[0.2, 0.4, 0.6]])


def test_light_count_must_be_one_or_the_batch():
    lit = R.lighting_of(R.PointLights(location=[[0, 1, 0], [1, 0, 0], [0, 0, 1]]), None, "cpu")
    assert lit.n == 3
    v = torch.zeros(4, 3)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    with pytest.raises(ValueError):
        R._lit_setup(lit, v, v, f, torch.eye(3)[None].expand(2, 3, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError):       # N of the parameters disagree
        R.PointLights(location=[[0, 1, 0], [1, 0, 0]], diffuse_color=[[1, 1, 1]] * 3)
    with pytest.raises(ValueError):
        R.PointLights(location=[[0, 1]])


@pytest.mark.parametrize("make", [
    lambda t: R.PointLights(location=t), lambda t: R.DirectionalLights(direction=t), lambda t: R.AmbientLights(ambient_color=t),
    lambda t: R.Materials(diffuse_color=t), lambda t: R.Materials(shininess=torch.tensor(8.0, requires_grad=True))])
def test_parameters_that_require_grad_raise(make):
    with pytest.raises(NotImplementedError):
        make(torch.ones(1, 3, requires_grad=True))


def test_requires_grad_set_after_construction_raises_at_render():
    p = R.PointLights()
    p.location.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        R.lighting_of(p, None, "cpu")


def test_routing_unlit_and_lit():
    # today's kernels: nothing, white ambient, white ambient with default Materials (any shininess / diffuse)
    for lights, mats in ((None, None), (R.AmbientLights(), None), (R.AmbientLights(), R.Materials()),
                         (R.AmbientLights(), R.Materials(shininess=3, diffuse_color=((0.1, 0.2, 0.3),)))):
        assert R.lighting_of(lights, mats, "cpu") is None
    # lit kernels
    assert R.lighting_of(R.AmbientLights(ambient_color=((0.5, 1, 1),)), None, "cpu").kind == 0
    assert R.lighting_of(R.AmbientLights(), R.Materials(ambient_color=((0.5, 0.5, 0.5),)), "cpu").kind == 0
    assert R.lighting_of(R.PointLights(), None, "cpu").kind == 1
    assert R.lighting_of(R.DirectionalLights(), None, "cpu").kind == 2
    assert R.lighting_of(R.HeadLights(), None, "cpu").kind == 3
    assert R.lighting_of(R.PointLights(ambient_color=((1, 1, 1),), diffuse_color=((0, 0, 0),),
                                       specular_color=((0, 0, 0),)), None, "cpu").kind == 1


def test_light_block_layout_and_bound():
    lit = R.lighting_of(R.PointLights(ambient_color=((0.1, 0.2, 0.3),), diffuse_color=((1, 2, 3),),
                                      specular_color=((4, 5, 6),), location=((7, 8, 9),)),
                        R.Materials(ambient_color=((2, 2, 2),), diffuse_color=((0.5, 0.5, 0.5),),
                                    specular_color=((3, 3, 3),), shininess=9), "cpu")
    b = lit.block[0].tolist()
    assert b[0:12] == pytest.approx([0.1, 0.2, 0.3, 1, 2, 3, 4, 5, 6, 7, 8, 9])
    assert b[12:22] == pytest.approx([2, 2, 2, 0.5, 0.5, 0.5, 3, 3, 3, 9])
    assert lit.weight_bound == pytest.approx(0.6 + 1.5)        # max_c |ka La| + |kd Ld|


def test_lighting_is_packed_once_per_object():
    p, m = R.PointLights(), R.Materials()
    assert R.lighting_of(p, m, "cpu") is R.lighting_of(p, m, "cpu")


def test_incidence_lists_every_face_corner_once_in_ascending_order():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [3, 4, 0], [1, 4, 2]], dtype=torch.int32)
    off, ref = R.vertex_incidence(faces, 5)
    assert sorted(ref.tolist()) == list(range(12))
    flat = faces.reshape(-1).tolist()
    for v in range(5):
        row = ref[off[v]:off[v + 1]].tolist()
        assert row == sorted(row) and all(flat[q] == v for q in row)
        assert len(row) == flat.count(v)


def test_restatement_normals_of_a_tetrahedron_and_a_cube():
    # tetrahedron with outward winding: the normal of a corner is the normalised sum of its three area-weighted face normals
    v = torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    n = PR.vertex_normals(v, f)
    # PyTorch3D's (v2 - v1) x (v0 - v1) of a counter-clockwise face points outwards: by symmetry n_v = v / |v|
    torch.testing.assert_close(n, v / math.sqrt(3.0) * torch.sign((n * v).sum(1, keepdim=True)))
    assert torch.allclose(n.norm(dim=1), torch.ones(4, dtype=torch.float64))
    # unit cube, two triangles per side, all wound alike: every corner's normal points along its diagonal
    c = torch.tensor([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=torch.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = torch.tensor([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))])
    nc = PR.vertex_normals(c, tris)
    d = (c - 0.5) / (c - 0.5).norm(dim=1, keepdim=True)
    s = torch.sign((nc * d).sum(1))
    assert bool((s == s[0]).all())
    # each corner touches 3 sides but a varying number of their triangles: the area weights still sum to the diagonal up
    # to a per-side weight in {1, 2} x 0.5; all normals lie in the corner's octant
    assert bool(((nc * d * s[0]) > 0).all(dim=1).all())


def _one_triangle(tilt):
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, math.cos(tilt), math.sin(tilt)]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]])
    return v, f


def test_restatement_diffuse_is_kd_ld_cos():
    v, f = _one_triangle(0.3)
    n = PR.vertex_normals(v, f)
    N = n[0:1]
    P = torch.tensor([[0.2, 0.2, 0.0]], dtype=torch.float64)
    d = torch.tensor([0.3, 0.5, 0.8], dtype=torch.float64)
    d = d / d.norm()
    light = dict(kind="directional", ambient=torch.zeros(3, dtype=torch.float64), diffuse=torch.tensor([0.7, 0.6, 0.5]).double(),
                 specular=torch.zeros(3, dtype=torch.float64), direction=d)
    mat = dict(ambient=torch.ones(3).double(), diffuse=torch.tensor([0.9, 0.8, 0.2]).double(), specular=torch.ones(3).double(),
               shininess=64.0)
    ad, sp = PR.phong(N, P, torch.tensor([0, 0, 5.0]).double(), light, mat)
    cos = float((N[0] / N[0].norm()) @ d)
    torch.testing.assert_close(ad[0], mat["diffuse"] * light["diffuse"] * max(cos, 0.0))
    assert float(sp.abs().max()) == 0.0


def test_restatement_specular_peak_at_the_mirror_direction_and_zero_behind():
    N = torch.tensor([[0, 0, 2.0]], dtype=torch.float64)         # unnormalised on purpose
    P = torch.zeros(1, 3, dtype=torch.float64)
    l = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
    C = torch.tensor([-0.6, 0.0, 0.8], dtype=torch.float64) * 3.0  # the mirror of l about n
    ks, Ls = torch.tensor([0.5, 0.25, 1.0]).double(), torch.tensor([0.2, 0.4, 0.6]).double()
    light = dict(kind="point", ambient=torch.zeros(3).double(), diffuse=torch.zeros(3).double(), specular=Ls, location=l * 4)
    for sh in (1.0, 64.0):
        mat = dict(ambient=torch.ones(3).double(), diffuse=torch.ones(3).double(), specular=ks, shininess=sh)
        _, sp = PR.phong(N, P, C, light, mat)
        torch.testing.assert_close(sp[0], ks * Ls)
        # light behind the surface: n.l <= 0 -> no specular even where e.r > 0
        light_b = dict(light, location=-l * 4)
        _, spb = PR.phong(N, P, -C, light_b, mat)
        assert float(spb.abs().max()) == 0.0


def test_restatement_normalize_eps_branch():
    x = torch.tensor([[1e-8, 0.0, 0.0], [3.0, 4.0, 0.0]], dtype=torch.float64)
    torch.testing.assert_close(PR.normalize(x), torch.tensor([[1e-2, 0, 0], [0.6, 0.8, 0]], dtype=torch.float64))


def test_cli_lighting_flags():
    from st3d import cli
    p = cli.make_parser([])
    a = p.parse_args([])
    assert a.lights == "ambient" and a.light_xyz == [0.0, 1.0, 0.0] and a.shininess == 64.0
    lights, mats = cli.make_lights(a, "cpu")
    assert isinstance(lights, R.AmbientLights) and mats is None and R.lighting_of(lights, mats, "cpu") is None
    a = p.parse_args(["--lights", "point", "--light_xyz", "1", "2", "3", "--shininess", "8"])
    lights, mats = cli.make_lights(a, "cpu")
    assert isinstance(lights, R.PointLights) and _close(lights.location, [[1, 2, 3]]) and float(mats.shininess) == 8.0
    a = p.parse_args(["--lights", "directional", "--light_xyz", "0", "0", "1"])
    lights, _ = cli.make_lights(a, "cpu")
    assert isinstance(lights, R.DirectionalLights) and _close(lights.direction, [[0, 0, 1]])
    lights, _ = cli.make_lights(p.parse_args(["--lights", "headlight"]), "cpu")
    assert R.lighting_of(lights, None, "cpu").kind == 3
    with pytest.raises(SystemExit):
        p.parse_args(["--lights", "spot"])
