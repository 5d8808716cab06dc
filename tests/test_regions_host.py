"""Style regions without a GPU: the labels (validation, usemtl groups, axis slabs, .npy files), every refusal of
second_approach.py's parser, the C ABI's declarations, and the numpy restatement's own identity -- the level sums of the
regions add up to the coverage's, exactly."""
import os
import re

import numpy as np
import pytest
import torch

import _guidedref as GR
import _regionsref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _regions():
    from st3d import regions
    return regions


# ---------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_and_bound():
    from st3d import _lib
    header = open(os.path.join(ROOT, "include", "st3d.h")).read()
    for name in ("st3d_region_planes_floats", "st3d_region_planes_partials", "st3d_region_planes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["st3d_region_planes"][1]) == 10
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    assert '"regions.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]' in build       # guide.hip's flags


# ---------------------------------------------------------------------------- labels
def test_check_face_regions_validates():
    Rg = _regions()
    t, R = Rg.check_face_regions(np.array([0, 2, 1, 1, 0]), 5, device="cpu")
    assert R == 3 and t.dtype == torch.uint8 and t.tolist() == [0, 2, 1, 1, 0]
    t, R = Rg.check_face_regions(torch.zeros(4, dtype=torch.int64), 4, device="cpu")
    assert R == 1 and t.tolist() == [0, 0, 0, 0]
    t, R = Rg.check_face_regions(list(range(8)), 8, device="cpu")
    assert R == 8
    for bad, F in ((np.array([0, 1, 3]), 3),                 # label 2 names no face
                   (np.array([1, 1, 1]), 3),                 # label 0 names no face
                   (np.array([0, -1, 1]), 3),                # negative
                   (np.arange(9), 9),                        # nine regions
                   (np.array([0, 1]), 3),                    # one label per face
                   (np.array([[0, 1, 0]]), 3),               # shape
                   (np.array([0.0, 1.0, 0.0]), 3),           # floats
                   (np.array([True, False, True]), 3),       # booleans
                   (np.array([0, 1, 0]), 0)):
        with pytest.raises(ValueError):
            Rg.check_face_regions(bad, F, device="cpu")


def test_regions_from_materials_on_a_two_material_obj(tmp_path):
    from st3d import io as stio
    Rg = _regions()
    obj = tmp_path / "two.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nv 2 0 0\n"
                   "usemtl skin\nf 1 2 3\nusemtl horn\nf 2 4 3\nusemtl skin\nf 2 5 4\nf 1 2 4 3\n")
    _, faces, _ = stio.load_obj(str(obj), load_textures=False)
    labels = Rg.regions_from_materials(faces.materials_idx)
    assert labels.tolist() == [0, 1, 0, 0, 0]                 # by first appearance; the quad is two triangles
    assert Rg.count_material_groups(str(obj)) == 2
    assert Rg.labels_from_spec("material", None, faces.verts_idx, faces.materials_idx).tolist() == [0, 1, 0, 0, 0]
    # numbered by first appearance, not by name or index; faces in front of the first usemtl are a group of their own
    assert Rg.regions_from_materials(np.array([3, 3, 0, 3, 1, 0])).tolist() == [0, 0, 1, 0, 2, 1]
    assert Rg.regions_from_materials(torch.tensor([-1, 0, -1, 1])).tolist() == [0, 1, 0, 2]
    one = tmp_path / "one.obj"
    one.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl skin\nf 1 2 3\nusemtl unused\n")
    assert Rg.count_material_groups(str(one)) == 1
    _, f1, _ = stio.load_obj(str(one), load_textures=False)
    with pytest.raises(ValueError, match="at least 2"):
        Rg.labels_from_spec("material", None, f1.verts_idx, f1.materials_idx)
    with pytest.raises(ValueError):
        Rg.labels_from_spec("material", None, f1.verts_idx, None)


def test_regions_from_axis_and_a_centroid_on_a_cut():
    Rg = _regions()
    # centroids along x: -1, 0 (exactly: corners -1, 0, 1), 1/3 (corners 0, 0, 1), 2
    verts = np.array([[-1, 0, 0], [-1, 1, 0], [-1, 0, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0], [2, 0, 1],
                      [0, 5, 5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 4], [3, 5, 4], [6, 7, 8]])
    assert Rg.regions_from_axis(verts, faces, "x", [0.0]).tolist() == [0, 0, 1, 1]        # exactly on the cut: stays below
    assert Rg.regions_from_axis(verts, faces, "x", [-0.5, 0.0, 1.0]).tolist() == [0, 1, 2, 3]
    assert Rg.regions_from_axis(torch.from_numpy(verts), torch.from_numpy(faces), "x", (0.25, 0.5)).tolist() == [0, 0, 1, 2]
    assert Rg.regions_from_axis(verts, faces, "y", [0.2]).tolist() == [1, 0, 1, 1]
    assert Rg.regions_from_axis(verts, faces, "z", [10.0]).tolist() == [0, 0, 0, 0]       # an empty slab: refused with the spec
    for spec in ("z:10", "z:-10", "x:-0.5,0.1,0.2"):
        with pytest.raises(ValueError, match="holds no face"):
            Rg.labels_from_spec(spec, verts, faces)
    for axis, cuts in (("w", [0.0]), ("x", []), ("x", [0.0, 0.0]), ("x", [1.0, 0.0]), ("x", [float("nan")]),
                       ("x", [float("inf")]), ("x", list(range(8)))):
        with pytest.raises(ValueError):
            Rg.regions_from_axis(verts, faces, axis, cuts)
    assert Rg.labels_from_spec("x:-0.5,0,1", verts, faces).tolist() == [0, 1, 2, 3]


def test_npy_labels(tmp_path):
    Rg = _regions()
    p = tmp_path / "labels.npy"
    np.save(p, np.array([0, 1, 1, 0], np.int32))
    assert Rg.load_face_regions(str(p)).tolist() == [0, 1, 1, 0]
    assert Rg.labels_from_spec(str(p), None, np.zeros((4, 3))).tolist() == [0, 1, 1, 0]
    np.save(p, np.array([0.0, 1.0]))
    with pytest.raises(ValueError):
        Rg.load_face_regions(str(p))
    np.save(p, np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        Rg.load_face_regions(str(p))
    with pytest.raises(ValueError):
        Rg.labels_from_spec(str(tmp_path / "missing.npy"), None, np.zeros((4, 3)))


def test_parse_spec():
    Rg = _regions()
    assert Rg.parse_spec("material") == ("material",)
    assert Rg.parse_spec("x:0") == ("axis", "x", (0.0,))
    assert Rg.parse_spec("z:-0.25,0.5,1e1") == ("axis", "z", (-0.25, 0.5, 10.0))
    assert Rg.parse_spec("some/dir/labels.npy") == ("file", "some/dir/labels.npy")
    for bad in ("", "materials", "x", "x:", "w:0", "x:a", "x:0,0", "x:1,0", "x:nan", "labels.txt", "x:0,1,2,3,4,5,6,7"):
        with pytest.raises(ValueError):
            Rg.parse_spec(bad)


def test_region_weights():
    import style_transfer as ST
    assert ST.check_region_weights(None, 3) == (1.0, 1.0, 1.0)
    assert ST.check_region_weights([0, 2.5], 2) == (0.0, 2.5)
    for bad, R in (([1.0], 2), ([1.0, -1.0], 2), ([1.0, float("nan")], 2), ([1.0, float("inf")], 2), (["a", 1], 2)):
        with pytest.raises(ValueError):
            ST.check_region_weights(bad, R)
    assert list(ST.REGION_STYLE_TAPS.values()) == ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]


# ---------------------------------------------------------------------------- the parser
def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_the_flags_are_second_approachs_alone_and_default_off():
    import st3d.cli as cli
    FA, SA, TA = _scripts()
    a = SA.build_parser().parse_args([])
    assert a.style_regions is None and a.region_styles is None and a.region_style_weights is None
    assert cli.check_args(a) is None
    for mod in (FA, TA):
        assert not hasattr(mod.build_parser().parse_args([]), "style_regions")
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--style_regions", "x:0", "--region_styles", "a.png", "b.png"])
    b = SA.build_parser().parse_args(["--style_regions", "y:0.1,0.3", "--region_styles", "a.png", "b.png", "c.png",
                                      "--region_style_weights", "1", "0", "2.5", "--style_scales", "1",
                                      "--texture_type", "vertex"])
    assert b.style_regions == "y:0.1,0.3" and b.region_styles == ["a.png", "b.png", "c.png"]
    assert b.region_style_weights == [1.0, 0.0, 2.5]


def test_every_refusal_of_the_parser(monkeypatch, capsys, tmp_path):
    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    SA = _scripts()[1]
    monkeypatch.setattr(SA, "Run", no_gpu)
    one = tmp_path / "one.obj"
    one.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl skin\nf 1 2 3\n")
    three = tmp_path / "three.obj"
    three.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl a\nf 1 2 3\nusemtl b\nf 1 2 3\nusemtl c\nf 1 2 3\n")
    ok = ["--style_regions", "x:0", "--region_styles", "a.png", "b.png"]
    for argv, word in (
            (["--region_styles", "a.png", "b.png"], "--region_styles needs --style_regions"),
            (["--region_style_weights", "1", "2"], "--region_style_weights needs --style_regions"),
            (["--style_regions", "x:0"], "--style_regions needs --region_styles"),
            (["--style_regions", "x:0", "--region_styles", "a.png"], "exactly one per region"),
            (["--style_regions", "x:0,1", "--region_styles", "a.png", "b.png"], "exactly one per region"),
            (ok + ["--region_style_weights", "1"], "one weight per region"),
            (ok + ["--region_style_weights", "1", "-1"], "--region_style_weights must be finite and >= 0"),
            (ok + ["--region_style_weights", "1", "nan"], "--region_style_weights must be finite and >= 0"),
            (ok + ["--region_style_weights", "inf", "1"], "--region_style_weights must be finite and >= 0"),
            (["--style_regions", "w:0", "--region_styles", "a.png", "b.png"], "--style_regions"),
            (["--style_regions", "x:1,0", "--region_styles", "a.png", "b.png", "c.png"], "--style_regions"),
            (["--style_regions", "labels.txt", "--region_styles", "a.png", "b.png"], "--style_regions"),
            (ok + ["--style_mask", "object"], "the regions already exclude the background"),
            (ok + ["--style_scales", "1,2", "--size", "64"], "--style_regions needs --style_scales 1"),
            (ok + ["--style_scales", "2", "--size", "64"], "--style_regions needs --style_scales 1"),
            (ok + ["--nnfm_weight", "1"], "cannot be combined with --nnfm_weight"),
            (ok + ["--swd_weight", "1"], "cannot be combined with --swd_weight"),
            (ok + ["--preserve_color", "match"], "--style_regions needs --preserve_color off"),
            (ok + ["--preserve_color", "luminance"], "--style_regions needs --preserve_color off"),
            (ok + ["--supersample", "2", "--size", "64"], "--style_regions needs --supersample 1"),
            (["--style_regions", "material", "--region_styles", "a.png", "b.png", "--obj_path", str(one)],
             "at least 2 usemtl groups"),
            (["--style_regions", "material", "--region_styles", "a.png", "b.png", "--obj_path", str(three)],
             "exactly one per region")):
        with pytest.raises(SystemExit) as e:
            SA.main(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    # what stays legal reaches the run
    for argv in (ok, ok + ["--region_style_weights", "0", "3"], ok + ["--style_scales", "1"], ok + ["--texture_type", "vertex"],
                 ok + ["--texture_atlas", "4"], ok + ["--optimization_target", "both"],
                 ["--style_regions", "material", "--region_styles", "a", "b", "c", "--obj_path", str(three)]):
        with pytest.raises(AssertionError, match="the run was set up"):
            SA.main(argv)


# ---------------------------------------------------------------------------- the restatement's own identity
def _synthetic_fragments(n, S, F, seed):
    """blocks of faces with holes: pix_to_face (n,S,S) int with -1 areas, labels for F faces"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, F, size=(n, S, S))
    yy, xx = np.mgrid[0:S, 0:S]
    for b in range(n):
        p[b][((yy - S * 0.4) ** 2 + (xx - S * (0.3 + 0.2 * b)) ** 2) < (S * 0.22) ** 2] = -1
        p[b][:, S - 3:] = -1
    return p


@pytest.mark.parametrize("S", [16, 24, 64])
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_the_level_sums_of_the_regions_add_up_to_the_coverages(S, R):
    """every a_l is a multiple of 4^-l and every sum a multiple of it well below 2^24: exact in fp32 in any order, so
    sum_r Sigma_l(region r) == Sigma_l(coverage) with no tolerance, and each region's level 0 counts its pixels"""
    F = 40
    p = _synthetic_fragments(2, S, F, seed=S + R)
    labels = np.arange(F) % R
    q, sums = RR.planes_ref(p, labels, R)
    _, cover = GR.planes_ref((p >= 0).astype(np.float32))
    assert sums.shape == (R, 5, 2) and sums.dtype == np.float32
    assert np.array_equal(sums.astype(np.float64).sum(0), cover.astype(np.float64))
    assert float(cover.max()) < 1 << 24
    hot = RR.one_hot(p, labels, R)
    assert np.array_equal(hot.sum(0), (p >= 0).astype(np.float32))                 # the regions partition the coverage
    for r in range(R):
        assert np.array_equal(sums[r, 0], hot[r].reshape(2, -1).sum(1))
        assert [x.shape for x in q[r]] == [(2, H, H) for H in GR.sides(S)]
        for l in range(5):
            assert np.array_equal(q[r][l] == 0, GR.pyramid_ref(hot[r])[l] == 0)     # q vanishes exactly where the region does
    assert RR.fold32([0.1, 0.2, 0.3]) == np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3))
