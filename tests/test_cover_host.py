"""Host side of --view_selection coverage: the C ABI's refusals (which launch nothing), the workspace query, the Python
wrappers' validation and their refusal of CPU tensors, words / unpack, the two flags on all three scripts and what check_args
rules out.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _coverref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_cover_mark", "st3d_cover_workspace_bytes", "st3d_cover_greedy", "st3d_cover_count")


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_bound_and_built_like_the_shading_kernels():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    flags = lambda src: re.search(r'"%s":\s*\[([^\]]*)\]' % re.escape(src), build).group(1)
    assert flags("cover.hip") == flags("shade.hip")             # the footprint it marks is the shading kernels' bit for bit
    source = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "csrc", "cover.hip")).read()
    assert "frag_uv(" in source and "uv_footprint(" in source and "uvs[2 *" not in source        # shared, not restated


def test_workspace_size_is_pure_host_logic():
    from st3d import _lib
    lib = _lib.load()
    for C in (1, 5, 256, 4096):
        assert lib.st3d_cover_workspace_bytes(C) == 8 * C           # C gains + C taken flags
    for C in (0, -1, 4097):
        assert lib.st3d_cover_workspace_bytes(C) == 0


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, q, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4098)           # never dereferenced

    def variants(good, pointers, values):
        out = [good[:i] + [None] + good[i + 1:] for i in pointers]
        out += [good[:i] + [v] + good[i + 1:] for i, vs in values.items() for v in vs]
        return out
    cases = {
        #                 p2f bary uvs fuv B  S   T   masks stream
        "st3d_cover_mark": variants([p, p, p, p, 3, 32, 32, q, None], (0, 1, 2, 3, 7),
                                    {4: (0, -1), 5: (0, -1, 4097), 6: (0, -1, 16385), 7: (odd,)}),
        #                   masks C   W   n  covered picks gains ws stream
        "st3d_cover_greedy": variants([p, 24, 32, 6, q, p, p, p, None], (0, 4, 5, 6, 7),
                                      {1: (0, -1, 5, 4097), 2: (0, -1, (1 << 26) + 1), 3: (0, -1, 25), 0: (odd,), 4: (odd, p),
                                       7: (odd,)}),
        #                  masks C  W   T   counts stream
        "st3d_cover_count": variants([p, 24, 32, 32, q, None], (0, 4),
                                     {1: (0, -1), 2: (0, 31, 33), 3: (0, -1, 31, 16385), 0: (odd,)}),
    }
    for name, bad in cases.items():
        assert len(bad) >= 9
        for args in bad:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 2. the Python layer
def test_words_and_unpack_round_trip():
    from st3d import cover
    assert [cover.words(T) for T in (1, 5, 8, 31, 32, 33, 512)] == [1, 1, 2, 31, 32, 35, 8192]
    for bad in (0, -1, 16385):
        with pytest.raises(ValueError):
            cover.words(bad)
    rng = np.random.default_rng(5)
    for T in (1, 5, 8, 31, 32, 33):                 # T*T a multiple of 32 and not
        assert cover.words(T) == CR.words(T)
        touch = rng.random((3, T, T)) < 0.5
        masks = torch.from_numpy(CR.pack(touch))
        assert masks.dtype == torch.int32 and tuple(masks.shape) == (3, cover.words(T))
        got = cover.unpack(masks, T)
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), touch)
        assert np.array_equal(CR.pack(got.numpy()), masks.numpy())
    top = torch.tensor([[-2147483648]], dtype=torch.int32)          # bit 31 alone: the shift must not smear the sign
    assert cover.unpack(top, 5).sum() == 0 and cover.unpack(torch.tensor([[1 << 24]], dtype=torch.int32), 5)[0, 4, 4]
    with pytest.raises(ValueError):
        cover.unpack(torch.zeros(3, 31, dtype=torch.int32), 32)
    with pytest.raises(ValueError):
        cover.unpack(torch.zeros(3, 32, dtype=torch.int64), 32)


def test_the_wrappers_live_outside_ops_and_refuse_cpu_tensors():
    from st3d import cover, ops
    for name in ("mark_texels", "greedy_views", "coverage_counts", "texel_masks", "select_cameras"):
        assert callable(getattr(cover, name)) and not hasattr(ops, name)
    masks = torch.zeros(4, 2, dtype=torch.int32)
    frag = (torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4))
    for call in (lambda: cover.greedy_views(masks, 2), lambda: cover.coverage_counts(masks, 8),
                 lambda: cover.mark_texels(frag, torch.zeros(3, 2), torch.zeros(1, 3, dtype=torch.int32), 8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_wrappers_validate_before_they_call():
    from st3d import cover
    from st3d.render import Meshes, TexturesAtlas, TexturesVertex
    masks = torch.zeros(4, 2, dtype=torch.int32)
    for n in (0, 5, -1, 2.5, True):
        with pytest.raises(ValueError, match="n must be"):
            cover.greedy_views(masks, n)
    with pytest.raises(ValueError, match="at most 4096"):
        cover.greedy_views(torch.zeros(4097, 1, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="covered"):
        cover.greedy_views(masks, 1, covered=torch.zeros(3, dtype=torch.int32))
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, 2), torch.zeros(0, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="masks"):
            cover.greedy_views(bad, 1)
        with pytest.raises(ValueError, match="masks"):
            cover.coverage_counts(bad, 8)
    with pytest.raises(ValueError, match="words per view"):
        cover.coverage_counts(masks, 9)
    frag = (torch.zeros(2, 4, 4, dtype=torch.int32), None, torch.zeros(2, 4, 4, 3), None)
    with pytest.raises(ValueError, match="masks must be"):
        cover.mark_texels(frag, torch.zeros(3, 2), torch.zeros(1, 3, dtype=torch.int32), 8, masks=torch.zeros(3, 2, dtype=torch.int32))
    verts, faces = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    R, T = torch.eye(3)[None], torch.tensor([[0.0, 0.0, 3.0]])
    for textures in (TexturesVertex(torch.rand(4, 3)), TexturesAtlas(torch.rand(2, 2, 2, 3))):
        with pytest.raises(NotImplementedError, match="TexturesUV"):
            cover.texel_masks(Meshes([verts], [faces], textures), R, T, 16)


def test_build_coverage_cameras_checks_its_counts():
    import utils as U
    for n, c in ((0, 8), (9, 8), (2, 4097), (2.5, 8), (True, 8)):
        with pytest.raises(ValueError, match="n_views <= candidates"):
            U.build_coverage_cameras(n, None, 16, candidates=c)


# ---------------------------------------------------------------------------- 3. the flags
def test_flag_defaults_are_the_untouched_path():
    from st3d import cli
    names = {f.name: (f.type, f.default, f.choices) for f in cli.SHARED_FLAGS}
    assert names["view_selection"] == (str, "random", ["random", "coverage"])
    assert names["view_candidates"] == (int, 256, None)
    help_text = next(f.help for f in cli.SHARED_FLAGS if f.name == "view_selection")
    assert "--supersample" in help_text and "--texture_mip_levels" in help_text and "plain" in help_text
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.view_selection == "random" and a.view_candidates == 256


def test_the_flags_parse_on_all_three_scripts_and_check_args_refuses(capsys):
    for mod in _scripts():
        parse = mod.build_parser().parse_args
        a = parse(["--view_selection", "coverage"])
        assert a.view_selection == "coverage" and a.view_candidates == 256
        a = parse(["--view_selection", "coverage", "--view_candidates", "16", "--n_views", "16", "--supersample", "2"])
        assert a.view_candidates == 16
        assert parse(["--view_selection", "coverage", "--view_candidates", "4096", "--texture_mip_levels", "0"]).view_candidates == 4096
        assert parse(["--view_selection", "random", "--view_candidates", "256"]).view_selection == "random"
        for argv, word in ((["--view_selection", "coverage", "--texture_type", "vertex"], "texture_type"),
                           (["--view_selection", "coverage", "--texture_atlas", "4"], "texture_atlas"),
                           (["--view_candidates", "16"], "view_selection coverage"),
                           (["--view_selection", "random", "--view_candidates", "16"], "view_selection coverage"),
                           (["--view_selection", "coverage", "--view_candidates", "5"], "view_candidates"),        # < n_views = 6
                           (["--view_selection", "coverage", "--view_candidates", "4097"], "view_candidates"),
                           (["--view_selection", "coverage", "--view_candidates", "0"], "view_candidates"),
                           (["--view_selection", "coverage", "--view_candidates", "8", "--n_views", "9"], "view_candidates"),
                           (["--view_selection", "nearest"], "view_selection")):
            with pytest.raises(SystemExit):
                parse(argv)
            assert word in capsys.readouterr().err, argv
