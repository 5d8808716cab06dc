"""Host side of --fill_unseen: the C ABI's workspace formula and refusals (which launch nothing), the wrappers' validation and
their refusal of CPU tensors, the flag on all three scripts and what check_args rules out.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _fillref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_fill_workspace_bytes", "st3d_fill_pushpull")


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_bound_and_built_like_bake():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    flags = lambda src: re.search(r'"%s":\s*\[([^\]]*)\]' % re.escape(src), build).group(1)
    assert flags("fill.hip") == flags("bake.hip") and "-ffp-contract=off" in flags("fill.hip")
    source = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "csrc", "fill.hip")).read()
    assert source.count("atomicAdd(") == 1 and "unsigned long long" in source and "asm" not in source     # the integer count only


def test_workspace_size_is_pure_host_logic():
    from st3d import _lib
    lib = _lib.load()
    for H, W in ((1, 1), (1, 2), (2, 2), (3, 5), (33, 17), (64, 64), (127, 129), (130, 70), (512, 512), (1024, 1024), (16384, 1),
                 (16384, 16384)):
        assert lib.st3d_fill_workspace_bytes(H, W) == FR.workspace_bytes(H, W) > 0, (H, W)
    assert lib.st3d_fill_workspace_bytes(1024, 1024) == 16 * (4 ** 10 - 1) // 3          # 5.3 MiB: a third of the map's float4s
    for H, W in ((0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385)):
        assert lib.st3d_fill_workspace_bytes(H, W) == 0


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, q, r, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384), ctypes.c_void_p(4100)   # never dereferenced
    need = FR.workspace_bytes(33, 17)
    #       tex valid domain H   W   ws  bytes out count stream
    good = [p, p, None, 33, 17, q, need, r, q, None]
    bad = [good[:i] + [None] + good[i + 1:] for i in (0, 1, 5, 7, 8)]
    values = {3: (0, -1, 16385), 4: (0, -1, 16385), 5: (odd,), 6: (need - 1, 0), 7: (p,), 8: (odd,)}
    bad += [good[:i] + [v] + good[i + 1:] for i, vs in values.items() for v in vs]
    assert len(bad) >= 16
    for args in bad:
        assert lib.st3d_fill_pushpull(*args) == -1, args
        assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 2. the Python layer
def test_the_wrappers_live_outside_ops_and_refuse_cpu_tensors():
    from st3d import fill, ops
    import utils as U
    for name in ("moved_texels", "push_pull", "fill_unseen"):
        assert callable(getattr(fill, name)) and not hasattr(ops, name)
    assert callable(U.fill_texture)
    tex = torch.rand(8, 6, 3)
    for call in (lambda: fill.push_pull(tex, torch.ones(8, 6, dtype=torch.uint8)),
                 lambda: fill.push_pull(tex, torch.ones(8, 6, dtype=torch.uint8), torch.ones(8, 6, dtype=torch.uint8)),
                 lambda: fill.fill_unseen(tex, tex.clone())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_moved_texels_compares_bits():
    from st3d import fill
    a = torch.rand(5, 7, 3)
    b = a.clone()
    b[1, 2, 0] += 1e-3
    b[3, 3, 2] = float("nan")
    a[3, 3, 2] = float("nan")                               # the same NaN bits: not moved
    a[4, 0, 1], b[4, 0, 1] = 0.0, -0.0                      # equal as numbers, different bits: moved
    moved = fill.moved_texels(a, b)
    assert moved.dtype == torch.uint8 and tuple(moved.shape) == (5, 7)
    want = torch.zeros(5, 7, dtype=torch.uint8)
    want[1, 2] = want[4, 0] = 1
    assert torch.equal(moved, want)


def test_the_wrappers_validate_shapes_and_dtypes_before_they_call():
    from st3d import fill
    ok = torch.ones(8, 6, dtype=torch.uint8)
    for tex in (torch.zeros(8, 6), torch.zeros(8, 6, 4), torch.zeros(8, 6, 3, dtype=torch.float64), torch.zeros(0, 6, 3),
                torch.zeros(1, 8, 6, 3), np.zeros((8, 6, 3), np.float32)):
        with pytest.raises(ValueError, match="texture"):
            fill.push_pull(tex, ok)
    tex = torch.zeros(8, 6, 3)
    for valid in (torch.ones(8, 6), torch.ones(6, 8, dtype=torch.uint8), torch.ones(8, 6, 1, dtype=torch.uint8),
                  torch.ones(8, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="valid"):
            fill.push_pull(tex, valid)
        with pytest.raises(ValueError, match="domain"):
            fill.push_pull(tex, ok, valid)
    for original in (torch.zeros(8, 6), torch.zeros(6, 8, 3), torch.zeros(8, 6, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="original"):
            fill.moved_texels(tex, original)
        with pytest.raises(ValueError, match="original"):
            fill.fill_unseen(tex, original)


def test_fill_texture_validates_before_any_gpu_work():
    import utils as U
    from st3d.render import Meshes, TexturesAtlas, TexturesVertex
    verts, faces = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    for textures in (TexturesVertex(torch.rand(4, 3)), TexturesAtlas(torch.rand(2, 2, 2, 3))):
        with pytest.raises(NotImplementedError, match="TexturesUV"):
            U.fill_texture(Meshes([verts], [faces], textures), torch.rand(1, 8, 8, 3), "map")
    wide = U.build_mesh(torch.rand(1, 4, 2), faces[None], torch.rand(1, 8, 6, 3), verts, faces)
    with pytest.raises(NotImplementedError, match="square texture map"):
        U.fill_texture(wide, torch.rand(1, 8, 6, 3), "chart")               # 'chart' with a non-square map
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.fill_texture(wide, torch.rand(1, 8, 6, 3), "map")                 # 'map' takes it: it gets as far as the device call
    for mode in ("off", "gutter", None):
        with pytest.raises(ValueError, match="mode"):
            U.fill_texture(wide, torch.rand(1, 8, 6, 3), mode)
    with pytest.raises(ValueError, match="original_map"):
        U.fill_texture(wide, torch.rand(1, 8, 8, 3), "map")
    square = U.build_mesh(torch.rand(1, 4, 2), faces[None], torch.rand(1, 8, 8, 3), verts, faces)
    with pytest.raises(ValueError, match="moved_from"):
        U.fill_texture(wide, torch.rand(1, 8, 6, 3), "map", moved_from=square)


# ---------------------------------------------------------------------------- 3. the flag
def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_flag_is_shared_and_defaults_to_the_untouched_path():
    from st3d import cli
    names = {f.name: (f.type, f.default, f.choices) for f in cli.SHARED_FLAGS}
    assert names["fill_unseen"] == (str, "off", ["off", "chart", "map"])
    help_text = next(f.help for f in cli.SHARED_FLAGS if f.name == "fill_unseen")
    assert "texel_filled.png" in help_text and "square" in help_text
    for mod in _scripts():
        assert mod.build_parser().parse_args([]).fill_unseen == "off"
        assert mod.build_parser().parse_args(["--fill_unseen", "off", "--optimization_target", "mesh"]).fill_unseen == "off"


def test_the_flag_parses_and_check_args_refuses(capsys):
    for mod in _scripts():
        parse = mod.build_parser().parse_args
        for mode in ("chart", "map"):
            assert parse(["--fill_unseen", mode]).fill_unseen == mode
            assert parse(["--fill_unseen", mode, "--optimization_target", "both"]).fill_unseen == mode
            # a pyramid run moves every texel: the fill then reports 0, nothing is refused
            assert parse(["--fill_unseen", mode, "--texture_pyramid_levels", "0"]).texture_pyramid_levels == 0
            assert parse(["--fill_unseen", mode, "--supersample", "2", "--view_selection", "coverage"]).supersample == 2
            for argv, word in (([ "--optimization_target", "mesh"], "optimization_target texture or both"),
                               (["--texture_type", "vertex"], "texture_type uv"),
                               (["--texture_atlas", "4"], "texture_atlas 0")):
                with pytest.raises(SystemExit):
                    parse(["--fill_unseen", mode] + argv)
                err = capsys.readouterr().err
                assert "--fill_unseen needs" in err and word in err, argv
        with pytest.raises(SystemExit):
            parse(["--fill_unseen", "gutter"])
        assert "fill_unseen" in capsys.readouterr().err
