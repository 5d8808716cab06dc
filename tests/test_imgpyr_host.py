"""Host side of the multi-scale style loss: the refusals of the pyramid entry points (which launch nothing), the wrappers'
validation and their refusal of CPU tensors, --style_scales / --style_scale_weights on all three scripts, and the checks
compute_perceptual_loss and style_transfer make before they touch the GPU.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_pyr_down_tile", "st3d_pyr_down_fwd", "st3d_pyr_down_bwd", "st3d_pyr_down_need")


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_bound_and_built_without_contraction():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    assert "-ffp-contract=off" in re.search(r'"imgpyr.hip":\s*\[([^\]]*)\]', build).group(1)
    source = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "csrc", "imgpyr.hip")).read()
    assert "atomicAdd" not in source and "fmaf" not in source         # a gather with the roundings written out


def test_the_tile_is_reported_without_a_device():
    from st3d import ops
    th, tw = ops.pyr_down_tile()
    assert th >= 2 and tw >= 2 and th % 2 == 0 and tw % 2 == 0
    assert (th, tw) == (16, 128)                # DESIGN.md 4 states it; the GPU tests build their planes around it


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)          # never dereferenced
    for fn in (lib.st3d_pyr_down_fwd, lib.st3d_pyr_down_bwd, lib.st3d_pyr_down_need):
        #       in N  H  W  out stream
        good = [p, 3, 8, 6, q, None]
        bad = [[None] + good[1:], good[:4] + [None, None], good[:4] + [p, None]]        # null in, null out, in place
        bad += [good[:1] + [n] + good[2:] for n in (0, -1)]
        bad += [good[:2] + [h] + good[3:] for h in (0, 1, 3, 7, -2, 32770)]
        bad += [good[:3] + [w] + good[4:] for w in (0, 1, 5, -4, 32770)]
        for args in bad:
            assert fn(*args) == -1, args
            assert b"invalid argument" in lib.st3d_last_error()
    assert lib.st3d_pyr_down_tile(None, None) == -1


# ---------------------------------------------------------------------------- 2. the Python layer
def test_the_wrappers_refuse_cpu_tensors():
    from st3d import imgpyr, ops
    x, m = torch.rand(1, 3, 8, 6), torch.ones(1, 8, 6, dtype=torch.uint8)
    for call in (lambda: ops.pyr_down_fwd(x), lambda: ops.pyr_down_bwd(x), lambda: ops.pyr_down_need(m),
                 lambda: imgpyr.pyr_down(x), lambda: imgpyr.reduce(x, 2), lambda: imgpyr.reduce_need(m, 2),
                 lambda: imgpyr.reduced_cached(x, 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert imgpyr.reduce(x, 1) is x and imgpyr.reduce_need(m, 1) is m and imgpyr.reduced_cached(x, 1) is x


def test_the_wrappers_validate_shapes_before_they_call():
    from st3d import imgpyr, ops
    for x in (torch.rand(3, 8, 6), torch.rand(1, 3, 7, 6), torch.rand(1, 3, 8, 5), torch.rand(1, 3, 0, 6), torch.rand(0, 3, 8, 6)):
        with pytest.raises(ValueError):
            ops.pyr_down_fwd(x)
    for g in (torch.rand(3, 4, 3), torch.rand(0, 3, 4, 3), torch.rand(1, 1, 0, 3)):
        with pytest.raises(ValueError):
            ops.pyr_down_bwd(g)
    for m in (torch.ones(1, 1, 8, 6, dtype=torch.uint8), torch.ones(1, 8, 6), torch.ones(1, 7, 6, dtype=torch.uint8),
              torch.ones(0, 8, 6, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.pyr_down_need(m)
    for f in (0, 3, 8, -2, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            imgpyr.reduce(torch.rand(1, 3, 8, 8), f)
        with pytest.raises(ValueError):
            imgpyr.reduced_cached(torch.rand(1, 3, 8, 8), f)


BAD_SCALES = [((), None), ((3,), None), ((0,), None), ((8,), None), ((2, 1), None), ((1, 1), None), ((1, 2, 2), None),
              ((1.5,), None), ("12", None), (None, None), ((1, 2), (1.0,)), ((1,), (1.0, 1.0)), ((1, 2), (1.0, -0.5)),
              ((1, 2), (1.0, float("inf"))), ((1, 2), (float("nan"), 1.0)), ((2,), ("x",))]


def test_check_scales_is_pure_host_logic():
    from st3d import imgpyr
    assert imgpyr.check_scales((1,)) == ((1,), (1.0,))
    assert imgpyr.check_scales([1, 2, 4], [1, 0.5, 0], 128) == ((1, 2, 4), (1.0, 0.5, 0.0))
    assert imgpyr.check_scales((2, 4), None, 512) == ((2, 4), (1.0, 1.0))
    for scales, weights in BAD_SCALES:
        with pytest.raises(ValueError):
            imgpyr.check_scales(scales, weights, 128)
    for scales, side in (((2,), 63), ((2,), 62), ((4,), 64), ((1, 4), 100), ((4,), 126), ((1,), 16)):
        with pytest.raises(ValueError, match="does not reduce"):
            imgpyr.check_scales(scales, None, side)
    assert imgpyr.check_scales((1, 2), None, 64) == ((1, 2), (1.0, 1.0)) and imgpyr.check_scales((4,), None, 128)[0] == (4,)


def test_the_losses_raise_on_bad_scales_before_touching_the_gpu():
    """CPU tensors and no VGG: anything but the scales check would raise another error first"""
    import losses as L
    import style_transfer as ST
    x = torch.rand(2, 3, 128, 128)
    for scales, weights in BAD_SCALES:
        with pytest.raises(ValueError):
            L.compute_perceptual_loss(x, x, x, None, scales=scales, scale_weights=weights)
        with pytest.raises(ValueError):
            L.compute_second_approach_loss(x, x, x, None, 1e6, 1.0, None, None, None, {}, "texture", style_scales=scales,
                                           style_scale_weights=weights)
        with pytest.raises(ValueError):
            ST.style_transfer(x, x, x, None, steps=1, style_scales=scales, style_scale_weights=weights)
    small = torch.rand(2, 3, 64, 64)
    with pytest.raises(ValueError, match="does not reduce"):
        L.compute_perceptual_loss(small, small, small, None, scales=(1, 4))
    with pytest.raises(ValueError, match="does not reduce"):
        ST.style_transfer(small, small, small, None, steps=1, style_scales=(4,))
    # the default takes the old road: the model check comes first, as it always did
    with pytest.raises(TypeError):
        L.compute_perceptual_loss(x, x, x, None)
    with pytest.raises(TypeError):
        L.compute_perceptual_loss(x, x, x, None, scales=(1,))
    with pytest.raises(TypeError):
        L.compute_perceptual_loss(x, x, x, None, scales=(1, 2))         # good scales: on to the next check


# ---------------------------------------------------------------------------- 3. the flags
def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_flags_are_shared_and_default_to_the_single_scale_loss():
    from st3d import cli
    names = {f.name: f.default for f in cli.SHARED_FLAGS}
    assert names["style_scales"] is None and names["style_scale_weights"] is None
    for mod in _scripts():
        args = mod.build_parser().parse_args([])
        assert args.style_scales == (1,) and args.style_scale_weights is None
        args = mod.build_parser().parse_args(["--style_scales", "1"])
        assert args.style_scales == (1,) and args.style_scale_weights is None


def test_the_flags_parse_and_refuse(capsys):
    for mod in _scripts():
        parse = mod.build_parser().parse_args
        assert parse(["--style_scales", "1,2", "--size", "64"]).style_scales == (1, 2)
        assert parse(["--style_scales", "1,2,4", "--size", "512"]).style_scales == (1, 2, 4)
        assert parse(["--style_scales", "2, 4", "--size", "128"]).style_scales == (2, 4)
        assert parse(["--style_scales", "4", "--size", "128"]).style_scales == (4,)
        args = parse(["--style_scales", "1,2,4", "--style_scale_weights", "1,0.5,0", "--size", "256"])
        assert args.style_scales == (1, 2, 4) and args.style_scale_weights == (1.0, 0.5, 0.0)
        assert parse(["--style_scales", "1", "--style_scale_weights", "2"]).style_scale_weights == (2.0,)
        # every combination of the run's other switches is left alone: the loss only sees images and their tags
        assert parse(["--style_scales", "1,2", "--size", "256", "--supersample", "2", "--style_mask", "object", "--lights", "point",
                      "--texture_pyramid_levels", "0"]).style_scales == (1, 2)
        assert parse(["--style_scales", "1,2", "--size", "256", "--texture_type", "vertex"]).style_scales == (1, 2)
        assert parse(["--style_scales", "2", "--size", "256", "--texture_atlas", "4", "--nnfm_weight", "1"]).style_scales == (2,)
        refused = [(["--style_scales", "3"], "1,2,4"), (["--style_scales", "0"], "1,2,4"), (["--style_scales", "8"], "1,2,4"),
                   (["--style_scales", "2,1"], "increasing"), (["--style_scales", "1,1"], "increasing"),
                   (["--style_scales", "1,,2"], "1,2,4"), (["--style_scales", "a"], "1,2,4"), (["--style_scales", ""], "1,2,4"),
                   (["--style_scales", "1,2", "--style_scale_weights", "1"], "one weight per factor"),
                   (["--style_scales", "1", "--style_scale_weights", "1,1"], "one weight per factor"),
                   (["--style_scales", "1,2", "--style_scale_weights", "1,-1"], "finite weights"),
                   (["--style_scales", "1,2", "--style_scale_weights", "1,inf"], "finite weights"),
                   (["--style_scales", "1,2", "--style_scale_weights", "nan,1"], "finite weights"),
                   (["--style_scales", "1,2", "--style_scale_weights", "1,x"], "numbers"),
                   (["--style_scale_weights", "1"], "needs --style_scales"),
                   (["--style_scales", "1,2", "--size", "63"], "divisible by 2"),
                   (["--style_scales", "1,4", "--size", "510"], "divisible by 4"),
                   (["--style_scales", "1,2", "--size", "62"], ">= 32"),
                   (["--style_scales", "2,4", "--size", "64"], ">= 32")]
        for argv, word in refused:
            with pytest.raises(SystemExit):
                parse(argv)
            err = capsys.readouterr().err
            assert "style_scale" in err and word in err, (argv, err)
