"""Host side of the Laplacian content term: the refusals of the lap entry points (which launch nothing), the wrappers'
validation, check_pools, --lap_weight / --lap_pools on all three scripts with every refusal check_args makes, and the checks
compute_laplacian_loss and style_transfer make before they touch the GPU.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_lap_tile", "st3d_lap_workspace_bytes", "st3d_lap_fwd", "st3d_lap_loss")
TILES = {1: (16, 128), 2: (32, 128), 4: (64, 128), 8: (128, 128), 16: (128, 256)}


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_bound_and_built_without_contraction():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    build = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    assert "-ffp-contract=off" in re.search(r'"lap.hip":\s*\[([^\]]*)\]', build).group(1)
    source = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "csrc", "lap.hip")).read()
    code = re.sub(r"//[^\n]*", "", source)
    assert "atomic" not in code.lower() and "fmaf" not in code      # gathers and ordered sums, the roundings written out
    # the device calls live in st3d/lap.py; st3d/ops.py only imports the names
    ops = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "st3d", "ops.py")).read()
    lap = open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "st3d", "lap.py")).read()
    assert 'call("st3d_lap_' in lap and "st3d_lap_" not in ops
    assert re.search(r"^from \.lap import lap_fwd, lap_loss, lap_tile\b", ops, flags=re.M)


def test_the_tile_and_the_workspace_are_reported_without_a_device():
    from st3d import _lib, lap, ops
    lib = _lib.load()
    for p, tile in TILES.items():
        assert ops.lap_tile(p) == tile and lap.lap_tile(p) == tile       # DESIGN.md 7 states them; the GPU tests build on them
        assert tile[0] % p == 0 and tile[1] % p == 0 and tile[1] % 4 == 0
        # one double per workgroup and r at pooled size
        th, tw = tile
        for N, H, W in ((1, 2 * p, 2 * p), (3, th + 2 * p, 2 * tw - 2 * p), (24, 512, 512)):
            blocks = N * -(-H // th) * -(-W // tw)
            assert lib.st3d_lap_workspace_bytes(N, H, W, p) == 8 * blocks + 4 * N * (H // p) * (W // p)
    for bad in ((0, 8, 8, 2), (1, 8, 8, 3), (1, 8, 8, 0), (1, 2, 8, 2), (1, 8, 6, 4), (1, 32770, 8, 1), (-1, 8, 8, 1)):
        assert lib.st3d_lap_workspace_bytes(*bad) == 0
    for p in (0, 3, 5, 32, -1):
        assert lib.st3d_lap_tile(p, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) == -1
        with pytest.raises(ValueError):
            lap.lap_tile(p)
    assert lib.st3d_lap_tile(4, None, None) == -1


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    a, b, c, d, e = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4, 5))        # never dereferenced

    #       x  N  H  W  p  out stream
    good = [a, 3, 8, 12, 2, b, None]
    bad = [[None] + good[1:], good[:5] + [None, None], good[:5] + [a, None]]        # null in, null out, in place
    bad += [good[:1] + [n] + good[2:] for n in (0, -1)]
    bad += [good[:2] + [h] + good[3:] for h in (0, 2, 7, -4, 32770)]                # (2: a pooled side of 1)
    bad += [good[:3] + [w] + good[4:] for w in (0, 2, 5, -4, 32770)]
    bad += [good[:4] + [p] + good[5:] for p in (0, 3, 8, 16, 32, -2)]               # (8, 16 do not divide the sides)
    for args in bad:
        assert lib.st3d_lap_fwd(*args) == -1, args
        assert b"invalid argument" in lib.st3d_last_error()
    assert lib.st3d_lap_fwd(a, 1 << 30, 32768, 32768, 1, b, None) == -1             # the grid does not fit one dimension

    size = lib.st3d_lap_workspace_bytes(3, 8, 12, 2)
    #       x  T  N  H  W  p  scale ws  bytes loss grad stream
    good = [a, b, 3, 8, 12, 2, 0.5, c, size, d, e, None]

    def swap(i, v):
        return good[:i] + [v] + good[i + 1:]

    bad = [swap(0, None), swap(1, None), swap(7, None), swap(9, None)]              # null x, target, workspace, loss
    bad += [swap(1, a), swap(10, a), swap(10, b), swap(7, a), swap(7, b), swap(7, e), swap(9, c), swap(9, e), swap(9, a), swap(9, b)]
    bad += [swap(7, ctypes.c_void_p(4096 * 3 + 4))]                                 # a workspace off its 8-byte alignment
    bad += [swap(8, size - 1), swap(8, 0)]
    bad += [swap(6, s) for s in (-1.0, float("nan"), float("inf"))]
    bad += [swap(2, n) for n in (0, -1)] + [swap(3, h) for h in (0, 2, 7, 32770)] + [swap(4, w) for w in (0, 2, 5, 32770)]
    bad += [swap(5, p) for p in (0, 3, 8, 16, -2)]
    for args in bad:
        assert lib.st3d_lap_loss(*args) == -1, args
        assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 2. the Python layer
def test_the_wrappers_validate_before_they_call():
    from st3d import lap, ops
    good = torch.rand(1, 3, 8, 12)
    for x, p in ((torch.rand(3, 8, 12), 2), (torch.rand(1, 3, 7, 12), 2), (torch.rand(1, 3, 8, 10), 4), (torch.rand(1, 3, 2, 12), 2),
                 (torch.rand(0, 3, 8, 12), 2), (good, 3), (good, 0), (good, 8), (good, 2.0), (good, True), (good, None)):
        with pytest.raises(ValueError):
            ops.lap_fwd(x, p)
        with pytest.raises(ValueError):
            ops.lap_loss(x, torch.rand(1, 3, 4, 6), p, 1.0)
    with pytest.raises(ValueError, match="need a target"):
        ops.lap_loss(good, torch.rand(1, 3, 8, 12), 2, 1.0)
    for scale in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            ops.lap_loss(good, torch.rand(1, 3, 4, 6), 2, scale)
    for fn in (lambda: ops.lap_fwd(good, 2), lambda: ops.lap_loss(good, torch.rand(1, 3, 4, 6), 2, 1.0),
               lambda: lap.lap_target_cached(good, 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    assert lap.term_scale((2, 3, 8, 12), 2) == 1.0 / (2 * 3 * 4 * 6) and lap.term_scale((2, 3, 8, 12), 4, 5) == 1.0 / (5 * 3 * 2 * 3)
    with pytest.raises(ValueError):
        lap.term_scale((2, 3, 8, 12), 2, 0)


BAD_POOLS = [(), (3,), (0,), (32,), (2, 1), (4, 4), (1, 2, 2), (2.0,), (True,), "4", None, 4, ("4",)]


def test_check_pools_is_pure_host_logic():
    from st3d import lap
    assert lap.POOLS == (1, 2, 4, 8, 16)
    assert lap.check_pools((4,)) == (4,) and lap.check_pools([1, 2, 4, 8, 16], 512) == (1, 2, 4, 8, 16)
    assert lap.check_pools((4, 16), (64, 32)) == (4, 16) and lap.check_pools((1,), 2) == (1,)
    for pools in BAD_POOLS:
        with pytest.raises(ValueError):
            lap.check_pools(pools, 512)
    for pools, side in (((2,), 63), ((4,), 4), ((16,), 16), ((4, 16), 72), ((1,), 1), ((8,), (64, 8)), ((2,), (3, 8))):
        with pytest.raises(ValueError, match="does not pool"):
            lap.check_pools(pools, side)


def test_the_losses_raise_on_bad_pools_before_touching_the_gpu():
    """CPU tensors and no VGG: anything but the checks would raise another error first"""
    import losses as L
    import style_transfer as ST
    assert L.check_lap_pools is ST.check_lap_pools and L.laplacian_targets is ST.laplacian_targets    # the star surface
    x = torch.rand(2, 3, 64, 64)
    for pools in BAD_POOLS:
        with pytest.raises(ValueError):
            L.compute_laplacian_loss(x, x, pools)
        with pytest.raises(ValueError):
            ST.style_transfer(x, x, x, None, steps=1, lap_weight=1.0, lap_pools=pools)
    with pytest.raises(ValueError, match="does not pool"):
        L.compute_laplacian_loss(torch.rand(1, 3, 24, 64), torch.rand(1, 3, 24, 64), (16,))
    with pytest.raises(ValueError, match="does not pool"):
        ST.style_transfer(x[:, :, :24], x[:, :, :24], x[:, :, :24], None, steps=1, lap_weight=1.0, lap_pools=(4, 16))
    with pytest.raises(ValueError, match="one shape"):
        L.compute_laplacian_loss(x, x[:1])
    with pytest.raises(TypeError):
        L.compute_laplacian_loss(x, None)
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lap_weight"):
            ST.style_transfer(x, x, x, None, steps=1, lap_weight=w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.compute_laplacian_loss(x, x, (4,))
    # weight 0 takes the old road whatever the pools say: the model check comes first, as it always did
    with pytest.raises(TypeError):
        ST.style_transfer(x, x, x, None, steps=1, lap_weight=0.0, lap_pools=(3,))
    with pytest.raises(TypeError):
        ST.style_transfer(x, x, x, None, steps=1)


# ---------------------------------------------------------------------------- 3. the flags
def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_flags_are_shared_and_default_to_off():
    from st3d import cli
    names = {f.name: f.default for f in cli.SHARED_FLAGS}
    assert names["lap_weight"] == 0.0 and names["lap_pools"] == (4,)
    for mod in _scripts():
        args = mod.build_parser().parse_args([])
        assert args.lap_weight == 0.0 and args.lap_pools == (4,)
        assert mod.build_parser().parse_args(["--lap_pools", "4"]).lap_pools == (4,)        # the default, spelled out


def test_the_flags_parse_and_refuse(capsys):
    for mod in _scripts():
        parse = mod.build_parser().parse_args
        assert parse(["--lap_weight", "1e4"]).lap_weight == 1e4
        args = parse(["--lap_weight", "10", "--lap_pools", "4,16", "--size", "64"])
        assert args.lap_weight == 10.0 and args.lap_pools == (4, 16)
        assert parse(["--lap_weight", "1", "--lap_pools", "1, 2,4,8,16", "--size", "512"]).lap_pools == (1, 2, 4, 8, 16)
        assert parse(["--lap_weight", "1", "--lap_pools", "16", "--size", "32"]).lap_pools == (16,)
        assert parse(["--lap_weight", "0", "--size", "63"]).lap_weight == 0.0      # off: the size is not looked at
        for bg in ("white", "style"):
            assert parse(["--lap_weight", "1", "--content_background", bg, "--current_background", bg]).lap_weight == 1.0
        # every combination of the run's other switches is left alone: the term only sees images
        assert parse(["--lap_weight", "1", "--size", "256", "--supersample", "2", "--style_mask", "object", "--lights", "point",
                      "--texture_pyramid_levels", "0", "--style_scales", "1,2"]).lap_weight == 1.0
        assert parse(["--lap_weight", "1", "--texture_type", "vertex"]).lap_weight == 1.0
        assert parse(["--lap_weight", "1", "--texture_atlas", "4", "--nnfm_weight", "1", "--swd_weight", "1"]).lap_weight == 1.0
        assert parse(["--lap_weight", "1", "--texture_mip_levels", "0", "--preserve_color", "luminance"]).lap_weight == 1.0
        refused = [(["--lap_weight", "-1"], "finite and >= 0"), (["--lap_weight", "nan"], "finite and >= 0"),
                   (["--lap_weight", "inf"], "finite and >= 0"),
                   (["--lap_weight", "1", "--lap_pools", "3"], "1,2,4,8,16"), (["--lap_weight", "1", "--lap_pools", "0"], "1,2,4,8,16"),
                   (["--lap_weight", "1", "--lap_pools", "32"], "1,2,4,8,16"), (["--lap_weight", "1", "--lap_pools", "a"], "1,2,4,8,16"),
                   (["--lap_weight", "1", "--lap_pools", ""], "1,2,4,8,16"), (["--lap_weight", "1", "--lap_pools", "4,,8"], "1,2,4,8,16"),
                   (["--lap_weight", "1", "--lap_pools", "4,2"], "increasing"), (["--lap_weight", "1", "--lap_pools", "4,4"], "increasing"),
                   (["--lap_pools", "2"], "needs --lap_weight"), (["--lap_pools", "4,16"], "needs --lap_weight"),
                   (["--lap_weight", "0", "--lap_pools", "2"], "needs --lap_weight"),
                   (["--lap_weight", "1", "--size", "66"], "divisible by 4"),
                   (["--lap_weight", "1", "--lap_pools", "4,16", "--size", "72"], "divisible by 16"),
                   (["--lap_weight", "1", "--lap_pools", "16", "--size", "16"], ">= 2"),
                   (["--lap_weight", "1", "--content_background", "style"], "--content_background equal to"),
                   (["--lap_weight", "1", "--current_background", "style"], "--content_background equal to"),
                   (["--lap_weight", "1", "--content_background", "noise", "--current_background", "noise"], "neither 'noise'"),
                   (["--lap_weight", "1", "--current_background", "noise"], "neither 'noise'")]
        for argv, word in refused:
            with pytest.raises(SystemExit):
                parse(argv)
            err = capsys.readouterr().err
            assert "lap_" in err and word in err, (argv, err)


def test_region_runs_take_the_flag():
    import second_approach as SA
    args = SA.build_parser().parse_args(["--lap_weight", "1", "--style_regions", "x:0", "--region_styles", "a.png", "b.png"])
    assert args.lap_weight == 1.0 and args.style_regions is not None
