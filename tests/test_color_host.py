"""The host side of --preserve_color (st3d/color.py, st3d/cli.py): the colour match against its restatement, the flag rules,
the checkpoint key and the cache keying.  No GPU: the one device call the cache makes is replaced by a CPU stand-in."""
import os

import numpy as np
import pytest
import torch

import _colorref as CR


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


def test_the_package_restates_the_reference_constants():
    from st3d import color
    assert color.EIG_FLOOR == CR.EIG_FLOOR and color.MODES == ("off", "match", "luminance")
    assert [v.tobytes() for v in color.LUMA_WEIGHTS] == [v.tobytes() for v in CR.W]
    rng = np.random.default_rng(0)
    for c in [(1.0, 1.0, 1.0), (0.0, 0.0, 0.0)] + [tuple(rng.random(3)) for _ in range(200)]:
        want = CR.luma_plane(np.asarray(c, np.float32).reshape(1, 3, 1))[0, 0]
        assert np.float32(color.luma_of_color(c)).tobytes() == want.tobytes(), c


def test_match_matrix_and_luma_match_are_the_restatement():
    from st3d import color
    rng = np.random.default_rng(1)
    for _ in range(20):
        m = rng.standard_normal((3, 3))
        src = {"n": 10, "mean": rng.random(3), "cov": m @ m.T * 0.05}
        m = rng.standard_normal((3, 3))
        dst = {"n": 10, "mean": rng.random(3), "cov": m @ m.T * 0.05}
        A, b = color.match_matrix(src, dst)
        A2, b2 = CR.match_matrix(src, dst)
        assert np.array_equal(A, A2) and np.array_equal(b, b2)
        assert color.luma_match(src, dst) == pytest.approx(CR.luma_match(src, dst), rel=1e-15)
    flat = {"n": 4, "mean": np.full(3, 0.5), "cov": np.zeros((3, 3))}
    A, b = color.match_matrix(flat, dst)
    assert np.isfinite(A).all() and np.isfinite(b).all()
    k, off = color.luma_match(flat, dst)
    assert np.isfinite(k) and np.isfinite(off)


def test_stats_from_sums():
    from st3d import color
    x = np.random.default_rng(2).random((2, 3, 50), dtype=np.float32)
    sums = CR.moments(x)
    got, want = color.stats_from_sums(sums), CR.stats(sums)
    assert got["n"] == 100 and np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["cov"], want["cov"])
    with pytest.raises(ValueError, match="no pixel"):
        color.stats_from_sums(np.zeros(10))


def test_check_args_refuses_mesh_and_accepts_the_rest():
    import st3d.cli as cli
    for mod in _scripts():
        parser = mod.build_parser()
        assert parser.parse_args([]).preserve_color == "off"
        for mode in ("match", "luminance"):
            for target in ("texture", "both"):
                args = parser.parse_args(["--preserve_color", mode, "--optimization_target", target])
                assert args.preserve_color == mode and cli.check_args(args) is None
            args = parser.parse_args(["--optimization_target", "mesh"])
            args.preserve_color = mode
            assert "no colour is optimised and there is nothing to preserve" in cli.check_args(args)
            with pytest.raises(SystemExit):
                parser.parse_args(["--preserve_color", mode, "--optimization_target", "mesh"])
        assert cli.check_args(parser.parse_args(["--preserve_color", "off", "--optimization_target", "mesh"])) is None
        with pytest.raises(SystemExit):
            parser.parse_args(["--preserve_color", "lab"])
    SA = _scripts()[1]
    for extra in (["--texture_type", "vertex"], ["--texture_atlas", "2"], ["--style_scales", "1,2", "--size", "64"],
                  ["--style_mask", "object"], ["--nnfm_weight", "1"], ["--swd_weight", "1"], ["--fill_unseen", "map"],
                  ["--texture_pyramid_levels", "0"], ["--supersample", "2"], ["--lights", "point"]):
        assert SA.build_parser().parse_args(["--preserve_color", "luminance"] + extra).preserve_color == "luminance"


def _bare_run(tmp_path, mode):
    import st3d.cli as cli
    run = cli.Run.__new__(cli.Run)
    run.rank, run.world, run.out_dir, run.device = 0, 1, str(tmp_path), torch.device("cpu")
    run.pyramid, run.vertex_colors, run.atlas_r, run.chamfer_generator, run.swd_generator = None, False, 0, None, None
    if mode is not None:
        run.color_mode = mode
    run.args = _scripts()[1].build_parser().parse_args([])
    run.opt = {"texture_map": torch.rand(4, 4, 3), "verts": torch.rand(5, 3)}

    class Opt:
        def state_dict(self):
            return {"step": 0}

        def load_state_dict(self, state):
            pass
    run.optimizer = Opt()
    return run


def test_the_mode_travels_in_the_checkpoint_and_another_mode_is_refused(tmp_path):
    ck = os.path.join(str(tmp_path), "checkpoint.pt")
    for mode in ("match", "luminance"):
        _bare_run(tmp_path, mode).save_checkpoint(3)
        assert torch.load(ck, map_location="cpu", weights_only=True)["preserve_color"] == mode
        again = _bare_run(tmp_path, mode)
        again.load_checkpoint(ck)
        assert again.progress == 3
        for other in ("off", None, "match" if mode == "luminance" else "luminance"):
            with pytest.raises(ValueError, match=f"--preserve_color {mode}, this run has {other or 'off'}"):
                _bare_run(tmp_path, other).load_checkpoint(ck)
    for mode in ("off", None):                          # a default run writes no key, as before
        _bare_run(tmp_path, mode).save_checkpoint(1)
        assert "preserve_color" not in torch.load(ck, map_location="cpu", weights_only=True)
        _bare_run(tmp_path, None).load_checkpoint(ck)
        with pytest.raises(ValueError, match="--preserve_color off, this run has luminance"):
            _bare_run(tmp_path, "luminance").load_checkpoint(ck)


def test_style_color_and_loss_images_of_a_default_run(tmp_path):
    run = _bare_run(tmp_path, None)
    assert run.style_color == "rgb"
    a, b = torch.rand(1, 3, 2, 2), torch.rand(1, 3, 2, 2)
    run.color_mode = "off"
    assert run.loss_images(a, b) == (a, b) and run.loss_images(a, b)[0] is a
    run.color_mode = "match"
    assert run.loss_images(a, b)[0] is a and run.style_color == "rgb"
    run.color_mode = "luminance"
    assert run.style_color == "luminance"


def test_style_transfer_refuses_an_unknown_color():
    import style_transfer as ST
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match="color must be 'rgb' or 'luminance'"):
        ST.style_transfer(x, x, x, None, steps=1, color="lab")


def test_luma_cached_keying(monkeypatch):
    """the same object on a hit, a new one after an in-place change, one image expanded stays expanded, bounded size"""
    from st3d import color
    calls = []

    def fake(x):
        calls.append(tuple(x.shape))
        return torch.from_numpy(CR.luma_fwd(x.reshape(x.shape[0], 3, -1).numpy())).reshape(x.shape)
    monkeypatch.setattr(color, "luma_fwd", fake)
    color.clear_cache()
    t = torch.rand(2, 3, 4, 5)
    y = color.luma_cached(t)
    assert color.luma_cached(t) is y and len(calls) == 1 and not y.requires_grad
    assert np.array_equal(y.numpy(), CR.luma_fwd(t.reshape(2, 3, -1).numpy()).reshape(2, 3, 4, 5))
    t.mul_(0.5)                                         # the version moves on: a new entry
    y2 = color.luma_cached(t)
    assert y2 is not y and len(calls) == 2 and color.luma_cached(t) is y2
    one = torch.rand(1, 3, 4, 5)
    e = color.luma_cached(one.expand(3, -1, -1, -1))
    assert calls[-1] == (1, 3, 4, 5) and e.shape == (3, 3, 4, 5) and e.stride(0) == 0
    view = t[:1]                                        # same address, another shape: another key
    assert color.luma_cached(view) is not y2
    color.clear_cache()
    kept = [torch.rand(1, 3, 2, 2) for _ in range(color.CACHE_ENTRIES + 3)]
    outs = [color.luma_cached(k) for k in kept]
    assert len(color._CACHE) == color.CACHE_ENTRIES
    assert color.luma_cached(kept[-1]) is outs[-1]                      # the newest is still there
    n = len(calls)
    assert color.luma_cached(kept[0]) is not outs[0] and len(calls) == n + 1      # the oldest went out
    color.clear_cache()
    assert len(color._CACHE) == 0


def test_invalid_arguments_are_refused_on_the_host_before_any_launch():
    """null pointers, B <= 0, P == 0, an output that is an input: ST3D_E_INVALID, nothing launched (no GPU needed)"""
    import __graft_entry__ as g
    g.build()
    from st3d import _lib
    lib = _lib.load()
    assert lib.st3d_color_stats_chunk() > 0 and lib.st3d_color_stats_chunk() % 256 == 0
    p, q, r = 0x1000, 0x2000, 0x3000           # never dereferenced: every call below is refused first
    for rc in (lib.st3d_luma_fwd(None, 1, 4, q, None), lib.st3d_luma_fwd(p, 1, 4, None, None), lib.st3d_luma_fwd(p, 0, 4, q, None),
               lib.st3d_luma_fwd(p, 1, 0, q, None), lib.st3d_luma_fwd(p, 1, 4, p, None), lib.st3d_luma_fwd(p, 65536, 4, q, None),
               lib.st3d_luma_bwd(p, -1, 4, q, None), lib.st3d_luma_bwd(p, 1, 4, p, None),
               lib.st3d_luma_recombine(p, None, 1, 4, r, None), lib.st3d_luma_recombine(p, q, 1, 4, q, None),
               lib.st3d_color_affine(p, None, q, 1, 1, 4, r, None), lib.st3d_color_affine(p, q, q, 1, 1, 4, p, None),
               lib.st3d_color_stats(p, None, 1, 4, None, r, None), lib.st3d_color_stats(p, None, 1, 4, q, q, None),
               lib.st3d_color_stats(p, None, 1, 0, q, r, None)):
        assert rc == -1
        assert b"invalid argument" in lib.st3d_last_error() or b"do not fit one grid" in lib.st3d_last_error()


def test_reserve_cache_makes_room_for_a_cycle_of_view_batches(monkeypatch):
    """a loop that cycles through more sources than the cache holds misses every time; reserve_cache(n) ends that"""
    from st3d import color
    calls = []
    monkeypatch.setattr(color, "luma_fwd", lambda x: (calls.append(1), x.clone())[1])
    monkeypatch.setattr(color, "CACHE_ENTRIES", color.CACHE_ENTRIES)        # restored afterwards
    color.clear_cache()
    n = color.CACHE_ENTRIES + 4
    batches = [torch.rand(1, 3, 2, 2) for _ in range(n)]
    for _ in range(3):
        for t in batches:
            color.luma_cached(t)
    assert len(calls) == 3 * n                          # the cliff: every call recomputed
    color.clear_cache()
    del calls[:]
    color.reserve_cache(n)
    assert color.CACHE_ENTRIES == n
    firsts = [color.luma_cached(t) for t in batches]
    for _ in range(2):
        assert all(color.luma_cached(t) is y for t, y in zip(batches, firsts))
    assert len(calls) == n
    color.reserve_cache(2)
    assert color.CACHE_ENTRIES == n                     # never fewer
    color.clear_cache()
