"""Host side of the sliced Wasserstein style term: the C ABI's refusals (which launch nothing), the geometry and workspace
arithmetic, argument validation in Python, the refusal of CPU tensors, the CLI flags on all three scripts, the checkpoint
key, and that with the flags at their defaults no swd entry point is called while a positive weight makes the documented calls
in the documented order.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_swd_project", "st3d_swd_geometry", "st3d_swd_workspace_bytes", "st3d_swd_sort", "st3d_swd_loss", "st3d_swd_bwd")
WRAPPERS = ("swd_project", "swd_geometry", "swd_workspace_bytes", "swd_sort", "swd_loss", "swd_bwd")
BIG = (1 << 20) + 1


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_and_bound():
    from st3d import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    assert "swd.hip" in open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()
    assert ops.SWD_MAX_POSITIONS == 1 << 20 and ops.SWD_MAX_CHANNELS == 512 and all(hasattr(ops, w) for w in WRAPPERS)


def _pow2(n):
    return 1 << (n - 1).bit_length()


def test_geometry_and_workspace_are_pure_host_logic():
    from st3d import _lib, ops
    lib = _lib.load()
    block, passes = ctypes.c_int(-1), ctypes.c_int(-1)
    out = (ctypes.byref(block), ctypes.byref(passes))
    assert lib.st3d_swd_geometry(1, *out) == 0
    blk = block.value
    assert blk >= 2 and blk & (blk - 1) == 0 and blk * 8 <= 64 * 1024       # a power of two of 8-byte words that fits LDS
    for N in (1, 2, 3, 1000, blk - 1, blk, blk + 1, 2 * blk, 2 * blk + 1, 40000, 1 << 18, (1 << 20) - 1, 1 << 20):
        assert lib.st3d_swd_geometry(N, *out) == 0 and block.value == blk
        assert passes.value == max(0, (_pow2(N) // blk).bit_length() - 1)  # one per doubling of the run length above the block
        for B, K in ((1, 1), (3, 5), (8, 512)):
            assert lib.st3d_swd_workspace_bytes(B, K, N) == (0 if N <= blk else B * K * _pow2(N) * 8)
        assert ops.swd_geometry(N) == (blk, passes.value) and ops.swd_workspace_bytes(3, 5, N) == lib.st3d_swd_workspace_bytes(3, 5, N)
    for bad in (0, -1, BIG):
        assert lib.st3d_swd_geometry(bad, *out) == -1 and lib.st3d_swd_workspace_bytes(1, 1, bad) == 0
    for B, K in ((0, 1), (65536, 1), (1, 0), (1, 513), (-1, 1)):
        assert lib.st3d_swd_workspace_bytes(B, K, 2 * blk) == 0
    assert lib.st3d_swd_geometry(5, None, out[1]) == -1 and lib.st3d_swd_geometry(5, out[0], None) == -1


def test_every_entry_point_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with a HIP error (-2), not ST3D_E_INVALID (-1)"""
    from st3d import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)            # never dereferenced
    big = 1 << 40

    def variants(good, pointers, sizes):
        out = [good[:i] + [None] + good[i + 1:] for i in pointers]
        out += [good[:i] + [v] + good[i + 1:] for i, values in sizes.items() for v in values]
        return out
    pos, chan, batch, styles = (0, -1, BIG), (0, -1, 513), (0, -1, 65536), (0, 2, 4, -1)
    cases = {
        #                   x  a  B  Q   R   N    out stream
        "st3d_swd_project": variants([p, p, 3, 64, 48, 300, p, None], (0, 1, 6), {2: batch, 3: chan, 4: chan, 5: pos}),
        #                proj w  B  K  N      ws bytes sorted perm count stream      (w, perm, count may be NULL)
        "st3d_swd_sort": variants([p, p, 3, 5, 20000, p, big, p, p, p, None], (0, 5, 7),
                                  {2: batch, 3: chan, 4: pos, 5: (odd,), 6: (0, 3 * 5 * 32768 * 8 - 1)}),
        #                sorted count tsorted B  Bs K  N    M    inv  ws bytes loss stream
        "st3d_swd_loss": variants([p, p, p, 3, 1, 5, 100, 300, 1.0, p, big, p, None], (0, 1, 2, 9, 11),
                                  {3: batch, 4: styles, 5: chan, 6: pos, 7: pos, 9: (odd,), 10: (0, 3 * 5 * 8 - 1)}),
        #               sorted perm count tsorted gout B  Bs K  N    M    inv  gproj stream      (gout may be NULL)
        "st3d_swd_bwd": variants([p, p, p, p, p, 3, 3, 5, 100, 300, 1.0, p, None], (0, 1, 2, 3, 11),
                                 {5: batch, 6: styles, 7: chan, 8: pos, 9: pos}),
    }
    for name, bad in cases.items():
        for args in bad:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert b"invalid argument" in lib.st3d_last_error()
    # rows that fit a block need no workspace: NULL is then legal, so the refusal above was about the workspace alone
    assert lib.st3d_swd_workspace_bytes(3, 5, 4096) == 0 and lib.st3d_swd_workspace_bytes(3, 5, 20000) == 3 * 5 * 32768 * 8


# ---------------------------------------------------------------------------- 2. the Python surface
def test_cpu_tensors_are_refused():
    import losses as L
    import style_transfer as ST
    from st3d import ops
    f, s, v = torch.rand(2, 4, 3, 3), torch.rand(1, 4, 5, 5), torch.rand(6, 4)
    rows, count = torch.rand(2, 6, 9), torch.full((2,), 9, dtype=torch.int32)
    for call in (lambda: ST.swd_loss(f, s, v), lambda: ops.swd_project(f, v), lambda: ops.swd_sort(rows),
                 lambda: ops.swd_loss(rows, count, rows), lambda: ops.swd_bwd(rows, rows.to(torch.int32), count, rows)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    model = object.__new__(__import__("st3d.vgg", fromlist=["Vgg19Features"]).Vgg19Features)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.compute_swd_loss(torch.rand(2, 3, 32, 32), torch.rand(1, 3, 32, 32), model)


def test_directions_are_unit_rows_from_the_generator():
    import style_transfer as ST
    a = ST.swd_directions(7, 16, torch.Generator().manual_seed(5))
    b = ST.swd_directions(7, 16, torch.Generator().manual_seed(5))
    assert a.shape == (7, 16) and a.dtype == torch.float32 and torch.equal(a, b)
    assert torch.allclose(a.norm(dim=1), torch.ones(7), atol=1e-6)
    g = torch.Generator().manual_seed(5)
    draw = ST.swd_draw(("conv3_1", "conv1_1"), 0, g)
    assert [tuple(draw[n].shape) for n in ("conv3_1", "conv1_1")] == [(256, 256), (64, 64)]
    assert tuple(ST.swd_draw(("conv5_1",), 9, g)["conv5_1"].shape) == (9, 512)
    for bad in (0, 513, -1, 2.0, True):
        with pytest.raises(ValueError):
            ST.swd_directions(bad, 4)
        with pytest.raises(ValueError):
            ST.swd_directions(4, bad)


def test_bad_types_shapes_and_names(monkeypatch):
    import losses as L
    import style_transfer as ST
    from st3d import ops
    with pytest.raises(TypeError):
        ST.swd_loss([1.0], torch.rand(1, 4, 2, 2), torch.rand(3, 4))
    with pytest.raises(TypeError):
        L.compute_swd_loss(torch.rand(2, 3, 32, 32), torch.rand(1, 3, 32, 32), torch.nn.Sequential())
    for bad in (0, -3, BIG, 2.5, True, None):
        with pytest.raises(ValueError):
            ops.swd_geometry(bad)
        with pytest.raises(ValueError):
            ops.swd_workspace_bytes(1, 1, bad)
    for B, K in ((0, 1), (65536, 1), (1, 0), (1, 513)):
        with pytest.raises(ValueError):
            ops.swd_workspace_bytes(B, K, 5)
    for layers in ((), ("conv3_1", "conv3_1"), ("relu3_1",), "conv3_1,conv9_9"):
        with pytest.raises(ValueError):
            ST.check_swd_layers(layers)
    assert ST.SWD_LAYERS == tuple(ST._DEFAULT_LAYERS.values()) and len(ST.SWD_LAYERS) == 6
    assert ST.check_swd_layers("conv1_1,conv4_2") == ("conv1_1", "conv4_2") and ST.check_swd_layers(["conv5_1"]) == ("conv5_1",)
    for bad in (-1, 513, 1.0, True, None):
        with pytest.raises(ValueError):
            ST.check_swd_directions(bad)
    assert ST.check_swd_directions(0) == 0 and ST.check_swd_directions(512) == 512
    # wrapper shapes, refused before the library is reached
    with pytest.raises(ValueError):
        ops.swd_project(torch.rand(2, 4, 9), torch.rand(3, 5))                 # a does not fit x
    with pytest.raises(ValueError):
        ops.swd_project(torch.rand(4, 9), torch.rand(3, 4))                    # not (B,Q,N)
    with pytest.raises(ValueError):
        ops.swd_project(torch.rand(1, 513, 2), torch.rand(3, 513))
    with pytest.raises(ValueError):
        ops.swd_sort(torch.rand(2, 3, 9), torch.rand(2, 8))                    # weights of another size
    with pytest.raises(ValueError):
        ops.swd_loss(torch.rand(2, 3, 9), torch.zeros(3, dtype=torch.int32), torch.rand(1, 3, 4))    # count of another batch
    with pytest.raises(ValueError):
        ops.swd_loss(torch.rand(2, 3, 9), torch.zeros(2, dtype=torch.int32), torch.rand(1, 4, 4))    # rows differ
    with pytest.raises(ValueError):
        ops.swd_bwd(torch.rand(2, 3, 9), torch.zeros(2, 3, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                    torch.rand(3, 3, 4))
    # past the device check, shapes are refused before any kernel is called
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    def boom(*a, **k):
        raise AssertionError("a kernel was called")
    for name in ("swd_project", "swd_sort", "swd_loss", "swd_bwd"):
        monkeypatch.setattr(ops, name, boom)
    f, v = torch.rand(2, 4, 8, 8), torch.rand(3, 4)
    with pytest.raises(ValueError):
        ST.swd_loss(torch.rand(4, 8, 8), torch.rand(1, 4, 5, 5), v)            # not (B,C,H,W)
    with pytest.raises(ValueError):
        ST.swd_loss(f, torch.rand(1, 5, 5, 5), v)                              # channels differ
    with pytest.raises(ValueError):
        ST.swd_loss(f, torch.rand(3, 4, 5, 5), v)                              # Bs not in {1, B}
    for bad in (torch.rand(3, 5), torch.rand(4), torch.rand(513, 4), torch.rand(0, 4)):
        with pytest.raises(ValueError):
            ST.swd_loss(f, torch.rand(1, 4, 5, 5), bad)
    for mask in (torch.rand(3, 8, 8), torch.rand(2, 24, 24), torch.rand(2, 8, 16), torch.rand(2, 2, 8, 8)):
        with pytest.raises(ValueError):
            ST.swd_loss(f, torch.rand(1, 4, 5, 5), v, mask=mask)
    for denom in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ST.swd_loss(f, torch.rand(1, 4, 5, 5), v, batch_denom=denom)
    model = object.__new__(__import__("st3d.vgg", fromlist=["Vgg19Features"]).Vgg19Features)
    cur, sty = torch.rand(2, 3, 32, 32), torch.rand(1, 3, 48, 48)
    with pytest.raises(ValueError):
        L.compute_swd_loss(cur, sty, model, layers=("conv0_1",))
    with pytest.raises(ValueError):
        L.compute_swd_loss(cur, torch.rand(3, 3, 32, 32), model)
    with pytest.raises(ValueError):
        L.compute_swd_loss(cur, sty, model, masks=torch.rand(2, 16, 16))
    with pytest.raises(ValueError):
        L.compute_swd_loss(cur, sty, model, directions=513)
    with pytest.raises(ValueError):
        L.compute_swd_loss(cur, sty, model, layers=("conv2_1",), directions={"conv3_1": torch.rand(4, 256)})
    for kw in (dict(swd_weight=-1.0), dict(swd_weight=float("nan")), dict(swd_weight=1.0, swd_layers=("conv0_0",)),
               dict(swd_weight=1.0, swd_directions=513), dict(swd_weight=1.0, swd_seed=1.5)):
        with pytest.raises(ValueError):
            ST.style_transfer(cur, cur, cur, model, steps=1, **kw)


# ---------------------------------------------------------------------------- 3. the CLI
def test_all_three_parsers_carry_the_flags_with_their_defaults():
    import st3d.cli as cli
    import style_transfer as ST
    assert tuple(cli._SWD_LAYERS) == ST.SWD_LAYERS
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.swd_weight == 0.0 and a.swd_layers == ("conv2_1", "conv3_1", "conv4_1", "conv5_1") == ST.SWD_DEFAULT_LAYERS
        assert a.swd_directions == 0
        b = mod.build_parser().parse_args(["--swd_weight", "2.5", "--swd_layers", "conv1_1,conv4_2", "--swd_directions", "64",
                                           "--style_weight", "0", "--style_mask", "object"])
        assert b.swd_weight == 2.5 and b.swd_layers == ("conv1_1", "conv4_2") and b.swd_directions == 64
        assert b.style_weight == 0.0 and cli.check_args(b) is None           # --style_weight 0 stays legal: the term alone


def test_bad_flags_are_refused_before_any_gpu_work(monkeypatch, capsys):
    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    for mod in _scripts():
        monkeypatch.setattr(mod, "Run", no_gpu)
        for argv, word in ((["--swd_weight", "-1"], "--swd_weight must be"),
                           (["--swd_weight", "nan"], "--swd_weight must be"),
                           (["--swd_weight", "inf"], "--swd_weight must be"),
                           (["--swd_directions", "513"], "--swd_directions must be"),
                           (["--swd_directions", "-1"], "--swd_directions must be"),
                           (["--swd_layers", "conv1_2"], "--swd_layers"),
                           (["--swd_layers", "conv3_1,conv3_1"], "--swd_layers"),
                           (["--swd_layers", ""], "--swd_layers")):
            with pytest.raises(SystemExit) as e:
                mod.main(argv)
            assert e.value.code == 2, argv
            assert word in capsys.readouterr().err


# ---------------------------------------------------------------------------- 4. what runs
def _recording_ops(monkeypatch, calls):
    """every wrapper of the new entry points replaced by a CPU stand-in that records its name"""
    from st3d import ops

    def rec(name, fn):
        def inner(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, inner)

    def project(x, a):
        return torch.einsum("rq,bqn->brn", a, x.reshape(x.shape[0], x.shape[1], -1))

    def sort(proj, weights=None, want_perm=True):
        values, perm = torch.sort(proj, dim=2)
        return values, perm.to(torch.int32) if want_perm else None, torch.full((proj.shape[0],), proj.shape[2], dtype=torch.int32)
    rec("swd_project", project)
    rec("swd_sort", sort)
    rec("swd_loss", lambda rows, count, tsorted, denom=None: torch.full((1,), 0.25 * rows.shape[0] / float(denom or rows.shape[0])))
    rec("swd_bwd", lambda rows, perm, count, tsorted, denom=None, g=None: torch.ones_like(rows))
    for name in ("swd_geometry", "swd_workspace_bytes"):
        rec(name, lambda *a: 0)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def _fake_vgg(monkeypatch, seen):
    """get_features replaced by a differentiable CPU stand-in with the real tap names and channel counts"""
    import style_transfer as ST
    from st3d import vgg

    def features(image, model, layers=None):
        seen.append((tuple(image.shape), image.requires_grad and torch.is_grad_enabled(), tuple(sorted(layers.values()))))
        return {name: image[:, :1].expand(-1, ST._SWD_CHANNELS[name], -1, -1)[:, :, ::4, ::4] * 1.0 for name in layers.values()}
    monkeypatch.setattr(ST, "get_features", features)
    return object.__new__(vgg.Vgg19Features)


def _run(model, argv):
    import st3d.cli as cli
    run = cli.Run.__new__(cli.Run)
    run.vgg, run.world = model, 1
    run.args = _scripts()[1].build_parser().parse_args(argv)
    run.swd_generator = (torch.Generator().manual_seed(run.args.seed if run.args.seed is not None else 0)
                         if run.args.swd_weight else None)
    return run


def test_defaults_call_nothing_and_the_term_is_these_calls_in_this_order(monkeypatch):
    calls, seen = [], []
    _recording_ops(monkeypatch, calls)
    model = _fake_vgg(monkeypatch, seen)
    current = torch.rand(2, 3, 32, 32, requires_grad=True)
    cov = torch.ones(2, 1, 32, 32)
    style = torch.rand(1, 3, 32, 32).expand(2, -1, -1, -1)
    run = _run(model, [])
    assert run.swd_term(current, cov, style, 2) == 0 and calls == [] and seen == []
    # switched on: the style taps once (features only, cached); per tap project -> sort (render), project -> sort (style), loss;
    # backward: per tap bwd -> project with the transposed directions
    run = _run(model, ["--swd_weight", "3", "--swd_layers", "conv3_1,conv2_1", "--swd_directions", "8", "--style_mask", "object"])
    before = run.swd_generator.get_state()
    term = run.swd_term(current, cov, style, 4)                            # 2 local views of a global batch of 4
    tap = ["swd_project", "swd_sort", "swd_project", "swd_sort", "swd_loss"]
    assert calls == tap * 2
    assert seen == [((1, 3, 32, 32), False, ("conv2_1", "conv3_1")), ((2, 3, 32, 32), True, ("conv2_1", "conv3_1"))]
    assert float(term.detach()) == pytest.approx(3.0 * 2 * (2 * 0.25 / 4))   # weight x taps x (sum over views / global batch)
    assert not torch.equal(run.swd_generator.get_state(), before)          # the step's directions were drawn
    del calls[:]
    term.backward()
    assert calls == ["swd_bwd", "swd_project"] * 2 and current.grad is not None
    # the next step reuses the cached style taps (no style forward) but projects and sorts them again: new directions
    del calls[:], seen[:]
    run.swd_term(current, cov, torch.Tensor.expand(style[:1], 2, -1, -1, -1), 4)
    assert calls == tap * 2 and len(seen) == 1
    # a rank without views adds nothing and calls nothing, but makes the step's draw like every other rank
    del calls[:]
    twin = _run(model, ["--swd_weight", "3", "--swd_layers", "conv3_1,conv2_1", "--swd_directions", "8"])
    twin.swd_generator.set_state(run.swd_generator.get_state())
    assert run.swd_term(None, None, None, 4) == 0 and calls == []
    twin.swd_term(current, cov, style, 4)
    assert torch.equal(run.swd_generator.get_state(), twin.swd_generator.get_state())
    assert run.swd_term(current[:0], cov[:0], style, 4) == 0


def test_directions_follow_the_seed_and_the_mask_needs_style_mask_object(monkeypatch):
    from st3d import ops
    import style_transfer as ST
    calls, seen, got, weights = [], [], [], []
    _recording_ops(monkeypatch, calls)
    model = _fake_vgg(monkeypatch, seen)
    inner_p, inner_s = ops.swd_project, ops.swd_sort
    monkeypatch.setattr(ops, "swd_project", lambda x, a: (got.append(a.clone()), inner_p(x, a))[1])
    monkeypatch.setattr(ops, "swd_sort", lambda p, w=None, want_perm=True: (weights.append(w), inner_s(p, w, want_perm))[1])
    current, style = torch.rand(2, 3, 32, 32, requires_grad=True), torch.rand(1, 3, 32, 32)
    cov = torch.zeros(2, 1, 32, 32)
    cov[:, :, :16] = 1
    argv = ["--swd_weight", "1", "--swd_layers", "conv2_1", "--swd_directions", "5", "--seed", "3"]
    run = _run(model, argv)
    run.swd_term(current, cov, style, 2)
    expect = ST.swd_directions(5, 128, torch.Generator().manual_seed(3))
    assert torch.equal(got[0], expect) and torch.equal(got[1], expect)      # render and style: the same directions
    assert weights == [None, None]
    run.swd_term(current, cov, style, 2)
    assert not torch.equal(got[2], expect)                                   # redrawn every step
    del weights[:]
    run = _run(model, argv + ["--style_mask", "object"])
    run.swd_term(current, cov, style, 2)
    assert weights[1] is None and tuple(weights[0].shape) == (2, 8, 8)       # the style side has no weights
    assert np.array_equal(weights[0][0].numpy(), np.repeat([[1.0], [0.0]], 4, 0).repeat(8, 1))


def test_style_transfer_defaults_call_no_swd_entry_point(monkeypatch):
    """the fused plan stands in as a stub: what is counted is the calls through ops"""
    import style_transfer as ST
    from st3d import optim as O
    calls, seen = [], []
    _recording_ops(monkeypatch, calls)
    model = _fake_vgg(monkeypatch, seen)

    class Plan:
        def set_content(self, *a, **k):
            pass
        set_style = set_content

        def loss(self, x, sw, cw, style_mask=None):
            return torch.zeros(()), torch.zeros_like(x)
    monkeypatch.setattr(type(model), "plan", lambda self, B, S: Plan(), raising=False)

    class Adam:
        def __init__(self, params, lr, reduce_grads):
            self.params = params

        def step(self):
            with torch.no_grad():
                self.params[0] -= 0.1 * self.params[0].grad
    monkeypatch.setattr(O, "Adam", Adam)
    monkeypatch.setattr(ST, "device", torch.device("cpu"))
    cur = torch.rand(2, 3, 32, 32)
    out = ST.style_transfer(cur, cur, cur, model, steps=2)
    assert calls == [] and seen == [] and torch.equal(out.detach(), cur)
    out = ST.style_transfer(cur, cur, cur, model, steps=2, swd_weight=1.0, swd_layers=("conv2_1",), swd_directions=4)
    assert calls == ["swd_project", "swd_sort", "swd_project", "swd_sort", "swd_loss", "swd_bwd", "swd_project"] * 2
    assert not torch.equal(out.detach(), cur)


# ---------------------------------------------------------------------------- 5. the checkpoint key
def _bare_run(tmp_path, generator):
    import st3d.cli as cli
    run = cli.Run.__new__(cli.Run)
    run.rank, run.world, run.out_dir, run.device = 0, 1, str(tmp_path), torch.device("cpu")
    run.pyramid, run.vertex_colors, run.atlas_r, run.chamfer_generator = None, False, 0, None
    run.swd_generator = generator
    run.args = _scripts()[1].build_parser().parse_args([])
    run.opt = {"texture_map": torch.rand(4, 4, 3), "verts": torch.rand(5, 3)}

    class Opt:
        def state_dict(self):
            return {"step": 0}

        def load_state_dict(self, state):
            pass
    run.optimizer = Opt()
    return run


def test_the_generator_state_travels_in_the_checkpoint_and_a_mismatch_is_refused(tmp_path):
    import style_transfer as ST
    g = torch.Generator().manual_seed(0)
    ST.swd_draw(("conv2_1",), 4, g)                                          # some steps in
    run = _bare_run(tmp_path, g)
    run.save_checkpoint(2)
    ck = os.path.join(str(tmp_path), "checkpoint.pt")
    blob = torch.load(ck, map_location="cpu", weights_only=True)
    assert blob["swd_generator_state"].dtype == torch.uint8 and torch.equal(blob["swd_generator_state"], g.get_state())
    ahead = ST.swd_draw(("conv2_1",), 4, g)["conv2_1"]
    resumed = _bare_run(tmp_path, torch.Generator().manual_seed(0))
    resumed.load_checkpoint(ck)
    assert resumed.progress == 2 and torch.equal(ST.swd_draw(("conv2_1",), 4, resumed.swd_generator)["conv2_1"], ahead)
    with pytest.raises(ValueError, match="with --swd_weight, this run is without"):
        _bare_run(tmp_path, None).load_checkpoint(ck)
    _bare_run(tmp_path, None).save_checkpoint(1)
    assert "swd_generator_state" not in torch.load(ck, map_location="cpu", weights_only=True)
    with pytest.raises(ValueError, match="without --swd_weight, this run is with"):
        _bare_run(tmp_path, torch.Generator().manual_seed(0)).load_checkpoint(ck)
