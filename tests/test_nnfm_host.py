"""Host side of the NNFM style term: the C ABI's refusals (which launch nothing), argument validation in Python, the refusal
of CPU tensors, the CLI flags on all three scripts, that weight 0 calls nothing and a positive weight makes the documented
calls in the documented order.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("st3d_nnfm_geometry", "st3d_nnfm_workspace_bytes", "st3d_nnfm_normalise", "st3d_nnfm_search", "st3d_nnfm_sum",
         "st3d_nnfm_bwd")
BIG = (1 << 20) + 1


def _scripts():
    import first_approach as FA
    import second_approach as SA
    import third_approach as TA
    return FA, SA, TA


# ---------------------------------------------------------------------------- 1. the C ABI
def test_symbols_are_declared_and_bound():
    from st3d import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st3d.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    assert "nnfm.hip" in open(os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "build.py")).read()


def test_geometry_and_sizes_are_pure_host_logic():
    from st3d import _lib
    lib = _lib.load()
    tq, ts, seg = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    out = (ctypes.byref(tq), ctypes.byref(ts), ctypes.byref(seg))
    for N, M, C in ((1, 1, 1), (63, 257, 3), (1000, 1000, 100), (4096, 4096, 512), (16384, 16384, 256), (8, 1 << 20, 64),
                    (1 << 20, 1 << 20, 512)):
        assert lib.st3d_nnfm_geometry(N, M, C, *out) == 0
        stiles = -(-M // ts.value)
        assert tq.value >= 1 and ts.value >= 1 and 1 <= seg.value <= stiles
        per_run = -(-stiles // seg.value)
        assert (seg.value - 1) * per_run < stiles                          # no run is empty
        for B in (1, 3):
            assert lib.st3d_nnfm_workspace_bytes(B, N, M, C) == seg.value * B * N * 8
    assert lib.st3d_nnfm_geometry(1, 1, 1, *out) == 0 and seg.value == 1
    for bad in ((0, 5, 4), (5, 0, 4), (5, 5, 0), (-1, 5, 4), (BIG, 5, 4), (5, BIG, 4), (5, 5, 513), (5, 5, -2)):
        assert lib.st3d_nnfm_geometry(*bad, *out) == -1
        assert lib.st3d_nnfm_workspace_bytes(1, *bad) == 0
    assert lib.st3d_nnfm_workspace_bytes(0, 5, 5, 4) == 0 and lib.st3d_nnfm_workspace_bytes(65536, 5, 5, 4) == 0
    for k in range(3):
        ptrs = list(out)
        ptrs[k] = None
        assert lib.st3d_nnfm_geometry(5, 5, 4, *ptrs) == -1


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
    pos, chan, batch = (0, -1, BIG), (0, -1, 513), (0, -1, 65536)
    cases = {
        #                      x  B  C   M    xhat norm stream          (xhat may be NULL)
        "st3d_nnfm_normalise": variants([p, 2, 64, 300, p, p, None], (0, 5), {1: batch, 2: chan, 3: pos}),
        #                   fhat fnorm shat w  B  Bs C   N    M    ws bytes idx dist stream          (w may be NULL)
        "st3d_nnfm_search": variants([p, p, p, p, 3, 1, 64, 100, 300, p, big, p, p, None], (0, 1, 2, 9, 11, 12),
                                     {4: batch, 5: (0, 2, 4, -1), 6: chan, 7: pos, 8: pos, 10: (0, 3 * 3 * 100 * 8 - 1), 9: (odd,)}),
        #                dist w  B  N   inv_denom loss wsum stream
        "st3d_nnfm_sum": variants([p, p, 3, 100, 1.0, p, p, None], (0, 5, 6), {2: batch, 3: pos, 6: (odd,)}),
        #                feat shat idx dist w wsum gout B  Bs C   N    M    inv_denom grad stream   (w, gout may be NULL)
        "st3d_nnfm_bwd": variants([p, p, p, p, p, p, p, 3, 3, 64, 100, 300, 1.0, p, None], (0, 1, 2, 3, 5, 13),
                                  {7: batch, 8: (0, 2, 4, -1), 9: chan, 10: pos, 11: pos, 5: (odd,)}),
    }
    for name, bad in cases.items():
        for args in bad:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert b"invalid argument" in lib.st3d_last_error()


# ---------------------------------------------------------------------------- 2. the Python surface
def test_cpu_tensors_are_refused():
    import losses as L
    import style_transfer as ST
    from st3d import ops
    f, s = torch.rand(2, 4, 3, 3), torch.rand(1, 4, 5, 5)
    for call in (lambda: ST.nnfm_loss(f, s), lambda: ST.nnfm_style(s), lambda: ops.nnfm_normalise(f),
                 lambda: ops.nnfm_search(f, s)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    model = object.__new__(__import__("st3d.vgg", fromlist=["Vgg19Features"]).Vgg19Features)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.compute_nnfm_loss(torch.rand(2, 3, 32, 32), torch.rand(1, 3, 32, 32), model)


def test_bad_types_shapes_and_names(monkeypatch):
    import losses as L
    import style_transfer as ST
    from st3d import ops
    with pytest.raises(TypeError):
        ST.nnfm_loss([1.0], torch.rand(1, 4, 2, 2))
    with pytest.raises(TypeError):
        L.compute_nnfm_loss(torch.rand(2, 3, 32, 32), torch.rand(1, 3, 32, 32), torch.nn.Sequential())
    for bad in (0, -3, BIG, 2.5, True, None):
        with pytest.raises(ValueError):
            ops.nnfm_geometry(bad, 5, 4)
        with pytest.raises(ValueError):
            ops.nnfm_geometry(5, bad, 4)
    with pytest.raises(ValueError):
        ops.nnfm_geometry(5, 5, 513)
    for layers in ((), ("conv1_1",), ("conv3_1", "conv3_1"), ("relu3_1",), "conv3_1,conv9_9"):
        with pytest.raises(ValueError):
            ST.check_nnfm_layers(layers)
    assert ST.check_nnfm_layers("conv2_1,conv4_2") == ("conv2_1", "conv4_2") and ST.check_nnfm_layers(["conv5_1"]) == ("conv5_1",)
    # past the device check, shapes are refused before any kernel is called
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    def boom(*a, **k):
        raise AssertionError("a kernel was called")
    for name in ("nnfm_search", "nnfm_sum", "nnfm_bwd"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(ops, "nnfm_normalise", lambda x, want_hat=True: (x.clone(), x.new_ones(x.shape[0], x.shape[2] * x.shape[3])))
    f = torch.rand(2, 4, 8, 8)
    with pytest.raises(ValueError):
        ST.nnfm_loss(torch.rand(4, 8, 8), torch.rand(1, 4, 5, 5))                  # not (B,C,H,W)
    with pytest.raises(ValueError):
        ST.nnfm_loss(f, torch.rand(1, 5, 5, 5))                                    # channels differ
    with pytest.raises(ValueError):
        ST.nnfm_loss(f, torch.rand(3, 4, 5, 5))                                    # Bs not in {1, B}
    for mask in (torch.rand(3, 8, 8), torch.rand(2, 24, 24), torch.rand(2, 8, 16), torch.rand(2, 256, 256), torch.rand(2, 2, 8, 8)):
        with pytest.raises(ValueError):
            ST.nnfm_loss(f, torch.rand(1, 4, 5, 5), mask=mask)
    for denom in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ST.nnfm_loss(f, torch.rand(1, 4, 5, 5), batch_denom=denom)
    model = object.__new__(__import__("st3d.vgg", fromlist=["Vgg19Features"]).Vgg19Features)
    cur, sty = torch.rand(2, 3, 32, 32), torch.rand(1, 3, 48, 48)
    with pytest.raises(ValueError):
        L.compute_nnfm_loss(cur, sty, model, layers=("conv1_1",))
    with pytest.raises(ValueError):
        L.compute_nnfm_loss(cur, torch.rand(3, 3, 32, 32), model)
    with pytest.raises(ValueError):
        L.compute_nnfm_loss(cur, sty, model, masks=torch.rand(2, 16, 16))
    with pytest.raises(ValueError):
        ST.style_transfer(cur, cur, cur, model, steps=1, nnfm_weight=-1.0)
    with pytest.raises(ValueError):
        ST.style_transfer(cur, cur, cur, model, steps=1, nnfm_weight=float("nan"))
    with pytest.raises(ValueError):
        ST.style_transfer(cur, cur, cur, model, steps=1, nnfm_weight=1.0, nnfm_layers=("conv0_0",))


# ---------------------------------------------------------------------------- 3. the CLI
def test_all_three_parsers_carry_the_flags_with_their_defaults():
    import st3d.cli as cli
    import style_transfer as ST
    assert tuple(cli._NNFM_LAYERS) == ST.NNFM_LAYERS
    assert all(name in ST._DEFAULT_LAYERS.values() for name in ST.NNFM_LAYERS)
    for mod in _scripts():
        a = mod.build_parser().parse_args([])
        assert a.nnfm_weight == 0.0 and a.nnfm_layers == ("conv3_1",)
        b = mod.build_parser().parse_args(["--nnfm_weight", "2.5", "--nnfm_layers", "conv2_1,conv4_2", "--style_weight", "0",
                                           "--style_mask", "object"])
        assert b.nnfm_weight == 2.5 and b.nnfm_layers == ("conv2_1", "conv4_2") and b.style_weight == 0.0
        assert cli.check_args(b) is None                                   # --style_weight 0 stays legal: NNFM alone


def test_bad_flags_are_refused_before_any_gpu_work(monkeypatch, capsys):
    def no_gpu(*a, **k):
        raise AssertionError("the run was set up")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    for mod in _scripts():
        monkeypatch.setattr(mod, "Run", no_gpu)
        for argv, word in ((["--nnfm_weight", "-1"], "--nnfm_weight must be"),
                           (["--nnfm_weight", "nan"], "--nnfm_weight must be"),
                           (["--nnfm_weight", "inf"], "--nnfm_weight must be"),
                           (["--nnfm_layers", "conv1_1"], "--nnfm_layers"),
                           (["--nnfm_layers", "conv3_1,conv3_1"], "--nnfm_layers"),
                           (["--nnfm_layers", ""], "--nnfm_layers")):
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

    def positions(x):
        return x.shape[2] * x.shape[3]
    rec("nnfm_normalise", lambda x, want_hat=True: (x.clone(), torch.ones(x.shape[0], positions(x))))
    rec("nnfm_search", lambda f, s, w=None, normalised=None: (torch.zeros(f.shape[0], positions(f), dtype=torch.int32),
                                                              torch.full((f.shape[0], positions(f)), 0.25)))
    rec("nnfm_sum", lambda d, w=None, denom=None: (d.mean(1).sum().reshape(1) / float(denom or d.shape[0]),
                                                   torch.full((d.shape[0],), float(d.shape[1]), dtype=torch.float64)))
    rec("nnfm_bwd", lambda f, s, i, d, ws, w=None, denom=None, g=None: torch.ones_like(f))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def _fake_vgg(monkeypatch, seen):
    """get_features replaced by a differentiable CPU stand-in with the real tap names"""
    import style_transfer as ST
    from st3d import vgg

    def features(image, model, layers=None):
        seen.append((tuple(image.shape), image.requires_grad and torch.is_grad_enabled(), tuple(sorted(layers.values()))))
        return {name: image[:, :1].expand(-1, 4, -1, -1)[:, :, ::4, ::4] * 1.0 for name in layers.values()}
    monkeypatch.setattr(ST, "get_features", features)
    return object.__new__(vgg.Vgg19Features)


def test_weight_zero_calls_nothing_and_the_term_is_these_calls_in_this_order(monkeypatch):
    import st3d.cli as cli
    calls, seen = [], []
    _recording_ops(monkeypatch, calls)
    model = _fake_vgg(monkeypatch, seen)
    run = cli.Run.__new__(cli.Run)
    run.vgg, run.world = model, 1
    current = torch.rand(2, 3, 32, 32, requires_grad=True)
    cov = torch.ones(2, 1, 32, 32)
    style = torch.rand(1, 3, 32, 32).expand(2, -1, -1, -1)
    run.args = _scripts()[1].build_parser().parse_args([])
    assert run.nnfm_term(current, cov, style, 2) == 0 and calls == [] and seen == []
    # switched on: the style taps once (normalised, cached), then per tap normalise -> search -> sum; backward: one bwd per tap
    run.args = _scripts()[1].build_parser().parse_args(["--nnfm_weight", "3", "--nnfm_layers", "conv3_1,conv4_1", "--style_mask",
                                                        "object"])
    term = run.nnfm_term(current, cov, style, 4)                           # 2 local views of a global batch of 4
    assert calls == ["nnfm_normalise", "nnfm_normalise"] + ["nnfm_normalise", "nnfm_search", "nnfm_sum"] * 2
    assert seen == [((1, 3, 32, 32), False, ("conv3_1", "conv4_1")), ((2, 3, 32, 32), True, ("conv3_1", "conv4_1"))]
    assert float(term.detach()) == pytest.approx(3.0 * 2 * (2 * 0.25 / 4))   # weight x taps x (sum over views / global batch)
    del calls[:]
    term.backward()
    assert calls == ["nnfm_bwd", "nnfm_bwd"] and current.grad is not None
    # the next step reuses the cached style taps: no style forward, no style normalisation
    del calls[:], seen[:]
    run.nnfm_term(current, cov, torch.Tensor.expand(style[:1], 2, -1, -1, -1), 4)
    assert calls == ["nnfm_normalise", "nnfm_search", "nnfm_sum"] * 2 and len(seen) == 1
    # an idle rank adds nothing
    del calls[:]
    assert run.nnfm_term(None, None, style, 4) == 0 and run.nnfm_term(current[:0], cov[:0], style, 4) == 0 and calls == []


def test_the_mask_reaches_the_search_only_with_style_mask_object(monkeypatch):
    import st3d.cli as cli
    from st3d import ops
    calls, seen, got = [], [], []
    _recording_ops(monkeypatch, calls)
    model = _fake_vgg(monkeypatch, seen)
    inner = ops.nnfm_search
    monkeypatch.setattr(ops, "nnfm_search", lambda f, s, w=None, normalised=None: (got.append(w), inner(f, s, w, normalised))[1])
    run = cli.Run.__new__(cli.Run)
    run.vgg, run.world = model, 1
    current, style = torch.rand(2, 3, 32, 32, requires_grad=True), torch.rand(1, 3, 32, 32)
    cov = torch.zeros(2, 1, 32, 32)
    cov[:, :, :16] = 1
    run.args = _scripts()[1].build_parser().parse_args(["--nnfm_weight", "1"])
    run.nnfm_term(current, cov, style, 2)
    assert got == [None]
    run.args = _scripts()[1].build_parser().parse_args(["--nnfm_weight", "1", "--style_mask", "object"])
    run.nnfm_term(current, cov, style, 2)
    assert tuple(got[1].shape) == (2, 8, 8) and np.array_equal(got[1][0].numpy(), np.repeat([[1.0], [0.0]], 4, 0).repeat(8, 1))
