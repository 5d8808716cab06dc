"""The guarded-allocation harness (tests/_guarded.py) on the CPU: four fake ops that allocate through this module's own
`torch`, with the shim applied to this module, and the coverage rule of tests/test_gpu_guarded.py.  No GPU, no library."""
import inspect
import sys

import pytest
import torch
import torch as real_torch         # `torch` is the name the shim replaces in this module; this one stays

import _guarded as G

ME = sys.modules[__name__]
N = 37


# ------------------------------------------------------------------------------------------------ the fake ops
def op_correct(x):
    out = torch.empty((N,), dtype=torch.float32)
    scratch = torch.empty((N,), dtype=torch.float32)
    count = torch.zeros((1,), dtype=torch.int32)
    lst = torch.full((N,), -1, dtype=torch.int32)
    scratch.copy_(x * 2)
    out.copy_(scratch + 1)
    count += N
    lst[:3] = 7
    return {"out": out, "count": count, "list": lst, "like": torch.zeros_like(x), "ones": torch.ones(3)}


def _raw(t, lo, hi):
    """elements lo..hi-1 counted from the payload's start, guards included: what a kernel's pointer arithmetic reaches"""
    return torch.as_strided(t, (hi - lo,), (1,), t.storage_offset() + lo)


def op_overrun_rear(x):
    out = torch.empty((N,), dtype=torch.float32)
    _raw(out, 0, N + 1).copy_(torch.cat([x, x[:1]]))       # one element past the end
    return {"out": out}


def op_overrun_front(x):
    out = torch.empty((N,), dtype=torch.float32)
    _raw(out, -1, N).copy_(torch.cat([x[:1], x]))          # one element before the start
    return {"out": out}


def op_skips_one(x):
    out = torch.empty((N,), dtype=torch.float32)
    out[:N - 1] = x[:N - 1]                                 # the last element is never written
    return {"out": out}


def op_reads_scratch(x):
    scratch = torch.empty((N,), dtype=torch.float32)
    out = torch.empty((N,), dtype=torch.float32)
    scratch[1:] = x[1:]                                     # scratch[0] is read below before anything wrote it
    out.copy_(scratch * 0.5)
    return {"out": out}


def op_escapes(x):
    return {"out": x.new_empty((N,)).copy_(x)}              # a tensor method: not seen by the shim


def _x():
    return torch.arange(N, dtype=torch.float32) + 1.0


def _ab(op, **kw):
    return G.compare_ab(lambda: op(_x()), modules=(ME,), **kw)


# ------------------------------------------------------------------------------------------------ the harness
def test_correct_op_passes_and_the_shim_is_removed():
    out = _ab(op_correct)
    assert torch.equal(out["out"], _x() * 2 + 1) and int(out["count"]) == N and int(out["list"][5]) == -1
    assert float(out["like"].abs().sum()) == 0.0 and float(out["ones"].sum()) == 3.0
    assert ME.torch is real_torch


def test_payload_is_aligned_between_pattern_guards():
    for pattern in (0xFF, 0x01):
        with G.Guarded(pattern, (ME,)) as g:
            t = torch.empty((3, 5), dtype=torch.float32)
            z = torch.zeros((2,), dtype=torch.int64)
            pinned_kw = torch.empty((1,), dtype=torch.int32, pin_memory=False)
        rec = g.records[0]
        assert rec.G == 64 * 1024 and rec.nbytes == 60 and rec.kind == "empty" and rec.site.startswith("test_payload_is_aligned")
        assert t.data_ptr() - rec.buffer.data_ptr() == rec.G and rec.buffer.numel() == 2 * rec.G + 60
        assert bool((rec.buffer == pattern).all())
        assert t.view(-1).view(torch.uint8).tolist() == [pattern] * 60 and z.tolist() == [0, 0]
        assert g.owns(t) and g.owns(t[1]) and g.owns(z) and g.owns(pinned_kw) and not g.owns(torch.empty(3))
        g.check()
    assert G.guard_bytes(0) == 65536 and G.guard_bytes(65537) == 66048 and G.guard_bytes(1 << 30) == 4 << 20
    assert all(G.guard_bytes(n) % 512 == 0 and (G.guard_bytes(n) >= n or n > 4 << 20) for n in (1, 511, 513, 100000, 5 << 20))
    assert torch.isnan(torch.tensor([0xFF] * 4, dtype=torch.uint8).view(torch.float32)).all()
    assert 0 < float(torch.tensor([0x01] * 4, dtype=torch.uint8).view(torch.float32)) < 1e-37


def test_restores_on_an_exception():
    with pytest.raises(ZeroDivisionError):
        with G.Guarded(0xFF, (ME,)):
            assert ME.torch is not real_torch
            1 / 0
    assert ME.torch is real_torch


@pytest.mark.parametrize("op,side,other,first", [(op_overrun_rear, "rear", "front", "offsets 0..3 from the payload's end"),
                                                  (op_overrun_front, "front", "rear", "offsets -4..-1 from the payload's start")])
def test_write_of_one_element_past_the_output_is_reported_with_its_side(op, side, other, first):
    with pytest.raises(AssertionError) as e:
        _ab(op, plain=False)            # (without the guards there is no room behind the output: no plain run)
    msg = str(e.value)
    assert "guard written" in msg and f"{op.__name__}:" in msg and f"the {side} guard changed" in msg and first in msg
    assert f"the {other} guard" not in msg
    assert ME.torch is real_torch


def test_element_left_unwritten_is_reported_by_the_ab_comparison():
    with pytest.raises(AssertionError) as e:
        _ab(op_skips_one)
    msg = str(e.value)
    assert "output 'out' depends on what its memory held" in msg and f"first at element {N - 1} of {N}" in msg
    assert "guard written" not in msg
    # and the specified part alone passes: what an UNSPECIFIED entry does
    _ab(op_skips_one, specified={"out": lambda t, outs: t[:N - 1]})


def test_scratch_read_before_it_is_written_is_reported():
    with pytest.raises(AssertionError) as e:
        _ab(op_reads_scratch)
    msg = str(e.value)
    assert "output 'out' depends on what its memory held" in msg and f"first at element 0 of {N}" in msg


def test_output_that_escapes_the_shim_is_reported_unless_it_is_the_callers_own():
    with pytest.raises(AssertionError, match="unguarded output 'out'"):
        _ab(op_escapes)
    keep = {}

    def own_buffer():
        keep["y"] = torch.zeros((N,))           # this module's torch is the real one out here: the case's own buffer
        keep["y"].copy_(_x())
        return {"y": keep["y"]}
    G.compare_ab(own_buffer, modules=(), own=lambda outs: [outs["y"]])


# ------------------------------------------------------------------------------------------------ coverage of st3d.ops
def _device_wrappers():
    from st3d import ops
    names = []
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        if 'call("st3d_' in inspect.getsource(fn):
            names.append(name)
    return ops, names


def test_every_device_wrapper_of_ops_has_a_guarded_case():
    """A public function of st3d.ops whose source holds call("st3d_ is covered by a case of tests/test_gpu_guarded.py or is
    named in NOT_COVERED with a reason; NOT_COVERED may hold only wrappers that launch nothing on the device or cannot run
    in one process on one GPU.  A wrapper added later fails here until it gets a case."""
    import test_gpu_guarded as TG
    ops, names = _device_wrappers()
    assert len(names) >= 90, names          # (96 today: the scan found the module)
    covered = {w for case in TG.CASES.values() for w in case.covers}
    missing = sorted(n for n in names if n not in covered and n not in TG.NOT_COVERED)
    assert not missing, f"no guarded case and no NOT_COVERED entry: {missing}"
    unknown = sorted(n for n in covered | set(TG.NOT_COVERED) | {u[0] for u in TG.UNSPECIFIED} if n not in names)
    assert not unknown, f"named in CASES / NOT_COVERED / UNSPECIFIED but no device wrapper of st3d.ops: {unknown}"
    both = sorted(covered & set(TG.NOT_COVERED))
    assert not both, both
    assert all(isinstance(r, str) and len(r) > 20 for r in TG.NOT_COVERED.values())
    # NOT_COVERED: host-side queries only -- none of them takes a stream
    for n in TG.NOT_COVERED:
        assert "stream_ptr()" not in inspect.getsource(getattr(ops, n)), f"{n} launches on a stream: it needs a case"
    for wrapper, output, part, sentence in TG.UNSPECIFIED:
        assert callable(part) and isinstance(sentence, str) and len(sentence) > 20, (wrapper, output)
    # the float-atomic entry points the issue names run once more with set_deterministic(False)
    atomic = {w for case in TG.CASES.values() if case.atomics for w in case.covers}
    assert {"shade_bwd", "shade_ss_bwd", "shade_soft_bwd", "shade_vc_bwd", "shade_atlas_bwd", "shade_mip_bwd", "raster_bwd",
            "raster_soft_bwd"} <= atomic
