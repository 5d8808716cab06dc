"""The guided style loss without a GPU: the --style_mask flag of the three scripts, the C ABI's refusals (checked on the
host before any launch, with pointers that are never dereferenced), the binding table against the header.

One refusal is not here: a guidance set for another n than the loss call's (ST3D_E_STATE).  It needs a plan, st3d_plan_create
allocates device memory, and a plan cannot exist on a machine without a GPU; tests/test_gpu_guided.py::
test_plan_guided_nan_and_state_and_bytes holds it.  Of the plan's door only the null plan can be refused here."""
import ctypes
import re

import pytest
import torch

import _guidedref as GR

FAKE = ctypes.c_void_p(0x1000)        # a non-null "device pointer": every call below is refused before it is used


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from st3d import _lib
    return _lib.load()


@pytest.mark.parametrize("script", ["first_approach", "second_approach", "third_approach"])
def test_style_mask_flag(script):
    mod = __import__(script)
    p = mod.build_parser()
    assert p.parse_args([]).style_mask == "none"
    assert p.parse_args(["--style_mask", "object"]).style_mask == "object"
    with pytest.raises(SystemExit):
        p.parse_args(["--style_mask", "background"])
    # every target, background, the pyramid and lighting go with it
    a = p.parse_args(["--style_mask", "object", "--optimization_target", "both", "--current_background", "noise",
                      "--content_background", "style", "--texture_pyramid_levels", "0", "--lights", "point"])
    assert a.style_mask == "object" and a.optimization_target == "both"


def test_guidance_sizes_are_host_arithmetic(lib):
    for n, S in ((1, 16), (2, 24), (8, 512), (3, 90)):
        assert lib.st3d_guidance_floats(n, S) == n * sum(h * h for h in GR.sides(S))
        assert lib.st3d_guidance_partials(n, S) == 5 * n * ((S + 15) // 16) ** 2
    assert lib.st3d_guidance_floats(8, 512) <= 1.34 * 8 * 512 * 512
    assert lib.st3d_guidance_floats(0, 64) == 0 and lib.st3d_guidance_floats(2, 15) == 0 and lib.st3d_guidance_partials(-1, 64) == 0


def test_refusals_before_any_launch(lib):
    bad = lambda rc: rc == -1 and b"invalid argument" in lib.st3d_last_error()
    # st3d_guidance_build: null, n <= 0, S < 16
    assert bad(lib.st3d_guidance_build(None, 2, 64, FAKE, FAKE, FAKE, None))
    assert bad(lib.st3d_guidance_build(FAKE, 2, 64, None, FAKE, FAKE, None))
    assert bad(lib.st3d_guidance_build(FAKE, 2, 64, FAKE, None, FAKE, None))
    assert bad(lib.st3d_guidance_build(FAKE, 2, 64, FAKE, FAKE, None, None))
    assert bad(lib.st3d_guidance_build(FAKE, 0, 64, FAKE, FAKE, FAKE, None))
    assert bad(lib.st3d_guidance_build(FAKE, -3, 64, FAKE, FAKE, FAKE, None))
    assert bad(lib.st3d_guidance_build(FAKE, 2, 15, FAKE, FAKE, FAKE, None))
    # weighted Gram forward / backward
    big = ctypes.c_size_t(1 << 40)
    assert bad(lib.st3d_gram_fwd_weighted(FAKE, None, 1, 64, 256, FAKE, big, FAKE, None))
    assert bad(lib.st3d_gram_fwd_weighted(None, FAKE, 1, 64, 256, FAKE, big, FAKE, None))
    assert bad(lib.st3d_gram_fwd_weighted(FAKE, FAKE, 0, 64, 256, FAKE, big, FAKE, None))
    assert bad(lib.st3d_gram_fwd_weighted(FAKE, FAKE, 1, 64, 256, FAKE, ctypes.c_size_t(16), FAKE, None))      # workspace too small
    assert bad(lib.st3d_gram_bwd_weighted(FAKE, FAKE, None, 1, 64, 256, 1.0, 0, 0, FAKE, None))
    assert bad(lib.st3d_gram_bwd_weighted(None, FAKE, FAKE, 1, 64, 256, 1.0, 0, 0, FAKE, None))
    assert bad(lib.st3d_gram_bwd_weighted(FAKE, FAKE, FAKE, 1, 48, 256, 1.0, 0, 1, FAKE, None))              # gated needs C % 32 == 0
    assert bad(lib.st3d_gram_bwd_weighted(FAKE, FAKE, FAKE, 1, 64, 0, 1.0, 0, 0, FAKE, None))
    from st3d import ops
    items = (ops._GramItem * 1)()
    items[0].feat, items[0].gram, items[0].B, items[0].C, items[0].HW = 0x1000, 0x1000, 1, 64, 256
    assert bad(lib.st3d_gram_fwd_multi_weighted(items, None, 1, FAKE, big, None))
    qs = (ctypes.c_void_p * 1)(None)
    assert bad(lib.st3d_gram_fwd_multi_weighted(items, qs, 1, ctypes.c_void_p(0x1000 * 256), big, None))     # a null plane
    assert bad(lib.st3d_gram_fwd_multi_weighted(None, qs, 1, FAKE, big, None))
    # the weighted bottom pass
    assert bad(lib.st3d_conv1_bwd_weighted(FAKE, FAKE, FAKE, 1.0, FAKE, FAKE, big, FAKE, 1, 64, 64, None, None, None, None))
    assert bad(lib.st3d_conv1_bwd_weighted(FAKE, FAKE, FAKE, 1.0, FAKE, FAKE, big, FAKE, 1, 64, 64, FAKE, FAKE, None, None))   # seg without mask
    assert bad(lib.st3d_conv1_bwd_weighted(FAKE, FAKE, FAKE, 1.0, FAKE, FAKE, big, FAKE, 0, 64, 64, FAKE, None, None, None))
    # the plan's door
    assert bad(lib.st3d_plan_set_style_guidance(None, FAKE, 2, None))


def test_python_doors_refuse_cpu_tensors_and_wrong_shapes(lib):
    from st3d import _lib, ops
    import losses as L
    with pytest.raises(_lib.St3dError):
        ops.guidance_build(torch.ones(2, 1, 64, 64))                    # a CPU mask
    with pytest.raises(_lib.St3dError):
        ops.guidance_build(torch.ones(2, 3, 64, 64))
    with pytest.raises(_lib.St3dError):
        ops.guidance_build(torch.ones(2, 1, 8, 8))
    with pytest.raises(_lib.St3dError):
        ops.guidance_build(torch.ones(2, 1, 64, 32))
    with pytest.raises(RuntimeError):
        L.check_style_masks(torch.ones(2, 1, 64, 64), 2, 64)
    with pytest.raises(TypeError):
        L.check_style_masks([[1.0]], 2, 64)
    assert L.check_style_masks(None, 2, 64) is None
    assert ops.guidance_sides(24) == [24, 12, 6, 3, 1] == GR.sides(24)


def test_binding_table_covers_the_new_entry_points(lib):
    from st3d import _lib
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "st3d.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(st3d_[a-z0-9_]+)\s*\(", hdr)))
    assert sorted(_lib.SIGNATURES) == declared
    for name in ("st3d_guidance_floats", "st3d_guidance_partials", "st3d_guidance_build", "st3d_gram_fwd_weighted",
                 "st3d_gram_fwd_multi_weighted", "st3d_gram_bwd_weighted", "st3d_conv1_bwd_weighted", "st3d_plan_set_style_guidance"):
        assert name in declared and hasattr(lib, name)
    # the arity of each binding is the header's
    for name in declared:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        args = m.group(1).strip()
        n = 0 if args in ("", "void") else args.count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == n, name
    # st3d_gram_item is unchanged: five fields
    item = re.search(r"typedef struct st3d_gram_item \{(.*?)\} st3d_gram_item;", hdr, flags=re.S).group(1)
    assert [t.strip() for t in item.split(";") if t.strip()] == ["const float *feat", "float *gram", "int B, C, HW"]
