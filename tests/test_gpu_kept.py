"""Kept lists: in a keyed call that finds the clean record its own, conv3_1, conv3_2 and conv3_3 recompute only the strips the
coverage can change (csrc/need.hip st3d_kept_build, csrc/wino43.hip st3d_wino43_fwd_strips, csrc/plan.hip forward()).  The
device's lists against the numpy restatement (tests/_keptref.py); the strip forward with bias and ReLU bit for bit against the
unlisted launch; a keyed plan against an unkeyed one along a call sequence, plain and on poisoned buffers; which launches run
under which family; and that an unlisted tile is in fact not written.  In the same calls conv1_2, conv2_1 and conv2_2 walk
their kept lists instead of their flat-field lists (ST3D_KEEP_SHALLOW).  ST3D_KEEP_FORCE=1: at S = 128 the two-rounds rule
would keep the path off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _keptref as KR
import _needstrips_ref as NS
import test_gpu_epochs as TE
import test_gpu_need_strips as TS

pytestmark = pytest.mark.gpu

S, B = TE.S, TE.B
A, EB = TE.A, TE.EB
WHITE, TEAL = TE.WHITE, TE.TEAL
KEPT_MODULES = (10, 12, 14)         # conv3_1, conv3_2, conv3_3
SENTINEL = -777.0
_SWITCHES = ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK", "ST3D_NEED_FORCE", "ST3D_KEEP_DEPTH",
             "ST3D_KEEP_TILE", "ST3D_KEEP_FORCE", "ST3D_KEEP_SHALLOW", "ST3D_FLAT_CONV1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _env(monkeypatch, **kw):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ 1. the builder
@pytest.mark.parametrize("first,cols", [(3, [16] * 6), (0, [16] * 6), (0, [0, 32, 0, 32, 16, 0]), (3, [0, 0, 0, 16, 32, 16])])
def test_device_lists_equal_the_restatement(dev, first, cols):
    """S = 128, N = 3: empty, full, corners, blob, an empty image between covered ones, strip counts 1, 2, 3 mod 4.  Entries,
    voids and counts exactly the model's, nothing written past a list's end, no list or count below `first` touched."""
    from st3d import ops
    N = 3
    covers = KR.covers(N, S)
    assert {"empty", "full", "corners", "blob", "empty_image_between", "mod1", "mod2", "mod3"} <= set(covers)
    for name, c in covers.items():
        ref = KR.kept_model(c, tile_cols=cols)
        got = ops.kept_build(torch.from_numpy(c).to(dev), first=first, tile_cols=cols)
        assert sorted(got) == list(range(first, 6))
        for k, (lst, cnt) in got.items():
            n = int(cnt)
            assert n == ref["counts"][k], (name, k, n, ref["counts"][k])
            e = lst.cpu().numpy()
            used = 4 * n if cols[k] == 16 else n
            assert np.array_equal(e[:used], ref["lists"][k]), (name, k)
            assert (e[used:] == -1).all(), (name, k, "entries past the end were written")
        if name.startswith("mod"):
            assert int(NS.strips_of(ref["K"][3][:1]).sum()) % 4 == int(name[3])


# ------------------------------------------------------------------------------------------------ 2. the strip forward
@pytest.mark.parametrize("slots", ["1", "4"])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 128)])
def test_forward_strips_with_bias_and_relu_are_bitwise_the_unlisted_launch(dev, monkeypatch, Cin, Cout, slots):
    """32 x 32 maps, N = 2, the hand-made strip lists of tests/test_gpu_need_strips.py: every block of a listed strip has the
    bits of st3d_wino43_fwd, the sentinel survives everywhere else, and NaN written into the input outside the listed strips'
    clipped patches changes nothing.  With and without bias and ReLU."""
    from st3d import ops
    monkeypatch.setenv("ST3D_W43_SLOTS", slots)
    N, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(2000 + Cin)
    uf, _ = ops.wino43_pack((torch.randn((Cout, Cin, 3, 3), generator=g) * 0.05).to(dev))
    bias = (torch.randn((Cout,), generator=g) * 0.3).to(dev)
    x = torch.randn((N, Cin, H, W), generator=g).to(dev)
    for vname, b, relu in (("bias_relu", bias, True), ("bias", bias, False), ("relu", None, True), ("plain", None, False)):
        ref = ops.wino43_fwd(x, uf, b, Cout, relu=relu)
        if relu:
            assert bool((ref == 0).any()) and bool((ref > 0).any())
        for lname, steps in TS._hand_lists(N, H, W).items():
            ent = np.asarray(steps, np.int32).reshape(-1)
            lst = torch.full((N * (H // 4) * (W // 16) + 8,), -1, dtype=torch.int32, device=dev)
            lst[:len(ent)] = torch.from_numpy(ent).to(dev)
            cnt = torch.tensor([len(steps)], dtype=torch.int32, device=dev)
            px = torch.from_numpy(NS.strip_pixels(ent, N, H, W)).to(dev)[:, None].expand(-1, Cout, -1, -1)
            inside = torch.from_numpy(TS._patch_mask(ent, N, H, W, False)).to(dev)[:, None].expand(-1, Cin, -1, -1)
            x_nan = torch.where(inside, x, torch.full_like(x, float("nan")))
            for tag, x_ in (("clean", x), ("nan_outside", x_nan)):
                out = torch.full((N, Cout, H, W), SENTINEL, device=dev)
                ops.wino43_fwd_strips(x_, uf, b, Cout, lst, cnt[0], out, relu=relu)
                assert torch.equal(out[px].view(torch.int32), ref[px].view(torch.int32)), (vname, lname, tag, "listed strips differ")
                assert bool((out[~px] == SENTINEL).all()), (vname, lname, tag, "something outside the listed strips was written")


def test_strips_have_no_fused_pool(dev):
    from st3d import _lib, ops
    uf, _ = ops.wino43_pack((torch.randn((64, 64, 3, 3)) * 0.05).to(dev))
    x = torch.randn((1, 64, 8, 32)).to(dev)
    lst = torch.full((16,), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    yp = torch.zeros((1, 64, 4, 16), device=dev)
    idx = torch.zeros((1, 64, 4, 16), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.St3dError):
        ops.wino43_fwd_tiles(x, uf, None, 64, lst, cnt[0], y=torch.zeros_like(x), yp=yp, idx=idx, relu=False, tile_cols=16)
    with pytest.raises(_lib.St3dError):
        ops.wino43_fwd_tiles(x, uf, None, 64, lst, cnt[0], yp=yp, idx=idx, relu=False, tile_cols=16)
    with pytest.raises(_lib.St3dError):                   # a step is read as one 16-byte vector
        ops.wino43_fwd_strips(x, uf, None, 64, lst[1:], cnt[0], torch.zeros_like(x))
    out = torch.full_like(x, SENTINEL)
    ops.wino43_fwd_strips(x, uf, torch.zeros((64,), device=dev), 64, lst, cnt[0], out)      # an empty list writes nothing
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 3. the plan, bit for bit
def _sequence(dev):
    """a keyed plan against an unkeyed one: every activation of TE.ACTS, the three losses and the gradient, call by call"""
    from st3d import _lib
    ca, cb = TE._cover("A"), TE._cover("B")
    x1, x2, y1 = TE._image(ca, WHITE, 1), TE._image(ca, WHITE, 2), TE._image(cb, WHITE, 3)
    pair = TE._Pair(dev)
    try:
        pair.step("A first", x1, ca, WHITE, A)
        pair.step("A, other texels", x2, ca, WHITE, A)                  # the kept lists are built here
        pair.step("A, a third time", x1, ca, WHITE, A)
        pair.step("A, a fourth", TE._image(ca, WHITE, 8), ca, WHITE, A)
        pair.step("B", y1, cb, WHITE, EB)
        pair.step("B again", TE._image(cb, WHITE, 4), cb, WHITE, EB)
        pair.step("A again", x1, ca, WHITE, A)
        pair.step("A twice", x2, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):
            p.set_content(pair.content2, force=True)
        pair.step("A after set_content", x2, ca, WHITE, A)
        pair.step("A", x1, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):
            p.set_style(pair.style, B, force=True)
        pair.step("A after set_style", x1, ca, WHITE, A)
        pair.step("A", x2, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):              # an unkeyed call on OTHER images and another coverage in between
            p.loss(TE._dev(y1, dev), 1e6, 1.0, need_mask=TE._dev(cb.astype(np.uint8), dev), flat_color=WHITE)
        pair.step("A after an unkeyed call", x1, ca, WHITE, A)
        pair.step("A", x2, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):              # a full forward of noise through conv3_3's buffer
            p.forward(torch.rand((B, 3, S, S), device=dev), upto=14)
        pair.step("A after plan.forward", x2, ca, WHITE, A)
        pair.step("A", x1, ca, WHITE, A)
        raw = torch.zeros((B * S * S + 16,), dtype=torch.uint8, device=dev)     # a failed call: refused before any launch
        off = raw[1:1 + B * S * S].view(B, S, S)
        with pytest.raises(_lib.St3dError):
            pair.keyed.loss(TE._dev(x1, dev), 1e6, 1.0, batch_denom=B, need_mask=off, flat_color=WHITE, epoch=A)
        pair.step("A after a failed call", x2, ca, WHITE, A)
        pair.step("A", x1, ca, WHITE, A)
        pair.step("A, two images", x1, ca, WHITE, A, n=2)
        pair.step("A, two images again", x2, ca, WHITE, A, n=2)
        pair.step("A, three again", x1, ca, WHITE, A)
        pair.step("A in another colour", TE._image(ca, TEAL, 5), ca, TEAL, A)
        pair.step("A in that colour again", TE._image(ca, TEAL, 6), ca, TEAL, A)
        pair.step("A back in white", x1, ca, WHITE, A)
        pair.step("A in white again", x2, ca, WHITE, A)
        for e in (21, 22, 23, 24):                      # more epochs than slots, then the first ones again
            pair.step("epoch %d" % e, y1 if e % 2 else x1, cb if e % 2 else ca, WHITE, e)
        pair.step("A after eviction", x2, ca, WHITE, A)
        pair.step("A after eviction, again", x1, ca, WHITE, A)
        pair.step("B after eviction", y1, cb, WHITE, EB)
    finally:
        pair.close()


@pytest.mark.parametrize("tile,shallow", [("16", None), ("32,16,0", "64,32,64"), ("16", "0,0,0"), ("16", "0,16,0")])
def test_keyed_calls_with_kept_lists_give_the_bits_of_unkeyed_calls(monkeypatch, dev, tile, shallow):
    """conv3_1 .. conv3_3 on strips or tiles; conv1_2, conv2_1, conv2_2 in their default geometries (8 x 32, strips, 8 x 32), in
    others, on their flat-field lists, and conv2_1 alone"""
    _env(monkeypatch, ST3D_KEEP_FORCE="1", ST3D_KEEP_TILE=tile, **({} if shallow is None else {"ST3D_KEEP_SHALLOW": shallow}))
    _sequence(dev)


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import torch
import test_gpu_kept as T
T._sequence(torch.device("cuda:0"))
print("child ok")
"""


def test_the_sequence_on_poisoned_buffers():
    """ST3D_POISON_PLAN=1 in a fresh child: every plan buffer starts as NaN / -1, so whatever a kept launch leaves out has to
    have been written by the full launch of the epoch's first call"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    for k in _SWITCHES:
        env.pop(k, None)
    env.update(ST3D_POISON_PLAN="1", ST3D_KEEP_FORCE="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


# ------------------------------------------------------------------------------------------------ 4. which launches run how
def _plan(dev):
    from st3d import vgg as V
    plan = V.PerceptualPlan(TE._net(), B, S)
    g = torch.Generator().manual_seed(5)
    content = torch.rand((B, 3, S, S), generator=g).to(dev)
    style = torch.rand((1, 3, S, S), generator=g).to(dev).expand(B, -1, -1, -1)
    plan.set_content(content, force=True)
    plan.set_style(style, B, force=True)
    return plan, content, style


def _kept_families(plan):
    """(families of modules 10, 12, 14 in launch order, number of `elementwise` brackets)"""
    torch.cuda.synchronize()
    ls = plan.profile_launches()
    fams = tuple(f for f, m, _ in ls if m in KEPT_MODULES and f.startswith("conv43_fwd"))
    assert [m for f, m, _ in ls if m in KEPT_MODULES and f.startswith("conv43_fwd")] == list(KEPT_MODULES)
    return fams, [f for f, _, _ in ls].count("elementwise")


def test_kept_launches_run_only_in_clean_calls_and_the_build_once_per_epoch(monkeypatch, dev):
    from st3d import vgg as V
    from st3d import _lib
    _env(monkeypatch, ST3D_KEEP_FORCE="1")
    ca, cb = TE._cover("A"), TE._cover("B")
    xa, xb, xt = (TE._dev(TE._image(c, col, 9), dev) for c, col in ((ca, WHITE), (cb, WHITE), (ca, TEAL)))
    ma, mb = TE._dev(ca.astype(np.uint8), dev), TE._dev(cb.astype(np.uint8), dev)
    net = TE._net()
    plan, content, style = _plan(dev)
    FULL, KEPT = ("conv43_fwd",) * 3, ("conv43_fwd_flat",) * 3
    try:
        plan.profile(True)
        plan.profile_launches()

        def call(x, m, col, epoch, n=B):
            plan.loss(x[:n], 1e6, 1.0, batch_denom=B, need_mask=m[:n], flat_color=col, epoch=epoch)
            return _kept_families(plan)

        fams, elem0 = call(xa, ma, WHITE, 0)            # unkeyed: builds the need lists and the flat lists
        assert fams == FULL
        first, clean = (FULL, elem0), (KEPT, elem0 - 2)
        assert call(xa, ma, WHITE, A) == first          # an epoch's first call: in full, and no kept build
        assert call(xa, ma, WHITE, A) == (KEPT, elem0 - 1)      # the first clean call builds the kept lists
        assert call(xa, ma, WHITE, A) == clean
        assert call(xb, mb, WHITE, EB) == first
        assert call(xb, mb, WHITE, EB) == (KEPT, elem0 - 1)
        assert call(xa, ma, WHITE, A) == (FULL, elem0 - 2)      # back: every list is still there, the buffers hold B
        assert call(xa, ma, WHITE, A) == clean
        for writer in (lambda: plan.set_content(content, force=True), lambda: plan.set_style(style, B, force=True),
                       lambda: plan.forward(xb, upto=14), lambda: plan.loss(xa, 1e6, 1.0),
                       lambda: plan.loss(xb, 1e6, 1.0, need_mask=mb, flat_color=WHITE),
                       lambda: net.load_state_dict(V.synthetic_state(0))):
            writer()
            torch.cuda.synchronize()
            plan.profile_launches()
            assert call(xa, ma, WHITE, A) == (FULL, elem0 - 2)
            assert call(xa, ma, WHITE, A) == clean
        assert call(xt, ma, TEAL, A) == (FULL, elem0 - 2)       # another colour
        assert call(xt, ma, TEAL, A) == clean
        assert call(xa, ma, WHITE, A, n=2) == first             # another n: other lists
        assert call(xa, ma, WHITE, A, n=2) == (KEPT, elem0 - 1)
        assert call(xa, ma, WHITE, A) == (FULL, elem0 - 2)
        raw = torch.zeros((B * S * S + 16,), dtype=torch.uint8, device=dev)
        off = raw[1:1 + B * S * S].view(B, S, S)
        with pytest.raises(_lib.St3dError):
            plan.loss(xa, 1e6, 1.0, batch_denom=B, need_mask=off, flat_color=WHITE, epoch=A)
        plan.profile_launches()
        assert call(xa, ma, WHITE, A) == (FULL, elem0 - 2)
        assert call(xa, ma, WHITE, A) == clean
        monkeypatch.setenv("ST3D_FLAT", "0")            # read by every call: the full forward
        assert call(xa, ma, WHITE, A)[0] == FULL
        monkeypatch.delenv("ST3D_FLAT")
        assert call(xa, ma, WHITE, A) == (FULL, elem0 - 2)
        plan.profile(False)
    finally:
        plan.close()


@pytest.mark.parametrize("env", [dict(), dict(ST3D_NEED_FORCE="1"), dict(ST3D_KEEP_FORCE="1", ST3D_KEEP_DEPTH="0"),
                                 dict(ST3D_KEEP_FORCE="1", ST3D_FLAT_DEPTH="2")])
def test_the_path_stays_off(monkeypatch, dev, env):
    """at this size the two-rounds rule keeps it off, ST3D_NEED_FORCE does not engage it, ST3D_KEEP_DEPTH=0 is the parent's
    behaviour, and it needs every flat-field level below it"""
    _env(monkeypatch, **env)
    ca = TE._cover("A")
    xa, ma = TE._dev(TE._image(ca, WHITE, 9), dev), TE._dev(ca.astype(np.uint8), dev)
    plan, _, _ = _plan(dev)
    try:
        plan.profile(True)
        plan.profile_launches()
        for _ in range(3):
            plan.loss(xa, 1e6, 1.0, batch_denom=B, need_mask=ma, flat_color=WHITE, epoch=A)
            assert _kept_families(plan)[0] == ("conv43_fwd",) * 3
    finally:
        plan.close()


def test_keep_depth_lists_bottom_up(monkeypatch, dev):
    _env(monkeypatch, ST3D_KEEP_FORCE="1", ST3D_KEEP_DEPTH="2")
    ca = TE._cover("A")
    xa, ma = TE._dev(TE._image(ca, WHITE, 9), dev), TE._dev(ca.astype(np.uint8), dev)
    plan, _, _ = _plan(dev)
    try:
        plan.profile(True)
        plan.profile_launches()
        got = []
        for _ in range(2):
            plan.loss(xa, 1e6, 1.0, batch_denom=B, need_mask=ma, flat_color=WHITE, epoch=A)
            got.append(_kept_families(plan)[0])
        assert got == [("conv43_fwd",) * 3, ("conv43_fwd_flat", "conv43_fwd_flat", "conv43_fwd")]
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ 5. kept means kept
@pytest.mark.parametrize("module,lst", [(12, 4), (5, 1)])
def test_an_unlisted_strip_is_not_written(monkeypatch, dev, module, lst):
    """between two clean calls: a sentinel put into act[12] (conv3_2; and act[5], conv2_1, which walks strips too) outside the
    listed strips survives the call, and the listed strips come out as the full launch's bits; the saved contents are put
    back afterwards"""
    _env(monkeypatch, ST3D_KEEP_FORCE="1")
    from st3d import vgg as V
    ca = TE._cover("A")
    assert not ca[1].any()                              # an empty view: none of its strips is listed
    x1, x2 = TE._image(ca, WHITE, 1), TE._image(ca, WHITE, 2)
    pair = TE._Pair(dev)
    try:
        pair.step("first", x1, ca, WHITE, A)
        pair.step("clean", x2, ca, WHITE, A)
        K = KR.kept_maps(ca.astype(np.uint8))[lst]      # the launch's may-change blocks, (B, R, R)
        listed = torch.from_numpy(NS.strip_pixels(NS.strip_list(K)[0], B, K.shape[1], K.shape[2])).to(dev)
        assert bool(listed.any()) and not bool(listed.all()) and not bool(listed[1].any())
        act = pair.keyed.activation(module, B)
        saved = act.clone()
        px = listed[:, None].expand_as(act)
        act[~px] = SENTINEL
        cur, mask = TE._dev(x1, dev), TE._dev(ca.astype(np.uint8), dev)
        pair.keyed.loss(cur, 1e6, 1.0, batch_denom=B, need_mask=mask, flat_color=WHITE, epoch=A)
        pair.plain.loss(cur, 1e6, 1.0, batch_denom=B, need_mask=mask, flat_color=WHITE)
        torch.cuda.synchronize()
        act = pair.keyed.activation(module, B)
        full = pair.plain.activation(module, B)
        assert bool((act[~px] == SENTINEL).all()), "the kept launch wrote an unlisted strip"
        assert TE._same(act[px], full[px])
        assert TE._same(saved[~px], full[~px]), "what the unlisted strips held was not the full launch's bits"
        act[~px] = saved[~px]                           # restored: the next calls are clean again and right
        pair.step("after the restore", x2, ca, WHITE, A)
    finally:
        pair.close()
