"""Flat-field forward (csrc/flat.hip, st3d_wino43_fwd_tiles, st3d_plan_loss_flat): a render holds its background colour
bit for bit at most pixels, so the forward launches of conv1_2, conv2_1 and conv2_2 compute the tiles that see anything else
plus one representative per border class, and the rest are copied.  Checked here: the device's lists and maps against the
numpy model (tests/_flatref.py), the listed forward kernels bit for bit against the unlisted ones, the fill, the two facts
the scheme rests on (a flat tile's output does not depend on where it lies; a tile reads nothing outside its patch), the
plan (every depth, need mask, graph replay, poisoned buffers, NaNs, another colour) and one second_approach step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _flatref as FR
import _needref as NR

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
WHITE = (1.0, 1.0, 1.0)
TEAL = (0.125, 0.5, 0.625)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """equal as bits (NaNs included)"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ lists
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("n", [1, 3])
def test_flat_lists_equal_the_numpy_model(dev, n, S):
    from st3d import ops
    assert ops.flat_levels(S) == 3 and ops.flat_levels(96) == 0
    rows, cols = NR.tile_geometry(S, S)
    cases = [(what, FR.images(n, S, col, what), col) for what in ("empty", "full", "one_pixel", "one_channel", "corners", "nan",
                                                                  "blobs", "first_view_only") for col in (WHITE, TEAL)]
    rows2, cols2 = NR.tile_geometry(S // 2, S // 2)
    for end in (-1, 0, 1):       # ending one short of, on and one past a tile border, both axes, both grids
        cases.append((f"rect_y{end}", FR.rect_image(n, S, WHITE, 5, 3 * rows - 3 + end, 20, 25, view=n - 1), WHITE))
        cases.append((f"rect_x{end}", FR.rect_image(n, S, WHITE, 9, 12, 3, cols - 3 + end), WHITE))
        cases.append((f"rect_y2{end}", FR.rect_image(n, S, WHITE, 5, 2 * (2 * rows2 - 2 + end) - 1, 20, 25), WHITE))
        cases.append((f"rect_x2{end}", FR.rect_image(n, S, WHITE, 9, 12, 3, 2 * (cols2 - 3 + end) - 1), WHITE))
    for name, img, col in cases:
        ref = FR.flat_model(img, col)
        got = ops.flat_build(torch.from_numpy(img).to(dev), torch.tensor(col, dtype=torch.float32, device=dev))
        assert len(got) == 3
        for launch, (lst, cnt, mp) in enumerate(got):
            k = int(cnt)
            assert k == len(ref[launch][0]), (name, launch, k, len(ref[launch][0]))
            assert np.array_equal(lst.cpu().numpy()[:k], ref[launch][0]), (name, launch)
            assert bool((lst[k:] == -7).all()), (name, launch, "entries past the count were written")
            assert np.array_equal(mp.cpu().numpy(), ref[launch][1]), (name, launch)
    # fewer levels: the same lists for the launches asked for
    img, col = cases[6][1], cases[6][2]
    for levels in (1, 2):
        got = ops.flat_build(torch.from_numpy(img).to(dev), torch.tensor(col, dtype=torch.float32, device=dev), levels)
        ref = FR.flat_model(img, col)
        assert len(got) == levels
        for launch, (lst, cnt, mp) in enumerate(got):
            assert np.array_equal(lst.cpu().numpy()[:int(cnt)], ref[launch][0]) and np.array_equal(mp.cpu().numpy(), ref[launch][1])


# ------------------------------------------------------------------------------------------------ kernels
def _tile_lists(total, seed):
    rng = np.random.default_rng(seed)
    pick = np.flatnonzero(rng.random(total) < 0.4)
    return {"empty": np.zeros(0, np.int64), "single": np.array([total - 1]), "all": np.arange(total),
            "every_other": np.arange(0, total, 2), "random": pick}


@pytest.mark.parametrize("slots", ["1", "4"])
@pytest.mark.parametrize("H,W", [(16, 128), (16, 64), (16, 96)])        # 4 x 64 tiles twice, 8 x 32 tiles
def test_listed_forward_tiles_are_bitwise_the_unlisted_launch(dev, monkeypatch, H, W, slots):
    """st3d_wino43_fwd_tiles against st3d_wino43_fwd, Cin = Cout = 64, N = 2, bias + ReLU: plain, and with the fused pool
    (full output + pooled + argmax, and pooled + argmax alone as the plan runs it).  Listed tiles: equal bits; the others
    keep the sentinel.  Then the same lists on an input that is NaN outside the listed tiles' patches (tile +- 1): a tile
    reads nothing else, so the listed tiles still come out as the clean input's."""
    from st3d import ops
    monkeypatch.setenv("ST3D_W43_SLOTS", slots)
    N, C = 2, 64
    g = torch.Generator().manual_seed(H * W + 1)
    w = torch.randn((C, C, 3, 3), generator=g) * 0.05
    uf, _ = ops.wino43_pack(w.to(dev))
    bias = (torch.randn((C,), generator=g) * 0.1).to(dev)
    x = torch.randn((N, C, H, W), generator=g).to(dev)
    ref = ops.wino43_fwd(x, uf, bias, C)
    ref_full, ref_p, ref_i = ops.wino43_fwd(x, uf, bias, C, pool=True, keep_full=True)
    assert _same(ref_full, ref)
    rows, cols = NR.tile_geometry(H, W)
    total = N * (H // rows) * (W // cols)
    for lname, ids in _tile_lists(total, total).items():
        lst = torch.full((total,), -1, dtype=torch.int32, device=dev)
        lst[:len(ids)] = torch.from_numpy(ids.astype(np.int32)).to(dev)
        cnt = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
        px_np = NR.tile_pixels(ids, N, H, W)
        px = torch.from_numpy(px_np).to(dev)[:, None].expand(-1, C, -1, -1)
        pp = px[:, :, ::2, ::2]
        patch = torch.from_numpy(NR.dilate(px_np)).to(dev)[:, None].expand(-1, C, -1, -1)
        x_nan = torch.where(patch, x, torch.full_like(x, float("nan")))
        for xin, xname in ((x, "clean"), (x_nan, "nan outside the patches")):
            y = torch.full((N, C, H, W), SENTINEL, device=dev)
            ops.wino43_fwd_tiles(xin, uf, bias, C, lst, cnt[0], y=y)
            assert torch.equal(y[px], ref[px]), (lname, xname, "plain: listed tiles differ")
            assert bool((y[~px] == SENTINEL).all()), (lname, xname, "plain: an unlisted tile was written")
            for keep_full in (True, False):
                y = torch.full((N, C, H, W), SENTINEL, device=dev) if keep_full else None
                yp = torch.full((N, C, H // 2, W // 2), SENTINEL, device=dev)
                yi = torch.full((N, C, H // 2, W // 2), 0xAB, dtype=torch.uint8, device=dev)
                ops.wino43_fwd_tiles(xin, uf, bias, C, lst, cnt[0], y=y, yp=yp, idx=yi)
                if keep_full:
                    assert torch.equal(y[px], ref[px]) and bool((y[~px] == SENTINEL).all()), (lname, xname, "pooled: full output")
                assert torch.equal(yp[pp], ref_p[pp]) and torch.equal(yi[pp], ref_i[pp]), (lname, xname, keep_full, "pooled tiles differ")
                assert bool((yp[~pp] == SENTINEL).all()) and bool((yi[~pp] == 0xAB).all()), (lname, xname, keep_full, "unlisted written")


@pytest.mark.parametrize("H,W,C", [(16, 128, 64), (16, 96, 128), (8, 64, 16)])
def test_fill_copies_the_representative_and_nothing_else(dev, H, W, C):
    """st3d_flat_fill: every unlisted tile equals its representative bit for bit -- full output, pooled output, argmax --
    and listed tiles keep what they held."""
    from st3d import ops
    N = 3
    rows, cols = NR.tile_geometry(H, W)
    total = N * (H // rows) * (W // cols)
    rng = np.random.default_rng(H + W + C)
    g = torch.Generator().manual_seed(C + W)
    for frac in (0.0, 0.3, 1.0):
        listed = rng.random(total) < frac
        listed[rng.integers(0, total)] = True
        ids = np.flatnonzero(listed)
        mp = np.where(listed, -1, ids[rng.integers(0, len(ids), total)]).astype(np.int32)
        mpd = torch.from_numpy(mp).to(dev)
        rest = torch.from_numpy(np.flatnonzero(~listed)).to(dev)
        src = torch.from_numpy(mp[~listed].astype(np.int64)).to(dev)
        for which in ("all", "pooled", "full"):
            y = torch.randn((N, C, H, W), generator=g).to(dev) if which != "pooled" else None
            yp = torch.randn((N, C, H // 2, W // 2), generator=g).to(dev) if which != "full" else None
            yi = torch.randint(0, 256, (N, C, H // 2, W // 2), generator=g, dtype=torch.uint8).to(dev) if which != "full" else None
            before = [None if t is None else t.clone() for t in (y, yp, yi)]
            ops.flat_fill(mpd, y=y, yp=yp, idx=yi)
            for t, b, (r, c) in zip((y, yp, yi), before, ((rows, cols), (rows // 2, cols // 2), (rows // 2, cols // 2))):
                if t is None:
                    continue
                want = FR.tiles_view(b, r, c).clone()
                want[rest] = want[src]
                assert torch.equal(FR.tiles_view(t, r, c), want), (frac, which, r, c)


# ------------------------------------------------------------------------------------------------ the premise
_NET = {}


def _net():
    from st3d import vgg as V
    return _NET.get("net") or _NET.setdefault("net", V.get_vgg(device=torch.device("cuda:0"), seed=0))


@pytest.mark.parametrize("color", [WHITE, TEAL])
def test_flat_tiles_of_one_class_are_bitwise_equal_in_the_full_forward(dev, color):
    """No new code involved: the full forward (st3d_plan_forward) of an image that is the flat colour except for one blob.
    conv_small_fwd_kernel runs one fixed fma chain per pixel and wino43_kernel one fixed operation order per in-tile
    position, so the outputs of conv1_1, conv1_2 (+ pool1), conv2_1 and conv2_2 (+ pool2) are bitwise equal between any
    two non-varying tiles of one border class.  "Non-varying" as tests/_flatref.py has it: behind a Winograd conv a whole
    4x4 output block varies when its 6x6 patch does, and the first two / last two tiles along an axis are classes of their
    own.  (Measured with the per-pixel rule -- every conv dilates by one pixel -- and classes from the first / last tile
    only: conv1_1, conv1_2, pool1 and conv2_1 equal, 74980 elements of conv2_2's flat tiles differ on this blob.)"""
    from st3d import vgg as V
    S, n = 128, 2
    img = FR.rect_image(n, S, color, 40, 70, 30, 90, view=0)
    plan = V.PerceptualPlan(_net(), n, S)
    try:
        plan.forward(torch.from_numpy(img).to(dev), upto=9)
        torch.cuda.synchronize()
        v0 = FR.varying_pixels(img, color)
        vary = FR.varying_tiles(img, color)
        r1, c1 = NR.tile_geometry(S, S)
        r2, c2 = NR.tile_geometry(S // 2, S // 2)
        checks = [(0, NR.tiles_any(NR.dilate(v0), r1, c1), r1, c1), (2, vary[0], r1, c1), (4, vary[0], r1 // 2, c1 // 2),
                  (5, vary[1], r2, c2), (7, vary[2], r2, c2), (9, vary[2], r2 // 2, c2 // 2)]
        for module, v, r, c in checks:
            lst, mp = FR.list_and_map(v)
            assert 0 < len(lst) < v.size
            rest = np.flatnonzero(mp >= 0)
            t = FR.tiles_view(plan.activation(module, n), r, c)
            a, b = t[torch.from_numpy(rest).to(dev)], t[torch.from_numpy(mp[rest].astype(np.int64)).to(dev)]
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
            assert _same(a, b), (module, "flat tiles of one class differ: %d elements" % int((_bits(a) != _bits(b)).sum()))
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ plan
def _views(S, color, kind, seed=0):
    """(3,3,S,S): a view with no flat pixel, a view that is entirely flat, a view with blobs"""
    img = FR.images(3, S, color, "blobs", seed)
    img[0] = np.random.default_rng(seed + 5).random((3, S, S), dtype=np.float32)
    img[1] = np.asarray(color, np.float32)[:, None, None]
    covered = FR.varying_pixels(img, color)[2]
    if kind == "nan_covered":
        y, x = np.argwhere(covered)[len(np.argwhere(covered)) // 2]
        img[2, 1, y, x] = np.nan
    elif kind == "nan_background":
        y, x = np.argwhere(~covered)[len(np.argwhere(~covered)) // 3]
        img[2, 0, y, x] = np.nan
    return img


_ACTS = (0, 4, 5, 9, 10, 19, 21, 28)        # what the loss call writes of the shallow layers, and the taps above


def _plan_case(color=WHITE, kind="mixed", need=False, graph=False, S=128, B=3):
    """plan.loss with and without the colour on a fresh plan (it reads ST3D_FLAT_DEPTH / ST3D_NEED_DEPTH / ST3D_POISON_PLAN
    as set now): the three losses, the gradient and the activations the call writes are the same bits.  With graph replay:
    three calls (plain, captured, replayed), the last on OTHER images, so the staged colour and the lists inside the graph
    are the call's own.  Returns the profile families of the shallow forward launches of one flat call."""
    from st3d import vgg as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(S + 3)
    content, style = (torch.rand((B, 3, S, S), generator=g).to(dev) for _ in range(2))
    curs = [torch.from_numpy(_views(S, color, kind, seed)).to(dev) for seed in ((0, 0, 1) if graph else (0,))]
    masks = [torch.from_numpy(FR.varying_pixels(c.cpu().numpy(), color).astype(np.uint8)).to(dev) if need else None for c in curs]
    plan = V.PerceptualPlan(_net(), B, S)
    try:
        plan.set_content(content)
        plan.set_style(style, B)
        refs = {}
        for i in (0, len(curs) - 1):
            loss, grad = plan.loss(curs[i], 1e6, 1.0, need_mask=masks[i])
            refs[i] = (loss.clone(), grad.clone(), [plan.activation(m, B).clone() for m in _ACTS])
        if kind == "mixed":
            assert bool(torch.isfinite(refs[0][1]).all()) and float(refs[0][1].abs().max()) > 0
        plan.use_graph(graph)
        for i, cur in enumerate(curs):
            loss, grad = plan.loss(cur, 1e6, 1.0, need_mask=masks[i], flat_color=color)
            if i in refs:
                assert _same(loss, refs[i][0]), (kind, need, graph, i, loss, refs[i][0])
                assert _same(grad, refs[i][1]), (kind, need, graph, i, "gradient differs")
                for m, a in zip(_ACTS, refs[i][2]):
                    assert _same(plan.activation(m, B), a), (kind, need, graph, i, "activation of module %d differs" % m)
        plan.use_graph(False)
        plan.profile(True)
        plan.loss(curs[0], 1e6, 1.0, need_mask=masks[0], flat_color=color)
        torch.cuda.synchronize()
        fams = sorted((f, m) for f, m, _ in plan.profile_launches() if m in (2, 5, 7) and "dgrad" not in f and "gram" not in f)
        plan.profile(False)
        # the ordinary call after flat ones: nothing of the flat path lingers
        loss, grad = plan.loss(curs[0], 1e6, 1.0, need_mask=masks[0])
        assert _same(loss, refs[0][0]) and _same(grad, refs[0][1])
        return fams
    finally:
        plan.close()


def _expected_families(depth):
    out = []
    for k, m in enumerate((2, 5, 7)):
        out += [("conv43_fwd_flat", m), ("flat_fill", m)] if k < depth else [("conv43_fwd", m)]
    return sorted(out)


@pytest.mark.parametrize("need", [False, True])
@pytest.mark.parametrize("depth", ["0", "1", "2", "3", None])
def test_plan_loss_flat_is_bitwise_the_full_forward(monkeypatch, dev, depth, need):
    monkeypatch.delenv("ST3D_FLAT", raising=False)
    if depth is None:
        monkeypatch.delenv("ST3D_FLAT_DEPTH", raising=False)
    else:
        monkeypatch.setenv("ST3D_FLAT_DEPTH", depth)
    fams = _plan_case(need=need)
    assert fams == _expected_families(3 if depth is None else int(depth)), fams


def test_plan_loss_flat_switched_off_per_call(monkeypatch, dev):
    monkeypatch.delenv("ST3D_FLAT_DEPTH", raising=False)
    monkeypatch.setenv("ST3D_FLAT", "0")
    assert _plan_case() == _expected_families(0)


@pytest.mark.parametrize("need", [False, True])
def test_plan_loss_flat_under_graph_replay(monkeypatch, dev, need):
    monkeypatch.delenv("ST3D_FLAT", raising=False)
    monkeypatch.delenv("ST3D_FLAT_DEPTH", raising=False)
    _plan_case(need=need, graph=True)


@pytest.mark.parametrize("kind", ["nan_covered", "nan_background"])
def test_plan_loss_flat_with_a_nan_pixel(monkeypatch, dev, kind):
    """A NaN texel in a covered pixel and a NaN in a background pixel: NaN differs from the colour, so its tiles are computed,
    and everything comes out as in the full path, NaNs included"""
    monkeypatch.delenv("ST3D_FLAT", raising=False)
    monkeypatch.delenv("ST3D_FLAT_DEPTH", raising=False)
    _plan_case(kind=kind)


def test_plan_loss_flat_with_another_colour_and_with_the_wrong_one(monkeypatch, dev):
    monkeypatch.delenv("ST3D_FLAT", raising=False)
    monkeypatch.delenv("ST3D_FLAT_DEPTH", raising=False)
    assert _plan_case(color=TEAL) == _expected_families(3)
    # a colour the images do not hold: every tile varies, the results are the same
    from st3d import vgg as V
    S, B = 128, 3
    cur = torch.from_numpy(_views(S, WHITE, "mixed")).to(dev)
    plan = V.PerceptualPlan(_net(), B, S)
    try:
        plan.set_content(cur * 0.5)
        plan.set_style(cur.flip(0), B)
        l0, g0 = plan.loss(cur, 1e6, 1.0)
        l0, g0 = l0.clone(), g0.clone()
        l1, g1 = plan.loss(cur, 1e6, 1.0, flat_color=TEAL)
        assert _same(l1, l0) and _same(g1, g0)
    finally:
        plan.close()


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import test_gpu_flat as T
for need in (False, True):
    T._plan_case(need=need)
    T._plan_case(need=need, graph=True)
print("child ok")
"""


def test_plan_loss_flat_on_poisoned_buffers():
    """ST3D_POISON_PLAN=1 (read once per process: a fresh child): every plan buffer starts as NaN / -1; the tiles the listed
    launches leave out are filled by the copies, so none of it may survive into a result"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    env["ST3D_POISON_PLAN"] = "1"
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


# ------------------------------------------------------------------------------------------------ end to end
def test_second_approach_step_with_and_without_the_flat_forward(monkeypatch, dev):
    """One second_approach step, cow, S = 128, 2 views: ST3D_FLAT=0 against the default.  Loss and texture gradient: the
    same bits.  The render carries the background tag and takes the listed launches; a noise composite carries none and
    takes the full ones."""
    import _scenes as SC
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import render as RD
    U.device = ST.device = L.device = dev
    S, B = 128, 2
    cow = SC.load_asset("cow")
    R, T = SC.random_cameras(B, seed=0)
    mesh0, renderer, cams = SC.device_scene(U, dev, cow["verts"], cow["faces"], cow["verts_uvs"], cow["faces_uvs"],
                                            SC.texture_at(cow, S), R, T, S)
    net = U.get_vgg(seed=0)
    out = U.setup_optimizations("texture", mesh0, 0.01)
    sty = SC.style_at(1, S).to(dev).expand(B, -1, -1, -1)
    weights = {"main_loss_weight": 3.0, "mesh_verts_weight": 1.0, "mesh_edge_loss_weight": 1.0,
               "mesh_laplacian_smoothing_weight": 1.0, "mesh_normal_consistency_weight": 1.0}
    verts0 = torch.from_numpy(cow["verts"]).to(dev)
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, mesh0, cams)
        out["texture_map"].add_(0.05 * torch.randn(out["texture_map"].shape, generator=torch.Generator().manual_seed(3)).to(dev))
    tex = out["texture_map"]
    plan = net.plan(B, S)

    def step(background):
        tex.grad = None
        mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], tex, out["verts"], out["faces"])
        cur, cov = U.render_meshes(renderer, mesh, cams)
        assert RD.flat_of(cur) == WHITE
        if background == "noise":
            torch.manual_seed(11)
            cur = U.apply_background(cur, cov, "noise")
            assert RD.flat_of(cur) is None
        plan.profile(True)
        loss = L.compute_second_approach_loss(cur, content, sty, net, 1e6, 1.0, out["verts"], verts0, mesh, weights, "texture")
        loss.backward()
        torch.cuda.synchronize()
        # (a set: the first step also runs the content and style forwards, which are full ones)
        fams = sorted({(f, m) for f, m, _ in plan.profile_launches() if m in (2, 5, 7) and "dgrad" not in f and "gram" not in f})
        plan.profile(False)
        return loss.detach().clone(), tex.grad.clone(), fams

    monkeypatch.delenv("ST3D_FLAT_DEPTH", raising=False)
    monkeypatch.setenv("ST3D_FLAT", "0")
    step("white")                                    # sets the content and style targets (full forwards)
    loss_full, grad_full, fams_full = step("white")
    monkeypatch.delenv("ST3D_FLAT")
    loss_flat, grad_flat, fams_flat = step("white")
    _, _, fams_noise = step("noise")
    assert fams_full == _expected_families(0) and fams_flat == _expected_families(3) and fams_noise == _expected_families(0)
    assert float(grad_full.abs().max()) > 0
    assert _same(loss_flat, loss_full) and _same(grad_flat, grad_full)
