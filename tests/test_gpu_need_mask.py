"""The need mask of the perceptual loss (csrc/need.hip, st3d_plan_loss_masked): the render backward reads the image
gradient at covered pixels only, so the bottom of the VGG backward computes what those pixels need and nothing else.
Checked here: the device's lists against the numpy model (tests/_needref.py), the listed kernels bit for bit against the
unlisted ones, the plan (every depth, graph replay, poisoned buffers) and one second_approach step end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _needref as NR

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _blobs(n, S, seed, count=3):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, S, S), np.uint8)
    for i in range(n):
        for _ in range(count):
            h, w = rng.integers(1, S // 2, 2)
            y, x = rng.integers(0, S - h + 1), rng.integers(0, S - w + 1)
            m[i, y:y + h, x:x + w] = rng.integers(1, 256)      # any non-zero byte counts
    return m


def _masks(n, S):
    """name -> (n, S, S) uint8: empty, full, corners, one pixel, blobs at and around a tile / segment border, random blobs"""
    out = {"empty": np.zeros((n, S, S), np.uint8), "full": np.ones((n, S, S), np.uint8)}
    c = np.zeros((n, S, S), np.uint8)
    c[:, 0, 0] = c[:, 0, -1] = c[:, -1, 0] = c[:, -1, -1] = 1
    out["corners"] = c
    one = np.zeros((n, S, S), np.uint8)
    one[n - 1, S // 2, S // 2 + 1] = 255
    out["one_pixel_last_image"] = one
    # a blob that ends exactly on a tile / segment border (the dilation then reaches one pixel into the neighbour), one that
    # stops a pixel short of it (the dilation stops at the border) and one a pixel past it
    for name, end in (("ends_on_border", 64), ("ends_before_border", 63), ("ends_past_border", 65)):
        b = np.zeros((n, S, S), np.uint8)
        if S > 64:
            b[:, 5:end // 8, 10:end] = 1          # rows 5 .. 7 (8: first row of the next 4-row / 8-row tile; 7: one short)
        else:
            b[:, 5:end // 2, 10:end // 2] = 1     # S = 64: the 32-pixel border of the 8 x 32 tiles of the S/2 map (doubled: 64 is the edge)
        out[name] = b
    for seed in (0, 1):
        out[f"blobs{seed}"] = _blobs(n, S, 10 * S + seed)
    return out


# ------------------------------------------------------------------------------------------------ propagation
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("n", [1, 3])
def test_need_lists_equal_the_numpy_model(dev, n, S):
    from st3d import ops
    assert ops.need_levels(S) == 3 and ops.need_levels(96) == 0
    assert ops.wino43_tile_geometry(S, S) == NR.tile_geometry(S, S) == (4, 64)
    assert ops.wino43_tile_geometry(S // 2, S // 2) == NR.tile_geometry(S // 2, S // 2) == ((8, 32) if S == 64 else (4, 64))
    for name, m in _masks(n, S).items():
        seg_ref, lists_ref = NR.need_model(m, 3)
        for levels in (1, 2, 3):
            seg, lists = ops.need_build(torch.from_numpy(m).to(dev), levels)
            assert np.array_equal(seg.cpu().numpy(), seg_ref), (name, levels)
            assert len(lists) == levels - 1
            for lvl, (lst, cnt) in enumerate(lists):
                k = int(cnt)
                assert k == len(lists_ref[lvl]), (name, levels, lvl, k, len(lists_ref[lvl]))
                assert np.array_equal(lst.cpu().numpy()[:k], lists_ref[lvl]), (name, levels, lvl)
                assert bool((lst[k:] == -1).all()), (name, "entries past the count were written")
        if name == "empty":
            assert not seg_ref.any() and all(len(l) == 0 for l in lists_ref)
        if name == "full":
            assert seg_ref.all() and len(lists_ref[0]) == n * (S // 4) * (S // 64) and len(lists_ref[1]) == n * (S // 2) ** 2 // 256


# ------------------------------------------------------------------------------------------------ kernels
def _tile_lists(total, seed):
    rng = np.random.default_rng(seed)
    pick = np.flatnonzero(rng.random(total) < 0.4)
    return {"empty": np.zeros(0, np.int64), "single": np.array([total - 1]), "all": np.arange(total),
            "every_other": np.arange(0, total, 2), "random": pick}


@pytest.mark.parametrize("slots", ["1", "4"])
@pytest.mark.parametrize("H,W", [(16, 128), (16, 64), (16, 96)])        # 4 x 64 tiles twice, 8 x 32 tiles
def test_listed_tiles_are_bitwise_the_unlisted_launch(dev, monkeypatch, H, W, slots):
    """st3d_wino43_dgrad_chain_tiles against st3d_wino43_dgrad_chain, Cin = Cout = 64, N = 2: plain, with the output gate,
    with the gate and the content term, and un-pooling a pooled gradient (alone and gated).  Listed tiles: equal bits;
    the others keep the sentinel.  ST3D_W43_SLOTS = 1 / 4: one workgroup walks several listed tiles, ragged shares."""
    from st3d import ops
    monkeypatch.setenv("ST3D_W43_SLOTS", slots)
    N, C = 2, 64
    g = torch.Generator().manual_seed(H * W)
    w = torch.randn((C, C, 3, 3), generator=g) * 0.05
    _, ud = ops.wino43_pack(w.to(dev))
    gy = torch.randn((N, C, H, W), generator=g).to(dev)
    gyp = torch.randn((N, C, H // 2, W // 2), generator=g).to(dev)
    pidx = torch.randint(0, 4, (N, C, H // 2, W // 2), generator=g, dtype=torch.uint8).to(dev)
    gate = torch.randn((N, C, H, W), generator=g).to(dev)
    addt = torch.randn((N, C, H, W), generator=g).to(dev)
    rows, cols = NR.tile_geometry(H, W)
    total = N * (H // rows) * (W // cols)
    variants = {"plain": dict(), "gate": dict(out_gate=gate), "gate_addt": dict(out_gate=gate, add_target=addt, add_coef=0.37),
                "unpool": dict(pool_idx=pidx), "unpool_gate": dict(pool_idx=pidx, out_gate=gate)}
    for vname, kw in variants.items():
        src = gyp if "pool_idx" in kw else gy
        ref = ops.wino43_dgrad_chain(src, ud, C, **kw)
        for lname, ids in _tile_lists(total, total).items():
            lst = torch.full((total,), -1, dtype=torch.int32, device=dev)
            lst[:len(ids)] = torch.from_numpy(ids.astype(np.int32)).to(dev)
            cnt = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
            out = torch.full((N, C, H, W), SENTINEL, device=dev)
            ops.wino43_dgrad_chain_tiles(src, ud, C, lst, cnt[0], out, **kw)
            px = torch.from_numpy(NR.tile_pixels(ids, N, H, W)).to(dev)[:, None].expand(-1, C, -1, -1)
            assert torch.equal(out[px], ref[px]), (vname, lname, "listed tiles differ")
            assert bool((out[~px] == SENTINEL).all()), (vname, lname, "an unlisted tile was written")


def test_masked_relu1_1_pass_is_bitwise_on_the_mask_and_zero_off_it(dev):
    """st3d_conv1_bwd_masked against st3d_conv1_bwd on 8 x 128, N = 2.  The incoming gradient is NaN in every segment the
    mask does not need: it must not be read there."""
    from st3d import ops
    N, H, W = 2, 8, 128
    g = torch.Generator().manual_seed(5)
    gy = torch.randn((N, 64, H, W), generator=g).to(dev)
    act = torch.relu(torch.randn((N, 64, H, W), generator=g)).to(dev)
    D = torch.randn((N, 64, 64), generator=g)
    D = (D + D.transpose(1, 2)).to(dev).contiguous()
    w = torch.randn((64, 3, 3, 3), generator=g) * 0.1
    _, wd = ops.conv3x3_pack(w.to(dev))
    masks = {"blob": np.zeros((N, H, W), np.uint8), "empty": np.zeros((N, H, W), np.uint8), "full": np.ones((N, H, W), np.uint8)}
    masks["blob"][0, 2:5, 60:64] = 1          # ends on the segment border: the dilation reaches into the next segment
    masks["blob"][1, 7, 127] = 1
    for name, m in masks.items():
        seg = NR.segments(m)
        segpx = torch.from_numpy(NR.expand(seg != 0, 1, 64)).to(dev)[:, None].expand(-1, 64, -1, -1)
        gyn = torch.where(segpx, gy, torch.full_like(gy, float("nan")))
        for gy_, gyn_, D_ in ((gy, gyn, D), (gy, gyn, None), (None, None, D)):
            ref = ops.conv1_bwd(gy_, act, D_, 0.25, wd)
            got = ops.conv1_bwd_masked(gyn_, act, D_, 0.25, wd, torch.from_numpy(seg).to(dev), torch.from_numpy(m).to(dev))
            px = torch.from_numpy(m != 0).to(dev)[:, None].expand(-1, 3, -1, -1)
            assert torch.equal(got[px], ref[px]), (name, "differs on the mask")
            assert bool((got[~px] == 0).all()), (name, "not exactly 0 off the mask")


# ------------------------------------------------------------------------------------------------ plan
_NET = {}


def _plan_case(S, B, graph=False, seed=0):
    """plan.loss with and without a need mask on a fresh plan (it reads ST3D_NEED_DEPTH / ST3D_POISON_PLAN as set now):
    losses bitwise equal; gradient bitwise equal on the mask and exactly 0 off it -- or, where nothing is masked (depth 0),
    the full gradient.  With graph replay: three calls (plain, captured, replayed), the last with ANOTHER mask, so the
    staged mask and the lists inside the graph are the call's own."""
    from st3d import vgg as V
    dev = torch.device("cuda:0")
    net = _NET.get("net") or _NET.setdefault("net", V.get_vgg(device=dev, seed=0))
    g = torch.Generator().manual_seed(seed + S)
    content, style, cur = (torch.rand((B, 3, S, S), generator=g).to(dev) for _ in range(3))
    depth = int(os.environ.get("ST3D_NEED_DEPTH", "3"))
    plan = V.PerceptualPlan(net, B, S)
    try:
        plan.set_content(content)
        plan.set_style(style, B)
        masks = [_blobs(B, S, 7 + seed), _blobs(B, S, 8 + seed, count=1), _blobs(B, S, 9 + seed)]
        loss0, grad0 = plan.loss(cur, 1e6, 1.0)
        loss0, grad0 = loss0.clone(), grad0.clone()
        assert bool(torch.isfinite(grad0).all()) and float(grad0.abs().max()) > 0
        plan.use_graph(graph)
        for m in (masks if graph else masks[:1]):
            md = torch.from_numpy(m).to(dev)
            loss1, grad1 = plan.loss(cur, 1e6, 1.0, need_mask=md)
            assert torch.equal(loss1, loss0), (S, B, depth, graph)
            px = (md != 0)[:, None].expand(-1, 3, -1, -1)
            if depth == 0:
                assert torch.equal(grad1, grad0)
            else:
                assert torch.equal(grad1[px], grad0[px]), (S, B, depth, graph, "differs on the mask")
                assert bool((grad1[~px] == 0).all()), (S, B, depth, graph, "not exactly 0 off the mask")
        plan.use_graph(False)
        # the ordinary call after masked ones: nothing of the masked path lingers
        loss2, grad2 = plan.loss(cur, 1e6, 1.0)
        assert torch.equal(loss2, loss0) and torch.equal(grad2, grad0)
    finally:
        plan.close()


@pytest.mark.parametrize("S,B", [(64, 2), (128, 1)])
@pytest.mark.parametrize("depth", ["0", "1", "2", "3", None])
def test_plan_loss_with_a_need_mask(monkeypatch, dev, S, B, depth):
    if depth is None:
        monkeypatch.delenv("ST3D_NEED_DEPTH", raising=False)
    else:
        monkeypatch.setenv("ST3D_NEED_DEPTH", depth)
    _plan_case(S, B)


@pytest.mark.parametrize("S,B", [(64, 2), (128, 1)])
def test_plan_loss_with_a_need_mask_under_graph_replay(monkeypatch, dev, S, B):
    monkeypatch.delenv("ST3D_NEED_DEPTH", raising=False)
    _plan_case(S, B, graph=True)


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import test_gpu_need_mask as T
for S, B in ((64, 2), (128, 1)):
    T._plan_case(S, B)
    T._plan_case(S, B, graph=True)
print("child ok")
"""


def test_plan_loss_with_a_need_mask_on_poisoned_buffers():
    """ST3D_POISON_PLAN=1 (read once per process: a fresh child): every plan buffer starts as NaN / -1, the regions the
    masked launches skip stay that way, and none of it may reach a needed pixel"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    env["ST3D_POISON_PLAN"] = "1"
    env.pop("ST3D_NEED_DEPTH", None)
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


# ------------------------------------------------------------------------------------------------ end to end
def _ulp32(x):
    x = np.abs(x.astype(np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


@pytest.mark.parametrize("target", ["texture", "both"])
def test_second_approach_step_with_and_without_the_need_mask(monkeypatch, dev, target):
    """One second_approach step, cow, S = 128, 2 views: ST3D_NEED_MASK=0 against the default.  Loss: same bits.  Texture
    and vertex gradients: within  ulp32(|unmasked|) + 2 n S^2 2^-60 sum|grad_rgb|  per element -- the deterministic
    scatter's fixed-point scale is bounded by sum|grad_rgb|, which no longer holds the background's share.  A tensor
    with retain_grad() and a render multiplied by 1.0 take the full path: the image gradient is the unmasked one."""
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
    out = U.setup_optimizations(target, mesh0, 0.01)
    sty = SC.style_at(1, S).to(dev).expand(B, -1, -1, -1)
    weights = {"main_loss_weight": 3.0, "mesh_verts_weight": 1.0, "mesh_edge_loss_weight": 1.0,
               "mesh_laplacian_smoothing_weight": 1.0, "mesh_normal_consistency_weight": 1.0}
    verts0 = torch.from_numpy(cow["verts"]).to(dev)
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, mesh0, cams)
        out["texture_map"].add_(0.05 * torch.randn(out["texture_map"].shape, generator=torch.Generator().manual_seed(3)).to(dev))
    leaves = [out[k] for k in ("texture_map", "verts") if out[k].requires_grad]

    def step(how):
        for t in leaves:
            t.grad = None
        mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
        cur, cov = U.render_meshes(renderer, mesh, cams)
        assert RD.need_of(cur) is not None and torch.equal(RD.need_of(cur), (cov[:, 0] > 0).to(torch.uint8))
        watched = None
        if how == "retain":
            cur.retain_grad()
            watched = cur
        elif how == "derived":
            watched = cur
            watched.register_hook(lambda g: kept.__setitem__("g", g.clone()))
            cur = cur * 1.0
        assert (RD.need_of(cur) is None) == (how in ("retain", "derived"))
        loss = L.compute_second_approach_loss(cur, content, sty, net, 1e6, 1.0, out["verts"], verts0, mesh, weights, target)
        loss.backward()
        gimg = watched.grad if how == "retain" else kept.get("g")
        return float(loss.detach()), [t.grad.clone() for t in leaves], gimg, cov

    kept = {}
    monkeypatch.setenv("ST3D_NEED_MASK", "0")
    loss_full, grads_full, _, _ = step("plain")
    _, _, gimg_full, cov = step("retain")
    monkeypatch.delenv("ST3D_NEED_MASK")
    loss_need, grads_need, _, _ = step("plain")
    _, grads_retain, gimg_retain, _ = step("retain")
    _, grads_derived, gimg_derived, _ = step("derived")
    assert loss_need == loss_full
    assert float(gimg_full.abs().sum()) > 0 and float(gimg_full[(cov == 0).expand(-1, 3, -1, -1)].abs().max()) > 0
    assert torch.equal(gimg_retain, gimg_full) and torch.equal(gimg_derived, gimg_full)       # the full path, background included
    sum_abs = float(gimg_full.double().abs().sum())
    for a, b, c, d in zip(grads_need, grads_full, grads_retain, grads_derived):
        assert torch.equal(c, b) and torch.equal(d, b)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        bound = _ulp32(b) + 2.0 * B * S * S * 2.0 ** -60 * sum_abs
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        print(f"\n{target}: {a.shape} largest |masked - unmasked| {diff.max():.3e} (bound there {bound.reshape(-1)[diff.argmax()]:.3e}), "
              f"{(diff > 0).mean():.2%} of the elements differ")
        assert bool((diff <= bound).all()), (target, float((diff - bound).max()))
