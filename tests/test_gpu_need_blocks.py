"""The per-block need lists (csrc/need.hip: st3d_need_blocks_build) and what rides on them: the device's lists against
the numpy model (tests/_needblocks_ref.py), the listed F(4x4,3x3) launch on 8 x 32 tiles where 4 x 64 is the kernel's own
choice bit for bit against the unlisted launch, and the plan with every new level engaged (ST3D_NEED_FORCE=1): same loss,
same gradient on the mask, 0 off it -- plain, under graph replay, on poisoned buffers, in either geometry."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _needblocks_ref as NB
import test_gpu_need_mask as T

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ (a) lists
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("n", [1, 3])
def test_block_lists_equal_the_numpy_model(dev, n, S):
    from st3d import ops
    nl = NB.n_lists(S)
    assert ops.need_blocks_lists(S) == nl == (3 if S == 64 else 6) and ops.need_blocks_lists(96) == 0
    mixed = [32, 0, 32, 0, 32, 0]
    for name, m in T._masks(n, S).items():
        for cols in (None, [32] * nl, [64 if (S >> NB.LIST_SHIFT[k]) % 64 == 0 else 0 for k in range(nl)], mixed[:nl]):
            ref = NB.need_blocks_model(m, tile_cols=cols)
            seg, lists = ops.need_blocks_build(torch.from_numpy(m).to(dev), tile_cols=cols)
            assert np.array_equal(seg.cpu().numpy(), ref["seg"]), (name, cols)
            assert len(lists) == nl
            for k, (lst, cnt) in enumerate(lists):
                c = int(cnt)
                assert lst.numel() == n * (S >> NB.LIST_SHIFT[k]) ** 2 // 256
                assert c == len(ref["lists"][k]), (name, cols, k, c, len(ref["lists"][k]))
                assert np.array_equal(lst.cpu().numpy()[:c], ref["lists"][k]), (name, cols, k)
                assert bool((lst[c:] == -1).all()), (name, cols, k, "entries past the count were written")
        # fewer lists: the same first ones; and the runs of the relu2_1 Gram backward where the size has them
        ref = NB.need_blocks_model(m)
        if S == 128:
            _, lists, (glist, gcount) = ops.need_blocks_build(torch.from_numpy(m).to(dev), nlists=2, gram=True)
            c = int(gcount)
            assert glist.numel() == n * 64 and c == len(ref["gram"]), (name, c, len(ref["gram"]))
            assert np.array_equal(glist.cpu().numpy()[:c], ref["gram"]) and bool((glist[c:] == -1).all()), name
        else:
            assert ref["gram"] is None
            _, lists = ops.need_blocks_build(torch.from_numpy(m).to(dev), nlists=2)
        assert len(lists) == 2
        for k, (lst, cnt) in enumerate(lists):
            assert np.array_equal(lst.cpu().numpy()[:int(cnt)], ref["lists"][k]), (name, k)


# ------------------------------------------------------------------------------------------------ (b) kernel bits
def _tile_lists(total, seed):
    rng = np.random.default_rng(seed)
    return {"empty": np.zeros(0, np.int64), "all": np.arange(total), "single": np.array([total - 1]),
            "random": np.flatnonzero(rng.random(total) < 0.4), "random2": np.flatnonzero(rng.random(total) < 0.7)}


@pytest.mark.parametrize("slots", [None, "1"])
@pytest.mark.parametrize("H,W,Cred,Cprod", [(8, 64, 64, 64), (16, 128, 128, 64)])
def test_listed_8x32_tiles_are_bitwise_the_default_launch(dev, monkeypatch, H, W, Cred, Cprod, slots):
    """st3d_wino43_dgrad_chain_tiles_geo with 32-pixel tile columns on maps whose own geometry is 4 x 64, N = 2, reducing over
    Cred channels into Cprod: plain, with the output gate, gate + content term (MODE 0), and un-pooling a pooled gradient with
    and without the gate (MODE 3).  Listed tiles: the bits of the unlisted default launch; every other element as it was.
    ST3D_W43_SLOTS=1: one workgroup walks the whole list."""
    from st3d import ops
    if slots is not None:
        monkeypatch.setenv("ST3D_W43_SLOTS", slots)
    assert ops.wino43_tile_geometry(H, W) == (4, 64)
    N = 2
    g = torch.Generator().manual_seed(H * W + Cred)
    w = torch.randn((Cred, Cprod, 3, 3), generator=g) * 0.05
    _, ud = ops.wino43_pack(w.to(dev))
    gy = torch.randn((N, Cred, H, W), generator=g).to(dev)
    gyp = torch.randn((N, Cred, H // 2, W // 2), generator=g).to(dev)
    pidx = torch.randint(0, 4, (N, Cred, H // 2, W // 2), generator=g, dtype=torch.uint8).to(dev)
    gate = torch.randn((N, Cprod, H, W), generator=g).to(dev)
    addt = torch.randn((N, Cprod, H, W), generator=g).to(dev)
    rows, cols = 8, 32
    total = N * (H // rows) * (W // cols)
    variants = {"plain": dict(), "gate": dict(out_gate=gate), "gate_addt": dict(out_gate=gate, add_target=addt, add_coef=0.37),
                "unpool": dict(pool_idx=pidx), "unpool_gate": dict(pool_idx=pidx, out_gate=gate)}
    for vname, kw in variants.items():
        src = gyp if "pool_idx" in kw else gy
        ref = ops.wino43_dgrad_chain(src, ud, Cprod, **kw)
        for lname, ids in _tile_lists(total, total + Cred).items():
            lst = torch.full((total,), -1, dtype=torch.int32, device=dev)
            lst[:len(ids)] = torch.from_numpy(ids.astype(np.int32)).to(dev)
            cnt = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
            out = torch.full((N, Cprod, H, W), SENTINEL, device=dev)
            ops.wino43_dgrad_chain_tiles(src, ud, Cprod, lst, cnt[0], out, tile_cols=32, **kw)
            px = torch.from_numpy(_tile_pixels(ids, N, H, W, rows, cols)).to(dev)[:, None].expand(-1, Cprod, -1, -1)
            assert torch.equal(out[px].view(torch.int32), ref[px].view(torch.int32)), (vname, lname, "listed tiles differ")
            assert bool((out[~px] == SENTINEL).all()), (vname, lname, "an unlisted tile was written")
        # the kernel's own geometry through the new entry point: the existing listed launch
        ids = np.arange(0, N * (H // 4) * (W // 64), 2)
        lst = torch.from_numpy(ids.astype(np.int32)).to(dev)
        cnt = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
        a = torch.full((N, Cprod, H, W), SENTINEL, device=dev)
        b = a.clone()
        ops.wino43_dgrad_chain_tiles(src, ud, Cprod, lst, cnt[0], a, **kw)
        ops.wino43_dgrad_chain_tiles(src, ud, Cprod, lst, cnt[0], b, tile_cols=64, **kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), vname


def _tile_pixels(tile_ids, n, H, W, rows, cols):
    t = np.zeros(n * (H // rows) * (W // cols), bool)
    t[np.asarray(tile_ids, np.int64)] = True
    return np.repeat(np.repeat(t.reshape(n, H // rows, W // cols), rows, axis=1), cols, axis=2)


def test_a_geometry_that_does_not_fit_is_an_error(dev):
    from st3d import _lib, ops
    w = torch.randn((64, 64, 3, 3)) * 0.05
    _, ud = ops.wino43_pack(w.to(dev))
    gy = torch.randn((1, 64, 8, 96)).to(dev)
    lst = torch.zeros((4,), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.St3dError):
        ops.wino43_dgrad_chain_tiles(gy, ud, 64, lst, lst[0], torch.zeros_like(gy), tile_cols=64)


# ------------------------------------------------------------------------------------------------ (c) plan
NEW_LEVELS = {128: [2, 5, 7, 10, 12, 14], 64: [2, 5, 7]}          # VGG modules whose input gradient runs listed under FORCE


def _listed_modules(S, B):
    """the modules of the conv43_dgrad_need brackets of one masked plan.loss"""
    from st3d import vgg as V
    dev = torch.device("cuda:0")
    net = T._NET.get("net") or T._NET.setdefault("net", V.get_vgg(device=dev, seed=0))
    g = torch.Generator().manual_seed(S)
    content, style, cur = (torch.rand((B, 3, S, S), generator=g).to(dev) for _ in range(3))
    plan = V.PerceptualPlan(net, B, S)
    try:
        plan.set_content(content)
        plan.set_style(style, B)
        plan.profile(True)
        plan.profile_launches()
        plan.loss(cur, 1e6, 1.0, need_mask=torch.from_numpy(T._blobs(B, S, 7)).to(dev))
        torch.cuda.synchronize()
        launches = [(f, m) for f, m, _ in plan.profile_launches()]
        plan.profile(False)
    finally:
        plan.close()
    return launches


def _env(monkeypatch, **kw):
    for k in ("ST3D_NEED_DEPTH", "ST3D_NEED_BLOCKS", "ST3D_NEED_TILE", "ST3D_NEED_FORCE", "ST3D_NEED_GRAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("S,B", [(128, 1), (64, 2)])
@pytest.mark.parametrize("tile", [None, "64", "32"])
def test_plan_loss_with_every_level_listed(monkeypatch, dev, S, B, tile):
    _env(monkeypatch, ST3D_NEED_FORCE="1", **({"ST3D_NEED_TILE": tile} if tile else {}))
    launches = _listed_modules(S, B)
    assert sorted(m for f, m in launches if f == "conv43_dgrad_need") == NEW_LEVELS[S], "the new levels did not engage"
    assert [m for f, m in launches if f == "gram_bwd_need"] == ([5] if S == 128 else []), "the relu2_1 Gram backward: listed at 64^2 only"
    T._plan_case(S, B)
    T._plan_case(S, B, graph=True)


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import test_gpu_need_mask as T
for S, B in ((128, 1), (64, 2)):
    T._plan_case(S, B)
    T._plan_case(S, B, graph=True)
print("child ok")
"""


def test_plan_loss_with_every_level_listed_on_poisoned_buffers():
    """ST3D_POISON_PLAN=1 in a fresh child: what the listed launches skip stays NaN / -1, and none of it reaches a needed pixel"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    env.update(ST3D_POISON_PLAN="1", ST3D_NEED_FORCE="1")
    for k in ("ST3D_NEED_DEPTH", "ST3D_NEED_BLOCKS", "ST3D_NEED_TILE", "ST3D_NEED_GRAM"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


# ------------------------------------------------------------------------------------------------ (d) launches
def test_default_plan_launches_are_those_of_the_tile_granular_lists(monkeypatch, dev):
    """S = 128: every workgroup of the launches above conv2_1 has one tile at the most, so no new level engages and the
    (family, module) list is the one the old builder gives"""
    _env(monkeypatch)
    new = _listed_modules(128, 1)
    _env(monkeypatch, ST3D_NEED_BLOCKS="0")
    old = _listed_modules(128, 1)
    assert new == old
    assert sorted(m for f, m in new if f == "conv43_dgrad_need") == [2, 5] and not [m for f, m in new if f == "gram_bwd_need"]


# ------------------------------------------------------------------------------------------------ (e) Gram runs
@pytest.mark.parametrize("weighted", [False, True])
def test_listed_gram_runs_are_bitwise_the_full_launch(dev, weighted):
    """st3d_gram_bwd_gated_segs at C = 128, HW = 64 x 64, N = 2 against the full gated launch, starting from zero and
    accumulating: listed runs have its bits, the others keep the sentinel.  Lists: empty, full, one run, random."""
    from st3d import ops
    N, C, H, W = 2, 128, 64, 64
    g = torch.Generator().manual_seed(11)
    feat = torch.relu(torch.randn((N, C, H, W), generator=g)).to(dev)
    D = torch.randn((N, C, C), generator=g)
    D = (D + D.transpose(1, 2)).to(dev).contiguous()
    prev = torch.randn((N, C, H, W), generator=g).to(dev)
    q = torch.rand((N, H, W), generator=g).to(dev) if weighted else None
    runs = N * H * W // 64
    rng = np.random.default_rng(3)
    lists = {"empty": np.zeros(0, np.int64), "all": np.arange(runs), "last": np.array([runs - 1]),
             "random": np.flatnonzero(rng.random(runs) < 0.5)}
    for accumulate in (False, True):
        ref = ops.gram_bwd(D, feat, 0.37, out=prev.clone() if accumulate else None, gated=True, q=q)
        for name, ids in lists.items():
            lst = torch.full((runs,), -1, dtype=torch.int32, device=dev)
            lst[:len(ids)] = torch.from_numpy(ids.astype(np.int32)).to(dev)
            cnt = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
            out = prev.clone() if accumulate else torch.full((N, C, H, W), SENTINEL, device=dev)
            keep = out.clone()
            ops.gram_bwd_gated_segs(D, feat, 0.37, lst, cnt[0], out, accumulate=accumulate, q=q)
            on = np.zeros(runs, bool)
            on[ids] = True
            px = torch.from_numpy(np.repeat(on.reshape(N, H * W // 64), 64, axis=1).reshape(N, 1, H, W)).to(dev).expand(-1, C, -1, -1)
            assert torch.equal(out[px].view(torch.int32), ref[px].view(torch.int32)), (accumulate, name, "listed runs differ")
            assert torch.equal(out[~px].view(torch.int32), keep[~px].view(torch.int32)), (accumulate, name, "an unlisted run was written")
