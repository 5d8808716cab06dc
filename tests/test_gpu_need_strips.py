"""Need lists per strip (csrc/need.hip with tile_cols = 16; csrc/wino43.hip, STRIPS): the device's lists against the numpy
model (tests/_needstrips_ref.py), the listed F(4x4,3x3) launch on hand-made strip lists bit for bit against the unlisted
launch of the same conv, and the plan with every level on strips (ST3D_NEED_FORCE=1 ST3D_NEED_TILE=16): same losses, same
gradient on the mask, 0 off it -- plain, on poisoned buffers, under graph replay."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _needblocks_ref as NB
import _needstrips_ref as NS
import test_gpu_need_blocks as TB
import test_gpu_need_mask as T

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ (a) builder
def test_strip_lists_equal_the_numpy_model(dev):
    """S = 128, N = 3: all six lists exist (S / 4 = 32).  Entries, voids and counts exactly the model's; nothing written past
    the last step; a mixed call (strips on some lists, tiles on the others) leaves the tile lists what they are alone."""
    from st3d import ops
    S, N = 128, 3
    assert ops.need_blocks_lists(S) == NB.n_lists(S) == 6
    for name, m in NS.masks(N, S).items():
        ref = NS.need_strips_model(m)
        md = torch.from_numpy(m).to(dev)
        seg, lists = ops.need_blocks_build(md, tile_cols=[16] * 6)
        assert np.array_equal(seg.cpu().numpy(), ref["seg"]), name
        for k, (lst, cnt) in enumerate(lists):
            R = S >> NB.LIST_SHIFT[k]
            assert lst.numel() == N * (R // 4) * (R // 16), (name, k)
            c = int(cnt)
            assert c == ref["steps"][k], (name, k, c, ref["steps"][k])
            got = lst.cpu().numpy()
            assert np.array_equal(got[:4 * c], ref["lists"][k]), (name, k)
            assert (got[4 * c:] == -1).all(), (name, k, "entries past the last step were written")
        mixed = [16, 0, 32, 16, 0, 16]
        tiles = NB.need_blocks_model(m, tile_cols=[c if c != 16 else 0 for c in mixed])
        _, lists = ops.need_blocks_build(md, tile_cols=mixed)
        for k, (lst, cnt) in enumerate(lists):
            c = int(cnt)
            if mixed[k] == 16:
                assert c == ref["steps"][k] and np.array_equal(lst.cpu().numpy()[:4 * c], ref["lists"][k]), (name, k)
            else:
                assert c == len(tiles["lists"][k]) and np.array_equal(lst.cpu().numpy()[:c], tiles["lists"][k]), (name, k)


# ------------------------------------------------------------------------------------------------ (b) kernel bits
def _strip(n, sy, sx, H, W):
    return (n * (H // 4) + sy) * (W // 16) + sx


def _hand_lists(N, H, W):
    """name -> steps, each four entries of ONE image (-1 = void)"""
    sy1, sx1 = H // 4 - 1, W // 16 - 1
    s = lambda n, sy, sx: _strip(n, sy, sx, H, W)
    corners = [s(0, 0, 0), s(0, 0, sx1), s(0, sy1, 0), s(0, sy1, sx1)]
    every = [[s(n, sy, sx) for sy in range(sy1 + 1) for sx in range(sx1 + 1)] for n in range(N)]
    return {
        "empty": [],
        "one_step_corners": [corners],
        "far_apart": [[s(1, 0, sx1), s(1, 3, 0), s(1, 5, sx1), s(1, sy1, 0)], [s(1, 1, 0), s(1, 2, sx1), s(1, 4, 0), s(1, 6, sx1)]],
        "voids": [[s(0, 1, 0), s(0, 2, 0), s(0, 2, sx1), -1], corners, [s(0, 4, 0), s(0, 6, sx1), -1, -1], [s(1, 0, 0), -1, -1, -1],
                  [s(1, sy1, sx1), s(1, 3, 0), s(1, 2, 0), -1], [s(1, 5, 0), -1, -1, -1]],
        "void_first": [[-1, s(0, 3, sx1), -1, s(0, 0, 0)], [s(1, 2, 0), -1, s(1, 7 % (sy1 + 1), sx1), -1]],
        "all": [e[i:i + 4] for e in every for i in range(0, len(e), 4)],
    }


def _patch_mask(entries, N, H, W, pooled):
    """(N, H or H/2, W or W/2) bool: the input pixels inside a listed strip's clipped 6 x (16 + 2) patch"""
    m = np.zeros((N, H, W), bool)
    for e in entries:
        if e < 0:
            continue
        n, r = divmod(int(e), (H // 4) * (W // 16))
        sy, sx = divmod(r, W // 16)
        m[n, max(0, 4 * sy - 1):min(H, 4 * sy + 5), max(0, 16 * sx - 1):min(W, 16 * sx + 17)] = True
    return m.reshape(N, H // 2, 2, W // 2, 2).any(axis=(2, 4)) if pooled else m


@pytest.mark.parametrize("slots", ["1", "4"])
@pytest.mark.parametrize("Cred,Cprod", [(64, 64), (128, 128)])
def test_listed_strips_are_bitwise_the_unlisted_launch(dev, monkeypatch, Cred, Cprod, slots):
    """st3d_wino43_dgrad_chain_tiles_geo with tile_cols = 16 on 32 x 32 maps, N = 2, reducing over Cred channels into Cprod
    (128 -> 128: two cout tiles, 8 stages through the 3-deep ring): MODE 0 plain, with the gate, with gate + content term;
    MODE 3 un-pooling a 16 x 16 pooled gradient, alone and gated.  Every block of a listed strip has the bits of the unlisted
    launch, every other element keeps the sentinel, and the same bits come out with NaN written into the input (and the gate
    operands) everywhere outside the listed strips' clipped patches (pixels).  ST3D_W43_SLOTS = 1 / 4: a workgroup crosses steps."""
    from st3d import ops
    monkeypatch.setenv("ST3D_W43_SLOTS", slots)
    N, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(1000 + Cred)
    w = torch.randn((Cred, Cprod, 3, 3), generator=g) * 0.05
    _, ud = ops.wino43_pack(w.to(dev))
    gy = torch.randn((N, Cred, H, W), generator=g).to(dev)
    gyp = torch.randn((N, Cred, H // 2, W // 2), generator=g).to(dev)
    pidx = torch.randint(0, 4, (N, Cred, H // 2, W // 2), generator=g, dtype=torch.uint8).to(dev)
    gate = torch.randn((N, Cprod, H, W), generator=g).to(dev)
    addt = torch.randn((N, Cprod, H, W), generator=g).to(dev)
    variants = {"plain": dict(), "gate": dict(out_gate=gate), "gate_addt": dict(out_gate=gate, add_target=addt, add_coef=0.37),
                "unpool": dict(pool_idx=pidx), "unpool_gate": dict(pool_idx=pidx, out_gate=gate)}
    nan = float("nan")
    for vname, kw in variants.items():
        pooled = "pool_idx" in kw
        src = gyp if pooled else gy
        ref = ops.wino43_dgrad_chain(src, ud, Cprod, **kw)
        for lname, steps in _hand_lists(N, H, W).items():
            ent = np.asarray(steps, np.int32).reshape(-1)
            lst = torch.full((N * (H // 4) * (W // 16) + 8,), -1, dtype=torch.int32, device=dev)
            lst[:len(ent)] = torch.from_numpy(ent).to(dev)
            cnt = torch.tensor([len(steps)], dtype=torch.int32, device=dev)
            px = torch.from_numpy(NS.strip_pixels(ent, N, H, W)).to(dev)[:, None].expand(-1, Cprod, -1, -1)
            inside = torch.from_numpy(_patch_mask(ent, N, H, W, pooled)).to(dev)[:, None].expand(-1, Cred, -1, -1)
            kw_nan = dict(kw)
            for key in ("out_gate", "add_target"):
                if key in kw:
                    kw_nan[key] = torch.where(px, kw[key], torch.full_like(kw[key], nan))
            src_nan = torch.where(inside, src, torch.full_like(src, nan))
            for tag, s_, k_ in (("clean", src, kw), ("nan_outside", src_nan, kw_nan)):
                out = torch.full((N, Cprod, H, W), SENTINEL, device=dev)
                ops.wino43_dgrad_chain_tiles(s_, ud, Cprod, lst, cnt[0], out, tile_cols=16, **k_)
                assert torch.equal(out[px].view(torch.int32), ref[px].view(torch.int32)), (vname, lname, tag, "listed strips differ")
                assert bool((out[~px] == SENTINEL).all()), (vname, lname, tag, "something outside the listed strips was written")


def test_strips_need_a_list_and_the_input_gradient_chain(dev):
    from st3d import _lib, ops
    w = torch.randn((64, 64, 3, 3)) * 0.05
    uf, ud = ops.wino43_pack(w.to(dev))
    lst = torch.full((16,), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    gy = torch.randn((1, 64, 8, 48)).to(dev)              # a map the kernel does not cover (W % 32)
    with pytest.raises(_lib.St3dError):
        ops.wino43_dgrad_chain_tiles(gy, ud, 64, lst, cnt[0], torch.zeros_like(gy), tile_cols=16)
    gy = torch.randn((1, 64, 8, 32)).to(dev)
    with pytest.raises(_lib.St3dError):                   # a step is read as one 16-byte vector
        ops.wino43_dgrad_chain_tiles(gy, ud, 64, lst[1:], cnt[0], torch.zeros_like(gy), tile_cols=16)
    with pytest.raises(_lib.St3dError):                   # bias / ReLU / pool: the forward has no strip instantiation
        ops.wino43_fwd_tiles(gy, uf, torch.zeros((64,), device=dev), 64, lst, cnt[0], y=torch.zeros_like(gy), tile_cols=16)
    out = torch.full_like(gy, SENTINEL)
    ops.wino43_dgrad_chain_tiles(gy, ud, 64, lst, cnt[0], out, tile_cols=16)       # an empty list writes nothing
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ (c) plan
def _env(monkeypatch, **kw):
    for k in ("ST3D_NEED_DEPTH", "ST3D_NEED_BLOCKS", "ST3D_NEED_TILE", "ST3D_NEED_FORCE", "ST3D_NEED_GRAM", "ST3D_GRAPH", "ST3D_NEED_MASK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("tile", ["16", "16,0,16,32,16,64"])
def test_plan_loss_with_every_level_on_strips(monkeypatch, dev, tile):
    """S = 128, N = 2: all six input gradients run listed; the three losses are the unmasked call's bits, the image gradient
    its bits on the mask and exactly 0 off it; once more under graph replay (three masks through one captured graph)"""
    _env(monkeypatch, ST3D_NEED_FORCE="1", ST3D_NEED_TILE=tile)
    launches = TB._listed_modules(128, 2)
    assert sorted(m for f, m in launches if f == "conv43_dgrad_need") == TB.NEW_LEVELS[128], "the levels did not engage"
    T._plan_case(128, 2)
    T._plan_case(128, 2, graph=True)


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import test_gpu_need_mask as T
T._plan_case(128, 2)
T._plan_case(128, 2, graph=True)
print("child ok")
"""


@pytest.mark.parametrize("graph_env", [None, "1"])
def test_plan_loss_on_strips_on_poisoned_buffers(graph_env):
    """ST3D_POISON_PLAN=1 in a fresh child (and once more with ST3D_GRAPH=1: every plan.loss through a captured graph): what
    the strip launches skip stays NaN / -1, and none of it reaches a needed pixel"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    for k in ("ST3D_NEED_DEPTH", "ST3D_NEED_BLOCKS", "ST3D_NEED_GRAM", "ST3D_GRAPH", "ST3D_NEED_MASK"):
        env.pop(k, None)
    env.update(ST3D_POISON_PLAN="1", ST3D_NEED_FORCE="1", ST3D_NEED_TILE="16")
    if graph_env:
        env["ST3D_GRAPH"] = graph_env
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
