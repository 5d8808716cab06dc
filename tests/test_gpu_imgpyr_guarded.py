"""Every wrapper of st3d/imgpyr.py and the pyramid ops between guard zones (tests/_guarded.py): no write outside its outputs,
no output element left unwritten, and the same bits under both fill patterns and in a plain run -- on the planes of
tests/test_gpu_imgpyr.py and inside the multi-scale loss at S = 64."""
import numpy as np
import pytest
import torch

import _guarded as G
import _imgpyrref as PR

pytestmark = pytest.mark.gpu
MODULES = ("st3d.ops", "st3d.imgpyr")
U32 = np.uint32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_every_wrapper_between_guard_zones(dev):
    from st3d import imgpyr, ops
    th, tw = ops.pyr_down_tile()
    rng = np.random.default_rng(21)
    for shape in ((1, 1, 2, 2), (2, 3, 4, 6), (2, 3, 6, 10), (1, 3, 34, 18), (1, 2, th + 2, tw + 2), (1, 2, 2 * th - 2, 2 * tw - 2)):
        B, C, H, W = shape
        x = rng.standard_normal(shape).astype(np.float32)
        g = rng.standard_normal((B, C, H // 2, W // 2)).astype(np.float32)
        m = (rng.random((B, H, W)) < 0.1).astype(np.uint8)
        d_x, d_g, d_m = _t(x, dev), _t(g, dev), _t(m, dev)
        out = G.compare_ab(lambda: {"fwd": ops.pyr_down_fwd(d_x), "bwd": ops.pyr_down_bwd(d_g), "need": ops.pyr_down_need(d_m)},
                           modules=MODULES)
        assert np.array_equal(out["fwd"].cpu().numpy().view(U32), PR.down(x, np.float32).view(U32)), shape
        assert np.array_equal(out["bwd"].cpu().numpy().view(U32), PR.down_transpose(g, np.float32).view(U32)), shape
        assert np.array_equal(out["need"].cpu().numpy(), PR.need(m)), shape

        def autograd():
            leaf = d_x.clone().requires_grad_(True)
            y = imgpyr.pyr_down(leaf)
            y.backward(d_g)
            return {"y": y.detach(), "grad": leaf.grad}

        # (autograd may hand the leaf the backward's own buffer or a copy of it: the gradient is the case's own either way)
        out = G.compare_ab(autograd, modules=MODULES, own=lambda raw: (raw["grad"],))
        assert np.array_equal(out["y"].cpu().numpy().view(U32), PR.down(x, np.float32).view(U32))
        assert np.array_equal(out["grad"].cpu().numpy().view(U32), PR.down_transpose(g, np.float32).view(U32))

    # two steps: sides divisible by 4, the second of them past one tile
    for shape in ((1, 2, 8, 12), (1, 1, 2 * th + 4, 2 * tw + 4)):
        B, C, H, W = shape
        x = rng.standard_normal(shape).astype(np.float32)
        m = (rng.random((B, H, W)) < 0.1).astype(np.uint8)
        d_x, d_m = _t(x, dev), _t(m, dev)
        out = G.compare_ab(lambda: {"r2": imgpyr.reduce(d_x, 2), "r4": imgpyr.reduce(d_x, 4), "n4": imgpyr.reduce_need(d_m, 4)},
                           modules=MODULES)
        assert np.array_equal(out["r2"].cpu().numpy().view(U32), PR.down(x, np.float32).view(U32))
        assert np.array_equal(out["r4"].cpu().numpy().view(U32), PR.down(PR.down(x, np.float32), np.float32).view(U32))
        assert np.array_equal(out["n4"].cpu().numpy(), PR.need(PR.need(m)))

    t = _t(np.full((3, 3, 8, 12), 0.25, np.float32), dev)

    def cached():
        imgpyr.clear_cache()
        one = t[:1].expand(3, -1, -1, -1)
        return {"c2": imgpyr.reduced_cached(t, 2), "c4": imgpyr.reduced_cached(t, 4), "e2": imgpyr.reduced_cached(one, 2)}

    out = G.compare_ab(cached, modules=MODULES)
    assert bool((out["c2"] == 0.25).all()) and tuple(out["e2"].shape) == (3, 3, 4, 6) and tuple(out["c4"].shape) == (3, 3, 2, 3)
    imgpyr.clear_cache()


def test_the_multi_scale_loss_between_guard_zones(dev):
    """the pyramid's buffers inside compute_perceptual_loss(scales=...) sit between guards; the loss and the gradient, which
    the plan and autograd allocate, are the case's own.  Same bits under both patterns and in a plain run."""
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import imgpyr
    from st3d import render as R
    U.device = ST.device = L.device = dev
    vgg = U.get_vgg(seed=0)
    B, S = 2, 64
    gen = torch.Generator().manual_seed(9)
    x, c, s = (torch.rand(B, 3, S, S, generator=gen).to(dev) for _ in range(3))
    need = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
    need[:, 9:41, 13:50] = 1
    mask = need[:, None].to(torch.float32)

    def loss(tagged):
        imgpyr.clear_cache()                                 # every run reduces content and style afresh, inside the guards
        leaf = x.clone().requires_grad_(True)
        cur = leaf * 1.0
        if tagged:
            setattr(cur, R.NEED_TAG, need)
        value = L.compute_perceptual_loss(cur, c, s, vgg, scales=(1, 2), scale_weights=(1.0, 0.5),
                                          style_masks=mask if tagged else None)
        value.backward()
        out = {"loss": value.detach(), "grad": leaf.grad}
        out["_own"] = tuple(out.values())
        return out

    for tagged in (False, True):
        out = G.compare_ab(lambda: loss(tagged), modules=MODULES, own=lambda raw: raw["_own"])
        assert torch.isfinite(out["loss"]) and torch.isfinite(out["grad"]).all() and bool((out["grad"] != 0).any())
    imgpyr.clear_cache()
