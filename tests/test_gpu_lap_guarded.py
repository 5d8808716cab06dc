"""Every wrapper of st3d/lap.py and the Laplacian content term between guard zones (tests/_guarded.py): no write outside its
outputs or its workspace, no output element left unwritten, and the same bits under both fill patterns and in a plain run --
on the planes of tests/test_gpu_lap.py and next to compute_second_approach_loss at S = 64."""
import numpy as np
import pytest
import torch

import _guarded as G
import _lapref as LR

pytestmark = pytest.mark.gpu
MODULES = ("st3d.ops", "st3d.lap")
U32 = np.uint32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cases():
    from st3d import ops
    cases = [((1, 1, 2, 2), 1), ((2, 3, 4, 6), 2), ((1, 3, 34, 18), 1), ((1, 3, 34, 18), 2), ((1, 1, 32, 48), 16)]
    for p in (1, 4, 16):
        th, tw = ops.lap_tile(p)
        cases += [((1, 2, th + 2 * p, tw + 2 * p), p), ((1, 2, 2 * th - 2 * p, 2 * tw - 2 * p), p)]
    return cases


def test_every_wrapper_between_guard_zones(dev):
    from st3d import lap, ops
    rng = np.random.default_rng(21)
    for shape, p in _cases():
        B, C, H, W = shape
        x, c = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        scale = 1.0 / (B * C * (H // p) * (W // p))
        d_x, d_c = _t(x, dev), _t(c, dev)

        def wrappers():
            T = ops.lap_fwd(d_c, p)
            loss, grad = ops.lap_loss(d_x, T, p, scale)
            value, _ = ops.lap_loss(d_x, T, p, scale, want_grad=False)
            return {"T": T, "loss": loss, "grad": grad, "value": value}

        out = G.compare_ab(wrappers, modules=MODULES)
        T_ref = LR.fwd(c, p, np.float32)
        want_loss, want_grad, _ = LR.loss_grad(x, T_ref, p, scale, ops.lap_tile(p))
        assert np.array_equal(out["T"].cpu().numpy().view(U32), T_ref.view(U32)), (shape, p)
        assert np.array_equal(out["grad"].cpu().numpy().view(U32), want_grad.view(U32)), (shape, p)
        assert np.array_equal(out["loss"].cpu().numpy().view(U32), np.array([want_loss]).view(U32)), (shape, p)
        assert np.array_equal(out["value"].cpu().numpy().view(U32), out["loss"].cpu().numpy().view(U32))

    t = _t(np.full((3, 3, 16, 32), 0.25, np.float32), dev)
    x = _t(rng.random((3, 3, 16, 32)).astype(np.float32), dev)

    def cached_and_combined():
        lap.clear_cache()
        targets = [lap.lap_target_cached(t, 2), lap.lap_target_cached(t, 8)]
        loss, grad = lap.lap_term(x, targets, (2, 8), batch_denom=6)
        return {"t2": targets[0], "t8": targets[1], "again": lap.lap_target_cached(t, 2), "loss": loss, "grad": grad}

    # (the sums of two pools come out of torch's own additions: the case's own)
    out = G.compare_ab(cached_and_combined, modules=MODULES, own=lambda raw: (raw["loss"], raw["grad"]))
    assert not bool(out["t2"].any()) and not bool(out["t8"].any()) and tuple(out["t8"].shape) == (3, 3, 2, 4)
    assert torch.equal(out["again"], out["t2"]) and float(out["loss"]) > 0 and bool((out["grad"] != 0).any())
    lap.clear_cache()


def test_the_term_next_to_the_second_approach_loss_between_guard_zones(dev):
    """a step of second_approach.py with --lap_weight: compute_second_approach_loss plus the weighted term, backpropagated
    together; the term's targets, workspaces and gradients sit between guards, the loss and the leaf's gradient, which the
    plan and autograd allocate, are the case's own.  Same bits under both patterns and in a plain run."""
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import lap
    from st3d import render as R
    U.device = ST.device = L.device = dev
    vgg = U.get_vgg(seed=0)
    B, S, w = 2, 64, 1e4
    gen = torch.Generator().manual_seed(9)
    x, c, s = (torch.rand(B, 3, S, S, generator=gen).to(dev) for _ in range(3))
    need = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
    need[:, 9:41, 13:50] = 1

    def step(tagged, pools):
        lap.clear_cache()                                    # every run builds the targets afresh, inside the guards
        leaf = x.clone().requires_grad_(True)
        cur = leaf * 1.0
        if tagged:
            setattr(cur, R.NEED_TAG, need)
        value = L.compute_second_approach_loss(cur, c, s, vgg, 1e6, 1.0, None, None, None, {}, "texture", batch_denom=B)
        detail = L.compute_laplacian_loss(cur, c, pools, batch_denom=B)
        (value + w * detail).backward()
        out = {"loss": value.detach(), "detail": detail.detach(), "grad": leaf.grad}
        out["_own"] = tuple(out.values())
        return out

    for tagged, pools in ((False, (4,)), (True, (4,)), (False, (1, 4, 16))):
        out = G.compare_ab(lambda: step(tagged, pools), modules=MODULES, own=lambda raw: raw["_own"])
        assert torch.isfinite(out["loss"]) and float(out["detail"]) > 0
        assert torch.isfinite(out["grad"]).all() and bool((out["grad"] != 0).any())
    lap.clear_cache()
