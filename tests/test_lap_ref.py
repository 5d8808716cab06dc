"""tests/_lapref.py, the numpy restatement of csrc/lap.hip, against an independent torch reference in fp64 on the CPU:
F.avg_pool2d, F.pad(mode='replicate'), a depthwise conv2d with the Laplacian kernel, autograd for the gradient.  The fp32
restatement is held per element against bounds that count the roundings the source writes (_lapref.bound_*)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lapref as LR

CASES = [((1, 1, 2, 2), 1), ((2, 3, 4, 6), 2), ((1, 3, 34, 18), 1), ((1, 3, 34, 18), 2), ((1, 1, 32, 48), 16)]
TILE = {1: (16, 128), 2: (32, 128), 4: (64, 128), 8: (128, 128), 16: (128, 256)}     # any tile: the bounds hold for every order


def torch_lap(x, p):
    """D(pool_p(x)) for a (B,C,H,W) fp64 tensor, by torch's own operators"""
    C = x.shape[1]
    P = F.avg_pool2d(x, p) if p > 1 else x
    k = torch.tensor([[0.0, -1.0, 0.0], [-1.0, 4.0, -1.0], [0.0, -1.0, 0.0]], dtype=x.dtype)
    return F.conv2d(F.pad(P, (1, 1, 1, 1), mode='replicate'), k.expand(C, 1, 3, 3).contiguous(), groups=C)


def torch_loss_grad(x, c, p, scale):
    leaf = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    T = torch_lap(torch.from_numpy(c.astype(np.float64)), p)
    loss = ((torch_lap(leaf, p) - T) ** 2).sum() * scale
    loss.backward()
    return float(loss.detach()), leaf.grad.numpy()


def _data(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("shape,p", CASES)
def test_fp64_restatement_equals_torch(shape, p):
    x, c = _data(shape, 3)
    B, C, H, W = shape
    scale = 1.0 / (B * C * (H // p) * (W // p))
    want = torch_lap(torch.from_numpy(x.astype(np.float64)), p).numpy()
    got = LR.fwd(x, p, np.float64)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13 * (1 + np.abs(want).max()))
    loss, grad = torch_loss_grad(x, c, p, scale)
    loss64, grad64, _ = LR.loss_grad64(x, LR.fwd(c, p, np.float64), p, scale)
    assert abs(loss64 - loss) <= 1e-12 * abs(loss)
    np.testing.assert_allclose(grad64, grad, rtol=0, atol=1e-12 * (1 + np.abs(grad).max()))


@pytest.mark.parametrize("shape,p", CASES)
def test_fp32_restatement_within_the_counted_roundings(shape, p):
    x, c = _data(shape, 4)
    B, C, H, W = shape
    scale = 1.0 / (B * C * (H // p) * (W // p))
    L32, L64 = LR.fwd(x, p, np.float32), LR.fwd(x, p, np.float64)
    assert L32.dtype == np.float32
    err, bound = np.abs(L32.astype(np.float64) - L64), LR.bound_fwd(x, p)
    assert (err <= bound).all(), (err / bound).max()
    assert err.max() > 0 or p == 1 and shape[-1] == 2        # the bound is not vacuous: fp32 does round
    assert (bound <= 64 * LR.U * (p * p + 3) * np.abs(x).max()).all()       # nor loose: a few ulps of the data per rounding

    loss32, grad32, r32 = LR.loss_grad(x, LR.fwd(c, p, np.float32), p, scale, TILE[p])
    loss64, grad64, r64 = LR.loss_grad64(x, LR.fwd(c, p, np.float64), p, scale)
    e_loss, e_grad, e_r = LR.bound_loss_grad(x, c, p, scale)
    assert loss32.dtype == np.float32 and grad32.dtype == np.float32 and grad32.shape == x.shape
    assert (np.abs(r32.astype(np.float64) - r64) <= e_r).all()
    assert (np.abs(grad32.astype(np.float64) - grad64) <= e_grad).all()
    assert abs(float(loss32) - loss64) <= e_loss


def test_the_ordered_sum_is_the_sum():
    rng = np.random.default_rng(5)
    for shape, p in (((2, 3, 20, 40), 1), ((1, 2, 9, 70), 4), ((1, 1, 10, 18), 16)):
        r = rng.standard_normal(shape).astype(np.float32)
        want = float((r.astype(np.float64) ** 2).sum())
        assert abs(LR.ordered_sum_sq(r, p, TILE[p]) - want) <= 1e-13 * want


@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (7, 4)])
def test_the_clamped_stencil_is_symmetric(shape):
    """<D a, b> = <a, D b> in fp64: along one axis row 0 of the matrix is [1, -1], so the backward applies the same stencil"""
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    lhs, rhs = float((LR.D(a) * b).sum()), float((a * LR.D(b)).sum())
    assert abs(lhs - rhs) <= 1e-12 * (1 + abs(lhs))
    n = shape[0] * shape[1]
    M = np.stack([LR.D(e.reshape(shape)).reshape(-1) for e in np.eye(n)], axis=1)
    assert np.array_equal(M, M.T)


@pytest.mark.parametrize("p", LR.POOLS)
def test_a_constant_image_gives_exactly_zero(p):
    for value in (0.1, 0.7, 1.0, -3.3):
        x = np.full((1, 2, 4 * p, 3 * p), value, np.float32)
        L = LR.fwd(x, p, np.float32)
        assert L.shape == (1, 2, 4, 3) and not L.any()
        loss, grad, _ = LR.loss_grad(x, L, p, 0.5, TILE[p])
        assert loss == 0 and not grad.any()


def test_the_gradient_is_the_transpose():
    """<grad, v> equals the directional derivative of the fp64 loss: pool^T D^T (2 scale r), with D^T = D"""
    x, c = _data((1, 2, 8, 12), 7)
    v = np.random.default_rng(8).standard_normal(x.shape)
    for p in (1, 2, 4):
        T = LR.fwd(c, p, np.float64)
        f = lambda t: LR.loss_grad64(x.astype(np.float64) + t * v, T, p, 0.37)[0]
        _, grad, _ = LR.loss_grad64(x, T, p, 0.37)
        eps = 1e-6
        assert abs((f(eps) - f(-eps)) / (2 * eps) - float((grad * v).sum())) <= 1e-6 * (1 + abs(float((grad * v).sum())))
