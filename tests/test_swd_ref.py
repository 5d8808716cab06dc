"""The numpy restatement of the sliced Wasserstein style loss (tests/_swdref.py) against torch autograd in fp64 (torch.sort +
gather), analytic cases, the quantile map and the total order.  No GPU."""
import numpy as np
import pytest
import torch

import _swdref as R

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------- torch autograd in fp64
def _torch_term(F, S, V, w=None, batch_denom=None):
    """the same term written with torch.sort and gather in fp64 -> (loss tensor, F leaf)"""
    Ft = torch.from_numpy(np.asarray(F, F64)).requires_grad_(True)
    St, Vt = torch.from_numpy(np.asarray(S, F64)), torch.from_numpy(np.asarray(V, F64))
    B, C, N = Ft.shape
    K, M = Vt.shape[0], St.shape[2]
    total = 0
    for b in range(B):
        p = Vt @ Ft[b]
        t = torch.sort(Vt @ St[b if St.shape[0] > 1 else 0], dim=1).values
        if w is not None:
            on = torch.from_numpy(np.asarray(w[b]) > 0)
            p = p[:, on]
        n = p.shape[1]
        if n == 0:
            continue
        j = torch.from_numpy(R.quantile(n, M))
        total = total + ((torch.sort(p, dim=1).values - t[:, j]) ** 2).sum() / (K * n)
    return total / float(batch_denom if batch_denom is not None else B), Ft


@pytest.mark.parametrize("B,Bs,C,K,N,M,masked,denom", [(1, 1, 4, 4, 7, 7, False, None), (2, 1, 8, 5, 33, 50, False, None),
                                                       (3, 3, 6, 9, 40, 17, True, 7), (2, 2, 3, 1, 1, 4, False, None)])
def test_loss_and_closed_form_gradient_against_fp64_autograd(B, Bs, C, K, N, M, masked, denom):
    rng = np.random.default_rng(0)
    F = rng.standard_normal((B, C, N)).astype(F32)                          # no ties: a continuous draw
    S = rng.standard_normal((Bs, C, M)).astype(F32)
    V = R.unit_rows(rng, K, C)
    w = None
    if masked:
        w = rng.random((B, N)).astype(F32)
        w[0, ::3] = 0
        w[1] = 0                                                             # an image without an active position
    L, g = R.term(F, S, V, w, denom)
    Lt, Ft = _torch_term(F, S, V, w, denom)
    Lt.backward()
    assert abs(L - float(Lt.detach())) <= 1e-12 * abs(float(Lt.detach()))
    assert np.abs(g - Ft.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(g).max())
    if masked:
        assert not g[1].any() and not g[0][:, ::3].any() and g[0].any()


def test_fp32_chain_is_within_its_bound_of_fp64():
    rng = np.random.default_rng(1)
    x, a = R.relu_like(rng, (2, 100, 37)), R.unit_rows(rng, 5, 100)
    p64, p32 = R.project(x, a), R.project(x, a, F32)
    assert p32.dtype == F32 and (np.abs(p32 - p64) <= R.project_bound(x, a)).all()
    # equal columns give equal bits; a chain of one term is the rounded product -- added to the +0 the chain starts from, so a
    # product of -0 comes out as +0: no projection is ever -0
    x[:, :, 5] = x[:, :, 20]
    p32 = R.project(x, a, F32)
    assert p32[:, :, 5].tobytes() == p32[:, :, 20].tobytes()
    one = R.project(x[:, :1], a[:, :1], F32)
    assert one.tobytes() == ((a[:, :1].astype(F64)[None] * x[:, :1].astype(F64)).astype(F32) + F32(0)).tobytes()
    assert (one == 0).any() and not np.signbit(one[one == 0]).any()


# ---------------------------------------------------------------------------- analytic cases
def test_a_shifted_permuted_copy_costs_the_mean_squared_projected_shift():
    rng = np.random.default_rng(2)
    C, N, K = 6, 200, 16
    cloud = rng.standard_normal((1, C, N))
    d = rng.standard_normal(C)
    shifted = (cloud + d[None, :, None])[:, :, rng.permutation(N)]
    V = R.unit_rows(rng, K, C).astype(F64)
    p = np.einsum("kc,bcn->bkn", V, cloud)                                   # fp32 inputs would round the shift: stay in fp64
    t = np.einsum("kc,bcn->bkn", V, shifted)
    L = R.loss(np.sort(p, axis=2), [N], np.sort(t, axis=2))
    expect = ((V @ d) ** 2).mean()
    print("shifted cloud: loss %.9f, mean_k (V_k . d)^2 %.9f" % (L, expect))
    assert abs(L - expect) <= 1e-12 * expect


def test_equal_distributions_cost_nothing_and_have_no_gradient():
    rng = np.random.default_rng(3)
    F = R.relu_like(rng, (2, 5, 30))
    S = F[:, :, rng.permutation(30)]
    L, g = R.term(F, S, R.unit_rows(rng, 7, 5), dtype=F32)
    assert L == 0 and not g.any()


def test_quantile_map():
    assert R.quantile(3, 7).tolist() == [1, 3, 5]
    assert R.quantile(7, 3).tolist() == [0, 0, 1, 1, 1, 2, 2]
    assert R.quantile(1, 4).tolist() == [2]
    assert R.quantile(4, 1).tolist() == [0, 0, 0, 0]
    assert R.quantile(5, 5).tolist() == [0, 1, 2, 3, 4]
    for n, M in ((1, 1), (1 << 20, 1 << 20), (1 << 20, 3), (5, 1 << 20)):
        j = R.quantile(n, M)
        assert j[0] >= 0 and j[-1] < M and (np.diff(j) >= 0).all()


# ---------------------------------------------------------------------------- the order
def _f(bits):
    return np.array(bits, np.uint32).view(F32)


def test_keys_order_signed_zeros_infinities_and_nans():
    nan_pos, nan_neg, nan_payload = 0x7FC00000, 0xFFC00000, 0x7F800001
    v = _f([nan_neg, 0x7F800000, 0x00000000, 0x80000000, 0xFF800000, nan_pos, 0x3F800000, 0xBF800000, nan_payload, 0x00000001,
            0x80000001])
    k = R.key(v)
    assert k[0] == k[5] == k[8]                                              # every NaN is the canonical one
    order = np.argsort(k, kind="stable")
    # -Inf, -1, -denormal, -0, +0, +denormal, 1, +Inf, then the NaNs by index
    assert order.tolist() == [4, 7, 10, 3, 2, 9, 6, 1, 0, 5, 8]
    srt, perm, count = R.sort_rows(v[None, None, :])
    assert perm[0, 0].tolist() == order.tolist() and count.tolist() == [11]
    assert srt.view(np.uint32)[0, 0].tolist() == v.view(np.uint32)[order].tolist()     # NaNs kept as they came


def test_ties_go_by_index_and_inactive_positions_go_last():
    v = np.array([[[2, 1, 2, 1, 1, 0, 2]]], F32)
    srt, perm, count = R.sort_rows(v)
    assert perm[0, 0].tolist() == [5, 1, 3, 4, 0, 2, 6] and count.tolist() == [7]
    w = np.array([[1, 0, 0.5, 1, -1, 0, np.nan]], F32)                       # active iff w > 0
    srt, perm, count = R.sort_rows(v, w)
    assert count.tolist() == [3] and perm[0, 0].tolist() == [3, 0, 2, 5, 1, 4, 6]
    assert srt[0, 0].tolist() == [1, 2, 2, 0, 1, 1, 2]
    # the gradient reaches the active positions only
    g = R.grad_proj(srt, perm, count, np.zeros((1, 1, 4), F32))
    assert (g[0, 0] != 0).tolist() == [True, False, True, True, False, False, False]
