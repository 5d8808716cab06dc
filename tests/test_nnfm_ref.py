"""The numpy restatement of the NNFM style loss (tests/_nnfmref.py) against hand cases, fp64 autograd, central differences
and torch's avg_pool2d.  No GPU."""
import numpy as np
import pytest
import torch

import _nnfmref as R

F32, F64 = np.float32, np.float64


def _cols(*vectors):
    """vectors -> (C, n) fp32, one vector per position"""
    return np.stack([np.asarray(v, F32) for v in vectors], axis=1)


# ---------------------------------------------------------------------------- hand cases, each exact
@pytest.mark.parametrize("dtype", (F64, F32))
def test_orthogonal_identical_and_duplicate_vectors(dtype):
    F = _cols([3, 0, 0, 0], [0, 0, 2, 0], [0, 5, 0, 0])
    S = _cols([0, 4, 0, 0], [0, 4, 0, 0], [0, 0, 0, 7], [8, 0, 0, 0], [8, 0, 0, 0])
    idx, d, n = R.search_image(F, S, dtype=dtype)
    assert n.tolist() == [3, 2, 5]
    assert idx.tolist() == [3, 0, 0]            # the lowest of the duplicates; all-orthogonal keeps the first of equal zeros
    assert d.tolist() == [0, 1, 0]              # identical directions: 0; orthogonal to everything: 1


@pytest.mark.parametrize("dtype", (F64, F32))
def test_zero_query_and_zero_style_vector(dtype):
    F = _cols([0, 0, 0], [1, 1, 0])
    S = _cols([0, 0, 0], [0, 2, 0])
    idx, d, n = R.search_image(F, S, dtype=dtype)
    assert idx.tolist() == [-1, 1] and d[0] == 1 and n[0] == 0          # the zero query: distance 1, index -1
    assert abs(d[1] - (1 - 1 / np.sqrt(2))) < 1e-7                       # the zero style vector has similarity 0: not chosen
    # against zero style vectors only, every similarity is 0: index 0, distance 1
    idx, d, _ = R.search_image(_cols([1, 2, 3]), _cols([0, 0, 0], [0, 0, 0]), dtype=dtype)
    assert idx.tolist() == [0] and d.tolist() == [1]
    g = R.grad(F[None], S[None], np.array([[-1, 1]], np.int32))
    assert not g[0][:, 0].any() and g[0][:, 1].any()                    # the zero query has gradient 0


@pytest.mark.parametrize("dtype", (F64, F32))
def test_nan_on_either_side(dtype):
    nan = float("nan")
    F = _cols([1, 0], [nan, 1], [0, 1])
    S = _cols([nan, 1], [1, 0], [0, 1])
    idx, d, _ = R.search_image(F, S, dtype=dtype)
    assert idx.tolist() == [1, 0, 2]            # a NaN style vector is never chosen; a NaN query keeps index 0
    assert d[0] == 0 and np.isnan(d[1]) and d[2] == 0
    idx, d, _ = R.search_image(_cols([1, 0]), _cols([nan, 0], [nan, nan]), dtype=dtype)
    assert idx.tolist() == [0] and np.isnan(d[0])        # nothing but NaN to choose from: index 0, NaN


def test_all_zero_mask_and_inactive_positions():
    rng = np.random.default_rng(0)
    F, S = R.relu_like(rng, (2, 5, 9)), R.relu_like(rng, (1, 5, 7))
    w = np.ones((2, 9), F32)
    w[0] = 0
    w[1, 3] = 0
    idx, d = R.search(F, S, w)
    full_idx, full_d = R.search(F, S)
    assert (idx[0] == -1).all() and not d[0].any() and idx[1, 3] == -1 and d[1, 3] == 0
    on = w != 0
    assert (idx[on] == full_idx[on]).all() and (d[on] == full_d[on]).all()
    assert R.loss(d, w) == pytest.approx(0.5 * (d[1].sum() / 8), rel=1e-14)      # the all-zero image contributes 0
    g = R.grad(F, S, idx, w)
    assert not g[0].any() and not g[1][:, 3].any() and g[1][:, 4].any()
    assert R.loss(np.zeros((1, 4)), np.zeros((1, 4))) == 0


def test_weighted_loss_and_batch_denom():
    d = np.array([[0.5, 0.25, 1.0], [0.0, 1.0, 0.5]])
    w = np.array([[1.0, 3.0, 0.0], [0.5, 0.5, 1.0]])
    assert R.loss(d) == ((1.75 / 3) + (1.5 / 3)) / 2
    assert R.loss(d, w) == ((0.5 + 0.75) / 4 + (0.5 + 0.5) / 2) / 2
    assert R.loss(d, w, batch_denom=8) == ((0.5 + 0.75) / 4 + (0.5 + 0.5) / 2) / 8


def test_fp32_chain_stays_far_inside_the_bound():
    """the fp32 restatement meets the GPU test's conditions with room: round-to-nearest costs at most half an ulp (2^-25 for
    partial sums <= 1) where E(C) budgets 2^-24 a rounding, so it stays within E(C) / 2 -- the conditions test the kernel,
    not the data"""
    rng = np.random.default_rng(1)
    for C, N, M in ((512, 96, 120), (64, 200, 300), (3, 50, 60)):
        F, S = R.relu_like(rng, (C, N)), R.relu_like(rng, (C, M))
        i64, d64, _ = R.search_image(F, S, dtype=F64)
        i32, d32, _ = R.search_image(F, S, dtype=F32)
        sim64 = R.sims(R.normalise(F)[0], R.normalise(S)[0])
        on = i32 >= 0
        rows = np.arange(N)[on]
        assert (sim64[rows, i32[on]] >= sim64[rows].max(axis=1) - 2 * R.E(C)).all()
        assert np.abs(d32[on] - (1 - sim64[rows, i32[on]])).max() <= 0.5 * R.E(C)
        assert (i32 == i64).mean() > 0.99


# ---------------------------------------------------------------------------- gradient
def _torch_loss(F, S, idx, w, denom):
    """the same expression under fp64 autograd: indices and weights constants"""
    total = 0
    for b in range(F.shape[0]):
        f, s = F[b], S[b if S.shape[0] > 1 else 0]
        on = torch.from_numpy((idx[b] >= 0) & (w[b] != 0))
        if not on.any() or not w[b].sum() > 0:
            continue
        fh = f[:, on] / f[:, on].pow(2).sum(0).sqrt()
        sj = s[:, torch.from_numpy(idx[b]).long()[on]]
        sh = sj / sj.pow(2).sum(0).sqrt()
        d = 1 - (fh * sh).sum(0)
        total = total + (torch.from_numpy(w[b])[on] * d).sum() / float(w[b].sum())
    return total / denom


def test_gradient_against_fp64_autograd():
    rng = np.random.default_rng(2)
    F, S = R.relu_like(rng, (3, 6, 40)).astype(F64), R.relu_like(rng, (3, 6, 33)).astype(F64) + 0.01
    w = rng.random((3, 40))
    w[1, ::3] = 0
    w[2] = 0
    idx, _ = R.search(F, S, w)
    for denom in (None, 7):
        g = R.grad(F, S, idx, w, denom)
        Ft = torch.from_numpy(F).requires_grad_(True)
        _torch_loss(Ft, torch.from_numpy(S), idx, w, float(denom or 3)).backward()
        ref = Ft.grad.numpy()
        assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max()
        assert not g[2].any() and not g[1][:, ::3].any()


def test_gradient_against_central_differences_away_from_index_switches():
    rng = np.random.default_rng(3)
    F, S = R.relu_like(rng, (2, 5, 12)).astype(F64) + 0.05, R.relu_like(rng, (1, 5, 9)).astype(F64) + 0.05
    w = rng.random((2, 12)) + 0.1
    idx, d = R.search(F, S, w)
    g = R.grad(F, S, idx, w)
    h, checked = 1e-6, 0
    for b, c, i in [(b, c, i) for b in range(2) for c in range(5) for i in range(0, 12, 3)]:
        Fp, Fm = F.copy(), F.copy()
        Fp[b, c, i] += h
        Fm[b, c, i] -= h
        ip, dp = R.search(Fp, S, w)
        im, dm = R.search(Fm, S, w)
        if ip[b, i] != idx[b, i] or im[b, i] != idx[b, i]:
            continue                                                       # the index switched inside the stencil
        fd = (R.loss(dp, w) - R.loss(dm, w)) / (2 * h)
        assert abs(fd - g[b, c, i]) <= 1e-6 * max(1.0, abs(g[b, c, i])), (b, c, i, fd, g[b, c, i])
        checked += 1
    assert checked >= 30


# ---------------------------------------------------------------------------- mask pooling
@pytest.mark.parametrize("ratio", (1, 2, 4, 8, 16))
def test_mask_pooling_against_avg_pool2d(ratio):
    rng = np.random.default_rng(ratio)
    H, W = 3, 5
    mask = (rng.integers(0, 257, (2, H * ratio, W * ratio)) / 256.0).astype(F32)      # exact under any order of the four adds
    ref = torch.from_numpy(mask)[:, None]
    for _ in range(int(np.log2(ratio))):
        ref = torch.nn.functional.avg_pool2d(ref, 2)
    assert (R.pool_mask(mask, H, W) == ref[:, 0].numpy()).all()
    import style_transfer as ST
    for m in (torch.from_numpy(mask), torch.from_numpy(mask)[:, None]):
        assert (ST.nnfm_pool_mask(m, 2, H, W).numpy() == ref[:, 0].numpy()).all()
