"""The numpy restatement of the image-pyramid step (tests/_imgpyrref.py) against hand-computed planes, against its own
transpose, against the dense matrix built from the definition and against torch's anti-aliased bilinear resize.  CPU only."""
import numpy as np
import pytest
import torch

import _imgpyrref as PR


def test_hand_computed_2x2():
    # every tap clamps: per row h = (a + b) + 3 (a + b) = 4 (a + b); v = 4 (h0 + h1); / 64 -> the mean of the four
    x = np.array([[1.0, 2.0], [3.0, 6.0]], np.float32)
    for dt in (np.float32, np.float64):
        out = PR.down(x, dt)
        assert out.shape == (1, 1) and out.dtype == dt
        assert out[0, 0] == dt(3.0)
    # the transpose hands every fine pixel 4 * 4 / 64 = 1/4 of the coarse one
    g = np.array([[8.0]], np.float32)
    assert np.array_equal(PR.down_transpose(g), np.full((2, 2), 2.0, np.float32))


def test_hand_computed_4x4():
    x = np.arange(16, dtype=np.float32).reshape(4, 4)
    # rows: h for output column 0 reads columns (0, 0, 1, 2), column 1 reads (1, 2, 3, 3)
    h = np.array([[(r[0] + r[2]) + 3 * (r[0] + r[1]), (r[1] + r[3]) + 3 * (r[2] + r[3])] for r in x], np.float64)
    want = np.array([[(h[0, c] + h[2, c]) + 3 * (h[0, c] + h[1, c]) for c in range(2)],
                     [(h[1, c] + h[3, c]) + 3 * (h[2, c] + h[3, c]) for c in range(2)]]) / 64.0
    assert np.array_equal(PR.down(x, np.float64), want)
    assert np.array_equal(PR.down(x, np.float32), want.astype(np.float32))     # small integers: every rounding is exact
    # by hand: column 0 has h = 5, 37, 69, 101 and (5 + 69) + 3 (5 + 37) = 200; column 1 has h = 19, 51, 83, 115 and
    # (51 + 115) + 3 (83 + 115) = 760
    assert want[0, 0] == 200 / 64 and want[1, 1] == 760 / 64
    # transpose of a one-hot coarse pixel (0, 0): rows carry (4, 3, 1, 0) / 8, columns the same
    g = np.zeros((2, 2), np.float32)
    g[0, 0] = 64.0
    k = np.array([4.0, 3.0, 1.0, 0.0])
    assert np.array_equal(PR.down_transpose(g, np.float64), np.outer(k, k))
    g[:] = 0
    g[1, 1] = 64.0
    assert np.array_equal(PR.down_transpose(g, np.float32), np.outer(k[::-1], k[::-1]).astype(np.float32))


@pytest.mark.parametrize("shape", [(2, 2), (4, 6), (34, 18), (2, 16), (16, 2)])
def test_constant_plane_stays_constant_bit_for_bit(shape):
    for c in (1.0, 0.1, -3.7e-5, 123456.789):
        x = np.full(shape, c, np.float32)
        out = PR.down(x, np.float32)
        # (c + c) + 3 (c + c) = 8 c and 8 (8 c) = 64 c are scalings by powers of two up to 3 * 2c + 2c, exact in binary
        assert np.array_equal(out.view(np.uint32), np.full((shape[0] // 2, shape[1] // 2), c, np.float32).view(np.uint32))


@pytest.mark.parametrize("shape", [(2, 2), (2, 8), (8, 2), (4, 6), (6, 10), (34, 18)])
def test_adjoint_identity_and_matrix(shape):
    rng = np.random.default_rng(3)
    H, W = shape
    x = rng.standard_normal((3, H, W))
    y = rng.standard_normal((3, H // 2, W // 2))
    lhs = float((PR.down(x, np.float64) * y).sum())
    rhs = float((x * PR.down_transpose(y, np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    D = PR.matrix(H, W)
    assert np.allclose(D @ x[0].ravel(), PR.down(x[0], np.float64).ravel(), rtol=1e-13, atol=1e-13)
    assert np.allclose(D.T @ y[0].ravel(), PR.down_transpose(y[0], np.float64).ravel(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("shape", [(2, 2), (2, 6), (4, 4), (10, 6)])
def test_transpose_weights_conserve_mass(shape):
    H, W = shape
    cols = PR.down_transpose(np.ones((H // 2, W // 2)), np.float64)      # column sums of D, one per fine pixel
    assert cols.shape == (H, W)
    # every row of D sums to 1, so the columns sum to the number of coarse pixels: 1/4 per fine pixel over the plane
    assert abs(cols.sum() - H * W / 4.0) <= 1e-12 * H * W
    if H >= 4 and W >= 4:
        assert np.array_equal(cols[1:-1, 1:-1], np.full((H - 2, W - 2), 0.25))      # interior: (3 + 1)^2 / 64
        assert cols[0, 0] == 0.25 and cols[0, 1] == 0.25                               # 4 * 4 / 64 and 4 * (3 + 1) / 64


def test_interior_matches_antialiased_bilinear_resize():
    rng = np.random.default_rng(5)
    x = rng.random((2, 3, 20, 28), dtype=np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(x), scale_factor=0.5, mode="bilinear", antialias=True).numpy()
    got = PR.down(x, np.float32)
    assert got.shape == want.shape
    inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))         # footprints that do not clamp
    ulp = np.spacing(np.abs(want[inner]).astype(np.float32))
    # torch adds 16 products of normalised weights in its own order: a few ulps of the result apart
    assert np.all(np.abs(got[inner] - want[inner]) <= 4 * ulp), float(np.max(np.abs(got[inner] - want[inner]) / ulp))


def test_need_rule_single_pixels():
    H, W = 8, 12
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 5), (H - 1, 6), (3, 0), (4, W - 1), (3, 5), (4, 6), (3, 6)):
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 200            # any non-zero byte
        got = PR.need(m)
        want = np.zeros((H // 2, W // 2), np.uint8)
        for i, j in PR.footprint_outputs(H, W, y, x):
            want[i, j] = 1
        assert np.array_equal(got, want), (y, x)
        # a fine pixel lies in at most 2 x 2 footprints, and exactly in those the transpose gathers it from
        near_y, far_y, _, has_y = (a[y] for a in PR.axis_taps(H))
        near_x, far_x, _, has_x = (a[x] for a in PR.axis_taps(W))
        gathered = {(i, j) for i in {near_y} | ({far_y} if has_y else set()) for j in {near_x} | ({far_x} if has_x else set())}
        assert gathered == PR.footprint_outputs(H, W, y, x)
    assert not PR.need(np.zeros((2, 4, 4), np.uint8)).any()
    assert PR.need(np.ones((1, 2, 2), np.uint8)).tolist() == [[[1]]]
