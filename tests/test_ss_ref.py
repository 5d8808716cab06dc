"""The supersampling reference itself (tests/_ssref.py), on the CPU: the ordered box filter against the fp64 mean, its
transpose, the pixel grid, and that the shared fixtures exercise partial coverage."""
import numpy as np
import pytest

import _ssref

U = 2.0 ** -24      # unit roundoff of fp32


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_ordered_box_is_the_fp64_mean_within_a2_u(a):
    """a^2 - 1 additions and one division of values in [0, 1): the sums stay below a^2, every rounding is at most u times
    the partial sum, so the quotient is within (a^2 - 1) u + u = a^2 u of the exact mean."""
    x = np.random.default_rng(a).random((2, 3, 7 * a, 7 * a), dtype=np.float32)
    got = _ssref.box_down(x, a)
    mean = x.astype(np.float64).reshape(2, 3, 7, a, 7, a).mean(axis=(3, 5))
    assert got.dtype == np.float32 and got.shape == (2, 3, 7, 7)
    assert np.abs(got.astype(np.float64) - mean).max() <= a * a * U


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_box_and_its_transpose_are_adjoint_in_fp64(a):
    rng = np.random.default_rng(10 + a)
    x, y = rng.standard_normal((2, 3, 5 * a, 5 * a)), rng.standard_normal((2, 3, 5, 5))
    lhs = (_ssref.box_down(x, a, np.float64) * y).sum()
    rhs = (x * _ssref.box_down_t(y, a, np.float64)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_a_equal_one_is_the_identity():
    x = np.random.default_rng(0).standard_normal((2, 3, 9, 9)).astype(np.float32)
    np.testing.assert_array_equal(_ssref.box_down(x, 1), x)
    np.testing.assert_array_equal(_ssref.box_down_t(x, 1), x)


@pytest.mark.parametrize("a", [1, 2, 3, 4])
@pytest.mark.parametrize("S", [16, 20])
def test_half_image_rectangle_splits_coverage_at_the_middle_column(S, a):
    """A rectangle over exactly the left half of the NDC square (PyTorch3D: +x points left) covers columns [0, S/2) fully and
    nothing else for every a: the a * S pixel grid spans the same square (a * S is even, no sub-pixel centre lies on x = 0)."""
    from oracle import render_ref as rr
    verts = np.array([[0.0, -2.0, 2.0], [3.0, -2.0, 2.0], [3.0, 2.0, 2.0], [0.0, 2.0, 2.0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    p2f = rr.rasterize(verts, faces, a * S)[0]
    cov = _ssref.box_down((p2f >= 0).astype(np.float32), a)
    np.testing.assert_array_equal(cov[:, :S // 2], 1.0)
    np.testing.assert_array_equal(cov[:, S // 2:], 0.0)


@pytest.mark.parametrize("S,T,a", _ssref.CASES)
def test_fixtures_have_partial_full_and_empty_pixels_in_every_view(S, T, a):
    c = _ssref.case(S, T, a)
    for b in range(_ssref.B):
        cov = c["cov"][b, 0]
        assert ((cov > 0) & (cov < 1)).sum() >= 20 and (cov == 1).sum() >= 40 and (cov == 0).sum() >= 100
        # coverage is a count over a^2 and uncovered pixels are exactly white
        np.testing.assert_array_equal(cov * (a * a), np.round(cov * (a * a)))
        assert (c["rgb"][b][:, cov == 0] == 1.0).all()
