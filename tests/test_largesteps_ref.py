"""tests/_largesteps_ref.py against itself and against scipy's sparse LU: the references the GPU tests of csrc/diffuse.hip
lean on are right before anything is compared with them.  No GPU, no libst3d."""
import numpy as np
import pytest
import torch

import _largesteps_ref as R

F32, F64 = np.float32, np.float64
LAMBDAS = (1.0, 19.0, 100.0)
TOL = 1e-6


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for name in ("cow", "teapot", "bob"):
        v, f = R.fixture(name)
        out[name] = (v, f, R.Rows(f, len(v)))
    return out


def test_the_matrix_is_symmetric_with_unit_row_sums_and_the_stated_degrees(fixtures):
    for name, (v, f, rows) in fixtures.items():
        M = R.system(f, len(v), 19.0)
        assert abs(M - M.T).max() == 0.0
        np.testing.assert_array_equal(np.asarray(M.sum(1)).ravel(), np.ones(len(v)))
        deg = np.diff(rows.off)
        np.testing.assert_array_equal(M.diagonal(), 1.0 + 19.0 * deg)
        assert rows.d_max == deg.max()
    assert np.diff(fixtures["teapot"][2].off).min() == 3 and fixtures["teapot"][2].d_max == 24


def test_the_row_form_annihilates_constants_exactly_and_matches_the_sparse_product():
    rng = np.random.default_rng(0)
    for name, (v, f) in R.meshes().items():
        rows = R.Rows(f, len(v))
        for c in (1.0, 0.1, -3.7):
            x = np.full(len(v), c, F32)
            assert np.array_equal(rows.apply32(19.0, x), x), (name, c)
        x = rng.standard_normal(len(v)).astype(F32)
        exact = R.system(f, len(v), 19.0) @ x.astype(F64)
        got = rows.apply32(19.0, x)
        # d + 1 fp32 roundings of terms no larger than 2 max|x| each, times lambda, plus the final two
        bound = (rows.d_max + 3) * 2.0 ** -24 * (1.0 + 19.0 * 2.0 * rows.d_max) * np.abs(x).max()
        assert np.abs(got - exact).max() <= bound, name


def test_a_constant_right_hand_side_is_solved_in_one_iteration_bit_for_bit():
    for name, (v, f) in R.meshes().items():
        rows = R.Rows(f, len(v))
        for c in (1.0, 0.1, -3.7):
            b = np.full(len(v), c, F32)
            x, it, ok = R.cg32(rows, 19.0, b, TOL, 5)
            assert it == 1 and ok and np.array_equal(x, b), (name, c)
        x, it, ok = R.cg32(rows, 19.0, np.zeros(len(v), F32), TOL, 5)
        assert it == 0 and ok and not x.any()


def test_the_restatement_agrees_with_the_direct_solve_within_the_derived_cap(fixtures):
    """lambda_min(M) >= 1, so the error is at most the true residual; the recursive residual stops at tol ||b||, and the
    bound here is loose on purpose (the GPU tests take 4 x what the restatement itself reaches): 50 tol in the maximum
    norm relative to the solution's."""
    rng = np.random.default_rng(1)
    for name, (v, f, rows) in fixtures.items():
        V = len(v)
        for lam in LAMBDAS:
            cap = R.iteration_cap(lam, rows.d_max, TOL)
            solve = R.direct_solver(f, V, lam)
            for what, b in (("noise", rng.standard_normal((V, 3))), ("M verts", R.system(f, V, lam) @ v.astype(F64))):
                b = b.astype(F32)
                x, its, ok = R.cg32_columns(rows, lam, b, TOL, cap)
                err = R.relative_max_error(x, solve(b))
                print(f"{name} lambda {lam:g} {what}: iterations {its} of {cap}, error {err:.2e}")
                assert all(ok) and max(its) <= cap, (name, lam, what, its, cap)
                assert err <= 50 * TOL, (name, lam, what, err)


def test_the_cap_is_what_the_derivation_gives():
    from st3d import largesteps as LS
    assert R.iteration_cap(19.0, 8, 1e-6) == 254 == LS.iteration_cap(19.0, 8, 1e-6)       # twice the 127 of the exact bound
    assert R.iteration_cap(1e-3, 1, 0.5) == 8 == LS.iteration_cap(1e-3, 1, 0.5)           # never below 8
    for lam in LAMBDAS:
        for d in (3, 6, 24):
            for tol in (1e-4, 1e-6):
                assert LS.iteration_cap(lam, d, tol) == R.iteration_cap(lam, d, tol)


def test_the_uniform_adam_restatement_has_one_denominator():
    g = torch.zeros(50)
    g[7] = 10.0
    p, m, s = torch.zeros(50), torch.zeros(50), torch.zeros(50)
    R.adam_uniform_step(p, g, m, s, 1, 0.01)
    assert torch.equal(p[:7], torch.zeros(7)) and abs(float(p[7]) + 0.01) < 1e-8         # lr g / (eps + |g|)
    g2 = 0.01 * torch.randn(50, generator=torch.Generator().manual_seed(0))
    before = p.clone()
    denom = R.adam_uniform_step(p, g2, m, s, 2, 0.01)
    mhat = m / (1 - 0.9 ** 2)
    keep = torch.arange(50) != 7
    torch.testing.assert_close((before - p)[keep], (0.01 * mhat / denom)[keep], rtol=1e-5, atol=1e-9)      # p is about 0 but for entry 7

    assert abs(float(denom) - float((s[7] / (1 - 0.999 ** 2)).sqrt())) < 1e-6             # the one large second moment sets it
