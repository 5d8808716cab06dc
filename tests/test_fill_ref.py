"""The fp64 restatement of the pull-push fill (tests/_fillref.py) on cases with a known answer.  No GPU, no library."""
import numpy as np
import pytest

import _fillref as FR


def _map(H, W, texels, rest=7.0):
    """an (H,W,3) map holding `rest` (a colour no valid texel has) except at {(y, x): value}, and the mask of those texels;
    channel k holds value + 10 k, so a mix-up of channels shows"""
    tex = np.full((H, W, 3), rest, np.float32)
    valid = np.zeros((H, W), np.uint8)
    for (y, x), v in texels.items():
        tex[y, x] = v + 10.0 * np.arange(3)
        valid[y, x] = 1
    return tex, valid


def _red(out):
    return out[..., 0].astype(np.float64)


def _channels_agree(out, take):
    for k in (1, 2):
        assert np.array_equal(out[..., k][take], out[..., 0][take] + np.float32(10 * k))


def test_level_sides_and_workspace_formula():
    assert FR.level_sides(1, 1) == [(1, 1)]
    assert FR.level_sides(3, 5) == [(3, 5), (2, 3), (1, 2), (1, 1)]
    assert FR.level_sides(130, 70)[:3] == [(130, 70), (65, 35), (33, 18)] and len(FR.level_sides(16384, 1)) == 15
    assert FR.workspace_bytes(1, 1) == 16 and FR.workspace_bytes(3, 5) == 16 * (6 + 2 + 1)
    assert FR.workspace_bytes(1024, 1024) == 16 * (4 ** 10 - 1) // 3
    assert FR.workspace_bytes(0, 4) == FR.workspace_bytes(4, 16385) == 0


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 5), (33, 17)])
def test_all_valid_is_the_identity(shape):
    tex = np.random.default_rng(0).random(shape + (3,), dtype=np.float32)
    out, count, detail = FR.push_pull(tex, np.ones(shape, np.uint8))
    assert count == 0 and not detail["take"].any() and np.array_equal(out.view(np.uint32), tex.view(np.uint32))


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 5), (33, 17)])
def test_none_valid_is_the_identity_with_count_0(shape):
    tex = np.random.default_rng(1).random(shape + (3,), dtype=np.float32)
    tex[0, 0, 1] = np.nan                                   # bit for bit: even a NaN comes back
    out, count, detail = FR.push_pull(tex, np.zeros(shape, np.uint8))
    assert count == 0 and not detail["take"].any() and np.array_equal(out.view(np.uint32), tex.view(np.uint32))
    assert all(np.all(w == 0) for w in detail["weights"])


@pytest.mark.parametrize("corner", [(0, 0), (0, 7), (7, 0), (7, 7)])
def test_one_valid_corner_of_8x8_colours_every_texel(corner):
    tex, valid = _map(8, 8, {corner: 0.625})
    out, count, _ = FR.push_pull(tex, valid)
    assert count == 63 and np.all(out == np.float32(0.625) + np.float32(10) * np.arange(3, dtype=np.float32))


def test_2x2_with_one_valid_texel():
    """level 1 is the one valid colour with W = 1; the three others take its upsample: every tap is that texel"""
    tex, valid = _map(2, 2, {(0, 1): 3.0})
    out, count, detail = FR.push_pull(tex, valid)
    assert count == 3 and np.all(_red(out) == 3.0)
    _channels_agree(out, detail["take"])


def test_1x5_odd_side_and_clamped_taps_by_hand():
    """valid: x = 0 (1) and x = 4 (5).
    pull:  level 1 (1x3) = [1, -, 5] (x = 1 has the children 2, 3: W = 0); level 2 (1x2) = [1, 5] (the second has the one
           child that exists); level 3 = (1 + 5) / 2 = 3.
    push:  level 2 keeps both.  Level 1, x = 1 (odd): taps 0 (3/4), 1 (1/4) -> 0.75 + 1.25 = 2; its two y taps both clamp
           to row 0, (1/4 + 3/4) of the same.  Level 0: x = 1 (odd): taps 0, 1 -> 0.75 1 + 0.25 2 = 1.25; x = 2 (even):
           taps 0 (1/4), 1 (3/4) -> 0.25 + 1.5 = 1.75; x = 3 (odd): taps 1 (3/4), 2 (1/4) -> 1.5 + 1.25 = 2.75."""
    tex, valid = _map(1, 5, {(0, 0): 1.0, (0, 4): 5.0})
    out, count, detail = FR.push_pull(tex, valid)
    assert count == 3 and np.array_equal(_red(out), [[1.0, 1.25, 1.75, 2.75, 5.0]])
    assert [w.ravel().tolist() for w in detail["weights"]] == [[1, 0, 0, 0, 1], [1, 0, 1], [1, 1], [1]]
    _channels_agree(out, detail["take"])


def test_3x5_odd_sides_by_hand():
    """valid: (0,0) = 1 and (2,4) = 5.
    pull:  level 1 (2x3) = [[1, -, -], [-, -, 5]] ((1,2) has the one child (2,4)); level 2 (1x2) = [1, 5]; level 3 = 3.
    push:  level 1 from [1, 5] (both y taps clamp to its one row): columns 0, 1, 2 -> 1, 0.75 + 1.25 = 2, 0.25 + 3.75 = 4, so
           level 1 = [[1, 2, 4], [1, 2, 5]].  Level 0 from it: along x, columns 1...4 of row [1, 2, 4] -> 1.25, 1.75, 2.5, 3.5
           and of row [1, 2, 5] -> 1.25, 1.75, 2.75, 4.25; y = 0 (even) takes row 0 twice (-1 clamps to 0), y = 1 (odd) 3/4 row 0
           + 1/4 row 1, y = 2 (even) 1/4 row 0 + 3/4 row 1: (1,3) = 0.75 2.5 + 0.25 2.75 = 2.5625, (1,4) = 0.75 3.5 + 0.25 4.25 =
           3.6875, (2,3) = 0.25 2.5 + 0.75 2.75 = 2.6875, and (2,4) keeps 5."""
    tex, valid = _map(3, 5, {(0, 0): 1.0, (2, 4): 5.0})
    out, count, detail = FR.push_pull(tex, valid)
    want = [[1.0, 1.25, 1.75, 2.5, 3.5], [1.0, 1.25, 1.75, 2.5625, 3.6875], [1.0, 1.25, 1.75, 2.6875, 5.0]]
    assert count == 13 and np.array_equal(_red(out), want)
    _channels_agree(out, detail["take"])


def test_4x4_three_of_four_children_by_hand():
    """valid: (0,0) = 1, (0,1) = 2, (1,0) = 6 and (3,3) = 8.
    pull:  level 1 = [[(1 + 2 + 6) / 3 = 3, -], [-, 8]]: the first coarse texel has W = 3, stored as w' = min(3, 1) = 1 -- a sum
           of weights that are 0 or 1, cut at 1, is 0 or 1 again, so under this contract no level ever holds a fractional
           weight (asserted below), and w c + (1 - w) up is the upsample alone wherever it is taken.  Level 2 = (3 + 8) / 2 = 5.5.
    push:  level 1 = [[3, 5.5], [5.5, 8]].  Level 0: (1,1) (odd, odd) = 9/16 3 + 3/16 5.5 + 3/16 5.5 + 1/16 8 = 4.25;
           (0,2) (y even: row 0 twice; x even: 1/4, 3/4) = 0.25 3 + 0.75 5.5 = 4.875; (0,3) (x odd: column 1, column 2 -> 1) =
           5.5; (2,2) (even, even) = 1/16 3 + 3/16 5.5 + 3/16 5.5 + 9/16 8 = 6.75; (3,2) = 0.25 5.5 + 0.75 8 = 7.375."""
    tex, valid = _map(4, 4, {(0, 0): 1.0, (0, 1): 2.0, (1, 0): 6.0, (3, 3): 8.0})
    out, count, detail = FR.push_pull(tex, valid)
    want = [[1.0, 2.0, 4.875, 5.5], [6.0, 4.25, 5.5, 6.125], [4.875, 5.5, 6.75, 7.375], [5.5, 6.125, 7.375, 8.0]]
    assert count == 12 and np.array_equal(_red(out), want)
    assert all(set(np.unique(w)) <= {0.0, 1.0} for w in detail["weights"])
    _channels_agree(out, detail["take"])


def test_domain_limits_the_writes_but_not_the_sources():
    rng = np.random.default_rng(2)
    tex = rng.random((12, 9, 3), dtype=np.float32)
    valid = (rng.random((12, 9)) < 0.3).astype(np.uint8)
    domain = np.zeros((12, 9), np.uint8)
    domain[3:8, 2:6] = 1
    valid[4, 3] = 0                                         # an invalid texel inside the domain
    valid[0, 0] = 1                                         # a source outside it
    whole, n_whole, _ = FR.push_pull(tex, valid)
    part, n_part, detail = FR.push_pull(tex, valid, domain)
    inside = domain != 0
    assert np.array_equal(part[inside], whole[inside])      # the same colours: sources outside the domain still count
    assert np.array_equal(part[~inside].view(np.uint32), tex[~inside].view(np.uint32))
    assert n_part == int(((valid == 0) & inside).sum()) and 0 < n_part < n_whole
    moved = tex.copy()
    moved[0, 0] += 1.0                                      # a valid texel outside the domain changes what is written inside
    again, _, _ = FR.push_pull(moved, valid, domain)
    assert not np.array_equal(again[inside], part[inside])


def test_nan_and_garbage_in_invalid_texels_change_nothing():
    rng = np.random.default_rng(3)
    tex = rng.random((17, 33, 3), dtype=np.float32)
    valid = (rng.random((17, 33)) < 0.4).astype(np.uint8)
    want, n, _ = FR.push_pull(tex, valid)
    for junk in (np.nan, np.inf, -3e38):
        dirty = tex.copy()
        dirty[valid == 0] = junk
        out, m, _ = FR.push_pull(dirty, valid)
        assert m == n and np.array_equal(out.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape,share", [((1, 2), 0.5), ((8, 8), 0.02), ((33, 17), 0.5), ((130, 70), 0.02), ((64, 65), 0.98)])
def test_output_stays_within_the_range_of_the_valid_colours_and_a_constant_stays_constant(shape, share):
    rng = np.random.default_rng(4)
    tex = rng.random(shape + (3,), dtype=np.float32)
    valid = (rng.random(shape) < share).astype(np.uint8)
    valid[-1, -1], valid[0, 0] = 1, 0
    tex[valid == 0] = 99.0
    out, _, detail = FR.push_pull(tex, valid)
    lo, hi = tex[valid != 0].min(), tex[valid != 0].max()
    filled = detail["filled"][detail["take"]]
    assert filled.min() >= lo - 1e-12 and filled.max() <= hi + 1e-12 and out.max() <= hi
    flat = np.full(shape + (3,), 99.0, np.float32)
    flat[valid != 0] = 0.3
    out, _, detail = FR.push_pull(flat, valid)
    assert np.abs(detail["filled"] - np.float64(np.float32(0.3))).max() <= 1e-14 and np.all(out == np.float32(0.3))


def test_fp32_restatement_stays_within_the_counted_bound_of_fp64():
    """the bound the GPU test uses, 8 roundings per level: (8 n + 1) 2^-24 max|valid colour|, n = ceil(log2 max(H, W))"""
    rng = np.random.default_rng(5)
    for shape, share in (((130, 70), 0.02), ((257, 3), 0.1), ((64, 64), 0.5)):
        tex = rng.random(shape + (3,), dtype=np.float32)
        valid = (rng.random(shape) < share).astype(np.uint8)
        valid[0, 0] = 1
        _, _, d64 = FR.push_pull(tex, valid)
        _, _, d32 = FR.push_pull(tex, valid, dtype=np.float32)
        assert d32["filled"].dtype == np.float32
        n = len(FR.level_sides(*shape)) - 1
        bound = (8 * n + 1) * 2.0 ** -24 * float(tex[valid != 0].max())
        err = np.abs(d32["filled"].astype(np.float64) - d64["filled"])[d64["take"]].max()
        assert err <= bound, (shape, err, bound)
