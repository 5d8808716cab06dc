"""The numpy flat-field model (tests/_flatref.py) on cases small enough to work out by hand, and the two mutants it must
tell from the real thing (no GPU)."""
import numpy as np
import pytest

import _flatref as FR
import _needref as NR

WHITE = (1.0, 1.0, 1.0)


def _grid(S, launch):
    res = S if launch == 0 else S // 2
    rows, cols = NR.tile_geometry(res, res)
    return res // rows, res // cols


def _classes_present(TY, TX):
    return len({(min(ty, 2), min(TY - 1 - ty, 2), min(tx, 2), min(TX - 1 - tx, 2)) for ty in range(TY) for tx in range(TX)})


@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("n", [1, 3])
def test_empty_and_full(n, S):
    for launch, (lst, mp, vary) in enumerate(FR.flat_model(FR.images(n, S, WHITE, "empty"), WHITE)):
        TY, TX = _grid(S, launch)
        assert not vary.any()
        # one representative per border class, all of them in view 0, every other tile mapped to the one of its class
        assert len(lst) == _classes_present(TY, TX) and lst.max() < TY * TX
        assert (mp[lst] == -1).all() and (mp >= 0).sum() == n * TY * TX - len(lst)
        cls = FR.tile_classes(n, TY, TX).reshape(-1)
        rest = np.flatnonzero(mp >= 0)
        assert (cls[mp[rest]] == cls[rest]).all() and (mp[rest] < rest).all()
    for launch, (lst, mp, vary) in enumerate(FR.flat_model(FR.images(n, S, WHITE, "full"), WHITE)):
        TY, TX = _grid(S, launch)
        assert vary.all() and np.array_equal(lst, np.arange(n * TY * TX)) and (mp == -1).all()


def test_one_pixel_by_hand():
    """S = 128, pixel (y 9, x 62) of view 1.  conv1_2 reaches rows 7..11, columns 60..64: 4 x 64 tiles, rows 1..2, both
    tile columns; in whole 4x4 blocks rows 4..11, columns 60..67.  Pooled: rows 2..5, columns 30..33.  conv2_1 reaches rows
    1..6 (tile rows 0..1 of the 16 x 1 grid of 4 x 64 tiles), in whole blocks rows 0..7; conv2_2 reaches rows 0..8 (tile
    rows 0..2)."""
    img = FR.images(2, 128, WHITE, "empty")
    img[1, 0, 9, 62] = 0.5
    (l0, m0, v0), (l1, m1, v1), (l2, m2, v2) = FR.flat_model(img, WHITE)
    want0 = np.zeros((2, 32, 2), bool)
    want0[1, 1:3, :] = True
    assert np.array_equal(v0, want0)
    want1 = np.zeros((2, 16, 1), bool)
    want1[1, 0:2, 0] = True
    want2 = np.zeros((2, 16, 1), bool)
    want2[1, 0:3, 0] = True
    assert np.array_equal(v1, want1) and np.array_equal(v2, want2)
    # view 0 is flat: its first tile of each class (rows 0, 1, interior, 14, 15) stands for view 1's flat tiles as well
    assert list(l1) == [0, 1, 2, 14, 15, 16, 17] and m1[18] == 2 and m1[31] == 15 and m1[30] == 14 and m1[3] == 2
    assert list(l2) == [0, 1, 2, 14, 15, 16, 17, 18] and m2[19] == 2
    assert list(l0[:7]) == [0, 1, 2, 3, 4, 5, 60] and m0[64 + 0] == 0 and m0[64 + 8] == 4 and m0[64 + 9] == 5 and m0[64 + 61] == 61


@pytest.mark.parametrize("S", [128, 192])
@pytest.mark.parametrize("axis", ["y", "x"])
@pytest.mark.parametrize("end", [-1, 0, 1])
def test_blob_at_a_tile_border(S, axis, end):
    """A rectangle whose grown extent ends one short of, on and one past a tile border -- of the S grid (growth 2) and of
    the S/2 grid (growth 1 and 2 in pooled pixels) -- against interval arithmetic on the rectangle"""
    rows, cols = NR.tile_geometry(S, S)
    rows2, cols2 = NR.tile_geometry(S // 2, S // 2)
    cases = []
    if axis == "y":
        cases.append((5, 3 * rows - 1 - 2 + end, 70, 75))                  # S grid: grown row reaches 3 rows - 1 (+ end)
        cases.append((5, 2 * (2 * rows2 - 1 - 1 + end) - 1, 70, 75))       # S/2 grid behind conv2_1
        cases.append((5, 2 * (2 * rows2 - 1 - 2 + end) - 1, 70, 75))       # S/2 grid behind conv2_2
    else:
        cases.append((9, 12, 3, cols - 1 - 2 + end))
        cases.append((9, 12, 3, 2 * (cols2 - 1 - 1 + end) - 1))
        cases.append((9, 12, 3, 2 * (cols2 - 1 - 2 + end) - 1))
    for (y0, y1, x0, x1) in cases:
        got = FR.flat_model(FR.rect_image(2, S, WHITE, y0, y1, x0, x1, view=1), WHITE)
        for launch, (a, b, c, d) in enumerate(FR.rect_expected(S, y0, y1, x0, x1)):
            want = np.zeros_like(got[launch][2])
            want[1, a:b + 1, c:d + 1] = True
            assert np.array_equal(got[launch][2], want), (S, axis, end, launch, (y0, y1, x0, x1))


def test_corner_pixels_by_hand():
    """the four corner pixels of every view: the corner tiles of each launch vary and nothing else.  The grown corner is
    3 x 3 pixels in conv1_2's output, 4 x 4 in whole blocks, 2 x 2 pooled; conv2_1 reaches 3 x 3 (one tile), in whole blocks
    4 x 4; conv2_2 reaches 5 x 5: one tile of 8 rows, two tiles of 4 rows."""
    for S in (128, 192):
        for launch, (lst, mp, vary) in enumerate(FR.flat_model(FR.images(2, S, WHITE, "corners"), WHITE)):
            TY, TX = _grid(S, launch)
            deep = 2 if launch == 2 and NR.tile_geometry(S // 2, S // 2)[0] == 4 else 1
            want = np.zeros((2, TY, TX), bool)
            want[:, :deep, 0] = want[:, :deep, -1] = want[:, -deep:, 0] = want[:, -deep:, -1] = True
            assert np.array_equal(vary, want), (S, launch)
            # the corner classes have no flat member left: no representative for them, and none of the others is a corner
            assert set(lst[:len(lst) // 2 + 1]) >= {0, TX - 1} and (mp[lst] == -1).all()


def test_corners_nan_and_single_channel():
    for what in ("corners", "nan", "one_channel"):
        img = FR.images(2, 128, (0.25, 0.5, 0.75), what)
        v = FR.varying_pixels(img, (0.25, 0.5, 0.75))
        assert v.sum() == {"corners": 8, "nan": 2, "one_channel": 1}[what]
    # -0.0 is not the colour 0.0: compared as bits
    img = FR.images(1, 64, (0.0, 0.0, 0.0), "empty")
    img[0, 1, 3, 3] = -0.0
    assert FR.varying_pixels(img, (0.0, 0.0, 0.0)).sum() == 1


def test_mutants_are_told_apart():
    """dilation off by one (either way) and a representative per view instead of per batch"""
    S = 128
    rows, _ = NR.tile_geometry(S, S)
    img = FR.rect_image(2, S, WHITE, 18, 6 * rows - 1 - 2, 70, 75, view=0)     # grown extent ends ON the border row 6 rows - 1
    good = FR.flat_model(img, WHITE)
    want = FR.rect_expected(S, 18, 6 * rows - 1 - 2, 70, 75)
    for launch, (a, b, c, d) in enumerate(want):
        assert good[launch][2][0, a:b + 1, c:d + 1].all() and good[launch][2].sum() == (b - a + 1) * (d - c + 1)
    for bad_d in (0, 2):
        bad = FR.flat_model(img, WHITE, conv_dilation=bad_d)
        assert any(not np.array_equal(bad[k][2], good[k][2]) for k in range(3)), bad_d
    assert not np.array_equal(FR.flat_model(img, WHITE, conv_dilation=2)[0][2], good[0][2])      # one past: the next tile row
    per_view = FR.flat_model(img, WHITE, per_view=True)
    for k in range(3):
        assert len(per_view[k][0]) > len(good[k][0]) and not np.array_equal(per_view[k][1], good[k][1])
    # the batch-wide representative of view 1's flat tiles lies in view 0
    TY, TX = _grid(S, 0)
    assert (good[0][1][TY * TX:] < TY * TX).all() and (good[0][1][TY * TX:] >= 0).all()
    assert (per_view[0][1][TY * TX:][per_view[0][1][TY * TX:] >= 0] >= TY * TX).all()


def test_tiles_view_numbers_tiles_like_the_launch():
    t = np.arange(2 * 3 * 8 * 128, dtype=np.float32).reshape(2, 3, 8, 128)
    tv = FR.tiles_view(t, 4, 64)
    assert tv.shape == (8, 3, 4, 64)
    assert np.array_equal(tv[(1 * 2 + 1) * 2 + 0], t[1, :, 4:8, 0:64])
