"""The numpy need model (tests/_needref.py) on cases small enough to work out by hand (no GPU)."""
import numpy as np

import _needref as NR


def test_empty_and_full_masks():
    for S in (64, 128):
        seg, lists = NR.need_model(np.zeros((2, S, S), np.uint8))
        assert not seg.any() and [len(l) for l in lists] == [0, 0]
        seg, lists = NR.need_model(np.ones((2, S, S), np.uint8))
        assert seg.all()
        assert np.array_equal(lists[0], np.arange(2 * (S // 4) * (S // 64)))
        assert np.array_equal(lists[1], np.arange(2 * (S // 2) ** 2 // 256))


def test_one_pixel_by_hand():
    """S = 128, pixel (y 8, x 64) of image 1: the dilation reaches row 7 and column 63, so segments (7..9, 0..1) are active;
    conv1_2 tiles are 4 x 64: tile rows 1 and 2, both tile columns; their dilated union covers rows 3..12 at every column,
    pooled rows 1..6; conv2_1 tiles on the 64 x 64 map are 4 x 64: tile rows 0 and 1."""
    m = np.zeros((2, 128, 128), np.uint8)
    m[1, 8, 64] = 1
    seg, lists = NR.need_model(m)
    want = np.zeros((2, 128, 2), np.uint8)
    want[1, 7:10, :] = 1
    assert np.array_equal(seg, want)
    per_img = 32 * 2
    assert list(lists[0]) == [per_img + 2 * 1, per_img + 2 * 1 + 1, per_img + 2 * 2, per_img + 2 * 2 + 1]
    assert list(lists[1]) == [16 + 0, 16 + 1]
    assert NR.tile_pixels(lists[0], 2, 128, 128).sum() == 4 * 4 * 64


def test_geometry_rule():
    assert NR.tile_geometry(512, 512) == (4, 64) and NR.tile_geometry(32, 32) == (8, 32) and NR.tile_geometry(48, 48) is None
    assert NR.tile_geometry(16, 96) == (8, 32) and NR.tile_geometry(12, 96) is None
