"""The per-block need model (tests/_needblocks_ref.py) on the CPU: hand cases, its lists against the tile-granular model's,
and that what it keeps is enough -- a torch emulation of the listed chain conv3_3 .. conv1_2 on NaN-poisoned inputs gives
the bits of the clean run wherever the relu1_1 pass reads, while two mutants of the rule do not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _needblocks_ref as NB
import _needref as NR


def _blobs(n, S, seed, count=3):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, S, S), np.uint8)
    for i in range(n):
        for _ in range(count):
            h, w = rng.integers(1, S // 2, 2)
            y, x = rng.integers(0, S - h + 1), rng.integers(0, S - w + 1)
            m[i, y:y + h, x:x + w] = 1
    return m


# ------------------------------------------------------------------------------------------------ hand cases
def test_lists_exist_where_the_kernel_covers_the_map():
    assert NB.n_lists(128) == 6 and NB.n_lists(512) == 6
    assert NB.n_lists(64) == 3          # 64^2, 32^2, 32^2; the 16^2 maps of conv3_x are not covered
    assert NB.n_lists(96) == 0
    assert NB.geometry(128) == (4, 64) and NB.geometry(32) == (8, 32) and NB.geometry(128, 32) == (8, 32)
    assert NB.geometry(32, 64) is None


def test_one_pixel():
    """S = 128, pixel (5, 70).  need_0 = rows 4..6 x cols 69..71 -> block (1, 17) -> 4 x 64 tile (1, 1) = 3; 8 x 32 tile (0, 2) = 2.
    need_1 = pool(rows 3..8 x cols 67..72) = rows 1..4 x cols 33..36 of 64^2 -> blocks (0..1, 8..9): 4 x 64 tiles 0, 1; 8 x 32
    tile (0, 1) = 1.  need_2 = rows 0..8 x cols 31..40 -> blocks (0..2, 7..10): 4 x 64 tiles 0..2; 8 x 32 tiles (0..1, 0..1).
    need_3 = pool(rows 0..12 x cols 27..44) = rows 0..6 x cols 13..22 of 32^2 -> blocks (0..1, 3..5): 8 x 32 tile 0."""
    m = np.zeros((1, 128, 128), np.uint8)
    m[0, 5, 70] = 1
    a = NB.need_blocks_model(m)
    assert [l.tolist() for l in a["lists"][:4]] == [[3], [0, 1], [0, 1, 2], [0]]
    assert a["geo"] == [(4, 64), (4, 64), (4, 64), (8, 32), (8, 32), (8, 32)]
    assert a["need"][1].sum() == 16 and a["need"][1][0, 1:5, 33:37].all()
    assert a["need"][3].sum() == 70 and a["need"][3][0, 0:7, 13:23].all()
    b = NB.need_blocks_model(m, tile_cols=[32] * 6)
    assert [l.tolist() for l in b["lists"][:4]] == [[2], [1], [0, 1, 2, 3], [0]]
    # the Gram runs of the 64^2 map (one per row): need_2 = rows 0..8
    assert a["gram"].tolist() == list(range(9)) and NB.need_blocks_model(np.zeros((1, 64, 64), np.uint8))["gram"] is None
    for k in range(6):          # the geometry changes the lists, never the need
        assert np.array_equal(a["need"][k], b["need"][k]) and np.array_equal(a["reads"][k], b["reads"][k])


def test_corner_pixel_is_clipped_to_the_map():
    m = np.zeros((2, 64, 64), np.uint8)
    m[1, 63, 63] = 1
    a = NB.need_blocks_model(m)
    # image 1: 4 x 64 tile (15, 0) of 16 per image; 8 x 32 tiles of the 32^2 maps: (3, 0) of 4 per image
    assert [l.tolist() for l in a["lists"]] == [[16 + 15], [4 + 3], [4 + 3]]
    assert a["need"][0].sum() == 4 and a["need"][1].sum() == 9 and a["need"][2].sum() == 25
    assert not a["need"][2][0].any()


def test_empty_and_full_masks():
    for S in (64, 128):
        e = NB.need_blocks_model(np.zeros((2, S, S), np.uint8))
        f = NB.need_blocks_model(np.ones((2, S, S), np.uint8))
        assert not e["seg"].any() and f["seg"].all()
        for k in range(NB.n_lists(S)):
            R = S >> NB.LIST_SHIFT[k]
            assert len(e["lists"][k]) == 0 and not e["reads"][k].any()
            assert np.array_equal(f["lists"][k], np.arange(2 * R * R // 256)) and f["reads"][k].all()


@pytest.mark.parametrize("S", [64, 128, 256])
def test_lists_are_subsets_of_the_tile_granular_model(S):
    for seed in range(4):
        m = _blobs(2, S, 100 * S + seed)
        seg, old = NR.need_model(m, 3)
        new = NB.need_blocks_model(m)
        assert np.array_equal(new["seg"], seg)
        assert np.array_equal(new["lists"][0], old[0])              # a segment of dilate(mask, 1) and a block of it: the same tiles
        assert set(new["lists"][1].tolist()) <= set(old[1].tolist())
        # and need only ever shrinks against the rule that hands whole tiles up
        assert not (new["reads"][0] & ~NR.pool_or(NR.dilate(NR.tile_pixels(old[0], 2, S, S)))).any()


# ------------------------------------------------------------------------------------------------ sufficiency
def _unpool(g, idx):
    """(n, C, R/2, R/2), argmax bytes 0..3 -> (n, C, R, R): the value at its window's argmax position, 0 elsewhere"""
    n, C, h, w = g.shape
    out = torch.zeros((n, C, 2 * h, 2 * w), dtype=g.dtype)
    for q in range(4):
        out[:, :, (q >> 1)::2, (q & 1)::2] = torch.where(idx == q, g, torch.zeros_like(g))
    return out


def _launch(x, w):
    """one input-gradient launch as the F(4x4,3x3) kernel sees it: a 3x3 convolution, and every aligned 4x4 output block
    whose 6x6 input patch holds a NaN is NaN throughout (the block is transformed as a whole)"""
    y = F.conv2d(x, w, padding=1)
    nan = torch.isnan(x).any(dim=1).numpy()
    bad = NR.expand(NR.tiles_any(NR.dilate(nan), 4, 4), 4, 4)
    y[torch.from_numpy(bad)[:, None].expand_as(y)] = float("nan")
    return y


def _chain(S, n, model, seed):
    """the listed chain top down on 2-channel maps; model = None: the clean run.  With a model, each launch's stored input
    is NaN outside what the model says the launch reads, and its output NaN outside what the model says is needed of it (a
    listed launch leaves the rest unwritten) -> the gradient the relu1_1 pass reads, (n, 2, S, S)."""
    g = torch.Generator().manual_seed(seed)
    nl = NB.n_lists(S)
    top = S >> NB.LIST_SHIFT[nl - 1]
    x = torch.randn((n, 2, top // 2, top // 2) if NB.LIST_UNPOOLS[nl - 1] else (n, 2, top, top), generator=g)

    def poison(t, keep):
        return t if model is None else torch.where(torch.from_numpy(keep)[:, None].expand_as(t), t, torch.full_like(t, float("nan")))

    for k in range(nl - 1, -1, -1):
        w = torch.randn((2, 2, 3, 3), generator=g)
        if model is not None:
            x = poison(x, model["reads"][k])
        if NB.LIST_UNPOOLS[k]:
            x = _unpool(x, torch.randint(0, 4, x.shape, generator=g))
        x = _launch(x, w)
        if model is not None:
            x = poison(x, model["need"][k])
    return x


def _sufficient(S, n, mask, mutant=None, tile_cols=None):
    clean = _chain(S, n, None, seed=S)
    got = _chain(S, n, NB.need_blocks_model(mask, mutant=mutant, tile_cols=tile_cols), seed=S)
    assert bool(torch.isfinite(clean).all())
    px = torch.from_numpy(NR.dilate(mask != 0))[:, None].expand_as(clean)
    return torch.equal(got[px].view(torch.int32), clean[px].view(torch.int32))


@pytest.mark.parametrize("S", [64, 128])
def test_the_model_keeps_enough(S):
    masks = [_blobs(2, S, 7 * S + s) for s in range(3)]
    one = np.zeros((2, S, S), np.uint8)
    one[1, S // 2, S // 2 + 1] = 1
    corners = np.zeros((2, S, S), np.uint8)
    corners[:, 0, 0] = corners[:, 0, -1] = corners[:, -1, 0] = corners[:, -1, -1] = 1
    for m in masks + [one, corners, np.ones((2, S, S), np.uint8)]:
        assert _sufficient(S, 2, m)
        assert _sufficient(S, 2, m, tile_cols=[32] * 6)


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("mutant", ["shrink", "no_pool_or"])
def test_mutants_of_the_rule_keep_too_little(S, mutant):
    assert not _sufficient(S, 2, _blobs(2, S, 7 * S), mutant=mutant)
