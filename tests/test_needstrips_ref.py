"""The strip lists' numpy model (tests/_needstrips_ref.py) against what a list has to be: every listed strip holds a block of
B_k, every block of B_k lies in a listed strip, entries ascend within an image, voids only close an image's last step, a
step's strips are one image's, and the count is the sum of the images' ceil(strips / 4)."""
import numpy as np
import pytest

import _needblocks_ref as NB
import _needref as NR
import _needstrips_ref as NS

S, N = 128, 3


def _check_list(need, entries, steps):
    n, R, _ = need.shape
    per_img = (R // 4) * (R // 16)
    blocks = NR.tiles_any(need, 4, 4)                                  # B_k, one flag per 4x4 block: (n, R/4, R/4)
    in_strip = blocks.reshape(n, R // 4, R // 16, 4)                   # [image][strip row][strip column][block of the strip]
    assert entries.dtype == np.int32 and len(entries) == 4 * steps
    real = entries[entries >= 0].astype(np.int64)
    assert len(np.unique(real)) == len(real) and (real < n * per_img).all()
    listed = np.zeros(n * per_img, bool)
    listed[real] = True
    listed = listed.reshape(n, R // 4, R // 16)
    assert in_strip.any(axis=3)[listed].all(), "a listed strip holds no block of B_k"
    assert not in_strip[~listed].any(), "a block of B_k lies in no listed strip"
    want_steps = 0
    pos = 0
    for i in range(n):
        c = int(listed[i].sum())
        padded = -(-c // 4) * 4
        run = entries[pos:pos + padded]
        assert (run[:c] // per_img == i).all() and (np.diff(run[:c]) > 0).all(), "entries ascend within their image"
        assert (run[c:] == -1).all() and padded - c < 4, "voids only close an image's last step"
        pos += padded
        want_steps += padded // 4
    assert pos == len(entries) and steps == want_steps
    for s in entries.reshape(-1, 4):                                   # every step is one image's, and never all void
        r = s[s >= 0]
        assert len(r) >= 1 and s[0] >= 0 and len(set((r // per_img).tolist())) == 1


@pytest.mark.parametrize("name", sorted(NS.masks(N, S)))
def test_strip_lists_cover_exactly_the_needed_blocks(name):
    m = NS.masks(N, S)[name]
    model = NS.need_strips_model(m)
    assert len(model["lists"]) == NB.n_lists(S) == 6
    for k in range(6):
        R = S >> NB.LIST_SHIFT[k]
        assert model["need"][k].shape == (N, R, R)
        _check_list(model["need"][k], model["lists"][k], model["steps"][k])
    if name == "empty":
        assert all(c == 0 and len(e) == 0 for e, c in zip(model["lists"], model["steps"]))
    if name == "full":
        for k in range(6):
            R = S >> NB.LIST_SHIFT[k]
            assert model["steps"][k] == N * (R // 4) * (R // 16) // 4 and (model["lists"][k] == np.arange(4 * model["steps"][k])).all()
    if name.startswith("mod"):
        per_image = NS.strips_of(model["need"][0]).reshape(N, -1).sum(axis=1)
        assert (per_image % 4 == int(name[3])).all(), per_image
    if name == "empty_image_between":
        per_image = NS.strips_of(model["need"][0]).reshape(N, -1).sum(axis=1)
        assert per_image[0] > 0 and per_image[1] == 0 and per_image[2] > 0


def test_strips_never_list_more_than_the_tiles_that_hold_them():
    """a strip is a quarter of a 4 x 64 tile and lies inside one 8 x 32 tile: listed strips <= 4 x listed tiles in either geometry,
    and at least the needed blocks / 4"""
    m = NS.masks(N, S)["blob"]
    model = NS.need_strips_model(m)
    for cols in (64, 32):
        tiles = NB.need_blocks_model(m, tile_cols=[cols if (S >> NB.LIST_SHIFT[k]) % cols == 0 else 0 for k in range(6)])
        for k in range(6):
            strips = int((model["lists"][k] >= 0).sum())
            assert strips <= 4 * len(tiles["lists"][k])
            assert 4 * strips >= int(NR.tiles_any(model["need"][k], 4, 4).sum())
