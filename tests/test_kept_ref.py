"""The kept rule (tests/_keptref.py, restating st3d_kept_build of csrc/need.hip) on the CPU: two images that are equal outside
a cover go through a conv / ReLU / pool chain whose convs have the dependence structure of the kernels (conv1_1 per pixel, the
others per aligned 4x4 block from the block's 6x6 patch), in fp64 on small integers so that every sum is exact.  No element
outside the may-change maps differs, at every launch up to conv3_3; two mutants of the rule fail that; and the lists are
ascending, padded per image and hold every may-change block."""
import numpy as np
import pytest

import _keptref as KR
import _needref as NR
import _needstrips_ref as NS

S, N, C = 64, 2, 2


def _weights(rng):
    cin = [3] + [C] * 6
    return [rng.integers(1, 3, size=(C, c, 3, 3)).astype(np.float64) for c in cin]


def _covers():
    z = lambda: np.zeros((N, S, S), np.uint8)
    out = {"empty": z(), "full": np.ones((N, S, S), np.uint8)}
    b = z()
    b[0, 22:31, 17:29] = 1
    b[1, 40:43, 50:52] = 1
    out["blob"] = b
    e = z()
    e[0, 0, 20:30] = e[0, 30:40, S - 1] = 1        # at the border
    e[1, S - 1, 5] = e[1, 13, 0] = 1
    out["border"] = e
    c = z()
    c[:, 0, 0] = c[:, 0, -1] = c[:, -1, 0] = c[:, -1, -1] = 1
    out["corners"] = c
    p = z()
    p[0, 27, 27] = 1               # the 3x3 window ends on a block edge, the 5x5 one crosses it
    p[1, 36, 33] = 1
    out["pixels"] = p
    return out


def _outside_differs(cover, maps, rng):
    """per launch: how many stored elements differ outside the maps (full resolution, and pooled where the launch pools)"""
    w = _weights(rng)
    a = rng.integers(0, 4, size=(N, 3, S, S)).astype(np.float64)
    b = np.where((cover != 0)[:, None], a + rng.integers(1, 3, size=a.shape), a)
    bad = []
    for k, ((fa, pa), (fb, pb)) in enumerate(zip(KR.chain(a, w), KR.chain(b, w))):
        assert max(fa.max(), fb.max()) < 2.0 ** 52, "the chain left the exact range"
        K = maps[k]
        n = int(((fa != fb) & ~K[:, None]).sum())
        if KR.LIST_POOLS[k]:
            n += int(((pa != pb) & ~NR.pool_or(K)[:, None]).sum())
        bad.append(n)
    return bad


@pytest.mark.parametrize("name", sorted(_covers()))
def test_nothing_outside_the_may_change_maps_differs(name):
    cover = _covers()[name]
    bad = _outside_differs(cover, KR.kept_maps(cover), np.random.default_rng(7))
    assert bad == [0] * 6, (name, bad)


def test_the_maps_are_whole_blocks_and_grow_with_depth():
    for name, cover in _covers().items():
        maps = KR.kept_maps(cover)
        for k, K in enumerate(maps):
            assert K.shape == (N, S >> KR.LIST_SHIFT[k], S >> KR.LIST_SHIFT[k])
            assert np.array_equal(K, NR.expand(NR.tiles_any(K, 4, 4), 4, 4)), (name, k)
        assert not maps[0].any() if name == "empty" else maps[0].any()
        if name == "full":
            assert all(K.all() for K in maps)


@pytest.mark.parametrize("mutant", ["no_dilate", "pixel_pool"])
def test_the_mutants_of_the_rule_fail(mutant):
    failed = []
    for name, cover in _covers().items():
        bad = _outside_differs(cover, KR.kept_maps(cover, mutant=mutant), np.random.default_rng(7))
        if any(bad):
            failed.append(name)
    assert failed, "the mutant passed on every cover"
    assert "empty" not in failed and "full" not in failed


@pytest.mark.parametrize("tile", [None, 64, 32, 16])
def test_the_lists_hold_every_may_change_block(tile):
    S2, n = 128, 3
    for name, cover in KR.covers(n, S2).items():
        cols = [tile] * 6
        if tile == 64:
            cols[3:] = [32] * 3         # (32-pixel rows above conv2_2)
        m = KR.kept_model(cover, tile_cols=cols)
        for k, K in enumerate(m["K"]):
            R = K.shape[1]
            e = np.asarray(m["lists"][k])
            if cols[k] == 16:
                assert len(e) == 4 * m["counts"][k]
                per_img = (R // 4) * (R // 16)
                steps = e.reshape(-1, 4)
                img = np.where(steps >= 0, steps // per_img, -1)
                assert all(len(set(r[r >= 0])) <= 1 for r in img), (name, k, "a step mixes images")
                assert ((steps[:, 1:] >= 0) <= (steps[:, :-1] >= 0)).all(), (name, k, "a void before a strip")
                real = e[e >= 0]
                assert (np.diff(real) > 0).all(), (name, k)
                # padded per image: no image has a whole step of voids, and at most three voids
                for i in range(n):
                    cnt = int(((real // per_img) == i).sum())
                    assert int((img == i).any(axis=1).sum()) == -(-cnt // 4), (name, k, i)
                listed = NS.strip_pixels(e, n, R, R)
            else:
                rows, c = KR.NB.geometry(R, cols[k])
                assert len(e) == m["counts"][k] and (np.diff(e) > 0).all(), (name, k)
                listed = KR.NB.tile_pixels(e, n, R, rows, c)
            assert not (K & ~listed).any(), (name, k, "a may-change block is not listed")
            unit = (4, 16) if cols[k] == 16 else (rows, c)
            assert np.array_equal(NR.tiles_any(listed, *unit), NR.tiles_any(K, *unit)), (name, k, "a listed unit holds no block")


def test_the_covers_reach_every_strip_count_mod_4():
    cv = KR.covers(3, 128)
    for r in (1, 2, 3):
        K3 = KR.kept_maps(cv["mod%d" % r][:1], 4)[3]
        assert int(NS.strips_of(K3).sum()) % 4 == r
