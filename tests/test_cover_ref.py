"""The numpy restatement of the texel coverage (tests/_coverref.py) pinned on the CPU, before any GPU test relies on it: its
marks are exactly the texels the C oracle's shade_bwd of an all-ones gradient writes a non-zero sum to, its greedy rule gives
the figures of the coverage study on the cow, and hand-made masks settle ties, duplicates, empty rows and n = C.  No GPU."""
import functools

import numpy as np
import pytest

import _coverref as CR
import _scenes


@functools.lru_cache(maxsize=None)
def _cow():
    return _scenes.load_asset("cow")


@functools.lru_cache(maxsize=None)
def _frags(S, C, seed=0):
    """the oracle's hard fragments of the cow through random_cameras(C, seed) at side S, computed once per (S, C)"""
    from oracle import render_ref as rr
    cow = _cow()
    R, T = _scenes.random_cameras(C, seed)
    return tuple(rr.rasterize(rr.project_verts(cow["verts"], R[b], T[b]), cow["faces"], S, 0.0, 4) for b in range(C))


def _oracle_touched(frag, T):
    """(T,T) bool: texels with a non-zero accumulated weight under shade_bwd of an all-ones gradient"""
    from oracle import render_ref as rr
    cow = _cow()
    S = frag[0].shape[0]
    acc = rr.shade_bwd(np.ones((3, S, S), np.float32), frag, cow["verts_uvs"], cow["faces_uvs"], np.zeros((T, T, 3), np.float32))
    return (acc != 0).any(-1)


@pytest.mark.parametrize("S", [16, 17, 32])
@pytest.mark.parametrize("T", [8, 31, 32, 33])
def test_marks_are_the_texels_shade_bwd_of_ones_reaches(S, T):
    cow = _cow()
    for frag in _frags(S, 3):
        want = _oracle_touched(frag, T)
        got = CR.touched(frag, cow["verts_uvs"], cow["faces_uvs"], T)
        assert want.any() and np.array_equal(got, want)
    masks = CR.mark(_frags(S, 3), cow["verts_uvs"], cow["faces_uvs"], T)
    assert masks.shape == (3, CR.words(T)) and masks.dtype == np.int32
    if T * T % 32:
        assert not (CR.as_u32(masks)[:, -1] >> np.uint32(T * T % 32)).any()         # tail bits are zero
    assert np.array_equal(CR.unpack(masks, T), np.stack([_oracle_touched(fr, T) for fr in _frags(S, 3)]))


def test_marks_are_ored_into_given_masks():
    cow = _cow()
    T = 31
    fr = _frags(16, 3)
    first = CR.mark(fr[:1], cow["verts_uvs"], cow["faces_uvs"], T)
    both = CR.mark(fr[1:2], cow["verts_uvs"], cow["faces_uvs"], T, masks=first)
    assert np.array_equal(CR.unpack(both, T)[0], _oracle_touched(fr[0], T) | _oracle_touched(fr[1], T))


def test_greedy_on_the_cow_gives_the_figures_of_the_study():
    """cow, 24 candidates of seed 0, S = T = 32: greedy 675 / 690 texels at n = 6 / 8 against 552 / 647 for the first n"""
    cow = _cow()
    T = 32
    masks = CR.mark(_frags(32, 24), cow["verts_uvs"], cow["faces_uvs"], T)
    assert CR.reached(masks) == 716
    picks, gains, covered = CR.greedy(masks, 8)
    assert list(gains[:4]) == [325, 179, 84, 48]
    assert len(set(picks.tolist())) == 8
    for n, want_greedy, want_first in ((6, 675, 552), (8, 690, 647)):
        p, g, cov = CR.greedy(masks, n)
        assert np.array_equal(p, picks[:n]) and np.array_equal(g, gains[:n])        # a prefix: the rounds do not look ahead
        assert CR.popcount(cov) == int(g.sum()) == CR.reached(masks[p]) == want_greedy
        assert CR.reached(masks[:n]) == want_first and want_greedy > want_first
    assert np.array_equal(CR.count(masks[picks], T), CR.unpack(masks[picks], T).sum(0))
    assert (CR.count(masks[picks], T) > 0).sum() == CR.popcount(covered) == 690


def _rows(*rows):
    return CR.as_i32(np.array(rows, np.uint32))


def test_greedy_ties_go_to_the_lowest_index():
    m = _rows([0b0011, 0], [0b1100, 0], [0b0110, 0])
    p, g, cov = CR.greedy(m, 3)
    assert p.tolist() == [0, 1, 2] and g.tolist() == [2, 2, 0] and CR.as_u32(cov).tolist() == [0b1111, 0]
    m = _rows([1, 0], [0, 0b111], [0b111, 0])
    assert CR.greedy(m, 2)[0].tolist() == [1, 2]


def test_greedy_never_takes_a_row_twice():
    m = _rows([0xFFFFFFFF, 0xF], [0xFFFFFFFF, 0xF], [0, 0], [0xFFFFFFFF, 0xF])          # duplicates and an all-zero row
    p, g, cov = CR.greedy(m, 4)             # n = C: every row is taken once, in index order once nothing adds anything
    assert p.tolist() == [0, 1, 2, 3] and g.tolist() == [36, 0, 0, 0] and CR.popcount(cov) == 36
    p, g, _ = CR.greedy(_rows([0], [0], [0]), 2)
    assert p.tolist() == [0, 1] and g.tolist() == [0, 0]
    p, g, _ = CR.greedy(_rows([7]), 1)
    assert p.tolist() == [0] and g.tolist() == [3]


def test_greedy_counts_only_what_the_initial_cover_lacks():
    m = _rows([0b0111], [0b1000], [0x80000000])
    p, g, cov = CR.greedy(m, 2, covered=_rows([0b0111])[0])
    assert p.tolist() == [1, 2] and g.tolist() == [1, 1] and CR.as_u32(cov).tolist() == [0x8000000F]


def test_pack_and_unpack_are_inverse_and_count_adds_rows():
    rng = np.random.default_rng(3)
    for T in (1, 5, 8, 31, 33):
        t = rng.random((4, T, T)) < 0.4
        m = CR.pack(t)
        assert m.shape == (4, CR.words(T)) and np.array_equal(CR.unpack(m, T), t)
        assert np.array_equal(CR.count(m, T), t.sum(0))
        r, x = T - 1, T // 2                  # the layout: texel (r, x) is bit (r*T + x) & 31 of word (r*T + x) >> 5
        one = np.zeros((1, T, T), bool)
        one[0, r, x] = True
        w = CR.as_u32(CR.pack(one))[0]
        assert w[(r * T + x) >> 5] == np.uint32(1) << np.uint32((r * T + x) & 31) and CR.popcount(w) == 1
