"""Pins tests/_silraster_ref.py -- the numpy restatement the silhouette rasteriser's GPU tests compare with -- to the C oracle
(oracle.render_ref.rasterize_k -> ref_rasterize_k3), which holds at most 16 fragments per pixel: candidate sets, depths and
distances bit for bit wherever a pixel has fewer than 16 candidates, and the K nearest at K = 4, 8, 12 including the pixels
with more candidates than K.  No GPU.

The one corner where the restatement differs from the oracle by definition ("halves first, then the K nearest": the oracle
decides between the halves of a split quadrilateral against its current K-list) needs more than K candidates on a clipped face
at one pixel; the comparison at K < 16 leaves those pixels out and says how many there were."""
import os

import numpy as np
import pytest

import _silraster_ref as SRR
import _silhouette_ref as SIL

NEAR_CAMERA = dict(dist=0.75, elev=[10.0], azim=[35.0], at=(0, 0.10, 0.25))      # tests/test_gpu_silhouette.py's
NT = min(8, os.cpu_count() or 1)


def _view(cow, near):
    from oracle import render_ref as rr
    cam = NEAR_CAMERA if near else dict(dist=2.1, elev=[20.0], azim=[30.0], at=(0, 0.10, 0.25))
    R, T = rr.look_at_view_transform(cam["dist"], cam["elev"], cam["azim"], at=cam["at"])
    return rr.project_verts(cow["verts"], R[0], T[0])


@pytest.mark.parametrize("near", [False, True])
def test_candidates_equal_the_oracle_bit_for_bit(cow, near):
    from oracle import render_ref as rr
    S, sigma = 64, 1e-4
    blur = SIL.blur_radius(sigma)
    ndc = _view(cow, near)
    cand = SRR.candidates(ndc, cow["faces"], S, blur, True, False, True, 0.5)
    p2f, zbuf, _, dists, slots = rr.rasterize_k(ndc, cow["faces"], S, 16, blur, True, NT, z_clip=0.5, return_slots=True)
    few = (cand.count < 16).reshape(S, S)
    assert int(few.sum()) > 0.5 * S * S and int((cand.count > 0).sum()) > 200
    sl, pz, sd = cand.fragments(16)
    assert np.array_equal(sl[few], slots[few])                 # the same records in the same order
    filled = few[..., None] & (sl >= 0)
    assert np.array_equal(pz[filled].view(np.int32), zbuf[filled].view(np.int32))
    assert np.array_equal(sd[filled].view(np.int32), dists[filled].view(np.int32))
    if near:
        assert int((cand.code[sl[filled]] >= 2).sum()) > 20     # fragments on clipped records
        both = (cand.code >= 2) & (cand.code < 8)
        assert both.any()
    for K in (4, 8, 12):
        p2f, zbuf, _, dists, slots = rr.rasterize_k(ndc, cow["faces"], S, K, blur, True, NT, z_clip=0.5, return_slots=True)
        sl, pz, sd = cand.fragments(K)
        over = (cand.count > K).reshape(S, S)
        assert int(over.sum()) > 0
        # the corner: a pixel with more than K candidates of which one lies on a split quadrilateral
        on_half = np.zeros(S * S, bool)
        on_half[cand.pix[(cand.code[cand.slot] >= 2) & (cand.code[cand.slot] < 8)]] = True
        corner = over & on_half.reshape(S, S)
        print(f"near={near} K={K}: {int(over.sum())} pixels with more than K candidates, {int(corner.sum())} in the corner")
        same = ~corner
        assert np.array_equal(sl[same], slots[same])
        filled = same[..., None] & (sl >= 0)
        assert np.array_equal(pz[filled].view(np.int32), zbuf[filled].view(np.int32))
        assert np.array_equal(sd[filled].view(np.int32), dists[filled].view(np.int32))
        ref = SIL.sigmoid_alpha_blend(__import__("torch").from_numpy(dists.astype(np.float64)),
                                      __import__("torch").from_numpy(p2f >= 0), sigma).numpy()
        assert float(np.abs(cand.alpha(K, sigma) - ref)[same].max()) <= 1e-12


def test_deck_has_exactly_n_candidates_per_covered_pixel():
    S, sigma, n = 64, 1e-4, 20
    ndc, faces = SRR.deck(n)
    cand = SRR.candidates(ndc, faces, S, SIL.blur_radius(sigma), True, False, True, 0.5)
    assert set(np.unique(cand.count).tolist()) == {0, n}
    covered = np.nonzero(cand.count)[0]
    assert 500 < covered.size < S * S
    sd = cand.sd.reshape(covered.size, n)
    assert np.array_equal(sd, np.repeat(sd[:, :1], n, axis=1))                 # the same d on every copy
    assert np.array_equal(cand.slot.reshape(covered.size, n), np.tile(2 * np.arange(n), (covered.size, 1)))    # depth order
    p = 1.0 / (1.0 + np.exp(sd[:, 0].astype(np.float64) / sigma))
    for K in (1, 8, 12, 20, 50):
        closed = 1.0 - (1.0 - p) ** min(K, n)
        assert float(np.abs(cand.alpha(K, sigma).reshape(-1)[covered] - closed).max()) <= 1e-12
    assert float(np.abs(cand.alpha(50, sigma) - cand.alpha(8, sigma)).max()) > 1e-3
