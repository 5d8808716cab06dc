"""The hard rasteriser's two phase-2 variants (csrc/raster.hip): faces in parallel per tile (default: (face, 4x4 block)
items, a 64-bit depth|index key per pixel in LDS) and the per-pixel walk (ST3D_RASTER_WALK=1), at the smallest shapes
that exercise each mechanism.  Every test compares all four outputs BIT FOR BIT (as int32 words: -0.0 is not +0.0, a NaN
is its own payload) with the C oracle, once per variant; the oracle's result is computed once per scene and shared.

Scenes are triangle soups given directly in NDC.  Pixel i has the NDC centre 1 - (2i+1)/S in both axes, so `_ndc` below
turns (fractional) pixel coordinates into NDC and a scene can say which pixels a face's bounding box holds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["faces", "walk"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


@pytest.fixture(params=MODES)
def mode(request, monkeypatch):
    if request.param == "walk":
        monkeypatch.setenv("ST3D_RASTER_WALK", "1")
    else:
        monkeypatch.delenv("ST3D_RASTER_WALK", raising=False)
    return request.param


def _ndc(pix, S):
    return (1.0 - (2.0 * np.asarray(pix, np.float64) + 1.0) / S).astype(np.float32)


def _tri(S, pts, z):
    """One face from three (x, y) pixel coordinates and a depth (scalar or three)."""
    v = np.empty((3, 3), np.float32)
    v[:, :2] = _ndc(pts, S)
    v[:, 2] = z
    return v


def _small(S, rng, n, lo, hi, size, zlo, zhi):
    """n triangles with centres in [lo, hi] pixels and vertices within `size` pixels of them."""
    c = rng.uniform(lo, hi, (n, 1, 2))
    out = np.empty((n, 3, 3), np.float32)
    out[:, :, :2] = _ndc(c + rng.uniform(-size, size, (n, 3, 2)), S)
    out[:, :, 2] = rng.uniform(zlo, zhi, (n, 1)) + rng.uniform(-0.05, 0.05, (n, 3))
    return out


def _soup(tris):
    v = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 3))
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


_REF = {}


def _oracle(name, views, faces, S):
    """Per scene, once: the oracle's (p2f, zbuf, bary, dists) of every view; shared by the variants, never modified."""
    if name not in _REF:
        from oracle import render_ref as rr
        ref = [rr.rasterize(v, faces, S, 0.0, nthreads=8) for v in views]
        for r in ref:
            for a in r:
                a.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _run(dev, ops, views, faces, S):
    ndc = torch.from_numpy(np.stack(views)).to(dev)
    out = ops.raster_fwd(ndc, torch.from_numpy(faces).to(dev), S)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(dev, ops, name, views, faces, S):
    ref = _oracle(name, views, faces, S)
    got = _run(dev, ops, views, faces, S)
    for b in range(len(views)):
        for g, r, what in zip(got, ref[b], ("pix_to_face", "zbuf", "bary", "dists")):
            np.testing.assert_array_equal(_bits(g[b]), _bits(r), err_msg=f"{name} view {b} {what}")
    return got, ref


# ---------------------------------------------------------------------------- scenes
def _scene_chunks():
    """S = 48: 3 x 3 tiles, one bin.  2600 small faces inside the middle tile (pixels 16..31): its list is longer than a
    super-round (2048) -- two super-rounds, six 512-face walks / eleven 256-face chunks.  Three pairs of exact duplicates,
    nearer than everything else: one pair inside one chunk, one across chunks, one across super-rounds."""
    S, F = 48, 2600
    rng = np.random.default_rng(11)
    t = _small(S, rng, F, 18.5, 29.5, 1.6, 1.0, 3.0)
    pairs = [(10, 20), (100, 700), (300, 2300)]
    for (lo, hi), (cx, cy) in zip(pairs, [(19.0, 19.0), (27.0, 19.0), (19.0, 27.0)]):
        t[lo] = t[hi] = _tri(S, [(cx - 1.6, cy - 1.4), (cx + 1.7, cy - 1.2), (cx + 0.1, cy + 1.8)], [0.5, 0.55, 0.6])
    return S, t, pairs


def _scene_overflow():
    """S = 64: one 64 x 64 bin.  9000 tiny faces: the bin's list exceeds its capacity (8194), the bin is marked -1 and its
    sixteen tiles sweep all faces (five super-rounds each)."""
    S, F = 64, 9000
    rng = np.random.default_rng(12)
    return S, _small(S, rng, F, 1.0, 62.0, 1.2, 0.8, 3.0)


def _scene_large():
    """S = 40: partial tiles at the right and bottom.  Two faces cover the whole image (sixteen blocks in every tile),
    twenty small ones in front of them and twenty behind, one face straddling the four tiles around pixel corner (16, 16)."""
    S = 40
    rng = np.random.default_rng(13)
    q = np.array([[-6.3, -5.1], [46.2, -7.4], [47.9, 45.5], [-8.2, 46.6]])
    big = [_tri(S, [q[0], q[1], q[2]], [2.0, 2.2, 1.9]), _tri(S, [q[0], q[2], q[3]], [2.0, 1.9, 2.1])]
    front = _small(S, rng, 20, 2.0, 38.0, 2.5, 0.9, 1.1)
    behind = _small(S, rng, 20, 2.0, 38.0, 2.5, 2.9, 3.1)
    corner = _tri(S, [(12.2, 13.1), (20.3, 14.4), (15.1, 21.2)], 0.8)
    return S, np.concatenate([np.stack(big), front, behind, corner[None]])


def _scene_blocks():
    """S = 48.  Face 0: bounding box = exactly pixel (21, 22).  Face 1: exactly the 16 x 16 tile (2, 0).  Face 2: the 5 x 5
    pixels 14..18 around the tile corner (16, 16): four tiles, one 4x4 block in each.  Face 3 lies behind all of them."""
    S = 48
    t = [_tri(S, [(20.7, 21.7), (21.4, 21.8), (20.9, 22.4)], 1.0),
         _tri(S, [(31.6, -0.4), (47.4, -0.4), (31.6, 15.4)], [1.0, 1.2, 1.4]),
         _tri(S, [(13.6, 13.7), (18.4, 14.2), (15.5, 18.4)], 1.1),
         _tri(S, [(-3.0, -2.0), (52.0, -4.0), (20.0, 55.0)], 2.5)]
    return S, np.stack(t)


def _scene_views():
    """Three views of one 200-face soup: as it is, translated off screen, mirrored.  Face 0 is behind the camera (all
    z < 0), face 1 has depths of both signs."""
    S = 40
    rng = np.random.default_rng(15)
    t = np.concatenate([_small(S, rng, 150, -2.0, 42.0, 3.0, 0.6, 3.0), _small(S, rng, 50, 5.0, 35.0, 12.0, 1.0, 3.0)])
    t[0, :, 2] = [-0.7, -1.1, -0.9]
    t[1, :, 2] = [0.9, -0.4, 1.3]
    v, faces = _soup(t)
    off, mirrored = v.copy(), v.copy()
    off[:, 0] += 5.0
    mirrored[:, 1] = -mirrored[:, 1]
    return S, [v, off, mirrored], faces


# ---------------------------------------------------------------------------- tests
def test_chunks_and_super_rounds_with_duplicates(dev, ops, mode):
    S, t, pairs = _scene_chunks()
    v, faces = _soup(t)
    got, ref = _check(dev, ops, "chunks", [v], faces, S)
    p2f = got[0][0]
    inside = ((ref[0][0][16:32, 16:32] >= 0).sum(), (ref[0][0] >= 0).sum())
    assert inside[0] == inside[1] > 100                     # everything drawn lies in the middle tile
    for lo, hi in pairs:                                    # equal depth: the smaller index wins, wherever the two are listed
        assert (p2f == lo).sum() >= 4 and (p2f == hi).sum() == 0, (lo, hi)


def test_bin_overflow_sweeps_all_faces(dev, ops, mode):
    S, t = _scene_overflow()
    v, faces = _soup(t)
    _, ref = _check(dev, ops, "overflow", [v], faces, S)
    assert (ref[0][0] >= 0).mean() > 0.5


def test_large_faces_and_partial_tiles(dev, ops, mode):
    S, t = _scene_large()
    v, faces = _soup(t)
    _, ref = _check(dev, ops, "large", [v], faces, S)
    p = ref[0][0]
    assert (p >= 0).mean() > 0.95 and (p == 0).sum() > 300 and (p == 1).sum() > 300
    n = t.shape[0]
    assert all((p[ys, xs] == n - 1).any() for ys in (slice(0, 16), slice(16, 32)) for xs in (slice(0, 16), slice(16, 32)))
    assert np.isin(p, np.arange(2, 22)).any() and not np.isin(p, np.arange(22, 42)).any()


def test_blocks_one_pixel_full_tile_and_tile_corner(dev, ops, mode):
    S, t = _scene_blocks()
    v, faces = _soup(t)
    _, ref = _check(dev, ops, "blocks", [v], faces, S)
    p = ref[0][0]
    assert np.argwhere(p == 0).tolist() == [[22, 21]]
    ys, xs = np.nonzero(p == 1)
    assert ys.min() == 0 and ys.max() <= 15 and xs.min() == 32 and xs.max() <= 47 and len(ys) > 100
    ys, xs = np.nonzero(p == 2)
    assert ys.min() < 16 <= ys.max() and xs.min() < 16 <= xs.max() and 14 <= min(ys.min(), xs.min()) and max(ys.max(), xs.max()) <= 18


def test_views_off_screen_view_and_faces_behind_the_camera(dev, ops, mode):
    S, views, faces = _scene_views()
    got, ref = _check(dev, ops, "views", views, faces, S)
    for a in got:
        assert (a[1] == -1).all()
    assert (got[0][0] >= 0).mean() > 0.3 and (got[0][2] >= 0).mean() > 0.3
    assert (got[0] == 0).sum() == 0


@pytest.mark.parametrize("primed", [False, True])
def test_two_calls_are_bitwise_equal(dev, ops, cow, mode, primed):
    from oracle import render_ref as rr
    S, B = 96, 2
    g = torch.Generator().manual_seed(5)
    elev, azim = rr.random_camera_angles(B, lambda k: torch.rand(k, generator=g).numpy())
    R, T = rr.look_at_view_transform(2.10, elev, azim, at=(0, 0.10, 0.25))
    views = [rr.project_verts(cow["verts"], R[b], T[b]) for b in range(B)]
    faces = cow["faces"].astype(np.int32)
    runs = []
    for poison in (-1, 7):
        if primed:      # the caching allocator hands the workspace recycled blocks of 0xFF.. / plausible small integers
            junk = [torch.full((n,), poison, dtype=torch.int32, device=dev) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16)]
            del junk
        runs.append(_check(dev, ops, "cow96", views, faces, S)[0])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(_bits(a), _bits(b))
