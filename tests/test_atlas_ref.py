"""The per-face texel atlas on the CPU: the C ABI's st3d_atlas_texel_index (the function the kernels call, csrc/atlas.h)
against the numpy restatement (tests/_atlasref.py), the restatement's index against the geometry of
st3d.io.atlas_to_triangle_soup, the soup itself, and the restatement's forward and backward."""
import ctypes

import numpy as np
import pytest
import torch

import _atlasref as AR

F32, F64 = np.float32, np.float64
ALL_R = list(range(1, 10)) + [16, 64]


def _c_index(b0, b1, R):
    from st3d import _lib
    lib = _lib.load()
    wy, wx = ctypes.c_int(-7), ctypes.c_int(-7)
    out = np.empty((len(b0), 2), np.int64)
    for n, (p, q) in enumerate(zip(b0, b1)):
        assert lib.st3d_atlas_texel_index(float(p), float(q), R, ctypes.byref(wy), ctypes.byref(wx)) == 0
        out[n] = (wy.value, wx.value)
    return out[:, 0], out[:, 1]


# ------------------------------------------------------------------ 1. the index
@pytest.mark.parametrize("R", ALL_R)
def test_c_index_is_the_restatement_on_texel_centres(R):
    b0, b1 = AR.texel_centres(R)
    b0, b1 = b0.astype(F32).reshape(-1), b1.astype(F32).reshape(-1)
    wy, wx = AR.texel_index(b0, b1, R)
    cy, cx = _c_index(b0, b1, R)
    assert np.array_equal(wy, cy) and np.array_equal(wx, cx)
    y, x = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    assert np.array_equal(wy, y.reshape(-1)) and np.array_equal(wx, x.reshape(-1))       # every centre maps back to its texel


@pytest.mark.parametrize("R", ALL_R)
def test_c_index_on_corners_midpoints_and_non_finite_values(R):
    nan, inf = float("nan"), float("inf")
    special = [nan, inf, -inf, 1e30, -1e30, -1e-7, 1.0 + 1e-7]
    pts = [(1, 0), (0, 1), (0, 0), (0.5, 0.5), (0.5, 0), (0, 0.5)]
    pts += [(a, b) for a in special for b in special] + [(a, 0.25) for a in special] + [(0.25, a) for a in special]
    b0, b1 = np.array([p[0] for p in pts], F32), np.array([p[1] for p in pts], F32)
    wy, wx = AR.texel_index(b0, b1, R)
    cy, cx = _c_index(b0, b1, R)
    assert np.array_equal(wy, cy) and np.array_equal(wx, cx)
    for a in (wy, wx, cy, cx):
        assert a.min() >= 0 and a.max() <= R - 1
    from st3d import _lib
    lib = _lib.load()
    wyc, wxc = ctypes.c_int(), ctypes.c_int()
    for bad in (0, -1, 65, 1 << 20):
        assert lib.st3d_atlas_texel_index(0.2, 0.2, bad, ctypes.byref(wyc), ctypes.byref(wxc)) == -1
    assert lib.st3d_atlas_texel_index(0.2, 0.2, R, None, ctypes.byref(wxc)) == -1
    assert lib.st3d_atlas_texel_index(0.2, 0.2, R, ctypes.byref(wyc), None) == -1


def _interior_points(n, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    return u.astype(F32), v.astype(F32)


@pytest.mark.parametrize("R", [1, 3, 8])
def test_index_is_the_sub_triangle_that_contains_the_point(R):
    """independent of the index arithmetic: the texel of a point is the one whose sub-triangle of atlas_to_triangle_soup
    contains it (point-in-triangle in fp64); points within 1e-6 of a sub-triangle edge are left out"""
    from st3d import io
    # the unit triangle with p0 = (1,0), p1 = (0,1), p2 = (0,0): a point's position is its (b0, b1)
    verts = torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=torch.float64)
    sv, sf, _ = io.atlas_to_triangle_soup(verts, torch.tensor([[0, 1, 2]]), torch.zeros(1, R, R, 3))
    tri = sv[sf].numpy()[:, :, :2]                                        # (R^2, 3, 2)
    b0, b1 = _interior_points(20000, 11 + R)
    p = np.stack([b0.astype(F64), b1.astype(F64)], -1)                    # (n,2)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]

    def edge(o, d):           # signed distance of p from the line o -> d, positive on the left
        e = d - o
        return (e[..., 0] * (p[:, None, 1] - o[..., 1]) - e[..., 1] * (p[:, None, 0] - o[..., 0])) / np.linalg.norm(e, axis=-1)
    dist = np.stack([edge(a, b), edge(b, c), edge(c, a)], -1)             # (n, R^2, 3)
    inside = (dist > 0).all(-1)
    near = (np.abs(dist).min(-1) < 1e-6).any(-1)                          # near an edge of ANY sub-triangle
    keep = ~near
    assert (inside[keep].sum(-1) == 1).all()
    assert near.mean() < 0.01
    wy, wx = AR.texel_index(b0, b1, R)
    assert np.array_equal(inside[keep].argmax(-1), (wy * R + wx)[keep])
    assert np.unique((wy * R + wx)[keep]).size == R * R                   # the points reach every texel


# ------------------------------------------------------------------ 2. the soup
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_soup_conserves_area_and_winding(R):
    from st3d import io
    m = AR.cow()
    verts = torch.from_numpy(m["verts"].astype(F64))[:400 * 3].clone()
    faces = torch.from_numpy(m["faces"].astype(np.int64))
    faces = faces[(faces < verts.shape[0]).all(1)][:300]
    nf = faces.shape[0]
    assert nf >= 50
    atlas = torch.from_numpy(AR.atlas(nf, R))
    sv, sf, sc = io.atlas_to_triangle_soup(verts, faces, atlas)
    assert sf.shape == (nf * R * R, 3) and sv.shape == (3 * nf * R * R, 3) and sc.shape == sv.shape and sv.dtype == torch.float64

    def normals(v, f):
        t = v[f]
        return torch.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=1)
    n_parent, n_soup = normals(verts, faces), normals(sv, sf)
    area, area_soup = n_parent.norm(dim=1).sum() / 2, n_soup.norm(dim=1).sum() / 2
    assert abs(float(area_soup - area)) <= 1e-12 * float(area)
    per_face = n_soup.reshape(nf, R * R, 3)
    assert ((per_face * n_parent[:, None]).sum(-1) > 0).all()             # every sub-triangle points with its parent
    assert torch.allclose(per_face.sum(1), n_parent, rtol=1e-10, atol=0)
    # sub-triangle (f R + y) R + x carries texel [f][y][x] on all three of its vertices
    assert torch.equal(sc.reshape(nf, R, R, 3, 3), atlas[:, :, :, None, :].expand(-1, -1, -1, 3, -1))
    with pytest.raises(ValueError):
        io.atlas_to_triangle_soup(verts, faces[:-1], atlas)


# ------------------------------------------------------------------ 3. the restatement
@pytest.fixture(scope="module")
def frags():
    from _vcolref import oracle_fragments
    return oracle_fragments(24)[0]


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_restatement_forward(frags, dt, R):
    nf = AR.cow()["faces"].shape[0]
    for fr in frags:
        cov = fr[0] >= 0
        assert 40 <= cov.sum() < cov.size
        rgb, mask = AR.shade_fwd(fr, AR.atlas(nf, R), dt)
        assert rgb.dtype == dt and (rgb[:, ~cov] == 1).all() and (mask[0, ~cov] == 0).all() and (mask[0, cov] == 1).all()
        colour = np.array([0.25, 0.5, 0.8125], F32)
        flat, _ = AR.shade_fwd(fr, np.broadcast_to(colour, (nf, R, R, 3)), dt)
        assert np.abs(flat[:, cov] - colour[:, None]).max() <= 1e-6


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_restatement_backward_is_autograd_of_gather_then_blend(frags, dt, R):
    """fp64 autograd of a torch restatement: a gather by the indices, then the blend"""
    import _vcolref as VC
    nf = AR.cow()["faces"].shape[0]
    g = AR.upstream(24)
    atlas = AR.atlas(nf, R)
    got = np.zeros((nf, R, R, 3), F64)
    want = torch.zeros((nf, R, R, 3), dtype=torch.float64)
    for b, fr in enumerate(frags):
        AR.shade_bwd(g[b], fr, R, nf, dt, got)
        p2f, zbuf, bary, dists = fr
        cov = p2f >= 0
        wy, wx = AR.texel_index(bary[cov][:, 0], bary[cov][:, 1], R)
        _, wnum, delta, denom = VC.blend(dists[cov], zbuf[cov], F64)
        A = torch.from_numpy(atlas.astype(F64)).requires_grad_(True)
        texel = A[torch.from_numpy(p2f[cov].astype(np.int64)), torch.from_numpy(wy), torch.from_numpy(wx)]       # (n,3)
        rgb = (torch.from_numpy(wnum)[:, None] * texel + torch.from_numpy(delta)[:, None]) / torch.from_numpy(denom)[:, None]
        (rgb * torch.from_numpy(g[b][:, cov].T.astype(F64))).sum().backward()
        want += A.grad
    want = want.numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print(f"R={R} {dt.__name__}: relative {err:.3e}")
    assert scale > 0
    if dt is F64:
        assert err <= 1e-12
    else:       # k, g k and the deposit's own rounding: at most 3 fp32 roundings on every deposit, summed exactly
        total = np.zeros((nf, R, R, 3), F64)
        for b, fr in enumerate(frags):
            AR.shade_bwd(np.abs(g[b]), fr, R, nf, F64, total)
        assert (np.abs(got - want) <= 3 * 2.0 ** -24 * total * (1 + 1e-6)).all()
    assert np.array_equal(got != 0, want != 0)
