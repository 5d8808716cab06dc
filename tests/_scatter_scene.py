"""Hand-made fragments for the texture-scatter tile tests (tests/test_gpu_scatter_tiles.py): S = 40 (three 16-pixel tiles
per side, the last one ragged), three views --
    view 0  no face anywhere: every tile is empty
    view 1  one covered pixel, (y, x) = (16, 31): a corner of tile (1, 1), every other tile empty
    view 2  covered everywhere by a two-triangle quad whose UVs span [0.03, 0.97]^2, so no footprint is clamped: at T = 1024
            neighbouring pixels are ~24 texels apart and the 4 x 256 corners of a full tile are all distinct, at T = 4 every
            deposit of the view lands on 16 texels
Every float comes from integer hashing (no random generator: the arrays recorded under tests/golden/ stay valid whatever
numpy ships), in float32 steps that are exact."""
import numpy as np

S, B = 40, 3
TEX_SIDES = (4, 64, 1024)
LONE = (1, 16, 31)        # view, y, x

VERTS_UVS = np.array([[0.03, 0.03], [0.97, 0.03], [0.03, 0.97], [0.97, 0.97]], np.float32)
FACES_UVS = np.array([[0, 1, 2], [3, 2, 1]], np.int32)


def hash01(n, salt):
    """n values in [0, 1), multiples of 2^-24: exact in float32"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)
    h = (i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return ((h >> np.uint64(8)).astype(np.float64) / float(1 << 24)).astype(np.float32)


def fragments():
    """-> (p2f (B,S,S) int32, zbuf (B,S,S), bary (B,S,S,3), dists (B,S,S)): the tuple st3d.ops.shade_bwd takes"""
    p2f = np.full((B, S, S), -1, np.int32)
    zbuf = np.full((B, S, S), -1.0, np.float32)
    bary = np.full((B, S, S, 3), -1.0, np.float32)
    dists = np.full((B, S, S), -1.0, np.float32)
    c = (np.arange(S, dtype=np.float32) + np.float32(0.5)) / np.float32(S)
    t, s = np.meshgrid(c, c, indexing="ij")             # t down the rows, s along them
    lower = s + t <= 1.0
    full_bary = np.where(lower[..., None], np.stack([1 - s - t, s, t], -1), np.stack([s + t - 1, 1 - s, 1 - t], -1))
    full_face = np.where(lower, 0, 1).astype(np.int32)
    z = np.float32(1.5) + hash01(S * S, 1).reshape(S, S)
    d = -np.float32(3e-4) * hash01(S * S, 2).reshape(S, S)          # inside the face, some close to its edge (k < 1)
    p2f[2], zbuf[2], bary[2], dists[2] = full_face, z, full_bary.astype(np.float32), d
    v, y, x = LONE
    p2f[v, y, x], zbuf[v, y, x], bary[v, y, x], dists[v, y, x] = full_face[y, x], z[y, x], full_bary[y, x], d[y, x]
    return p2f, zbuf, bary, dists


def grad_rgb():
    return (hash01(B * 3 * S * S, 3) - np.float32(0.5)).reshape(B, 3, S, S)


def texture(T):
    return hash01(T * T * 3, 4 + T).reshape(T, T, 3)


def to_sparse(a):
    """flat indices and the bit patterns of the non-zero entries of a float32 array"""
    flat = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
    idx = np.flatnonzero(flat).astype(np.int32)
    return idx, flat[idx]


def from_sparse(idx, bits, shape):
    flat = np.zeros(int(np.prod(shape)), np.uint32)
    flat[idx] = bits
    return flat.view(np.float32).reshape(shape)
