"""Hand-made fragments for the scatter tile tests (tests/test_gpu_scatter_tiles.py): S = 40 (three 16-pixel tiles
per side, the last one ragged), three views --
    view 0  no face anywhere: every tile is empty
    view 1  one covered pixel, (y, x) = (16, 31): a corner of tile (1, 1), every other tile empty
    view 2  covered everywhere by a two-triangle quad whose UVs span [0.03, 0.97]^2, so no footprint is clamped: at T = 1024
            neighbouring pixels are ~24 texels apart and the 4 x 256 corners of a full tile are all distinct, at T = 4 every
            deposit of the view lands on 16 texels
Every float comes from integer hashing (no random generator: the arrays recorded under tests/golden/ stay valid whatever
numpy ships), in float32 steps that are exact.

variants() runs the same scene through every K = 1 shading entry point and the K = 1 case of the soft one: the cases
tools/record_scatter_parent.py records and the tests replay.  Changing anything below changes what the recorded bits mean."""
import hashlib

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


# ------------------------------------------------------------------------------------------------ the variants
SS_A = 2                  # supersampling factor of the ss cases: the S = 40 fragments shade a 20-pixel image
VARIANT_TEX = (4, 64)
MIP = ((64, 3), (4, 2))   # (T, L) of the mip cases
AMBIENT = 0.5             # material x light colour of the lit case: the lighting factor is not 1


def grad_rgb_ss():
    n = S // SS_A
    return (hash01(B * 3 * n * n, 5) - np.float32(0.5)).reshape(B, 3, n, n)


def lod_plane(L):
    """multiples of 1/64 over [0, 2], about one pixel in 64 on each of 0 and 1 and one in nine clamped to 2: whole numbers
    (t == 0: one level alone) and fractions (two levels); cut at L - 1"""
    lam = np.minimum(np.floor(hash01(B * S * S, 6) * np.float32(144.0)) / np.float32(64.0), np.float32(2.0))
    return np.minimum(lam, np.float32(L - 1)).astype(np.float32).reshape(B, S, S)


def colours(V):
    return hash01(V * 3, 7).reshape(V, 3)


def own_faces():
    """-> (p2f, faces): every covered pixel has a face of its own with three vertices of its own (V = 3 S^2): a full tile
    deposits into 768 distinct vertices, the vertex table's worst case"""
    p2f = fragments()[0]
    own = np.arange(S * S, dtype=np.int32).reshape(S, S)
    p2f = np.where(p2f >= 0, own[None], -1).astype(np.int32)
    faces = np.arange(3 * S * S, dtype=np.int32).reshape(S * S, 3)
    return p2f, faces


def digest(a):
    """(number of non-zero 32-bit patterns, SHA-256 of the bytes) of a float32 array: 32 bytes stand for every bit of it"""
    raw = np.ascontiguousarray(a, np.float32)
    return np.int64(np.count_nonzero(raw.view(np.uint32))), np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), np.uint8)


class _Lit:
    """what st3d.ops.shade_lit_* read of a lit setup: ambient light only, so no vertices and no normals"""

    def __init__(self, torch, dev):
        block = np.zeros((1, 24), np.float32)
        block[0, 0:3] = AMBIENT           # the light's ambient colour
        block[0, 12:15] = 1.0             # the material's ambient colour
        self.block, self.kind, self.weight_bound = torch.from_numpy(block).to(dev), 0, AMBIENT
        self.verts = self.normals = None
        self.faces_i32 = torch.from_numpy(FACES_UVS).to(dev)
        self.R = torch.eye(3, device=dev).repeat(B, 1, 1).contiguous()
        self.T = torch.zeros((B, 3), device=dev)


def variants(ops, dev):
    """-> {name: float32 array}: every recorded output of the scene, fixed point on.  Uses only st3d.ops calls."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    frag_np = fragments()
    frag = tuple(t(a) for a in frag_np)
    uvs, fuv, g, g_ss = t(VERTS_UVS), t(FACES_UVS), t(grad_rgb()), t(grad_rgb_ss())
    tex = {T: t(texture(T)) for T in VARIANT_TEX}
    out = {}

    def put(name, *pairs):
        for key, val in pairs:
            out["%s.%s" % (name, key)] = val.detach().cpu().numpy()

    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        rgb, m = ops.shade_fwd(frag, uvs, fuv, tex[64])
        put("fwd", ("rgb", rgb), ("mask", m))
        rgb, m = ops.shade_ss_fwd(frag, uvs, fuv, tex[64], SS_A)
        put("ss_fwd", ("rgb", rgb), ("coverage", m))
        for T in VARIANT_TEX:
            gt, gb = ops.shade_ss_bwd(g_ss, frag, uvs, fuv, tex[T], SS_A, want_bary=True)
            put("ss_bwd_T%d" % T, ("grad_texture", gt), ("grad_bary", gb))
        gt, gb, _ = ops.shade_lit_bwd(g, frag, uvs, fuv, tex[64], _Lit(torch, dev), want_texture=True, want_geometry=True)
        put("lit_bwd", ("grad_texture", gt), ("grad_bary", gb))
        for T, L in MIP:
            pyr, lod = ops.mip_build(tex[T], L), t(lod_plane(L))
            if T == 64:
                rgb, m = ops.shade_mip_fwd(frag, uvs, fuv, pyr, lod, T, L)
                put("mip_fwd", ("rgb", rgb), ("mask", m))
            gt, gb = ops.shade_mip_bwd(g, frag, uvs, fuv, pyr, lod, T, L, want_bary=True)
            put("mip_bwd_T%d" % T, ("grad_texture", gt), ("grad_bary", gb))
        faces, col = t(FACES_UVS), t(colours(4))
        rgb, m = ops.shade_vc_fwd(frag, faces, col)
        put("vc_fwd", ("rgb", rgb), ("mask", m))
        gc, gb = ops.shade_vc_bwd(g, frag, faces, col, want_bary=True)
        put("vc_bwd_shared", ("grad_colors", gc), ("grad_bary", gb))
        p2f_own, faces_own = own_faces()
        gc, gb = ops.shade_vc_bwd(g, (t(p2f_own),) + frag[1:], t(faces_own), t(colours(3 * S * S)), want_bary=True)
        put("vc_bwd_own", ("grad_colors", gc), ("grad_bary", gb))
        soft = (frag[0][..., None].contiguous(), frag[1][..., None].contiguous(), frag[2][..., None, :].contiguous(),
                frag[3][..., None].contiguous())
        rgb, alpha = ops.shade_soft_fwd(soft, uvs, fuv, tex[64])
        put("soft_fwd", ("rgb", rgb), ("alpha", alpha))
        gt, _ = ops.shade_soft_bwd(g, soft, uvs, fuv, tex[64], want_geometry=False)
        put("soft_bwd", ("grad_texture", gt))
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    return out
