"""Coverage-driven view selection: which texels of the map each candidate view touches, as bit masks, and a greedy
choice of the n views that together touch the most.

The loss reaches a texel only through the pixels of the run's views, and the run's views are drawn once.  Instead of taking
the first n random directions, draw a few dozen candidates, mark the texels each would move (the texels to which shade_bwd of
a positive gradient adds a non-zero weight, at the plain bilinear footprint), and pick greedily:

    cams, report = select_cameras(mesh, candidates, n, image_size)

A mask is W = words(T) int32 words per view; texel (row r, column x) of the map as stored is bit (r*T + x) & 31 of word
(r*T + x) >> 5, bits at or above T*T are 0.  Everything is integer work: two runs give the same bits, and tests/_coverref.py
restates it in numpy.  The device wrappers of csrc/cover.hip live here: mark_texels, greedy_views, coverage_counts.
"""
import torch

from . import _lib, ops
from . import render as _render
from ._lib import call, dptr, stream_ptr

F32, I32 = torch.float32, torch.int32
MAX_CANDIDATES = 4096
MAX_SIDE = 16384


def words(T):
    """32-bit words of one view's mask over a T x T map"""
    T = int(T)
    if not 1 <= T <= MAX_SIDE:
        raise ValueError(f"the texture side must be in 1...{MAX_SIDE}, got {T}")
    return (T * T + 31) // 32


def _check_masks(masks, T=None):
    if not torch.is_tensor(masks) or masks.dim() != 2 or masks.dtype != I32 or masks.shape[0] < 1 or masks.shape[1] < 1:
        raise ValueError("masks must be a (C, W) int32 tensor with C >= 1 and W >= 1")
    if T is not None and masks.shape[1] != words(T):
        raise ValueError(f"masks of a {T} x {T} map hold {words(T)} words per view, got {masks.shape[1]}")
    return int(masks.shape[0]), int(masks.shape[1])


def unpack(masks, T):
    """masks (C, W) int32 -> bool (C, T, T): [c, r, x] = view c touches texel (row r, column x).  Plain torch, any device."""
    C, W = _check_masks(masks, T)
    bits = (masks[:, :, None] >> torch.arange(32, dtype=I32, device=masks.device)) & 1
    return bits.reshape(C, W * 32)[:, :T * T].reshape(C, T, T).bool()


def mark_texels(frag, verts_uvs, faces_uvs_i32, T, masks=None):
    """The hard K = 1 fragments of ops.raster_fwd (B views at side S) -> masks (B, words(T)) int32 with the texels each view
    touches ORed in.  masks: a (B, W) tensor to OR into (bits already set stay), None = a fresh one of zeros.  verts_uvs
    (VT,2) float32, faces_uvs_i32 (F,3) int32 indexing it; the fragments' faces index faces_uvs_i32."""
    p2f, _, bary, _ = frag
    B, S = int(p2f.shape[0]), int(p2f.shape[1])
    W = words(T)
    if masks is None:
        masks = torch.zeros((B, W), dtype=I32, device=p2f.device)
    elif tuple(masks.shape) != (B, W) or masks.dtype != I32:
        raise ValueError(f"masks must be ({B}, {W}) int32, got {tuple(masks.shape)} {masks.dtype}")
    call("st3d_cover_mark", dptr(p2f, I32), dptr(bary, F32), dptr(verts_uvs, F32), dptr(faces_uvs_i32, I32), B, S, int(T),
         dptr(masks, I32), stream_ptr())
    return masks


def greedy_views(masks, n, covered=None):
    """n greedy rounds over masks (C, W), C <= 4096: each picks the view not yet taken that adds the most texels to `covered`,
    the lowest index among equals (a taken view is never picked again, so once nothing adds anything the picks go on in
    index order with gain 0).  covered (W,) int32: texels counted as seen before the first round (None = none); it is not
    modified.  -> (picks (n,) int32, gains (n,) int32, covered (W,) int32 = the input's union with the picked rows).  The
    rounds are enqueued without a host read in between."""
    C, W = _check_masks(masks)
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= C:
        raise ValueError(f"n must be an integer in 1...C = {C}, got {n!r}")
    if C > MAX_CANDIDATES:
        raise ValueError(f"at most {MAX_CANDIDATES} candidates, got {C}")
    dev = masks.device
    out = torch.zeros((W,), dtype=I32, device=dev)
    if covered is not None:
        if tuple(covered.shape) != (W,) or covered.dtype != I32:
            raise ValueError(f"covered must be ({W},) int32, got {tuple(covered.shape)} {covered.dtype}")
        out.copy_(covered)
    picks = torch.empty((int(n),), dtype=I32, device=dev)
    gains = torch.empty((int(n),), dtype=I32, device=dev)
    ws = torch.empty((_lib.load().st3d_cover_workspace_bytes(C) // 4,), dtype=I32, device=dev)
    call("st3d_cover_greedy", dptr(masks, I32), C, W, int(n), dptr(out), dptr(picks), dptr(gains), dptr(ws), stream_ptr())
    return picks, gains, out


def coverage_counts(masks, T):
    """masks (C, words(T)) -> (T, T) int32: how many of the C views touch each texel"""
    C, W = _check_masks(masks, T)
    counts = torch.empty((T, T), dtype=I32, device=masks.device)
    call("st3d_cover_count", dptr(masks, I32), C, W, int(T), dptr(counts), stream_ptr())
    return counts


def texel_masks(meshes, R, T, image_size, batch=8):
    """The masks of the views (R (C,3,3), T (C,3)) of a UV-textured mesh -> (C, words(side)) int32, side the map's.  The
    views are rasterised `batch` at a time on the hard K = 1 path at image_size and marked with the plain footprint, whatever
    the run's supersampling or mip-mapping.  A TexturesVertex or TexturesAtlas mesh has no map: NotImplementedError."""
    tex = meshes.textures
    if not isinstance(tex, _render.TexturesUV):
        raise NotImplementedError(f"texel coverage needs a TexturesUV mesh (a texture map to cover), got {type(tex).__name__}")
    if isinstance(batch, bool) or int(batch) != batch or batch < 1:
        raise ValueError(f"batch must be an integer >= 1, got {batch!r}")
    S = int(image_size)
    if not 1 <= S <= 4096:
        raise ValueError(f"image_size must be in 1...4096, got {image_size!r}")
    maps = tex.maps_padded()
    side = int(maps.shape[-2])
    if maps.shape[-3] != side:
        raise NotImplementedError("square texture maps only (the reference resizes to size x size)")
    W = words(side)
    dev = meshes.device
    R, T = R.to(dev, F32).reshape(-1, 3, 3).contiguous(), T.to(dev, F32).reshape(-1, 3).contiguous()
    C = int(R.shape[0])
    if C < 1 or T.shape[0] != C:
        raise ValueError(f"R and T must hold the same number (>= 1) of views, got {tuple(R.shape)} and {tuple(T.shape)}")
    verts = meshes.verts_packed().detach().to(F32).contiguous()
    if _render.reaches_near_plane(verts, R, T, _render.RasterizationSettings.Z_CLIP_DEFAULT):
        raise NotImplementedError("a candidate view has the mesh at its near clipping plane: texel coverage is marked from "
                                  "the hard K = 1 fragments, which do not clip")
    faces_i32, fuv_i32 = meshes.faces_i32(), tex.faces_uvs_i32()
    uvs = tex.verts_uvs_padded().detach().to(F32).reshape(-1, 2).contiguous()
    masks = torch.zeros((C, W), dtype=I32, device=dev)
    for lo in range(0, C, int(batch)):
        hi = min(lo + int(batch), C)
        ndc = ops.project_verts(verts, R[lo:hi], T[lo:hi])
        mark_texels(ops.raster_fwd(ndc, faces_i32, S), uvs, fuv_i32, side, masks[lo:hi])
    return masks


def _reached(masks, T):
    """how many texels any row of masks touches, as a device scalar"""
    return (coverage_counts(masks, T) > 0).sum()


def select_cameras(meshes, cameras, n, image_size):
    """The n of the candidate `cameras` that greedy_views picks on the loaded mesh, in pick order -> (cameras, report).
    report: {"candidates": C, "pool": texels the candidates reach together, "picked": texels the n picks reach, "first_n":
    texels the first n candidates reach, "picks": [n indices], "gains": [n gains], "counts": (side, side) int32, how many of
    the picks touch each texel}.  One host read, at the end."""
    R, T = _render.join_cameras(cameras)
    masks = texel_masks(meshes, R, T, image_size)
    side = int(meshes.textures.maps_padded().shape[-2])
    picks, gains, _ = greedy_views(masks, n)
    index = picks.long()
    counts = coverage_counts(masks[index].contiguous(), side)
    figures = torch.stack([_reached(masks, side), (counts > 0).sum(), _reached(masks[:int(n)].contiguous(), side)]).cpu()
    report = {"candidates": int(masks.shape[0]), "pool": int(figures[0]), "picked": int(figures[1]), "first_n": int(figures[2]),
              "picks": [int(p) for p in picks.cpu()], "gains": [int(g) for g in gains.cpu()], "counts": counts}
    chosen = _render.FoVPerspectiveCameras(R=R.to(index.device)[index], T=T.to(index.device)[index], device=R.device)
    return chosen, report
