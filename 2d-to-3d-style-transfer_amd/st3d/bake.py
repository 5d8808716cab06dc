"""Baking views into the texture map: UV-space back-projection, the closed-form alternative to fitting the map to
a batch of images by gradient descent through the renderer.

Walk the texels, not the pixels: find each texel's point on the surface (texel_surface, once per mesh -- the UVs are static),
project it into every view, test that it is visible there, read the view's colour at that point and blend the views by how
squarely they see it (bake_views, one launch per batch of views).  A gather visits every texel of the chart whatever the
pixel density, so magnified regions get no holes, and there is no optimiser state:

    texture, acc = bake_texture(mesh, images, cameras, image_size)

No float atomics anywhere: two runs give the same bits, and tests/_bakeref.py restates both stages in fp64.  The device
wrappers of csrc/bake.hip live here: texel_surface, bake_views, baked_texture.
"""
import torch

from . import _lib, ops
from . import render as _render
from ._lib import call, dptr, stream_ptr

F32, I32 = torch.float32, torch.int32
MAX_SIDE = 16384
MAX_PAD = 8.0
PAD_DEFAULT = 1.5           # the bilinear footprint of an in-chart sample touches texels < sqrt(2) away from the chart
MODES = {"mean": 0, "best": 1}      # ST3D_BAKE_MEAN, ST3D_BAKE_BEST


def _side(T):
    if isinstance(T, bool) or int(T) != T or not 2 <= T <= MAX_SIDE:
        raise ValueError(f"the texture side must be an integer in 2...{MAX_SIDE}, got {T!r}")
    return int(T)


def _check_surface(t2f, tbary):
    if not torch.is_tensor(t2f) or t2f.dim() != 2 or t2f.dtype != I32 or t2f.shape[0] != t2f.shape[1]:
        raise ValueError("t2f must be a (T, T) int32 tensor")
    side = _side(t2f.shape[0])
    if not torch.is_tensor(tbary) or tuple(tbary.shape) != (side, side, 3) or tbary.dtype != F32:
        raise ValueError(f"tbary must be ({side}, {side}, 3) float32")
    return side


def _check_acc(acc, side):
    if not torch.is_tensor(acc) or tuple(acc.shape) != (side, side, 4) or acc.dtype != F32:
        raise ValueError(f"acc must be ({side}, {side}, 4) float32")


def texel_surface(verts_uvs, faces_uvs_i32, T, pad=PAD_DEFAULT):
    """verts_uvs (VT,2) float32, faces_uvs_i32 (F,3) int32 indexing it -> t2f (T,T) int32, tbary (T,T,3) float32.
    t2f[r, x]: the face whose UV triangle is nearest to texel (row r, column x) of the map as stored, within `pad` texels
    (inside or on the triangle counts as distance 0, either winding; the lowest face among equals), else -1.  tbary: the
    barycentrics of the triangle's closest point, 0 where t2f = -1.  pad in 0...8; 1.5 covers every gutter texel a
    chart-border pixel reads."""
    side = _side(T)
    if not 0.0 <= float(pad) <= MAX_PAD:
        raise ValueError(f"pad must be in 0...{MAX_PAD:g} texels, got {pad!r}")
    if verts_uvs.dim() != 2 or verts_uvs.shape[1] != 2 or verts_uvs.shape[0] < 1:
        raise ValueError(f"verts_uvs must be (VT, 2) with VT >= 1, got {tuple(verts_uvs.shape)}")
    if faces_uvs_i32.dim() != 2 or faces_uvs_i32.shape[1] != 3 or faces_uvs_i32.shape[0] < 1:
        raise ValueError(f"faces_uvs_i32 must be (F, 3) with F >= 1, got {tuple(faces_uvs_i32.shape)}")
    dev = verts_uvs.device
    ws_bytes = _lib.load().st3d_bake_workspace_bytes(side)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    t2f = torch.empty((side, side), dtype=I32, device=dev)
    tbary = torch.empty((side, side, 3), dtype=F32, device=dev)
    call("st3d_bake_surface", dptr(verts_uvs, F32), dptr(faces_uvs_i32, I32), int(verts_uvs.shape[0]),
         int(faces_uvs_i32.shape[0]), side, float(pad), dptr(ws), ws_bytes, dptr(t2f), dptr(tbary), stream_ptr())
    return t2f, tbary


def bake_views(verts, faces_i32, t2f, tbary, R, T, images, p2f, zbuf, mode="mean", power=2.0, min_cos=0.1, depth_tol=0.01,
               acc=None):
    """One launch over the texels for a batch of B views -> acc (Tt,Tt,4) float32: rgb = sum of w x colour, w = sum of weights
    (mode 'mean'), or those of the single view of the largest weight, the earliest among equals (mode 'best').
    verts (V,3) float32, faces_i32 (F,3); t2f, tbary: texel_surface's; R (B,3,3), T (B,3): the views; images (B,3,S,S); p2f,
    zbuf (B,S,S): the hard K = 1 fragments of ops.raster_fwd for these views at side S.  A texel takes part in a view when
    its surface point lies beyond the near plane (zv > 0.5), its nearest pixel is in the image and shows the texel's face or
    one at its depth within depth_tol x zv, and the face is seen at |cos| >= min_cos; the weight is |cos|^power.  acc: an
    earlier result to continue (it is written and returned), None = a fresh one of zeros."""
    side = _check_surface(t2f, tbary)
    if mode not in MODES:
        raise ValueError(f"mode must be 'mean' or 'best', got {mode!r}")
    if not (float(power) >= 0.0 and 0.0 <= float(min_cos) <= 1.0 and float(depth_tol) >= 0.0):
        raise ValueError(f"need power >= 0, min_cos in 0...1 and depth_tol >= 0, got {power!r}, {min_cos!r}, {depth_tol!r}")
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3] or images.shape[0] < 1:
        raise ValueError(f"images must be (B, 3, S, S) with B >= 1, got {tuple(images.shape)}")
    B, S = int(images.shape[0]), int(images.shape[2])
    if not 1 <= S <= 4096:
        raise ValueError(f"the image side must be in 1...4096, got {S}")
    if tuple(p2f.shape) != (B, S, S) or tuple(zbuf.shape) != (B, S, S):
        raise ValueError(f"p2f and zbuf must be ({B}, {S}, {S}), got {tuple(p2f.shape)} and {tuple(zbuf.shape)}")
    if tuple(R.shape) != (B, 3, 3) or tuple(T.shape) != (B, 3):
        raise ValueError(f"R and T must be ({B}, 3, 3) and ({B}, 3), got {tuple(R.shape)} and {tuple(T.shape)}")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces_i32.dim() != 2 or faces_i32.shape[1] != 3:
        raise ValueError(f"verts must be (V, 3) and faces_i32 (F, 3), got {tuple(verts.shape)} and {tuple(faces_i32.shape)}")
    if acc is None:
        acc = torch.zeros((side, side, 4), dtype=F32, device=images.device)
    else:
        _check_acc(acc, side)
    call("st3d_bake_views", dptr(verts, F32), dptr(faces_i32, I32), int(verts.shape[0]), int(faces_i32.shape[0]), dptr(t2f, I32),
         dptr(tbary, F32), side, dptr(R, F32), dptr(T, F32), dptr(images, F32), dptr(p2f, I32), dptr(zbuf, F32), B, S,
         ops.INV_TAN_HALF_FOV, MODES[mode], float(power), float(min_cos), float(depth_tol), dptr(acc, F32), stream_ptr())
    return acc


def baked_texture(acc, fallback):
    """acc (T,T,4) of bake_views, fallback (T,T,3) float32 -> (T,T,3): acc.rgb / acc.w where acc.w > 0, the fallback map bit
    for bit elsewhere"""
    if not torch.is_tensor(acc) or acc.dim() != 3 or acc.shape[0] != acc.shape[1]:
        raise ValueError("acc must be (T, T, 4) float32")
    side = _side(acc.shape[0])
    _check_acc(acc, side)
    if tuple(fallback.shape) != (side, side, 3) or fallback.dtype != F32:
        raise ValueError(f"fallback must be ({side}, {side}, 3) float32, got {tuple(fallback.shape)} {fallback.dtype}")
    out = torch.empty((side, side, 3), dtype=F32, device=acc.device)
    call("st3d_bake_resolve", dptr(acc, F32), dptr(fallback, F32), side, dptr(out), stream_ptr())
    return out


def bake_texture(meshes, images, cameras, image_size, mode="mean", power=2.0, min_cos=0.1, depth_tol=0.01, pad=PAD_DEFAULT,
                 batch=8, surface=None, acc=None):
    """Bake `images` (B,3,S,S), seen through `cameras` (B views) at S = image_size, into the map of a TexturesUV mesh ->
    (texture (T,T,3): the baked colour where a view reached the texel, the mesh's own map elsewhere; acc (T,T,4)).
    The views are rasterised `batch` at a time on the hard K = 1 path at image_size, whatever the run's supersampling or
    mip-mapping.  surface: texel_surface's (t2f, tbary) of this mesh when the caller kept it, None = computed here.  acc
    continues an earlier bake.  A TexturesVertex or TexturesAtlas mesh has no map: NotImplementedError."""
    tex = meshes.textures
    if not isinstance(tex, _render.TexturesUV):
        raise NotImplementedError(f"baking needs a TexturesUV mesh (a texture map to bake into), got {type(tex).__name__}")
    if isinstance(batch, bool) or int(batch) != batch or batch < 1:
        raise ValueError(f"batch must be an integer >= 1, got {batch!r}")
    S = int(image_size)
    if not 1 <= S <= 4096:
        raise ValueError(f"image_size must be in 1...4096, got {image_size!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be 'mean' or 'best', got {mode!r}")
    maps = tex.maps_padded()
    side = int(maps.shape[-2])
    if maps.shape[-3] != side:
        raise NotImplementedError("square texture maps only (the reference resizes to size x size)")
    dev = meshes.device
    R, T = _render.join_cameras(cameras)
    R, T = R.to(dev, F32).reshape(-1, 3, 3).contiguous(), T.to(dev, F32).reshape(-1, 3).contiguous()
    B = int(R.shape[0])
    if B < 1 or T.shape[0] != B:
        raise ValueError(f"R and T must hold the same number (>= 1) of views, got {tuple(R.shape)} and {tuple(T.shape)}")
    if images.dim() != 4 or tuple(images.shape) != (B, 3, S, S):
        raise ValueError(f"images must be ({B}, 3, {S}, {S}): one per camera at image_size, got {tuple(images.shape)}")
    images = images.detach().to(dev, F32).contiguous()
    verts = meshes.verts_packed().detach().to(F32).contiguous()
    if _render.reaches_near_plane(verts, R, T, _render.RasterizationSettings.Z_CLIP_DEFAULT):
        raise NotImplementedError("a view has the mesh at its near clipping plane: the bake tests visibility against the "
                                  "hard K = 1 fragments, which do not clip")
    faces_i32 = meshes.faces_i32()
    if surface is None:
        uvs = tex.verts_uvs_padded().detach().to(F32).reshape(-1, 2).contiguous()
        surface = texel_surface(uvs, tex.faces_uvs_i32(), side, pad)
    t2f, tbary = surface
    for lo in range(0, B, int(batch)):
        hi = min(lo + int(batch), B)
        ndc = ops.project_verts(verts, R[lo:hi], T[lo:hi])
        p2f, zbuf, _, _ = ops.raster_fwd(ndc, faces_i32, S)
        acc = bake_views(verts, faces_i32, t2f, tbary, R[lo:hi], T[lo:hi], images[lo:hi], p2f, zbuf, mode=mode, power=power,
                         min_cos=min_cos, depth_tol=depth_tol, acc=acc)
    fallback = maps.detach().to(F32).reshape(side, side, 3).contiguous()
    return baked_texture(acc, fallback), acc
