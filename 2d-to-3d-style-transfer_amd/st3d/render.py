"""Scene containers, cameras and the differentiable renderer on libst3d.

Host-side mirror of the PyTorch3D objects the reference builds (first_approach.py:104-113,
second_approach.py:98-108, utils.py:6-9,121-170,207-210): thin structs with the same
constructor arguments and accessor names, so the drop-in ``utils.py`` / approach scripts read
like the reference.  Rendering itself is NOT a per-camera Python loop of ~20 small launches as
upstream: all views of a batch go through four HIP launches (project, face setup + tile
raster, fused shade) and the backward is one launch (texture scatter).

The reference's own configuration (blur_radius=0, faces_per_pixel=1, default BlendParams;
first_approach.py:107) runs on the specialised hard kernels.  Any other RasterizationSettings /
BlendParams (K <= 8 faces per pixel, blur_radius > 0, clipped barycentrics, sigma/gamma/background)
runs on the general soft rasteriser + softmax blend (csrc/soft.hip).  Cameras: FoV
perspective with default fov/znear/zfar.

Lights: AmbientLights, PointLights, DirectionalLights (N = 1 or one per view) and Materials, as SoftPhongShader
(phong_shading) lights them, on both kernel families, forward and backward (csrc/phong.h, csrc/lighting.hip):
vertex normals n_v = normalize(sum of (v2 - v1) x (v0 - v1) over v's faces); per fragment N = sum b_i n_i,
P = sum b_i v_i; L = location - P (point) or direction; D = kd Ld relu(n.l); r = -l + 2 (n.l) n,
e = normalize(C - P) with C the camera centre, Sp = ks Ls (relu(e.r) [n.l > 0])^shininess, A = ka La;
colour = (A + D) texel + Sp replaces the texel in the blend.  lights=None means white AmbientLights -- today's unlit
render on the unchanged kernels (PyTorch3D's own default is PointLights(); the one deliberate divergence).  No
gradient flows to lights, materials or cameras (a parameter with requires_grad raises).

Silhouettes: SoftSilhouetteShader (sigmoid_alpha_blend: alpha = 1 - prod_k (1 - sigmoid(-dists_k / sigma))) renders alpha
alone, without a texture, and alpha -- its own and SoftPhongShader's under soft settings -- is differentiable in the
vertices through the signed edge distance (csrc/silhouette.hip); losses.compute_silhouette_loss is the fused loss on it.

Per-vertex colours: a mesh whose textures are a TexturesVertex renders on csrc/vcolor.hip (hard settings, unlit): the colour
is the barycentric interpolation of the three vertex colours of the fragment's face, differentiable in colours and vertices.

Texel atlas: a mesh whose textures are a TexturesAtlas renders on csrc/atlas.hip (hard settings, unlit, supersample 1...4):
the colour is the nearest texel of the R x R block its face owns, differentiable in the atlas alone.
"""
import itertools
import math
import os
from collections import OrderedDict

import torch

from . import ops

# ------------------------------------------------------------------------ containers

_I32_CACHE = {}


def _checked_i32(idx, limit, what):
    """int64 index tensor -> validated contiguous int32 copy, cached on the tensor's identity:
    the reference rebuilds its Meshes every step (second_approach.py:164) from the SAME index
    tensors, and the range check costs a host sync, so it must not be repeated per step.
    (An out-of-range index would fault the GPU inside the raster/shade kernels.)"""
    key = (idx.data_ptr(), tuple(idx.shape), idx._version, int(limit), str(idx.device))
    hit = _I32_CACHE.get(key)
    if hit is None:
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= limit):
            raise ValueError(f"{what} holds indices outside [0, {limit})")
        if len(_I32_CACHE) > 64:
            _I32_CACHE.clear()
        hit = (idx.to(torch.int32).contiguous(), idx)        # keep the source alive: data_ptr stays unique
        _I32_CACHE[key] = hit
    return hit[0]



class TexturesUV:
    """utils.py:208 ``TexturesUV(verts_uvs=..., faces_uvs=..., maps=...)``; maps (1,T,T,3)."""

    def __init__(self, maps, faces_uvs, verts_uvs):
        if isinstance(maps, (list, tuple)):
            maps = torch.stack(list(maps))
        if isinstance(verts_uvs, (list, tuple)):
            verts_uvs = torch.stack(list(verts_uvs))
        if isinstance(faces_uvs, (list, tuple)):
            faces_uvs = torch.stack(list(faces_uvs))
        self._maps = maps if maps.dim() == 4 else maps[None]
        self._verts_uvs = verts_uvs if verts_uvs.dim() == 3 else verts_uvs[None]
        self._faces_uvs = faces_uvs if faces_uvs.dim() == 3 else faces_uvs[None]
        self._faces_uvs_i32 = None

    def maps_padded(self):
        return self._maps

    def verts_uvs_padded(self):
        return self._verts_uvs

    def faces_uvs_padded(self):
        return self._faces_uvs

    def faces_uvs_i32(self):
        if self._faces_uvs_i32 is None:
            self._faces_uvs_i32 = _checked_i32(self._faces_uvs[0], self._verts_uvs.shape[1], "faces_uvs")
        return self._faces_uvs_i32

    def clone(self):
        t = TexturesUV(self._maps.clone(), self._faces_uvs.clone(), self._verts_uvs.clone())
        return t

    def detach(self):
        return TexturesUV(self._maps.detach(), self._faces_uvs, self._verts_uvs.detach())


class TexturesVertex:
    """PyTorch3D ``TexturesVertex(verts_features=...)``: one RGB triple per vertex, interpolated with each fragment's
    barycentrics (csrc/vcolor.hip).  verts_features: (V,3), (1,V,3) or a one-element list of (V,3); indexed by
    the mesh's own faces."""

    def __init__(self, verts_features):
        if isinstance(verts_features, (list, tuple)):
            if len(verts_features) != 1:
                raise ValueError("one mesh per batch: verts_features takes a one-element list")
            verts_features = verts_features[0]
        if verts_features.dim() == 3:
            if verts_features.shape[0] != 1:
                raise ValueError(f"one mesh per batch: verts_features must be (V, 3) or (1, V, 3), got "
                                 f"{tuple(verts_features.shape)}")
            self._padded, self._packed = verts_features, None
        elif verts_features.dim() == 2:
            self._padded, self._packed = None, verts_features
        else:
            raise ValueError(f"verts_features must be (V, 3) or (1, V, 3), got {tuple(verts_features.shape)}")
        if verts_features.shape[-1] != 3:
            raise ValueError(f"verts_features holds RGB triples: the last dimension must be 3, got "
                             f"{tuple(verts_features.shape)}")

    def verts_features_padded(self):
        if self._padded is None:
            self._padded = self._packed[None]
        return self._padded

    def verts_features_packed(self):
        if self._packed is None:
            self._packed = self._padded[0]
        return self._packed

    def clone(self):
        return TexturesVertex(self.verts_features_packed().clone())

    def detach(self):
        return TexturesVertex(self.verts_features_packed().detach())


class TexturesAtlas:
    """PyTorch3D ``TexturesAtlas(atlas=...)``: every face owns an R x R block of RGB texels, addressed by the fragment's
    barycentrics (nearest texel, csrc/atlas.hip) -- no UV chart, no seams.  atlas: (F,R,R,3), (1,F,R,R,3) or a
    one-element list of (F,R,R,3), 1 <= R <= 64, one block per face of the mesh.

    The lookup is piecewise constant in the barycentrics, so NO gradient reaches the vertices through the colour: a render
    of such a mesh is differentiable in the atlas only (``verts.grad`` stays None)."""

    def __init__(self, atlas):
        if isinstance(atlas, (list, tuple)):
            if len(atlas) != 1:
                raise ValueError("one mesh per batch: atlas takes a one-element list")
            atlas = atlas[0]
        if atlas.dim() == 5:
            if atlas.shape[0] != 1:
                raise ValueError(f"one mesh per batch: atlas must be (F, R, R, 3) or (1, F, R, R, 3), got {tuple(atlas.shape)}")
            self._padded, self._packed = atlas, None
        elif atlas.dim() == 4:
            self._padded, self._packed = None, atlas
        else:
            raise ValueError(f"atlas must be (F, R, R, 3) or (1, F, R, R, 3), got {tuple(atlas.shape)}")
        if atlas.shape[-1] != 3:
            raise ValueError(f"atlas holds RGB triples: the last dimension must be 3, got {tuple(atlas.shape)}")
        if atlas.shape[-2] != atlas.shape[-3]:
            raise ValueError(f"atlas blocks are square (F, R, R, 3), got {tuple(atlas.shape)}")
        if not 1 <= atlas.shape[-2] <= ops.ATLAS_MAX_R:
            raise ValueError(f"atlas resolution R must be 1...{ops.ATLAS_MAX_R}, got {atlas.shape[-2]}")

    def atlas_padded(self):
        if self._padded is None:
            self._padded = self._packed[None]
        return self._padded

    def atlas_packed(self):
        if self._packed is None:
            self._packed = self._padded[0]
        return self._packed

    def clone(self):
        return TexturesAtlas(self.atlas_packed().clone())

    def detach(self):
        return TexturesAtlas(self.atlas_packed().detach())


class Meshes:
    """utils.py:209 ``Meshes(verts=[verts], faces=[faces], textures=textures)`` (one mesh)."""

    def __init__(self, verts, faces, textures=None):
        if isinstance(verts, (list, tuple)):
            assert len(verts) == 1, "one mesh per batch (the reference never batches meshes)"
            verts = verts[0]
        if isinstance(faces, (list, tuple)):
            faces = faces[0]
        if verts.dim() == 3:
            assert verts.shape[0] == 1
            self._verts_padded = verts
            self._verts = None
        else:
            self._verts = verts
            self._verts_padded = None
        self._faces = faces[0] if faces.dim() == 3 else faces
        self.textures = textures
        self._faces_i32 = None
        if isinstance(textures, TexturesVertex):
            vertex_colours_of(self)         # one colour per vertex, or a ValueError now rather than at the first render
        if isinstance(textures, TexturesAtlas):
            atlas_of(self)                  # one block per face, likewise

    def verts_packed(self):
        if self._verts is None:
            self._verts = self._verts_padded[0]
        return self._verts

    def verts_padded(self):
        if self._verts_padded is None:
            self._verts_padded = self._verts[None]
        return self._verts_padded

    def faces_packed(self):
        return self._faces

    def faces_padded(self):
        return self._faces[None]

    def faces_i32(self):
        if self._faces_i32 is None:
            self._faces_i32 = _checked_i32(self._faces, self.verts_packed().shape[0], "faces")
        return self._faces_i32

    def clone(self):
        return Meshes(self.verts_packed().clone(), self._faces.clone(),
                      self.textures.clone() if self.textures is not None else None)

    def detach(self):
        return Meshes(self.verts_packed().detach(), self._faces,
                      self.textures.detach() if self.textures is not None else None)

    @property
    def device(self):
        return self.verts_packed().device


def vertex_colours_of(meshes):
    """The (V,3) colours of a mesh whose textures are a TexturesVertex, checked against its vertex count: the kernels index
    the colours with the mesh's own faces, so a shorter array would be read out of bounds on the GPU (ValueError)."""
    col = meshes.textures.verts_features_packed()
    V = meshes.verts_packed().shape[0]
    if col.shape[0] != V:
        raise ValueError(f"TexturesVertex holds {col.shape[0]} colours for a mesh of {V} vertices: verts_features must have "
                         "one row per vertex (it is indexed by the mesh's faces)")
    return col


def atlas_of(meshes):
    """The (F,R,R,3) atlas of a mesh whose textures are a TexturesAtlas, checked against its face count: the kernels index
    the atlas with the rasterised face, so a shorter array would be read out of bounds on the GPU (ValueError)."""
    atlas = meshes.textures.atlas_packed()
    F = meshes.faces_packed().shape[0]
    if atlas.shape[0] != F:
        raise ValueError(f"TexturesAtlas holds {atlas.shape[0]} blocks for a mesh of {F} faces: atlas must have one R x R block "
                         "per face (it is indexed by the rasterised face)")
    return atlas


# ------------------------------------------------------------------------ cameras


class FoVPerspectiveCameras:
    """R (n,3,3), T (n,3) in the row-vector convention X_view = X_world R + T; defaults
    fov=60 deg, znear=1, zfar=100, aspect=1 (the reference never overrides them)."""

    def __init__(self, R=None, T=None, device="cpu", fov=60.0, znear=1.0, zfar=100.0):
        dev = torch.device(device)
        self.R = (torch.eye(3)[None] if R is None else R).to(dev, torch.float32).reshape(-1, 3, 3)
        self.T = (torch.zeros(1, 3) if T is None else T).to(dev, torch.float32).reshape(-1, 3)
        if (fov, znear, zfar) != (60.0, 1.0, 100.0):
            raise NotImplementedError("only the FoVPerspectiveCameras defaults the reference uses are supported")
        self.device = dev

    def __len__(self):
        return self.R.shape[0]

    def __getitem__(self, i):
        if isinstance(i, int):
            i = slice(i, i + 1)
        return FoVPerspectiveCameras(self.R[i], self.T[i], device=self.device)


def join_cameras(cameras):
    """list of cameras (as utils.py:68 iterates) or one batched camera -> (R (B,3,3), T (B,3))."""
    if isinstance(cameras, FoVPerspectiveCameras):
        return cameras.R, cameras.T
    return torch.cat([c.R for c in cameras], 0), torch.cat([c.T for c in cameras], 0)


def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0, at=((0, 0, 0),), up=((0, 1, 0),), device="cpu"):
    """PyTorch3D look_at_view_transform with degrees=True (utils.py:161-166)."""
    def _t(x):
        x = torch.as_tensor(x, dtype=torch.float32)
        return x.reshape(-1) if x.dim() <= 1 else x
    dist, elev, azim = _t(dist), _t(elev) * (math.pi / 180.0), _t(azim) * (math.pi / 180.0)
    at = torch.as_tensor(at, dtype=torch.float32).reshape(-1, 3)
    up = torch.as_tensor(up, dtype=torch.float32).reshape(-1, 3)
    n = max(dist.numel(), elev.numel(), azim.numel(), at.shape[0])
    dist, elev, azim = (t.expand(n) for t in (dist, elev, azim))
    at, up = at.expand(n, 3), up.expand(n, 3)
    x = dist * torch.cos(elev) * torch.sin(azim)
    y = dist * torch.sin(elev)
    z = dist * torch.cos(elev) * torch.cos(azim)
    C = torch.stack([x, y, z], dim=1) + at
    z_axis = torch.nn.functional.normalize(at - C, eps=1e-5)
    x_axis = torch.nn.functional.normalize(torch.cross(up, z_axis, dim=1), eps=1e-5)
    y_axis = torch.nn.functional.normalize(torch.cross(z_axis, x_axis, dim=1), eps=1e-5)
    is_close = torch.isclose(x_axis, torch.tensor(0.0), atol=5e-3).all(dim=1, keepdim=True)
    if is_close.any():
        repl = torch.nn.functional.normalize(torch.cross(y_axis, z_axis, dim=1), eps=1e-5)
        x_axis = torch.where(is_close, repl, x_axis)
    R = torch.cat((x_axis[:, None, :], y_axis[:, None, :], z_axis[:, None, :]), dim=1).transpose(1, 2)
    T = -torch.bmm(R.transpose(1, 2), C[:, :, None])[:, :, 0]
    return R.to(device), T.to(device)


class RotateAxisAngle:
    """utils.py:142 ``RotateAxisAngle(angle, axis=axis).get_matrix()[..., :3, :3]``."""

    def __init__(self, angle, axis="X", degrees=True, device="cpu"):
        a = float(angle) * (math.pi / 180.0 if degrees else 1.0)
        c, s = math.cos(a), math.sin(a)
        if axis == "X":
            m = [[1, 0, 0], [0, c, -s], [0, s, c]]
        elif axis == "Y":
            m = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        elif axis == "Z":
            m = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        else:
            raise ValueError("axis must be X, Y or Z")
        M = torch.eye(4, dtype=torch.float32)
        M[:3, :3] = torch.tensor(m, dtype=torch.float32).t()     # row-vector convention
        self._m = M[None].to(device)

    def get_matrix(self):
        return self._m


# ------------------------------------------------------------------------ renderer


# what a mip-mapped render (texture_mip_levels != 1) refuses, by limitation (NotImplementedError, before any launch)
MIP_REFUSALS = {
    "lights": "texture_mip_levels != 1 is implemented for unlit renders only (lights=None or white AmbientLights with default "
              "Materials): the lit kernels have no mip-mapped sampling",
    "supersample": "texture_mip_levels != 1 cannot be combined with supersample > 1: the supersampled kernels have no mip-mapped "
                   "sampling",
    "soft": "texture_mip_levels != 1 is implemented for the hard settings only (faces_per_pixel = 1, blur_radius = 0, default "
            "clipping, culling and BlendParams): the general soft kernels have no mip-mapped sampling",
    "silhouette": "texture_mip_levels != 1 means nothing to an alpha-only (silhouette) render, which samples no texture: a "
                  "SoftSilhouetteShader takes RasterizationSettings(texture_mip_levels=1)",
}
MIP_NEAR_PLANE_MESSAGE = ("the mesh reaches the near clipping plane (z < znear / 2) under texture_mip_levels != 1: the clipping "
                          "kernels have no mip-mapped sampling, and the render is not silently rerouted to unfiltered sampling "
                          "-- render with texture_mip_levels=1 or keep the mesh in front of the plane")


# what a render of a TexturesVertex mesh refuses, by limitation (NotImplementedError, before any launch)
VERTEX_COLOUR_REFUSALS = {
    "lights": "TexturesVertex is implemented for unlit renders only (lights=None or white AmbientLights with default "
              "Materials): the lit kernels have no vertex-colour path",
    "supersample": "TexturesVertex cannot be combined with supersample > 1: the supersampled kernels have no vertex-colour "
                   "path",
    "mip": "TexturesVertex cannot be combined with texture_mip_levels != 1: there is no texture map to filter",
    "soft": "TexturesVertex is implemented for the hard settings only (faces_per_pixel = 1, blur_radius = 0, default "
            "clipping, culling and BlendParams): the general soft kernels have no vertex-colour path",
    "silhouette": "SilhouetteRasterizationSettings render on the silhouette rasteriser, which produces alpha only: the "
                  "colours of a TexturesVertex mesh need RasterizationSettings and a SoftPhongShader (a "
                  "SoftSilhouetteShader renders the same mesh's alpha)",
}
VERTEX_COLOUR_NEAR_PLANE_MESSAGE = ("the mesh reaches the near clipping plane (z < znear / 2) and its textures are a "
                                    "TexturesVertex: the clipping kernels have no vertex-colour path, and the render is not "
                                    "silently rerouted -- keep the mesh in front of the plane")


# what a render of a TexturesAtlas mesh refuses, by limitation (NotImplementedError, before any launch)
ATLAS_REFUSALS = {
    "lights": "TexturesAtlas is implemented for unlit renders only (lights=None or white AmbientLights with default "
              "Materials): the lit kernels have no atlas path",
    "mip": "TexturesAtlas cannot be combined with texture_mip_levels != 1: the atlas is sampled at its nearest texel and has "
           "no mip chain (supersample is its anti-aliasing)",
    "soft": "TexturesAtlas is implemented for the hard settings only (faces_per_pixel = 1, blur_radius = 0, default "
            "clipping, culling and BlendParams): the general soft kernels have no atlas path",
    "silhouette": "SilhouetteRasterizationSettings render on the silhouette rasteriser, which produces alpha only: the "
                  "colours of a TexturesAtlas mesh need RasterizationSettings and a SoftPhongShader (a "
                  "SoftSilhouetteShader renders the same mesh's alpha)",
}
ATLAS_NEAR_PLANE_MESSAGE = ("the mesh reaches the near clipping plane (z < znear / 2) and its textures are a "
                            "TexturesAtlas: the clipping kernels have no atlas path, and the render is not "
                            "silently rerouted -- keep the mesh in front of the plane")


class RasterizationSettings:
    """PyTorch3D RasterizationSettings: image_size, blur_radius, faces_per_pixel, clip_barycentric_coords
    (None = clip iff blur_radius > 0, the PyTorch3D default), perspective_correct (None = True: every camera here is a
    perspective camera), cull_backfaces.  bin_size / max_faces_per_bin only pick PyTorch3D's binning strategy and are
    accepted and ignored.  Anything but the reference's own values (first_approach.py:107) runs on the general kernels.
    supersample = a in 1..4 (not PyTorch3D's; 1 = off): rasterise and shade at a * image_size, hand out the a x a
    box-filtered image at image_size (PyTorch3D's documented anti-aliasing, render larger then avg_pool2d, without the
    larger image: csrc/shade.hip).  Coverage then is the covered share of the pixel's a^2 sub-pixels.
    texture_mip_levels = L (not PyTorch3D's; 1 = off, 0 = the full chain under the map's side) and texture_lod_bias: sample the
    texture trilinearly from an L-level mip chain at each pixel's own level of detail (csrc/mipmap.hip) -- hard
    settings, unlit, supersample = 1 only.  The levels are checked against the map's side when a render knows it."""
    MAX_FACES_PER_PIXEL = 8

    Z_CLIP_DEFAULT = 0.5        # PyTorch3D MeshRasterizer: z_clip_value None -> znear / 2 for perspective cameras (znear = 1)

    def __init__(self, image_size=256, blur_radius=0.0, faces_per_pixel=1, bin_size=None, max_faces_per_bin=None,
                 perspective_correct=None, clip_barycentric_coords=None, cull_backfaces=False, z_clip_value=None,
                 cull_to_frustum=False, supersample=1, texture_mip_levels=1, texture_lod_bias=0.0, **kw):
        if isinstance(image_size, (tuple, list)):
            if len(image_size) != 2 or image_size[0] != image_size[1]:
                raise NotImplementedError("square images only")
            image_size = image_size[0]
        if not 1 <= int(faces_per_pixel) <= self.MAX_FACES_PER_PIXEL:
            raise NotImplementedError(f"faces_per_pixel must be in 1..{self.MAX_FACES_PER_PIXEL}")
        if blur_radius < 0.0:
            raise ValueError("blur_radius must be >= 0")
        self.image_size, self.blur_radius, self.faces_per_pixel = int(image_size), float(blur_radius), int(faces_per_pixel)
        self.clip_barycentric_coords = (self.blur_radius > 0.0) if clip_barycentric_coords is None \
            else bool(clip_barycentric_coords)
        self.perspective_correct = True if perspective_correct is None else bool(perspective_correct)
        self.cull_backfaces = bool(cull_backfaces)
        if cull_to_frustum:
            raise NotImplementedError("cull_to_frustum=True is not implemented (PyTorch3D's default is False)")
        if z_clip_value is not None and not z_clip_value > 0.0:
            raise ValueError("z_clip_value must be positive")
        # None: PyTorch3D's default plane.  The general kernels clip at it; the specialised K = 1 kernels only WATCH it
        # (st3d.ops.check_near_plane) -- an explicit value sends the render to the general kernels
        self.z_clip_value = None if z_clip_value is None else float(z_clip_value)
        self.supersample = ops.check_supersample(supersample, self.image_size)
        self.texture_mip_levels = ops.check_mip(texture_mip_levels)
        self.texture_lod_bias = ops.check_lod_bias(texture_lod_bias)
        if self.texture_mip_levels != 1 and self.supersample > 1:
            raise NotImplementedError(MIP_REFUSALS["supersample"])

    @property
    def z_clip(self):
        return self.Z_CLIP_DEFAULT if self.z_clip_value is None else self.z_clip_value

    @property
    def is_hard(self):
        return (self.faces_per_pixel == 1 and self.blur_radius == 0.0 and not self.clip_barycentric_coords
                and self.perspective_correct and not self.cull_backfaces and self.z_clip_value is None)


class SilhouetteRasterizationSettings(RasterizationSettings):
    """RasterizationSettings for the silhouette rasteriser (csrc/silraster.hip): faces_per_pixel up to 64 (PyTorch3D's
    silhouette tutorial uses 50), because that rasteriser goes from the faces to alpha without keeping fragments.  Only a
    MeshRenderer with a SoftSilhouetteShader accepts them; every other shader needs each fragment's depth and colour and
    stays at RasterizationSettings' 8."""
    MAX_FACES_PER_PIXEL = 64

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if self.supersample > 1:
            raise NotImplementedError("supersample > 1 is not implemented for alpha-only (silhouette) renders")
        if self.texture_mip_levels != 1:
            raise NotImplementedError(MIP_REFUSALS["silhouette"])


class BlendParams:
    """PyTorch3D BlendParams (sigma, gamma, background_color) for softmax_rgb_blend."""

    def __init__(self, sigma=1e-4, gamma=1e-4, background_color=(1.0, 1.0, 1.0)):
        self.sigma, self.gamma = float(sigma), float(gamma)
        bg = torch.as_tensor(background_color, dtype=torch.float32).reshape(-1).tolist()
        if len(bg) != 3:
            raise ValueError("background_color must have 3 components")
        self.background_color = tuple(bg)
        if self.sigma <= 0.0 or self.gamma <= 0.0:
            raise ValueError("sigma and gamma must be positive")


# ------------------------------------------------------------------------ lights and materials (csrc/phong.h)


def _param(value, what, device):
    """PyTorch3D light / material parameter -> (N,3) float32 tensor on `device`.  No gradient flows to lights or materials:
    a tensor that asks for one is refused instead of silently getting none."""
    if isinstance(value, torch.Tensor) and value.requires_grad:
        raise NotImplementedError(f"{what}: gradients to lights and materials are not implemented (requires_grad=True)")
    t = torch.as_tensor(value, dtype=torch.float32)
    t = t.reshape(1, 3) if t.dim() <= 1 else t
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{what} must have shape (N, 3), got {tuple(t.shape)}")
    return t.to(device)


def _batch(*params):
    """the common N of (N,3) parameters (each N is 1 or that N)"""
    n = max(p.shape[0] for p in params)
    if any(p.shape[0] not in (1, n) for p in params):
        raise ValueError("light / material parameters must all have N = 1 or the same N")
    return n


class AmbientLights:
    """PyTorch3D AmbientLights: ambient_color (N,3), no diffuse or specular light.  White with default Materials is today's
    unlit render (the specialised ambient kernels); any other colour scales the texel per channel."""

    def __init__(self, ambient_color=((1.0, 1.0, 1.0),), device="cpu"):
        self.device = torch.device(device)
        self.ambient_color = _param(ambient_color, "ambient_color", self.device)
        self.diffuse_color = torch.zeros_like(self.ambient_color)
        self.specular_color = torch.zeros_like(self.ambient_color)
        _batch(self.ambient_color)

    def _params(self):
        return (self.ambient_color, self.diffuse_color, self.specular_color, torch.zeros_like(self.ambient_color))


class PointLights:
    """PyTorch3D PointLights (defaults: ambient 0.5, diffuse 0.3, specular 0.2, location (0, 1, 0)); N = 1 or one per view."""
    KIND = 1

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),), location=((0.0, 1.0, 0.0),), device="cpu"):
        self.device = torch.device(device)
        self.ambient_color = _param(ambient_color, "ambient_color", self.device)
        self.diffuse_color = _param(diffuse_color, "diffuse_color", self.device)
        self.specular_color = _param(specular_color, "specular_color", self.device)
        self.location = _param(location, "location", self.device)
        _batch(*self._params())

    def _params(self):
        return (self.ambient_color, self.diffuse_color, self.specular_color, self.location)


class DirectionalLights:
    """PyTorch3D DirectionalLights (same colours as PointLights, direction (0, 1, 0) pointing TOWARDS the light)."""
    KIND = 2

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),), direction=((0.0, 1.0, 0.0),), device="cpu"):
        self.device = torch.device(device)
        self.ambient_color = _param(ambient_color, "ambient_color", self.device)
        self.diffuse_color = _param(diffuse_color, "diffuse_color", self.device)
        self.specular_color = _param(specular_color, "specular_color", self.device)
        self.direction = _param(direction, "direction", self.device)
        _batch(*self._params())

    def _params(self):
        return (self.ambient_color, self.diffuse_color, self.specular_color, self.direction)


class HeadLights(PointLights):
    """A PointLights at every view's own camera centre (the CLIs' --lights headlight): the kernels take the location from
    the view's R and T, so it follows the views through batching and sharding.  Colours as PointLights."""
    KIND = 3

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),), device="cpu"):
        super().__init__(ambient_color, diffuse_color, specular_color, ((0.0, 0.0, 0.0),), device)


class Materials:
    """PyTorch3D Materials (defaults: ambient = diffuse = specular = (1, 1, 1), shininess 64)."""

    def __init__(self, ambient_color=((1.0, 1.0, 1.0),), diffuse_color=((1.0, 1.0, 1.0),),
                 specular_color=((1.0, 1.0, 1.0),), shininess=64, device="cpu"):
        self.device = torch.device(device)
        self.ambient_color = _param(ambient_color, "ambient_color", self.device)
        self.diffuse_color = _param(diffuse_color, "diffuse_color", self.device)
        self.specular_color = _param(specular_color, "specular_color", self.device)
        if isinstance(shininess, torch.Tensor) and shininess.requires_grad:
            raise NotImplementedError("shininess: gradients to lights and materials are not implemented (requires_grad=True)")
        self.shininess = torch.as_tensor(shininess, dtype=torch.float32).reshape(-1).to(self.device)
        _batch(self.ambient_color, self.diffuse_color, self.specular_color, self.shininess[:, None].expand(-1, 3))


_LIGHT_FLOATS = 24          # include/st3d.h: the light block layout
_PACK_CACHE = {}


class Lighting:
    """What the lit kernels need of a (lights, materials) pair: the packed block (n,24) on the device, the kind
    (0 ambient only, 1 point, 2 directional, 3 headlight) and the bound of the lighting factor (A + D) for the fixed-point
    texture scatter."""

    def __init__(self, block, kind, weight_bound):
        self.block, self.kind, self.weight_bound = block, kind, weight_bound

    @property
    def n(self):
        return self.block.shape[0]


def _tensors_of(lights, materials):
    ts = list(lights._params())
    if materials is not None:
        ts += [materials.ambient_color, materials.diffuse_color, materials.specular_color, materials.shininess]
    return ts


def lighting_of(lights, materials, device):
    """(lights, materials) -> None for today's unlit kernels (lights None, or white AmbientLights with absent or default
    Materials: those render bit for bit as before), else a Lighting.  Packed once per object pair and cached on the
    identity and version of its tensors: steady state costs no host work."""
    if lights is None:
        return None
    if not isinstance(lights, (AmbientLights, PointLights, DirectionalLights)):
        raise NotImplementedError(f"{type(lights).__name__} is not implemented (AmbientLights, PointLights, DirectionalLights)")
    ts = _tensors_of(lights, materials)
    if any(t.requires_grad for t in ts):
        raise NotImplementedError("gradients to lights and materials are not implemented (a parameter has requires_grad=True)")
    key = (id(lights), id(materials), tuple((t.data_ptr(), t._version) for t in ts), str(device))
    hit = _PACK_CACHE.get(key)
    if hit is not None:
        return hit[0]
    mat = materials if materials is not None else Materials()
    la, ld, ls, pos = (t.detach().cpu() for t in lights._params())
    ka, kd, ks = (t.detach().cpu() for t in (mat.ambient_color, mat.diffuse_color, mat.specular_color))
    sh = mat.shininess.detach().cpu()[:, None]
    n = _batch(la, ld, ls, pos, ka, kd, ks, sh.expand(-1, 3))
    kind = 0 if isinstance(lights, AmbientLights) else lights.KIND
    if kind == 0 and bool((la == 1).all()) and bool((ka == 1).all()):
        out = None                                         # white ambient x default ambient material: the unlit kernels
    else:
        block = torch.zeros((n, _LIGHT_FLOATS), dtype=torch.float32)
        for j, t in enumerate((la, ld, ls, pos, ka, kd, ks)):
            block[:, 3 * j:3 * j + 3] = t.expand(n, 3)
        block[:, 21] = sh[:, 0].expand(n)
        bound = float(((ka * la).abs() + (kd * ld).abs()).max())
        out = Lighting(block.to(device), kind, bound if math.isfinite(bound) else float("nan"))
    if len(_PACK_CACHE) > 64:
        _PACK_CACHE.clear()
    _PACK_CACHE[key] = (out, lights, materials)            # keep the keyed objects alive: their ids stay unique
    return out


_INCIDENCE_CACHE = {}


def vertex_incidence(faces_i32, V):
    """vertex -> (face, corner) incidence in CSR form: inc_off (V+1) and inc_ref (3F) = face * 3 + corner, every entry once,
    ascending within each vertex (the fixed order of the vertex-normal gathers).  Built once per topology."""
    key = (faces_i32.data_ptr(), tuple(faces_i32.shape), faces_i32._version, int(V), str(faces_i32.device))
    hit = _INCIDENCE_CACHE.get(key)
    if hit is None:
        idx = faces_i32.reshape(-1).to(torch.int64)
        ref = torch.argsort(idx, stable=True)
        off = torch.zeros(V + 1, dtype=torch.int64, device=idx.device)
        off[1:] = torch.cumsum(torch.bincount(idx, minlength=V), 0)
        if len(_INCIDENCE_CACHE) > 64:
            _INCIDENCE_CACHE.clear()
        hit = ((off.to(torch.int32).contiguous(), ref.to(torch.int32).contiguous()), faces_i32)
        _INCIDENCE_CACHE[key] = hit
    return hit[0]


_NORMAL_CACHE = {}


def _vertex_normals(verts, v32, faces_i32, incidence):
    """-> (normals, unnormalised sums) of the mesh; cached on the vertices' identity and version when they are not being
    optimised (texture-only runs compute them once)."""
    key = None
    if not verts.requires_grad:
        key = (v32.data_ptr(), v32._version, tuple(v32.shape), faces_i32.data_ptr(), str(v32.device))
        hit = _NORMAL_CACHE.get(key)
        if hit is not None:
            return hit[0]
    out = ops.vertex_normals(v32, faces_i32, incidence)
    if key is not None:
        if len(_NORMAL_CACHE) > 16:
            _NORMAL_CACHE.clear()
        _NORMAL_CACHE[key] = (out, v32, faces_i32)
    return out


class LitSetup:
    """Per-render arguments of the lit kernels (st3d.ops.shade_lit_*)."""

    def __init__(self, lighting, verts, faces_i32, R, T, normals=None, unnormalised=None, incidence=None):
        self.block, self.kind, self.weight_bound = lighting.block, lighting.kind, lighting.weight_bound
        self.verts, self.faces_i32, self.R, self.T = verts, faces_i32, R.to(torch.float32).contiguous(), \
            T.to(torch.float32).contiguous()
        self.normals, self.unnormalised, self.incidence = normals, unnormalised, incidence


def _lit_setup(lighting, verts_in, v, faces_i32, R, T):
    if lighting is None:
        return None
    if lighting.n not in (1, R.shape[0]):
        raise ValueError(f"lights have N = {lighting.n} entries; a batch of {R.shape[0]} views takes N = 1 or N = "
                         f"{R.shape[0]}")
    if lighting.kind == 0:
        return LitSetup(lighting, v, faces_i32, R, T)
    inc = vertex_incidence(faces_i32, v.shape[0])
    n, m = _vertex_normals(verts_in, v, faces_i32, inc)
    return LitSetup(lighting, v, faces_i32, R, T, n, m, inc)


def _lit_vertex_grad(lit, gverts, gnp, p2f, bary):
    """gverts (V,3) += the lighting's direct world-space terms: d/dP and, through the vertex normals, d/dN"""
    if lit.kind == 0:
        return gverts
    V = lit.verts.shape[0]
    s = ops.phong_scatter(gnp, p2f, bary, lit.faces_i32, V)
    return ops.vertex_normals_bwd(lit.verts, lit.faces_i32, lit.incidence, lit.unnormalised, s[1], s[0], gverts)


_EPOCH_IDS = itertools.count(1)


class FragmentCache:
    """The fragments of the last few (vertices, faces, cameras, size) batches one rasteriser has seen on the hard K = 1 path.

    In a texture-only run the geometry of a view batch never changes, so projecting and rasterising it again every step
    recomputes the same fragments.  An entry holds the projected vertices, the fragments, the uint8 coverage tag (made
    when first asked for) and a fresh geometry-epoch id, under a key of the identity and version of the vertex, face, R and
    T tensors plus the image size -- the style of key ``reaches_near_plane`` uses; the keyed tensors are held, so their
    addresses cannot be handed to other tensors while the entry lives.  Vertices that require a gradient never enter.

    One entry is 24 bytes per pixel of fragments (+ 1 of coverage): 50 MB for 8 views at 512^2.  ENTRIES = 4 keeps the content
    render and two or three alternating view batches of one run, 0.2 GB next to a plan's 4.4 GB; least recently used first
    out.  The cache belongs to its MeshRasterizer: a new renderer starts empty."""
    ENTRIES = 4

    class Entry:
        __slots__ = ("ndc", "frag", "cover", "cover_version", "epoch", "held")

        def coverage(self):
            """the entry's uint8 coverage tensor, made when first asked for.  It names the epoch, so one that somebody has
            written to since is replaced, under a new epoch id"""
            if self.cover is None or self.cover._version != self.cover_version:
                if self.cover is not None:
                    self.epoch = next(_EPOCH_IDS)
                self.cover = (self.frag[0] >= 0).view(torch.uint8)
                self.cover_version = self.cover._version
            return self.cover

    def __init__(self):
        self._entries = OrderedDict()

    @staticmethod
    def key(verts, faces_i32, R, T, S):
        return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in (verts, faces_i32, R, T)) + (int(S), str(verts.device))

    def get(self, key):
        e = self._entries.get(key)
        if e is not None:
            self._entries.move_to_end(key)
        return e

    def put(self, key, held, ndc, frag):
        e = FragmentCache.Entry()
        e.ndc, e.frag, e.cover, e.cover_version, e.epoch, e.held = ndc, frag, None, 0, next(_EPOCH_IDS), held
        while len(self._entries) >= max(self.ENTRIES, 1):
            self._entries.popitem(last=False)
        self._entries[key] = e
        return e

    def __len__(self):
        return len(self._entries)


_ACTIVE_CACHE = [None]      # innermost last: the FragmentCache _RenderFn.forward may use (None: it rasterises)


class MeshRasterizer:
    def __init__(self, cameras=None, raster_settings=None):
        self.cameras, self.raster_settings = cameras, raster_settings or RasterizationSettings()
        self.fragment_cache = FragmentCache()


class SoftPhongShader:
    """PyTorch3D SoftPhongShader: lights (None = white AmbientLights -- PyTorch3D's own default is PointLights(); this is
    the one deliberate divergence, it keeps the reference's unlit renders) and materials (None = Materials())."""

    def __init__(self, device="cpu", cameras=None, lights=None, materials=None, blend_params=None, **kw):
        self.cameras, self.lights, self.materials = cameras, lights, materials
        self.blend_params = blend_params if blend_params is not None else BlendParams()
        lighting_of(lights, materials, device)      # validate now (N, requires_grad)


class SoftSilhouetteShader:
    """PyTorch3D SoftSilhouetteShader (blending.sigmoid_alpha_blend): the renderer returns (n,S,S,4) with RGB = 1 and
    alpha = 1 - prod_k (1 - sigmoid(-dists_k / sigma)) over the K nearest faces in channel 3.  Only blend_params.sigma is
    read; no texture is needed.  It always renders on the general rasteriser (near-plane clipping included), whatever the
    raster settings: at K = 1 / blur 0 alpha is sigmoid(-d / sigma) in [0.5, 1) on covered pixels.  alpha is differentiable
    in the vertices (csrc/silhouette.hip).  K <= 8 faces per pixel with RasterizationSettings; with
    SilhouetteRasterizationSettings the renderer uses the silhouette rasteriser (csrc/silraster.hip), K <= 64 (PyTorch3D's
    silhouette tutorial uses 50)."""

    def __init__(self, blend_params=None, **kw):
        self.blend_params = blend_params if blend_params is not None else BlendParams()


def _refuse_supersampled_silhouette(raster_settings):
    if getattr(raster_settings, "supersample", 1) > 1:
        raise NotImplementedError("supersample > 1 is not implemented for alpha-only (silhouette) renders: a "
                                  "SoftSilhouetteShader takes RasterizationSettings(supersample=1)")
    if getattr(raster_settings, "texture_mip_levels", 1) != 1:
        raise NotImplementedError(MIP_REFUSALS["silhouette"])


# ---- what the autograd Functions below share: the prologue of every forward (inputs as the kernels take them) and the
# vertex tail of every backward.  A new shading family is expected to use these rather than copy a neighbour.
def _verts32(verts):
    return verts.detach().to(torch.float32).contiguous()


def _square_map(tex_map):
    """a texture map (..., T, T, 3) as the kernels take it: (T,T,3) float32"""
    tex = tex_map.detach().to(torch.float32).reshape(tex_map.shape[-3], tex_map.shape[-2], 3).contiguous()
    if tex.shape[0] != tex.shape[1]:
        raise NotImplementedError("square texture maps only (the reference resizes to size x size)")
    return tex


def _uvs32(verts_uvs):
    return verts_uvs.detach().to(torch.float32).reshape(-1, 2).contiguous()


def _rasterise(v, faces_i32, R, T, side):
    """-> (projected vertices, hard K = 1 fragments at `side`).  No near-plane watch: the callers of the Functions have looked
    at the vertices' depths before choosing these kernels."""
    ndc = ops.project_verts(v, R, T)
    return ndc, ops.raster_fwd(ndc, faces_i32, side)


def _verts_grad(ctx, gbary, gnp=None):
    """The hard path's vertex tail: d/d(bary) -> raster backward -> projection backward [-> the lighting's
    direct terms, given the lit kernels' gnp] -> the vertices' own shape.  ctx: frag, geom, verts_shape [, lit]."""
    v, ndc, faces_i32, R, T = ctx.geom
    gverts = ops.project_verts_bwd(v, R, T, ops.raster_bwd(gbary, ctx.frag[0], ndc, faces_i32))
    if gnp is not None:
        gverts = _lit_vertex_grad(ctx.lit, gverts, gnp, ctx.frag[0], ctx.frag[2])
    return gverts.reshape(ctx.verts_shape)


def _soft_verts_grad(ctx, geo, gnp=None):
    """_verts_grad on the general path: geo = (d/d(bary), d/d(zbuf), d/d(dists)), each may be None.  ctx: frag, geom,
    verts_shape, clip, persp, slots, z_clip [, lit]."""
    v, ndc, faces_i32, R, T = ctx.geom
    gndc = ops.raster_soft_bwd(geo, ctx.frag[0], ndc, faces_i32, ctx.clip, ctx.persp, ctx.slots, ctx.z_clip)
    gverts = ops.project_verts_bwd(v, R, T, gndc)
    if gnp is not None:
        gverts = _lit_vertex_grad(ctx.lit, gverts, gnp, ctx.frag[0], ctx.frag[2])
    return gverts.reshape(ctx.verts_shape)


class _SilhouetteFn(torch.autograd.Function):
    """verts -> alpha (B,1,S,S): project, general raster, silhouette_fwd; backward silhouette_bwd -> raster_soft_bwd with
    d/d(dists) alone -> project_verts_bwd."""

    @staticmethod
    def forward(ctx, verts, faces_i32, R, T, S, K, blur, clip, sigma, cull, persp, z_clip):
        v = _verts32(verts)
        ndc = ops.project_verts(v, R, T)
        p2f, _zbuf, _bary, dists, slots = ops.raster_soft_fwd(ndc, faces_i32, S, K, blur, clip, cull, persp, z_clip)
        ctx.frag, ctx.slots = (p2f, dists), slots
        ctx.clip, ctx.sigma, ctx.persp, ctx.z_clip = clip, sigma, persp, z_clip
        ctx.geom, ctx.verts_shape = (v, ndc, faces_i32, R, T), verts.shape
        return ops.silhouette_fwd(p2f, dists, sigma)

    @staticmethod
    def backward(ctx, grad_alpha):
        with ops.trace("render_backward"):
            gverts = None
            if ctx.needs_input_grad[0]:
                gd = ops.silhouette_bwd(grad_alpha.to(torch.float32), ctx.frag[0], ctx.frag[1], ctx.sigma)
                gverts = _soft_verts_grad(ctx, (None, None, gd))
            return (gverts,) + (None,) * 11


class _SilhouetteRasterFn(torch.autograd.Function):
    """verts -> alpha (B,1,S,S) on the silhouette rasteriser (csrc/silraster.hip, K = 1..64): project, one raster pass to
    alpha; backward from the saved per-pixel state (keep and the cut: 12 bytes per pixel whatever K is) to the vertices.
    Projected vertices and face records are recomputed in the backward rather than kept."""

    @staticmethod
    def forward(ctx, verts, faces_i32, R, T, S, K, blur, clip, sigma, cull, persp, z_clip):
        v = _verts32(verts)
        ndc = ops.project_verts(v, R, T)
        alpha, state = ops.silraster_fwd(ndc, faces_i32, S, K, blur, sigma, clip, cull, persp, z_clip)
        ctx.saved = (state if verts.requires_grad else None, v, faces_i32, R, T)
        ctx.settings = (blur, clip, sigma, cull, persp, z_clip)
        ctx.verts_shape = verts.shape
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        with ops.trace("render_backward"):
            gverts = None
            state, v, faces_i32, R, T = ctx.saved
            if state is not None and ctx.needs_input_grad[0]:
                blur, clip, sigma, cull, persp, z_clip = ctx.settings
                ndc = ops.project_verts(v, R, T)
                gndc = ops.silraster_bwd(state, ndc, faces_i32, blur, sigma, grad_alpha, 1.0, clip, cull, persp, z_clip)
                gverts = ops.project_verts_bwd(v, R, T, gndc).reshape(ctx.verts_shape)
            return (gverts,) + (None,) * 11


def render_silhouette(meshes, R, T, image_size, raster_settings=None, blend_params=None):
    """SoftSilhouetteShader's alpha (B,1,S,S) of all B views; the mesh needs no textures.  SilhouetteRasterizationSettings
    select the silhouette rasteriser (no fragments, faces_per_pixel up to 64)."""
    dev = meshes.device
    rs = raster_settings if raster_settings is not None else RasterizationSettings(image_size=image_size)
    _refuse_supersampled_silhouette(rs)
    bp = blend_params if blend_params is not None else BlendParams()
    fn = _SilhouetteRasterFn if isinstance(rs, SilhouetteRasterizationSettings) else _SilhouetteFn
    with ops.trace("render"):
        return fn.apply(meshes.verts_packed(), meshes.faces_i32(), R.to(dev), T.to(dev), int(image_size), rs.faces_per_pixel,
                        rs.blur_radius, rs.clip_barycentric_coords, bp.sigma, rs.cull_backfaces, rs.perspective_correct,
                        rs.z_clip)


class _RenderFn(torch.autograd.Function):
    """(verts, texture_map) -> (rgb (B,3,S,S), mask (B,1,S,S)); backward = texture scatter and,
    when the vertices need a gradient, shade d/d(bary) -> raster backward -> projection backward."""

    @staticmethod
    def forward(ctx, verts, tex_map, faces_i32, verts_uvs, faces_uvs_i32, R, T, S, lighting=None):
        v, tex, uvs = _verts32(verts), _square_map(tex_map), _uvs32(verts_uvs)
        # the calling rasteriser's FragmentCache (_render_views names it for the length of this call): geometry that is not
        # being optimised is projected and rasterised once per batch of views
        cache, entry, key = _ACTIVE_CACHE[-1], None, None
        if cache is not None and lighting is None and not verts.requires_grad:
            key = FragmentCache.key(verts, faces_i32, R, T, S)
            entry = cache.get(key)
        if entry is None:
            ndc, frag = _rasterise(v, faces_i32, R, T, S)
            if key is not None:
                entry = cache.put(key, (verts, faces_i32, R, T), ndc, frag)
        else:
            ndc, frag = entry.ndc, entry.frag
        ctx.entry = entry
        ctx.lit = _lit_setup(lighting, verts, v, faces_i32, R, T)
        if ctx.lit is None:
            rgb, mask = ops.shade_fwd(frag, uvs, faces_uvs_i32, tex)
        else:
            rgb, mask = ops.shade_lit_fwd(frag, uvs, faces_uvs_i32, tex, ctx.lit)
        ctx.frag, ctx.uvs, ctx.fuv, ctx.tex = frag, uvs, faces_uvs_i32, tex
        ctx.tex_shape, ctx.verts_shape = tex_map.shape, verts.shape
        ctx.geom = (v, ndc, faces_i32, R, T)
        ctx.mark_non_differentiable(mask)
        return rgb, mask

    @staticmethod
    def backward(ctx, grad_rgb, _grad_mask):
        with ops.trace("render_backward"):
            need_v, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            gtex = gverts = None
            if need_v or need_t:
                g = grad_rgb.to(torch.float32)
                gnp = None
                if ctx.lit is not None:
                    gt, gbary, gnp = ops.shade_lit_bwd(g, ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, ctx.lit, want_texture=need_t,
                                                       want_geometry=need_v)
                else:
                    res = ops.shade_bwd(g, ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, want_bary=need_v, want_texture=need_t)
                    gt, gbary = (res if need_v else (res, None))
                if need_t:
                    gtex = gt.reshape(ctx.tex_shape)
                if need_v:
                    gverts = _verts_grad(ctx, gbary, gnp)
            return (gverts, gtex) + (None,) * 7


class _MipRenderFn(torch.autograd.Function):
    """_RenderFn with mip-mapped trilinear sampling (L >= 2 levels): project, raster, mip_build, mip_lod, shade_mip_fwd.  The
    chain and the level-of-detail plane are kept for the backward, which treats the plane as a constant: texel gradients of
    both levels of every pixel's pair are folded back onto the map by the chain's adjoint; d/d(bary) goes through the
    unchanged raster / projection backward."""

    @staticmethod
    def forward(ctx, verts, tex_map, faces_i32, verts_uvs, faces_uvs_i32, R, T, S, L, bias):
        v, tex, uvs = _verts32(verts), _square_map(tex_map), _uvs32(verts_uvs)
        side = tex.shape[0]
        ndc, frag = _rasterise(v, faces_i32, R, T, S)
        pyr = ops.mip_build(tex, L)
        lod = ops.mip_lod(frag, ndc, faces_i32, uvs, faces_uvs_i32, side, L, bias)
        rgb, mask = ops.shade_mip_fwd(frag, uvs, faces_uvs_i32, pyr, lod, side, L)
        ctx.frag, ctx.uvs, ctx.fuv, ctx.pyr, ctx.lod, ctx.mip = frag, uvs, faces_uvs_i32, pyr, lod, (side, L)
        ctx.tex_shape, ctx.verts_shape = tex_map.shape, verts.shape
        ctx.geom = (v, ndc, faces_i32, R, T)
        ctx.mark_non_differentiable(mask)
        return rgb, mask

    @staticmethod
    def backward(ctx, grad_rgb, _grad_mask):
        with ops.trace("render_backward"):
            need_v, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            gtex = gverts = None
            if need_v or need_t:
                side, L = ctx.mip
                res = ops.shade_mip_bwd(grad_rgb.to(torch.float32), ctx.frag, ctx.uvs, ctx.fuv, ctx.pyr, ctx.lod, side, L,
                                        want_bary=need_v, want_texture=need_t)
                gt, gbary = (res if need_v else (res, None))
                if need_t:
                    gtex = gt.reshape(ctx.tex_shape)
                if need_v:
                    gverts = _verts_grad(ctx, gbary)
            return (gverts, gtex) + (None,) * 8


class _VertexColourRenderFn(torch.autograd.Function):
    """(verts, colours (V,3)) -> (rgb (B,3,S,S), mask (B,1,S,S)) for a TexturesVertex mesh: project, raster, shade_vc_fwd.
    Backward: the colour scatter and, when the vertices need a gradient, d/d(bary) -> the unchanged raster / projection
    backward.  With the vertices alone under optimisation nothing is scattered."""

    @staticmethod
    def forward(ctx, verts, colours, faces_i32, R, T, S):
        v = _verts32(verts)
        col = colours.detach().to(torch.float32).reshape(-1, 3).contiguous()
        ndc, frag = _rasterise(v, faces_i32, R, T, S)
        rgb, mask = ops.shade_vc_fwd(frag, faces_i32, col)
        ctx.frag, ctx.col = frag, col
        ctx.col_shape, ctx.verts_shape = colours.shape, verts.shape
        ctx.geom = (v, ndc, faces_i32, R, T)
        ctx.mark_non_differentiable(mask)
        return rgb, mask

    @staticmethod
    def backward(ctx, grad_rgb, _grad_mask):
        with ops.trace("render_backward"):
            need_v, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            gcol = gverts = None
            if need_v or need_c:
                res = ops.shade_vc_bwd(grad_rgb.to(torch.float32), ctx.frag, ctx.geom[2], ctx.col, want_colours=need_c,
                                       want_bary=need_v)
                gc, gbary = res if (need_v and need_c) else ((res, None) if need_c else (None, res))
                if need_c:
                    gcol = gc.reshape(ctx.col_shape)
                if need_v:
                    gverts = _verts_grad(ctx, gbary)
            return gverts, gcol, None, None, None, None


class _AtlasRenderFn(torch.autograd.Function):
    """(verts, atlas (F,R,R,3)) -> (rgb (B,3,S,S), mask (B,1,S,S)) for a TexturesAtlas mesh: project, raster,
    shade_atlas_fwd.  Backward: the atlas scatter alone.  The nearest-texel lookup is piecewise constant in the barycentrics
    and the hard path sends nothing through dists / zbuf, so the vertices get None."""

    @staticmethod
    def forward(ctx, verts, atlas, faces_i32, R, T, S):
        at = atlas.detach().to(torch.float32).reshape(atlas.shape[-4:]).contiguous()
        _ndc, frag = _rasterise(_verts32(verts), faces_i32, R, T, S)
        rgb, mask = ops.shade_atlas_fwd(frag, at)
        ctx.frag = frag
        ctx.atlas_shape = atlas.shape
        ctx.block = (at.shape[1], at.shape[0])          # R, F
        ctx.mark_non_differentiable(mask)
        return rgb, mask

    @staticmethod
    def backward(ctx, grad_rgb, _grad_mask):
        with ops.trace("render_backward"):
            gatlas = None
            if ctx.needs_input_grad[1]:
                gatlas = ops.shade_atlas_bwd(grad_rgb.to(torch.float32), ctx.frag, *ctx.block).reshape(ctx.atlas_shape)
            return None, gatlas, None, None, None, None


class _SSRenderFn(torch.autograd.Function):
    """_RenderFn supersampled: fragments at side a * S on the same rasteriser, (rgb (B,3,S,S), coverage (B,1,S,S)) from the
    fused kernels (st3d.ops.shade_ss_*); the backward hands the S-sized gradient to them and the a * S barycentric
    gradients to the unchanged raster / projection backward."""

    @staticmethod
    def forward(ctx, verts, tex_map, faces_i32, verts_uvs, faces_uvs_i32, R, T, S, a, lighting=None):
        v, tex, uvs = _verts32(verts), _square_map(tex_map), _uvs32(verts_uvs)
        ndc, frag = _rasterise(v, faces_i32, R, T, a * S)
        ctx.lit = _lit_setup(lighting, verts, v, faces_i32, R, T)
        if ctx.lit is None:
            rgb, cov = ops.shade_ss_fwd(frag, uvs, faces_uvs_i32, tex, a)
        else:
            rgb, cov = ops.shade_ss_lit_fwd(frag, uvs, faces_uvs_i32, tex, ctx.lit, a)
        ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, ctx.a = frag, uvs, faces_uvs_i32, tex, a
        ctx.tex_shape, ctx.verts_shape = tex_map.shape, verts.shape
        ctx.geom = (v, ndc, faces_i32, R, T)
        ctx.mark_non_differentiable(cov)
        return rgb, cov

    @staticmethod
    def backward(ctx, grad_rgb, _grad_cov):
        with ops.trace("render_backward"):
            need_v, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            gtex = gverts = None
            if need_v or need_t:
                g = grad_rgb.to(torch.float32)
                gnp = None
                if ctx.lit is not None:
                    gt, gbary, gnp = ops.shade_ss_lit_bwd(g, ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, ctx.lit, ctx.a,
                                                          want_texture=need_t, want_geometry=need_v)
                else:
                    res = ops.shade_ss_bwd(g, ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, ctx.a, want_bary=need_v,
                                           want_texture=need_t)
                    gt, gbary = (res if need_v else (res, None))
                if need_t:
                    gtex = gt.reshape(ctx.tex_shape)
                if need_v:
                    gverts = _verts_grad(ctx, gbary, gnp)
            return (gverts, gtex) + (None,) * 8


class _BoxDownFn(torch.autograd.Function):
    """(B,C,a*S,a*S) -> (B,C,S,S) box filter (st3d.ops.box_down_fwd) and its transpose"""

    @staticmethod
    def forward(ctx, x, a):
        ctx.a = a
        ctx.set_materialize_grads(False)
        return ops.box_down_fwd(x.detach().to(torch.float32), a)

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None:
            return None, None
        return ops.box_down_bwd(grad_out.to(torch.float32), ctx.a), None


class _SoftRenderFn(torch.autograd.Function):
    """General path: K faces per pixel, blur_radius, softmax_rgb_blend -> (rgb (B,3,S,S), alpha (B,1,S,S)).
    Gradients flow from rgb to the texture and, through barycentrics, depth and the signed edge distance, to
    the vertices; a gradient for alpha joins them through the signed edge distance (silhouette_bwd accumulates into the
    grad_dists of the RGB backward before the one raster backward).  Without one the launches are those of the RGB
    backward alone (the reference only ever thresholds alpha, utils.py:72)."""

    @staticmethod
    def forward(ctx, verts, tex_map, faces_i32, verts_uvs, faces_uvs_i32, R, T, S, K, blur, clip, sigma, gamma, bg,
                cull=False, persp=True, z_clip=None, lighting=None):
        v, tex, uvs = _verts32(verts), _square_map(tex_map), _uvs32(verts_uvs)
        ndc = ops.project_verts(v, R, T)
        frag = ops.raster_soft_fwd(ndc, faces_i32, S, K, blur, clip, cull, persp, z_clip)
        ctx.slots = frag[4] if z_clip is not None else None
        frag = frag[:4]
        ctx.lit = _lit_setup(lighting, verts, v, faces_i32, R, T)
        if ctx.lit is None:
            rgb, alpha = ops.shade_soft_fwd(frag, uvs, faces_uvs_i32, tex, sigma, gamma, bg)
        else:
            rgb, alpha = ops.shade_soft_lit_fwd(frag, uvs, faces_uvs_i32, tex, ctx.lit, sigma, gamma, bg)
        ctx.frag, ctx.uvs, ctx.fuv, ctx.tex = frag, uvs, faces_uvs_i32, tex
        ctx.blend, ctx.clip, ctx.persp, ctx.z_clip = (sigma, gamma, bg), clip, persp, z_clip
        ctx.tex_shape, ctx.verts_shape = tex_map.shape, verts.shape
        ctx.geom = (v, ndc, faces_i32, R, T)
        ctx.set_materialize_grads(False)        # an output nobody differentiates arrives as None, not as zeros
        return rgb, alpha

    @staticmethod
    def backward(ctx, grad_rgb, grad_alpha):
        with ops.trace("render_backward"):
            need_v, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            sigma, gamma, bg = ctx.blend
            gtex = gverts = None
            if grad_rgb is None:
                # only alpha carries a gradient (or nothing does): no RGB backward, no texture gradient
                if need_v and grad_alpha is not None:
                    gd = ops.silhouette_bwd(grad_alpha.to(torch.float32), ctx.frag[0], ctx.frag[3], sigma)
                    gverts = _soft_verts_grad(ctx, (None, None, gd))
            elif need_v or need_t:
                g = grad_rgb.to(torch.float32)
                gnp = None
                if ctx.lit is None:
                    gt, geo = ops.shade_soft_bwd(g, ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, sigma, gamma, bg, want_texture=need_t,
                                                 want_geometry=need_v)
                else:
                    gt, geo, gnp = ops.shade_soft_lit_bwd(g, ctx.frag, ctx.uvs, ctx.fuv, ctx.tex, ctx.lit, sigma, gamma, bg,
                                                          want_texture=need_t, want_geometry=need_v)
                if need_t:
                    gtex = gt.reshape(ctx.tex_shape)
                if need_v:
                    if grad_alpha is not None:      # d alpha / d dists joins the RGB backward's grad_dists
                        ops.silhouette_bwd(grad_alpha.to(torch.float32), ctx.frag[0], ctx.frag[3], sigma, out=geo[2])
                    gverts = _soft_verts_grad(ctx, geo, gnp)
            return (gverts, gtex) + (None,) * 16


NEED_TAG = "_st3d_need"


def tag_need(rgb, p2f):
    """Tag the colour tensor a render returns with its coverage: (n,S,S) uint8, 1 where any layer of p2f (n,S,S[,K]) holds
    a face.  The render backward reads the gradient of `rgb` at exactly those pixels (shade_bwd and its soft and lit
    siblings walk the fragments; the background is a constant), so a loss that produces that gradient may skip whatever
    only the other pixels would need (losses.compute_perceptual_loss -> PerceptualPlan.loss(need_mask=...)).  The tag
    describes the tensor's PRODUCER: it stays true whatever else consumes the tensor.  Only tensors that will get a
    gradient are tagged."""
    if rgb.requires_grad:
        hit = p2f >= 0
        setattr(rgb, NEED_TAG, (hit.any(dim=-1) if hit.dim() == 4 else hit).view(torch.uint8))      # (bool is one 0/1 byte)
    return rgb


def tag_need_mask(rgb, need, epoch=None):
    """tag_need for a producer that knows its coverage as a boolean (n,S,S) rather than as fragments.
    epoch (an id of FragmentCache): `need` is the coverage tensor of that geometry epoch -- the same tensor, unmodified, for
    every render of the epoch -- and every pixel it does not cover holds the background colour of the render's flat tag bit
    for bit (the hard path's blend writes the constant there)."""
    if rgb.requires_grad:
        if need.dtype != torch.uint8:
            need = need.view(torch.uint8)
        setattr(rgb, NEED_TAG, need)
        if epoch:
            setattr(rgb, EPOCH_TAG, (int(epoch), need, need._version))
    return rgb


EPOCH_TAG = "_st3d_epoch"


def epoch_of(t, need):
    """The geometry epoch of `t`'s coverage tag, if `need` (what need_of(t) returned) is that epoch's coverage tensor,
    unmodified since the tag was made; else 0.  A loss hands it on to PerceptualPlan.loss(epoch=...), which then keeps what
    depends on the coverage alone from step to step."""
    tag = getattr(t, EPOCH_TAG, None)
    if tag is None or need is None or tag[1] is not need or need._version != tag[2]:
        return 0
    return tag[0]


def need_of(t):
    """The coverage tag of `t` if a gradient consumer may rely on it, else None: the tag must fit the tensor, and nobody
    may be watching the tensor's own gradient (retain_grad, backward hooks) -- they would see the zeros."""
    tag = getattr(t, NEED_TAG, None)
    if tag is None or t.dim() != 4 or tuple(tag.shape) != (t.shape[0], t.shape[2], t.shape[3]) or tag.device != t.device:
        return None
    if t.is_leaf or t.retains_grad or getattr(t, "_backward_hooks", None):
        return None
    return tag


FLAT_TAG = "_st3d_flat"


def tag_flat(rgb, background_color):
    """Tag the colour tensor a render returns with the blend's background colour (3 floats): every pixel without a
    fragment holds it, so a loss may compute the part of its forward that sees nothing else once and copy it
    (losses.compute_perceptual_loss -> PerceptualPlan.loss(flat_color=...)).  A hint, never a premise: the device compares
    the pixels themselves, a wrong tag costs the list build and changes no result.  Composites onto another background
    (utils._composite) do not inherit it."""
    setattr(rgb, FLAT_TAG, tuple(float(c) for c in background_color))
    return rgb


def flat_of(t):
    """The background tag of `t` (3 floats) if it fits the tensor, else None."""
    tag = getattr(t, FLAT_TAG, None)
    if tag is None or t.dim() != 4 or t.shape[1] != 3 or len(tag) != 3:
        return None
    return tag


def uses_hard_path(raster_settings, blend_params):
    """True for the reference's own configuration (K=1, blur 0, unclipped, default BlendParams): there
    softmax_rgb_blend reduces to texel-or-white and the specialised kernels apply."""
    rs, bp = raster_settings, blend_params
    if rs is not None and not rs.is_hard:
        return False
    return bp is None or (bp.sigma, bp.gamma, bp.background_color) == (1e-4, 1e-4, (1.0, 1.0, 1.0))


_DEPTH_CACHE = {}


def reaches_near_plane(verts, R, T, z_clip):
    """True if any vertex lies nearer than `z_clip` to any of the cameras (view depth = X_world R[:, :, 2] + T[2]).
    PyTorch3D clips every mesh at z_clip before rasterising; the specialised K = 1 kernels do not, so render_views asks
    BEFORE it renders and sends such a batch to the clipping kernels -- no frame is ever rendered unclipped.  The answer
    needs one host read of a device scalar: for tensors that are not being optimised it is cached on their identity and
    version (texture-only runs: one read per camera batch, ever); vertices under optimisation are asked every step (the
    read waits for the previous step, ~1 % of a config-5 step)."""
    v = verts.detach()
    key = None
    if not verts.requires_grad:
        key = (v.data_ptr(), v._version, tuple(v.shape), R.data_ptr(), R._version, T.data_ptr(), T._version, R.shape[0],
               float(z_clip), str(v.device))
        hit = _DEPTH_CACHE.get(key)
        if hit is not None:
            return hit[0]
    zmin = (v.to(torch.float32) @ R[:, :, 2].to(torch.float32).t() + T[:, 2].to(torch.float32)).min()
    near = bool(zmin.item() < z_clip)
    if key is not None:
        if len(_DEPTH_CACHE) > 256:
            _DEPTH_CACHE.clear()
        _DEPTH_CACHE[key] = (near, verts, R, T)         # keep the keyed tensors alive: their addresses stay unique
    return near


def _near_plane_reached(meshes, R, T):
    """the specialised kernels must not render this batch: the watch has fired, or a vertex lies nearer than PyTorch3D's plane"""
    return ops.near_plane_triggered() or reaches_near_plane(meshes.verts_packed(), R, T, RasterizationSettings.Z_CLIP_DEFAULT)


def _tag_hard(rgb):
    """the tags of a hard-path render whose Function kept its fragments: coverage from p2f, a white background"""
    if rgb.requires_grad:
        tag_need(rgb, rgb.grad_fn.frag[0])
    return tag_flat(rgb, (1.0, 1.0, 1.0))


_REFUSAL_CONDITIONS = (         # name in the *_REFUSALS tables, does it hold; in order of precedence
    ("silhouette", lambda rs, bp, lighting: isinstance(rs, SilhouetteRasterizationSettings)),
    ("lights", lambda rs, bp, lighting: lighting() is not None),
    ("supersample", lambda rs, bp, lighting: getattr(rs, "supersample", 1) > 1),
    ("mip", lambda rs, bp, lighting: getattr(rs, "texture_mip_levels", 1) != 1),
    ("soft", lambda rs, bp, lighting: not uses_hard_path(rs, bp)),
)


def _refuse(table, refused, rs, bp, lighting):
    """NotImplementedError with `table`'s message for the first condition named in `refused` that holds (before any launch).
    lighting: a callable -> Lighting or None, asked only once "lights" is reached (making one validates the lights)."""
    for name, holds in _REFUSAL_CONDITIONS:
        if name in refused and holds(rs, bp, lighting):
            raise NotImplementedError(table[name])


def _clipping_settings(image_size):
    """The specialised kernels do not clip: a mesh at the near plane renders with the same (hard) settings on the general
    kernels at PyTorch3D's default clipping depth -> those settings, with one warning (ST3D_NEAR_PLANE=raise: an error).
    Every rank decides for its own views; both kernel families give the same pixels where nothing is clipped, so ranks need
    not agree."""
    if ops.NEAR_PLANE_POLICY == "raise":
        raise RuntimeError(ops.NEAR_PLANE_MESSAGE)
    ops.note_near_plane()
    return RasterizationSettings(image_size=image_size, z_clip_value=RasterizationSettings.Z_CLIP_DEFAULT)


def _uv_args(meshes, R, T):
    """what every Function that samples a texture map takes first"""
    tex = meshes.textures
    return (meshes.verts_packed(), tex.maps_padded(), meshes.faces_i32(), tex.verts_uvs_padded(), tex.faces_uvs_i32(), R, T)


def _soft_args(rs, bp, lighting):
    """what _SoftRenderFn takes after the image side"""
    return (rs.faces_per_pixel, rs.blur_radius, rs.clip_barycentric_coords, bp.sigma, bp.gamma, bp.background_color,
            rs.cull_backfaces, rs.perspective_correct, rs.z_clip, lighting)


def render_views(meshes, R, T, image_size, raster_settings=None, blend_params=None, lights=None, materials=None, cache=None):
    """``_render_views`` inside a named range (``ST3D_ROCTX=1``: rocprofv3 --marker-trace shows the step's phases)."""
    with ops.trace("render"):
        return _render_views(meshes, R, T, image_size, raster_settings, blend_params, lights, materials, cache)


def _render_views(meshes, R, T, image_size, raster_settings=None, blend_params=None, lights=None, materials=None, cache=None):
    """All B views in one batch of launches -> (rgb (B,3,S,S), coverage (B,1,S,S)).  Coverage is the 0/1 mask under
    the reference's hard settings (whichever kernels render them) and softmax_rgb_blend's alpha under soft settings;
    both satisfy ``coverage > 0`` == covered.  lights / materials: the shading (lighting_of: None = today's unlit
    kernels); both kernel families light, so a batch rerouted to the clipping kernels keeps its lighting.  cache: the calling
    rasteriser's FragmentCache (None: every call rasterises); only the unlit hard K = 1 path with a texture map uses it."""
    tex = meshes.textures
    dev = meshes.device
    rs, bp = raster_settings, blend_params
    if isinstance(tex, TexturesVertex):         # decided on the texture's type before any path is chosen
        return _render_views_vertex(meshes, R, T, int(image_size), rs, bp, lights, materials)
    if isinstance(tex, TexturesAtlas):
        return _render_views_atlas(meshes, R, T, int(image_size), rs, bp, lights, materials)
    if isinstance(rs, SilhouetteRasterizationSettings):
        raise NotImplementedError("SilhouetteRasterizationSettings render on the silhouette rasteriser, which produces alpha "
                                  "only: they need a SoftSilhouetteShader")
    R, T = R.to(dev), T.to(dev)
    lighting = lighting_of(lights, materials, dev)
    if getattr(rs, "texture_mip_levels", 1) != 1:
        out = _render_views_mip(meshes, R, T, int(image_size), rs, bp, lighting)
        if out is not None:
            return out
    if getattr(rs, "supersample", 1) > 1:
        return _render_views_ss(meshes, R, T, int(image_size), rs, bp, lighting)
    hard_settings = uses_hard_path(rs, bp)
    if hard_settings and _near_plane_reached(meshes, R, T):
        rs = _clipping_settings(image_size)
    args = _uv_args(meshes, R, T)
    if uses_hard_path(rs, bp):
        # K=1, blur 0: the blend weight cancels and the pixel is the sampled texel itself
        _ACTIVE_CACHE.append(cache if os.environ.get("ST3D_FRAG_CACHE", "1") != "0" else None)    # (the A/B switch, read per render)
        try:
            rgb, mask = _RenderFn.apply(*args, int(image_size), lighting)
        finally:
            _ACTIVE_CACHE.pop()
        entry = getattr(rgb.grad_fn, "entry", None) if rgb.requires_grad else None
        if entry is None:
            return _tag_hard(rgb), mask         # (uses_hard_path: the default BlendParams, a white background)
        cover = entry.coverage()    # fragments of the cache: their coverage tag is made once and names its geometry epoch
        tag_need_mask(rgb, cover, epoch=entry.epoch)
        return tag_flat(rgb, (1.0, 1.0, 1.0)), mask
    bp = bp if bp is not None else BlendParams()
    rs = rs if rs is not None else RasterizationSettings(image_size=image_size)
    rgb, alpha = _SoftRenderFn.apply(*args, int(image_size), *_soft_args(rs, bp, lighting))
    if rgb.requires_grad:
        tag_need(rgb, rgb.grad_fn.frag[0])
    tag_flat(rgb, bp.background_color)
    if hard_settings:
        # the caller asked for the hard configuration and is handed what the hard path hands out: the 0/1 coverage mask
        # (alpha of a K = 1 / blur 0 blend is in [0.5, 1) on covered pixels; the reference thresholds it, utils.py:72)
        alpha = (alpha.detach() > 0).to(torch.float32)
    return rgb, alpha


def _render_views_vertex(meshes, R, T, S, rs, bp, lights, materials):
    """_render_views for a mesh whose textures are a TexturesVertex -> (rgb, 0/1 mask) from csrc/vcolor.hip.  Everything
    the kernels do not cover is refused before any launch; a batch at the near plane is an error whatever ST3D_NEAR_PLANE
    says, never a silent reroute (the clipping kernels have no vertex-colour path)."""
    dev = meshes.device
    _refuse(VERTEX_COLOUR_REFUSALS, ("silhouette", "lights", "supersample", "mip", "soft"), rs, bp,
            lambda: lighting_of(lights, materials, dev))
    colours = vertex_colours_of(meshes)
    faces_i32 = meshes.faces_i32()              # range-checked against the vertex count (= the colour count)
    R, T = R.to(dev), T.to(dev)
    if _near_plane_reached(meshes, R, T):
        raise RuntimeError(VERTEX_COLOUR_NEAR_PLANE_MESSAGE)
    rgb, mask = _VertexColourRenderFn.apply(meshes.verts_packed(), colours, faces_i32, R, T, S)
    return _tag_hard(rgb), mask


def _render_views_atlas(meshes, R, T, S, rs, bp, lights, materials):
    """_render_views for a mesh whose textures are a TexturesAtlas -> (rgb, coverage) from csrc/atlas.hip.  supersample = a
    > 1: fragments and shading at a * S, then the box filter (rgb through _BoxDownFn, whose backward is the filter's
    transpose; the mask through ops.box_down_fwd) -- the composition of the ST3D_SS_FUSED=0 branch of _render_views_ss;
    coverage is then fractional.  Everything the kernels do not cover is refused before any launch; a batch at the near
    plane is an error whatever ST3D_NEAR_PLANE says, never a silent reroute (the clipping kernels have no atlas path)."""
    dev = meshes.device
    _refuse(ATLAS_REFUSALS, ("silhouette", "lights", "mip", "soft"), rs, bp, lambda: lighting_of(lights, materials, dev))
    a = getattr(rs, "supersample", 1)
    if a > 1:
        a = ops.check_supersample(a, S)
    atlas = atlas_of(meshes)
    faces_i32 = meshes.faces_i32()
    R, T = R.to(dev), T.to(dev)
    if _near_plane_reached(meshes, R, T):
        raise RuntimeError(ATLAS_NEAR_PLANE_MESSAGE)
    if a > 1:
        rgb_hi, mask_hi = _AtlasRenderFn.apply(meshes.verts_packed(), atlas, faces_i32, R, T, a * S)
        rgb, cov = _BoxDownFn.apply(rgb_hi, a), ops.box_down_fwd(mask_hi, a)
        tag_need_mask(rgb, cov[:, 0] > 0)
        tag_flat(rgb, (1.0, 1.0, 1.0))
        return rgb, cov
    rgb, mask = _AtlasRenderFn.apply(meshes.verts_packed(), atlas, faces_i32, R, T, S)
    return _tag_hard(rgb), mask


def _render_views_mip(meshes, R, T, S, rs, bp, lighting):
    """_render_views at texture_mip_levels != 1 -> (rgb, 0/1 mask) from the mip-mapped kernels, or None when the map's side
    allows one level only (texture_mip_levels = 0 under an odd side: the plain render).  Everything the kernels do not cover
    is refused before any launch; a batch at the near plane is an error, never a silent unfiltered render."""
    _refuse(MIP_REFUSALS, ("lights", "supersample", "soft"), rs, bp, lambda: lighting)
    maps = meshes.textures.maps_padded()
    if maps.shape[-3] != maps.shape[-2]:
        raise NotImplementedError("square texture maps only (the reference resizes to size x size)")
    L = ops.check_mip(rs.texture_mip_levels, maps.shape[-2])
    if L == 1:
        return None
    if _near_plane_reached(meshes, R, T):
        raise RuntimeError(MIP_NEAR_PLANE_MESSAGE)
    rgb, mask = _MipRenderFn.apply(*_uv_args(meshes, R, T), S, L, rs.texture_lod_bias)
    return _tag_hard(rgb), mask


def ss_fused():
    """ST3D_SS_FUSED=0: the hard path of a supersampled render runs the plain kernels at a * S and the box filter (the
    composition the fused kernels are compared with) instead of the fused kernels.  Read at every render."""
    return os.environ.get("ST3D_SS_FUSED", "1") not in ("", "0")


def _render_views_ss(meshes, R, T, S, rs, bp, lighting):
    """_render_views at supersample = a > 1 -> (rgb (B,3,S,S), coverage (B,1,S,S)): everything is rasterised and shaded at
    a * S and box-filtered.  Hard settings: the fused kernels on the specialised rasteriser.  Everything else (K > 1,
    blur, another blend, the near-plane reroute): _SoftRenderFn at a * S, then the box filter over rgb and alpha, whose
    gradients go back through its transpose.  Coverage is fractional either way; ``coverage > 0`` == some sub-pixel
    covered."""
    a = ops.check_supersample(rs.supersample, S)
    hard_settings = uses_hard_path(rs, bp)
    rs_hi = rs
    if hard_settings and _near_plane_reached(meshes, R, T):
        rs_hi = _clipping_settings(S)           # (the decision is about vertices, not pixels: as at a = 1)
    args = _uv_args(meshes, R, T)
    if uses_hard_path(rs_hi, bp):
        if ss_fused():
            rgb, cov = _SSRenderFn.apply(*args, S, a, lighting)
        else:
            rgb_hi, mask_hi = _RenderFn.apply(*args, a * S, lighting)
            rgb, cov = _BoxDownFn.apply(rgb_hi, a), ops.box_down_fwd(mask_hi, a)
        tag_need_mask(rgb, cov[:, 0] > 0)
        tag_flat(rgb, (1.0, 1.0, 1.0))
        return rgb, cov
    bp = bp if bp is not None else BlendParams()
    rgb_hi, alpha_hi = _SoftRenderFn.apply(*args, a * S, *_soft_args(rs_hi, bp, lighting))
    if hard_settings:       # thresholded at a * S first, as at a = 1; the filter then hands out the same fractional coverage
        alpha_hi = (alpha_hi.detach() > 0).to(torch.float32)
    rgb, alpha = _BoxDownFn.apply(rgb_hi, a), _BoxDownFn.apply(alpha_hi, a)
    if rgb.requires_grad:
        hit = (rgb_hi.grad_fn.frag[0] >= 0).any(dim=-1)           # (B,aS,aS): the RGB backward reads its gradient there
        tag_need_mask(rgb, hit.view(hit.shape[0], S, a, S, a).any(dim=4).any(dim=2))
    tag_flat(rgb, bp.background_color)
    return rgb, alpha


class MeshRenderer:
    """``renderer(meshes_world=mesh, cameras=camera)`` -> (n,S,S,4) RGBA like PyTorch3D's
    MeshRenderer (utils.py:69); ``render_meshes`` in the drop-in utils.py calls
    ``render`` and skips the RGBA repack."""

    def __init__(self, rasterizer, shader):
        if isinstance(getattr(rasterizer, "raster_settings", None), SilhouetteRasterizationSettings) \
                and not isinstance(shader, SoftSilhouetteShader):
            raise NotImplementedError("SilhouetteRasterizationSettings render on the silhouette rasteriser, which produces "
                                      "alpha only: they need a SoftSilhouetteShader, got " + type(shader).__name__)
        if isinstance(shader, SoftSilhouetteShader):
            _refuse_supersampled_silhouette(getattr(rasterizer, "raster_settings", None))
        self.rasterizer, self.shader = rasterizer, shader

    @property
    def image_size(self):
        return self.rasterizer.raster_settings.image_size

    @property
    def supersample(self):
        return getattr(self.rasterizer.raster_settings, "supersample", 1)

    @property
    def texture_mip_levels(self):
        return getattr(self.rasterizer.raster_settings, "texture_mip_levels", 1)

    @property
    def is_hard(self):
        if isinstance(self.shader, SoftSilhouetteShader):
            return False
        return uses_hard_path(self.rasterizer.raster_settings, getattr(self.shader, "blend_params", None))

    def render(self, meshes_world, cameras=None, lights=None, materials=None):
        """-> (rgb (n,3,S,S), coverage (n,1,S,S)) under this renderer's raster settings, blend params and shading;
        lights / materials given here replace the shader's for this call (as PyTorch3D's ``renderer(mesh, lights=...)``)."""
        cameras = cameras if cameras is not None else self.rasterizer.cameras
        R, T = join_cameras(cameras)
        if isinstance(self.shader, SoftSilhouetteShader):       # RGB = 1, alpha = sigmoid_alpha_blend's; nothing is lit
            alpha = render_silhouette(meshes_world, R, T, self.image_size, self.rasterizer.raster_settings,
                                      self.shader.blend_params)
            return torch.ones((alpha.shape[0], 3) + tuple(alpha.shape[2:]), dtype=alpha.dtype, device=alpha.device), alpha
        lights = lights if lights is not None else getattr(self.shader, "lights", None)
        materials = materials if materials is not None else getattr(self.shader, "materials", None)
        return render_views(meshes_world, R, T, self.image_size, self.rasterizer.raster_settings,
                            getattr(self.shader, "blend_params", None), lights, materials,
                            getattr(self.rasterizer, "fragment_cache", None))

    def __call__(self, meshes_world, cameras=None, lights=None, materials=None, **kw):
        rgb, cov = self.render(meshes_world, cameras, lights, materials)
        # hard path: alpha of softmax_rgb_blend with K=1 is in [0.5,1) on covered pixels, 0 elsewhere; only
        # (alpha > 0) is ever consumed (utils.py:72), so the 0/1 mask stands in for it.  Soft path: the real alpha.
        return torch.cat([rgb, cov], dim=1).permute(0, 2, 3, 1)

    def to(self, *a, **k):
        return self
