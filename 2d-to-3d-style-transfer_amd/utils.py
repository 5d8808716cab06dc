"""Host helpers with the reference's ``utils.py`` surface (names, arguments, return layouts of
reference utils.py:19-210) implemented on libst3d -- no torchvision, no PyTorch3D.

What differs from the reference, none of it visible in results:
  * ``render_meshes`` submits every camera of the batch in one set of launches (the reference calls the
    renderer once per camera, :68-69) and takes NCHW colour + coverage straight from the shade kernel
    instead of slicing and permuting an RGBA image (:70-76);
  * ``get_vgg`` never downloads: a local state_dict (argument or ST3D_VGG19_WEIGHTS) or seeded weights;
  * ``setup_optimizations`` returns the fused HIP Adam (st3d.optim.Adam), which also sums the gradient
    over ranks when the view batch is sharded across GPUs.
"""
import math
import os
import random

import numpy as np
import torch
from PIL import Image

from st3d import ops as _ops
from st3d import optim as _st3d_optim
from st3d import render as _render
from st3d import vgg as _vgg
from st3d.render import (FoVPerspectiveCameras, Meshes, RotateAxisAngle, TexturesAtlas, TexturesUV,  # noqa: F401
                         TexturesVertex, look_at_view_transform)
from style_transfer import *  # noqa: F401,F403  (star re-export relied on by the CLIs, reference utils.py:12)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


# ------------------------------------------------------------------------------------------ compositing
class _Composite(torch.autograd.Function):
    """out = img * mask + bg * (1 - mask) in one launch; d out / d img = mask."""

    @staticmethod
    def forward(ctx, img, mask, bg):
        ctx.mask = mask
        return _ops.apply_background(img.detach(), mask, bg)

    @staticmethod
    def backward(ctx, grad_out):
        return _ops.apply_background(grad_out.contiguous(), ctx.mask, None), None, None


def _composite(tensors, masks, background):
    out = _Composite.apply(tensors, masks, background)
    # the composite hands its gradient to the render and to nobody else (the background is a constant): the render's
    # coverage tag (st3d.render.tag_need) holds for the composite too
    tag = _render.need_of(tensors)
    if tag is not None and out.requires_grad:
        setattr(out, _render.NEED_TAG, tag)
        if getattr(tensors, _render.EPOCH_TAG, None) is not None:       # (the coverage's geometry epoch with it; not the flat tag)
            setattr(out, _render.EPOCH_TAG, getattr(tensors, _render.EPOCH_TAG))
    return out


def apply_background(tensors, masks, background_type='noise', background=None):
    """reference :19-30 -- 'white' is the identity because the renderer's own background is white;
    'noise' draws a fresh U[0,1) image per call; any other type returns None like the reference."""
    if background_type == 'white':
        return tensors
    if background_type == 'style':
        return _composite(tensors, masks, background)
    if background_type == 'noise':
        return _composite(tensors, masks, torch.rand(tensors.shape, device=tensors.device))
    return None


# ------------------------------------------------------------------------------------------ images
def load_as_tensor(image_path, size=512):
    """File -> (3,size,size) float32 in [0,1] on `device`: RGB decode, PIL's antialiased bilinear
    resize, /255 -- what transforms.Resize((size,size)) + ToTensor() give for a PIL image (:34-44)."""
    with Image.open(image_path) as im:
        rgb = im.convert('RGB').resize((size, size), Image.BILINEAR)
    hwc = torch.from_numpy(np.array(rgb, dtype=np.uint8))
    return (hwc.permute(2, 0, 1).float() / 255.0).contiguous().to(device)


def tensor_to_image(tensor):
    """(1,3,H,W) or (3,H,W) -> PIL image; values clamped to [0,1], scaled by 255 and truncated
    (ToPILImage semantics, :56-61)."""
    chw = tensor.detach().reshape(tensor.shape[-3:]).clamp(0, 1).cpu()
    return Image.fromarray((chw * 255).to(torch.uint8).permute(1, 2, 0).numpy())


def get_vgg(weights=None, seed=0):
    """Frozen VGG-19 feature stack (:48-52) as an st3d.vgg.Vgg19Features."""
    return _vgg.get_vgg(weights=weights, device=device, seed=seed)


# ------------------------------------------------------------------------------------------ rendering
def render_meshes(renderer, meshes, cameras):
    """-> colour (n,3,H,W), mask (n,1,H,W) with mask = (alpha > 0) as float (:65-77)."""
    colour, coverage = renderer.render(meshes, cameras)
    if not renderer.is_hard or getattr(renderer, "supersample", 1) > 1:
        # soft settings hand back alpha itself, a supersampled render the covered share of each pixel
        coverage = (coverage.detach() > 0).float()
    return colour, coverage


def save_render(renderer, meshes, cameras, path):
    """view_<k>.png for every camera (:81-91)."""
    os.makedirs(path, exist_ok=True)
    colour, _ = render_meshes(renderer, meshes, cameras)
    for k, img in enumerate(colour):
        tensor_to_image(img).save(os.path.join(path, f"view_{k}.png"))


def finalize_tensor(tensor):
    return tensor.detach().clamp(0.0, 1.0)


def finalize_mesh(mesh):
    """Same geometry and UVs, texture clamped to displayable range and detached (:95-104)."""
    tex = mesh.textures
    if isinstance(tex, TexturesVertex):
        return Meshes(verts=mesh.verts_padded(), faces=mesh.faces_padded(),
                      textures=TexturesVertex(finalize_tensor(tex.verts_features_packed())))
    if isinstance(tex, TexturesAtlas):
        return Meshes(verts=mesh.verts_padded(), faces=mesh.faces_padded(),
                      textures=TexturesAtlas(finalize_tensor(tex.atlas_packed())))
    clamped = TexturesUV(maps=finalize_tensor(tex.maps_padded()), faces_uvs=tex.faces_uvs_padded(),
                         verts_uvs=tex.verts_uvs_padded())
    return Meshes(verts=mesh.verts_padded(), faces=mesh.faces_padded(), textures=clamped)


def build_mesh(verts_uvs, faces_uvs, texture_map, verts, faces):
    """Fresh containers around the (possibly leaf) tensors, rebuilt every step like the reference (:207-210)."""
    return Meshes(verts=[verts], faces=[faces],
                  textures=TexturesUV(maps=texture_map, faces_uvs=faces_uvs, verts_uvs=verts_uvs))


def build_mesh_vertex(verts_features, verts, faces):
    """build_mesh for per-vertex colours: verts_features (V,3) or (1,V,3), one RGB triple per vertex (TexturesVertex)."""
    return Meshes(verts=[verts], faces=[faces], textures=TexturesVertex(verts_features))


def build_mesh_atlas(atlas, verts, faces):
    """build_mesh for a per-face texel atlas: atlas (F,R,R,3) or (1,F,R,R,3), one R x R block per face (TexturesAtlas)."""
    return Meshes(verts=[verts], faces=[faces], textures=TexturesAtlas(atlas))


# ------------------------------------------------------------------------------------------ cameras
def build_fixed_cameras(n_views, dist=3.0, shuffle=True):
    """Turntable: the first n//2 views rotate the object about X by linspace(0,315), the rest about Y by
    linspace(45,315); the camera sits at T=(0,0,dist); order shuffled with Python's RNG (:121-151)."""
    n_x = n_views // 2
    plan = [("X", float(a)) for a in torch.linspace(0, 315, n_x)]
    plan += [("Y", float(a)) for a in torch.linspace(45, 315, n_views - n_x)]
    if shuffle:
        random.shuffle(plan)
    rot = [RotateAxisAngle(angle, axis=axis).get_matrix()[0, :3, :3] for axis, angle in plan]
    R = torch.stack(rot) if rot else torch.zeros(0, 3, 3)
    T = torch.tensor([0.0, 0.0, dist]).expand(len(plan), 3).clone()
    return FoVPerspectiveCameras(R=R, T=T, device=device)


def build_random_cameras(n_views, dist=2.10, generator=None):
    """Uniform directions on the sphere around the look-at point (0, 0.10, 0.25): cos(polar) ~ U(-1,1),
    azimuth ~ U(-180,180) degrees (:154-170).  `generator` seeds the draws (the reference is unseeded)."""
    u = torch.rand(n_views, generator=generator)
    elev = torch.acos(2.0 * u - 1.0) * 180 / torch.pi - 90        # same op order as the reference: bit-equal angles
    azim = 360.0 * torch.rand(n_views, generator=generator) - 180.0
    R, T = look_at_view_transform(dist=dist, elev=elev, azim=azim, at=((0, 0.10, 0.25),))
    return FoVPerspectiveCameras(R=R, T=T, device=device)


def build_coverage_cameras(n_views, mesh, image_size, candidates=256, dist=2.10, generator=None):
    """n_views of `candidates` directions drawn by build_random_cameras(candidates, dist, generator), chosen greedily so that
    together they touch as many texels of the mesh's map as they can (st3d.cover.select_cameras, rendered at image_size)
    -> (cameras in pick order, the selection's report).  A TexturesUV mesh only (NotImplementedError otherwise)."""
    from st3d import cover as _cover
    if isinstance(n_views, bool) or int(n_views) != n_views or isinstance(candidates, bool) or int(candidates) != candidates \
            or not 1 <= n_views <= candidates <= _cover.MAX_CANDIDATES:
        raise ValueError(f"need 1 <= n_views <= candidates <= {_cover.MAX_CANDIDATES}, got n_views = {n_views!r}, "
                         f"candidates = {candidates!r}")
    pool = build_random_cameras(int(candidates), dist=dist, generator=generator)
    return _cover.select_cameras(mesh, pool, int(n_views), image_size)


def bake_texture(mesh, images, cameras, image_size, mode='mean', power=2.0, min_cos=0.1, **kwargs):
    """Bake `images` (B,3,S,S), one per camera of `cameras` at S = image_size, into the texture map of `mesh` by UV-space
    back-projection (st3d.bake.bake_texture): every texel of the chart takes the colour the views show at its surface
    point, blended by |cos|^power of the viewing angle ('mean') or from the squarest view alone ('best')
    -> (texture (T,T,3): baked where a view reached the texel, the mesh's own map elsewhere; acc (T,T,4): weighted colour
    sums and weights).  A TexturesUV mesh only (NotImplementedError otherwise)."""
    from st3d import bake as _bake
    return _bake.bake_texture(mesh, images, cameras, image_size, mode=mode, power=power, min_cos=min_cos, **kwargs)


FILL_MODES = ('chart', 'map')


def fill_texture(mesh, original_map, mode='chart', moved_from=None):
    """Fill the texels of `mesh`'s texture map that never moved away from `original_map` ((H,W,3) or (1,H,W,3), the map the
    run started from) by a pull-push fill from the texels that did (st3d.fill.fill_unseen) -> (a mesh of the same geometry
    and UVs with the filled map, report).  mode 'chart' writes only texels the chart or its 1.5-texel gutter owns
    (st3d.bake.texel_surface; a square map only), 'map' every texel -- the dilation a mip-mapping viewer needs.  moved_from:
    the mesh whose map is compared with original_map bit for bit (a run compares its unclamped leaf and fills the clamped
    map), None = `mesh` itself.  report: 'moved', 'filled', 'domain' (texel counts: moved at all, filled, open to the fill),
    'mask' ((H,W) uint8, 1 = filled).  A TexturesUV mesh only (NotImplementedError otherwise)."""
    from st3d import bake as _bake
    from st3d import fill as _fill
    tex = mesh.textures
    if not isinstance(tex, TexturesUV):
        raise NotImplementedError(f"the fill needs a TexturesUV mesh (a texture map to fill), got {type(tex).__name__}")
    if mode not in FILL_MODES:
        raise ValueError(f"mode must be 'chart' or 'map', got {mode!r}")
    maps = tex.maps_padded()
    H, W = int(maps.shape[-3]), int(maps.shape[-2])
    if mode == 'chart' and H != W:
        raise NotImplementedError(f"mode 'chart' needs a square texture map (the texel -> surface map is square), got {H} x {W}; "
                                  "mode 'map' fills any")
    texture = maps.detach().to(torch.float32).reshape(H, W, 3).contiguous()
    source = tex if moved_from is None else moved_from.textures
    if not isinstance(source, TexturesUV) or tuple(source.maps_padded().shape[-3:]) != (H, W, 3):
        raise ValueError(f"moved_from must be a TexturesUV mesh with a {H} x {W} map")
    leaf = source.maps_padded().detach().to(torch.float32).reshape(H, W, 3).contiguous()
    if original_map.numel() != H * W * 3:
        raise ValueError(f"original_map must be ({H}, {W}, 3), got {tuple(original_map.shape)}")
    original = original_map.detach().to(torch.float32).reshape(H, W, 3).contiguous()
    valid = _fill.moved_texels(leaf, original)
    domain = None
    if mode == 'chart':
        uvs = tex.verts_uvs_padded().detach().to(torch.float32).reshape(-1, 2).contiguous()
        t2f, _ = _bake.texel_surface(uvs, tex.faces_uvs_i32(), H)
        domain = (t2f >= 0).to(torch.uint8)
    filled, count = _fill.push_pull(texture, valid, domain)
    moved = int(valid.sum())
    open_ = valid == 0 if domain is None else (valid == 0) & (domain != 0)      # filled, unless nothing moved at all
    report = {"moved": moved, "filled": int(count), "domain": H * W if domain is None else int(domain.sum()),
              "mask": (open_ if moved else torch.zeros_like(open_)).to(torch.uint8)}
    out = Meshes(verts=mesh.verts_padded(), faces=mesh.faces_padded(),
                 textures=TexturesUV(maps=filled.reshape(maps.shape), faces_uvs=tex.faces_uvs_padded(),
                                     verts_uvs=tex.verts_uvs_padded()))
    return out, report


# ------------------------------------------------------------------------------------------ optimiser
_LEAVES ={'texture': ('texture_map',), 'mesh': ('verts',), 'both': ('verts', 'texture_map')}
_VERTEX_LEAVES = {'texture': ('verts_features',), 'mesh': ('verts',), 'both': ('verts', 'verts_features')}
_ATLAS_LEAVES = {'texture': ('atlas',), 'mesh': ('verts',), 'both': ('verts', 'atlas')}


def _diffused_optimizer(parts, lam, colour_leaves, lr):
    """verts_diffusion > 0: the vertex leaf becomes the parameters of an st3d.largesteps.DiffusedVertices (under
    'verts_diffusion'), 'verts' the vertices they stand for, and Adam sees them first, in a group of their own."""
    from st3d.largesteps import DiffusedVertices
    dv = DiffusedVertices(parts['verts'], parts['faces'], lam)
    parts['verts_diffusion'] = dv
    parts['verts'] = dv.verts()
    groups = [{"params": [dv.params], "uniform": True}]
    if colour_leaves:
        groups.append({"params": list(colour_leaves)})
    return _st3d_optim.Adam(groups, lr=lr)


def refresh_verts(parts):
    """After an optimiser step of a verts_diffusion run: parts['verts'] = the vertices of the stepped parameters (one
    solve).  Without diffusion 'verts' is the leaf itself and nothing happens.  -> parts['verts']"""
    dv = parts.get('verts_diffusion')
    if dv is not None:
        parts['verts'] = dv.verts()
    return parts['verts']


def setup_optimizations(optimization_target, mesh, lr, texture_pyramid_levels=1, verts_diffusion=0.0):
    """Clone the mesh, mark the tensors `optimization_target` names as leaves and put ONE Adam (single lr,
    default betas/eps) over them (:173-204).  Keys of the returned dict are the reference's.

    texture_pyramid_levels != 1 (0 = auto, L >= 2; targets 'texture' / 'both'): the texture leaf is the flat parameter
    tensor of an st3d.texpyr.TexturePyramid, returned under 'texture_pyramid' (for 'both' Adam sees the vertices first,
    then the pyramid).  The dict then has NO 'texture_map' entry -- the map is pyramid.texture(), rebuilt every step.

    A mesh whose textures are a TexturesVertex: 'verts_features' (V,3) takes the place of 'texture_map' / 'verts_uvs' /
    'faces_uvs'; leaves are 'texture' -> the colours, 'mesh' -> the vertices, 'both' -> the vertices, then the colours.
    There is no map to build a pyramid of: texture_pyramid_levels != 1 is a ValueError.

    A mesh whose textures are a TexturesAtlas: 'atlas' (F,R,R,3) takes that place in the same way ('texture' -> the atlas,
    'mesh' -> the vertices, 'both' -> the vertices, then the atlas; the colour moves no vertex, so under 'mesh' and 'both'
    the vertices move by the other terms of the loss alone); texture_pyramid_levels != 1 is a ValueError.

    verts_diffusion = lambda > 0 (targets 'mesh' / 'both', any of the three texture kinds): the vertex leaf is the (V,3)
    parameter tensor u = (I + lambda L) verts of an st3d.largesteps.DiffusedVertices, returned under 'verts_diffusion', in an
    Adam group with "uniform": True; 'verts' holds verts() of the current parameters (refresh_verts(dict) after a step).
    0 (the default) is the plain vertex leaf: no object is made and no call is added.  With 'texture', or a negative or
    non-finite value: ValueError."""
    lam = float(verts_diffusion)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"verts_diffusion must be finite and >= 0, got {verts_diffusion!r}")
    if lam > 0.0 and optimization_target == 'texture':
        raise ValueError("verts_diffusion needs optimization_target 'mesh' or 'both': with 'texture' the vertices do not move")
    if isinstance(mesh.textures, TexturesAtlas):
        if optimization_target not in _ATLAS_LEAVES:
            raise UnboundLocalError("local variable 'optimizer' referenced before assignment "
                                    f"(optimization_target={optimization_target!r})")
        if texture_pyramid_levels != 1:
            raise ValueError("texture_pyramid_levels != 1 needs a texture map: a TexturesAtlas mesh has per-face texel blocks "
                             "and no map to build a pyramid of")
        work = mesh.clone()
        parts = {'atlas': work.textures.atlas_packed(), 'verts': work.verts_packed(), 'faces': work.faces_packed()}
        if lam > 0.0:
            colour = [parts['atlas'].requires_grad_(True)] if optimization_target == 'both' else []
            return dict(parts, optimizable_mesh=work, optimizer=_diffused_optimizer(parts, lam, colour, lr))
        leaves = [parts[name].requires_grad_(True) for name in _ATLAS_LEAVES[optimization_target]]
        return dict(parts, optimizable_mesh=work, optimizer=_st3d_optim.Adam(leaves, lr=lr))
    if isinstance(mesh.textures, TexturesVertex):
        if optimization_target not in _VERTEX_LEAVES:
            raise UnboundLocalError("local variable 'optimizer' referenced before assignment "
                                    f"(optimization_target={optimization_target!r})")
        if texture_pyramid_levels != 1:
            raise ValueError("texture_pyramid_levels != 1 needs a texture map: a TexturesVertex mesh has per-vertex colours "
                             "and no map to build a pyramid of")
        work = mesh.clone()
        parts = {'verts_features': work.textures.verts_features_packed(), 'verts': work.verts_packed(),
                 'faces': work.faces_packed()}
        if lam > 0.0:
            colour = [parts['verts_features'].requires_grad_(True)] if optimization_target == 'both' else []
            return dict(parts, optimizable_mesh=work, optimizer=_diffused_optimizer(parts, lam, colour, lr))
        leaves = [parts[name].requires_grad_(True) for name in _VERTEX_LEAVES[optimization_target]]
        return dict(parts, optimizable_mesh=work, optimizer=_st3d_optim.Adam(leaves, lr=lr))
    work = mesh.clone()
    parts = {
        'texture_map': work.textures.maps_padded(),
        'verts': work.verts_packed(),
        'faces': work.faces_packed(),
        'verts_uvs': work.textures.verts_uvs_padded(),
        'faces_uvs': work.textures.faces_uvs_padded(),
    }
    if optimization_target not in _LEAVES:      # the reference falls through to an unbound `optimizer`
        raise UnboundLocalError("local variable 'optimizer' referenced before assignment "
                                f"(optimization_target={optimization_target!r})")
    if texture_pyramid_levels != 1:
        if optimization_target == 'mesh':
            raise ValueError("a texture pyramid needs optimization_target 'texture' or 'both': with 'mesh' the texture is "
                             "not optimised")
        from st3d.texpyr import TexturePyramid
        parts['texture_pyramid'] = TexturePyramid(parts.pop('texture_map'), texture_pyramid_levels)
        if lam > 0.0:           # 'both': the target 'mesh' was refused above
            return dict(parts, optimizable_mesh=work,
                        optimizer=_diffused_optimizer(parts, lam, [parts['texture_pyramid'].params], lr))
        leaves = [parts['verts'].requires_grad_(True)] if optimization_target == 'both' else []
        leaves.append(parts['texture_pyramid'].params)
        return dict(parts, optimizable_mesh=work, optimizer=_st3d_optim.Adam(leaves, lr=lr))
    if lam > 0.0:
        colour = [parts['texture_map'].requires_grad_(True)] if optimization_target == 'both' else []
        return dict(parts, optimizable_mesh=work, optimizer=_diffused_optimizer(parts, lam, colour, lr))
    leaves = [parts[name].requires_grad_(True) for name in _LEAVES[optimization_target]]
    return dict(parts, optimizable_mesh=work, optimizer=_st3d_optim.Adam(leaves, lr=lr))
