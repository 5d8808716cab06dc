"""Drop-in for the reference's ``losses.py`` (same five functions, argument order, defaults and
error behaviour: reference losses.py:12,48,55,68,101) on libst3d.

``compute_perceptual_loss`` returns a scalar tensor whose ``.backward()`` (called by the caller,
second_approach.py:188) delivers d loss / d current_imgs from the fused plan: the VGG forward,
Gram/content losses and the whole backward run inside ONE autograd node (the gradient is
produced together with the loss, so ``backward()`` only scales and hands it on).  Content
features and style Grams (reference :18-25) do not depend on the optimised parameters and are
cached on the tensors' identity/version, i.e. recomputed exactly when the caller passes new or
modified content/style images.
"""
import math
import os

import torch
from torch.nn import functional as F  # noqa: F401  (star-import surface of the reference module)

from st3d import lap as _lap
from st3d import mesh_losses as _mesh_losses
from st3d import ops as _ops
from st3d import render as _render
from st3d import vgg as _vgg
from st3d.mesh_losses import mesh_edge_loss, mesh_laplacian_smoothing, mesh_normal_consistency  # noqa: F401
from st3d.mesh_losses import chamfer_distance, knn_points, sample_points_from_meshes  # noqa: F401
from style_transfer import *  # noqa: F401,F403  (the reference does the same, losses.py:5)

# Check if CUDA is available
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class _PerceptualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, current, plan, style_weight, content_weight, batch_denom, need_mask=None, flat_color=None, style_mask=None,
                epoch=0):
        loss, grad = plan.loss(current, style_weight, content_weight, batch_denom=batch_denom,
                               want_grad=current.requires_grad, need_mask=need_mask, flat_color=flat_color,
                               style_mask=style_mask, epoch=epoch)
        ctx.grad = grad
        ctx.parts = loss.clone()
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.grad * grad_out if ctx.grad is not None else None
        return g, None, None, None, None, None, None, None, None


#method for the second approach
def check_style_masks(style_masks, n, S):
    """None, or the guidance of the style term: (n,1,S,S) or (n,S,S) on the GPU, values in [0,1] (a render's coverage)"""
    if style_masks is None:
        return None
    if not torch.is_tensor(style_masks):
        raise TypeError("style_masks must be a tensor (n,1,S,S) or (n,S,S)")
    if not style_masks.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU style_masks -- there is no CPU fallback")
    shp = tuple(style_masks.shape)
    if shp not in ((n, 1, S, S), (n, S, S)):
        raise ValueError(f"style_masks must be ({n},1,{S},{S}) or ({n},{S},{S}), got {shp}")
    return style_masks.detach().to(torch.float32)


class _MultiScaleFn(torch.autograd.Function):
    """sum_f w_f L_f over an image pyramid (st3d.imgpyr): L_f is the fused loss of the images reduced by f
    against the content and style reduced by f, on the plan of side S / f.  Scales are visited in ascending f; the loss is
    added in that order in fp32, and so is the gradient, w_f x the pyramid's transpose of the coarse plan's gradient.  f = 1
    is the single-scale call with its need / flat / epoch tags; a coarse plan gets the need mask reduced with the images
    (reduce_need), no flat colour and no epoch.  A weight of 0 skips its scale: no plan, no launch."""

    @staticmethod
    def forward(ctx, current, model, content, style, style_weight, content_weight, batch_denom, style_masks, scales, weights,
                tags):
        from st3d import imgpyr as _imgpyr
        need, flat, epoch = tags
        B, S = current.shape[0], current.shape[2]
        want = current.requires_grad
        cur = current.detach().to(torch.float32).contiguous()
        masks = style_masks.reshape(B, 1, S, S) if style_masks is not None else None
        total = grad = None
        for f, w in zip(scales, weights):
            if w == 0.0:
                continue
            plan = model.plan(B, S // f)
            plan.set_content(_imgpyr.reduced_cached(content, f))
            plan.set_style(_imgpyr.reduced_cached(style, f), B)
            if f == 1:
                loss, g = plan.loss(cur, style_weight, content_weight, batch_denom=batch_denom, want_grad=want, need_mask=need,
                                    flat_color=flat, style_mask=style_masks, epoch=epoch)
            else:
                loss, g = plan.loss(_imgpyr.reduce(cur, f), style_weight, content_weight, batch_denom=batch_denom,
                                    want_grad=want, need_mask=_imgpyr.reduce_need(need, f) if need is not None else None,
                                    style_mask=_imgpyr.reduce(masks, f) if masks is not None else None)
                while g is not None and g.shape[2] < S:
                    g = _ops.pyr_down_bwd(g)
            term = loss[0] * w
            total = term if total is None else total + term
            if g is not None:
                g = g * w if w != 1.0 else g
                grad = g if grad is None else grad + g
        if total is None:       # every weight is 0
            total = torch.zeros((), dtype=torch.float32, device=cur.device)
            grad = torch.zeros_like(cur) if want else None
        ctx.grad = grad
        return total.clone()

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.grad * grad_out if ctx.grad is not None else None
        return (g,) + (None,) * 10


def compute_perceptual_loss(current_imgs, content_imgs, style_imgs, model, style_weight=1e6, content_weight=1, *,
                            batch_denom=None, style_masks=None, scales=(1,), scale_weights=None):
    # scales / scale_weights: the multi-scale loss (Gatys et al. 2017; Heitz et al. 2021) -- sum_f w_f L_f, L_f this loss
    # of the images reduced by f in {1, 2, 4} (st3d.imgpyr: the [1 3 3 1] / 8 pyramid) against content and style reduced
    # alike, on the plan of side S / f: VGG's receptive fields, fixed in pixels, then also cover the large shapes of the
    # style.  S % f == 0 and S / f >= 32.  The default is the single-scale loss and runs none of this.

    # Ensure content_imgs and style_imgs are batched tensors
    assert current_imgs.shape[0] == content_imgs.shape[0] == style_imgs.shape[0]
    multi_scale = not (isinstance(scales, tuple) and scales == (1,) and scale_weights is None)
    if multi_scale:
        from st3d import imgpyr as _imgpyr
        scales, scale_weights = _imgpyr.check_scales(scales, scale_weights, current_imgs.shape[2])
    if not isinstance(model, _vgg.Vgg19Features):
        raise TypeError("compute_perceptual_loss needs the st3d VGG returned by utils.get_vgg()")
    if not current_imgs.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")

    B, S = current_imgs.shape[0], current_imgs.shape[2]
    # style_masks: the guided style loss (Gatys et al. 2017) -- each style tap's Gram of the current images is taken over
    # the masked region (the object's coverage), so the background neither takes part in the style term nor draws its
    # gradient; the style targets stay the plain Grams, the content term is unchanged, the masks carry no gradient
    style_masks = check_style_masks(style_masks, B, S)
    if not multi_scale:
        plan = model.plan(B, S)
        plan.set_content(content_imgs)          # conv4_2 of content      (reference :18)
        plan.set_style(style_imgs, B)           # Grams of style features (reference :19-25)

    # A render tags its colour tensor with its coverage (st3d.render.tag_need): its backward reads the image gradient at
    # covered pixels only, so the plan computes the gradient there (bit for bit) and writes 0 elsewhere, skipping the part
    # of the VGG backward only the background would need.  Anything else -- pixels optimised directly, a tensor derived
    # from the render, somebody watching the tensor's own gradient, ST3D_NEED_MASK=0 -- takes the full path.
    need = None if os.environ.get("ST3D_NEED_MASK", "1") == "0" else _render.need_of(current_imgs)

    # A render also tags its colour tensor with its background colour (st3d.render.tag_flat): the shallow forward convs
    # then compute the tiles that see anything but the flat field and copy the rest -- the same bits (the device compares the
    # pixels, the tag only decides whether the lists are built; ST3D_FLAT=0 is read by the library).  Composites onto a
    # style / noise background and pixels optimised directly carry no tag and take the full forward.
    flat = _render.flat_of(current_imgs)

    # A render whose fragments came from its rasteriser's cache also names the geometry epoch of its coverage tag
    # (st3d.render.FragmentCache): views whose vertices, faces and cameras have not changed since the tag was made.  The plan
    # then keeps what depends on the coverage alone -- its need lists, its flat-field lists, the background it has copied into
    # the shallow buffers -- from one step to the next (PerceptualPlan.loss(epoch=...)); 0 = no epoch, every call rebuilds.
    # ST3D_EPOCHS=0 (read per call): the A/B switch -- every call rebuilds and fills.
    epoch = 0 if os.environ.get("ST3D_EPOCHS", "1") == "0" else _render.epoch_of(current_imgs, need)

    if multi_scale:         # every scale sets the targets of its own plan; the tags above serve f = 1
        return _MultiScaleFn.apply(current_imgs, model, content_imgs, style_imgs, float(style_weight), float(content_weight),
                                   batch_denom, style_masks, scales, scale_weights, (need, flat, epoch))

    # batch_denom: the batch the means divide by -- the GLOBAL batch when views are sharded over ranks
    return _PerceptualFn.apply(current_imgs, plan, float(style_weight), float(content_weight), batch_denom, need, flat, style_masks, epoch)


def _region_content_target(content_imgs, model):
    """conv4_2 of the content images, computed once: cached on the model under the tensor's identity and version"""
    import style_transfer as _st
    key = (content_imgs.data_ptr(), content_imgs._version, tuple(content_imgs.shape), tuple(content_imgs.stride()))
    cache = model.__dict__.setdefault("_region_content_cache", {})
    hit = cache.get(key)
    if hit is not None and hit[0].data_ptr() == content_imgs.data_ptr():
        return hit[1]
    with torch.no_grad():
        tap = {k: v for k, v in _st._DEFAULT_LAYERS.items() if v == _st.REGION_CONTENT_TAP}
        target = _st.get_features(content_imgs.detach().to(torch.float32).contiguous(), model, tap)[_st.REGION_CONTENT_TAP]
    if len(cache) >= 8:         # (the alternating view batches of a run, as PerceptualPlan.CONTENT_CACHE)
        cache.pop(next(iter(cache)))
    cache[key] = (content_imgs, target)
    return target


def compute_region_style_loss(current_imgs, content_imgs, style_imgs, pix_to_face, face_regions, model, style_weight=1e6,
                              content_weight=1, *, region_weights=None, batch_denom=None, planes=None):
    """compute_perceptual_loss with one style image per region of the mesh (st3d.regions; Gatys et al. 2017, spatial
    control): content_weight x the conv4_2 content term + style_weight x style_transfer.region_style_loss.
    ``style_imgs`` (R,3,S,S): region r's style image; ``pix_to_face`` (B,S,S) int32: the fragments of the renders that
    ``current_imgs`` are (st3d.regions.fragments_of gives them); ``face_regions``: the uint8 labels of
    regions.check_face_regions (R = style_imgs.shape[0]).  For R = 1 with every face in region 0 the value is the one
    compute_perceptual_loss(style_masks=coverage) defines; background pixels belong to no region.  ``planes``: the
    (planes, sums) of regions.region_planes for these fragments, when the caller keeps them (unchanged geometry).
    One differentiable get_features over the current images, the R x 5 guided Grams, the ordered loss sums, per tap R
    accumulating Gram backwards, then the plan's backward: the term gives up the fused plan's need / flat / epoch
    shortcuts.  The scalar carries ``parts`` (3,) [total, content, style].  Gradient to ``current_imgs`` only."""
    import style_transfer as _st
    from st3d import regions as _regions
    if not isinstance(model, _vgg.Vgg19Features):
        raise TypeError("compute_region_style_loss needs the st3d VGG returned by utils.get_vgg()")
    if not all(torch.is_tensor(t) for t in (current_imgs, content_imgs, style_imgs)):
        raise TypeError("current_imgs, content_imgs and style_imgs must be tensors")
    if not (current_imgs.is_cuda and content_imgs.is_cuda and style_imgs.is_cuda):
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    if current_imgs.dim() != 4 or current_imgs.shape[1] != 3 or current_imgs.shape[2] != current_imgs.shape[3]:
        raise ValueError(f"current_imgs must be (B,3,S,S), got {tuple(current_imgs.shape)}")
    B, S = current_imgs.shape[0], current_imgs.shape[2]
    if tuple(content_imgs.shape) != (B, 3, S, S):
        raise ValueError(f"content_imgs must be ({B},3,{S},{S}), got {tuple(content_imgs.shape)}")
    R = int(style_imgs.shape[0]) if style_imgs.dim() == 4 else 0
    if tuple(style_imgs.shape) != (R, 3, S, S) or not 1 <= R <= _regions.MAX_REGIONS:
        raise ValueError(f"style_imgs must be (R,3,{S},{S}) with R in 1..{_regions.MAX_REGIONS}, one image per region; got "
                         f"{tuple(style_imgs.shape)}")
    lambdas = _st.check_region_weights(region_weights, R)
    targets = _regions.region_targets(style_imgs, model)
    content_target = _region_content_target(content_imgs, model)
    if planes is None:
        if tuple(pix_to_face.shape[:3]) != (B, S, S):
            raise ValueError(f"pix_to_face must be ({B},{S},{S}), got {tuple(pix_to_face.shape)}")
        planes = _regions.region_planes(pix_to_face, face_regions, R)
    q, sums = planes
    layers = dict(_st.REGION_STYLE_TAPS)
    layers.update({k: v for k, v in _st._DEFAULT_LAYERS.items() if v == _st.REGION_CONTENT_TAP})
    feats = _st.get_features(current_imgs, model, layers)           # targets first: this forward is the plan's last
    taps, _, bd = _st._region_check(feats, q, sums, targets, lambdas, batch_denom)
    masked = _st._region_masked_targets(sums, targets, B)
    with _ops.trace("region_style_loss"):
        loss, parts = _st._RegionLossFn.apply((q, masked, lambdas, bd, float(style_weight), float(content_weight),
                                               content_target), *taps, feats[_st.REGION_CONTENT_TAP])
    loss.parts = parts
    return loss


def compute_nnfm_loss(current_imgs, style_imgs, model, layers=('conv3_1',), *, masks=None, batch_denom=None):
    """The NNFM style term (Zhang et al., "ARF", ECCV 2022; style_transfer.nnfm_loss) of ``current_imgs`` (B,3,S,S) against
    ``style_imgs`` ((1 or B,3,Ss,Ss); one image expanded over the batch is searched as one style), summed over ``layers``
    (names from conv2_1, conv3_1, conv4_1, conv4_2, conv5_1).  The taps come through ``get_features``: differentiable for
    the current images, without gradient and cached on the style tensor's identity and version for the style.  ``masks``
    (B,1,S,S) | (B,S,S) in [0,1], e.g. the renders' coverage, weight the positions; ``batch_denom`` is the global batch when
    the views are sharded.  Cost: the term makes its own partial VGG forward and backward up to its deepest tap, next to
    the fused plan's of compute_perceptual_loss.  The term always looks at the full-resolution images: the image pyramid of
    compute_perceptual_loss(scales=...) does not reach it."""
    import style_transfer as _st
    if not isinstance(model, _vgg.Vgg19Features):
        raise TypeError("compute_nnfm_loss needs the st3d VGG returned by utils.get_vgg()")
    if not torch.is_tensor(current_imgs) or not torch.is_tensor(style_imgs):
        raise TypeError("current_imgs and style_imgs must be tensors")
    if not current_imgs.is_cuda or not style_imgs.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    layers = _st.check_nnfm_layers(layers)
    if current_imgs.dim() != 4 or current_imgs.shape[1] != 3 or style_imgs.dim() != 4 or style_imgs.shape[1] != 3:
        raise ValueError("current_imgs and style_imgs must be (B,3,S,S)")
    B, S = current_imgs.shape[0], current_imgs.shape[2]
    if style_imgs.shape[0] not in (1, B):
        raise ValueError(f"style_imgs must hold 1 or {B} images, got {style_imgs.shape[0]}")
    masks = check_style_masks(masks, B, S)
    return _st._nnfm_term(current_imgs, style_imgs, model, layers, masks, batch_denom)


def compute_swd_loss(current_imgs, style_imgs, model, layers=('conv2_1', 'conv3_1', 'conv4_1', 'conv5_1'), *, directions=0,
                     generator=None, masks=None, batch_denom=None):
    """The sliced Wasserstein style term (Heitz et al., CVPR 2021; style_transfer.swd_loss) of ``current_imgs`` (B,3,S,S)
    against ``style_imgs`` ((1 or B,3,Ss,Ss); one image expanded over the batch is one style), summed over ``layers`` (names
    from conv1_1, conv2_1, conv3_1, conv4_1, conv4_2, conv5_1).  ``directions``: how many random unit directions each tap is
    projected onto, 0 = as many as it has channels, 1..512; they are drawn from ``generator`` (None: torch's default) in the
    order of ``layers`` on every call, as the paper redraws them every step -- or a dict {layer: (K,C) tensor} to hand them
    in.  The style taps are cached on the style tensor's identity and version; their projection and sort follow the
    directions.  ``masks`` (B,1,S,S) | (B,S,S) in [0,1], e.g. the renders' coverage, select the positions that take part;
    ``batch_denom`` is the global batch when the views are sharded.  Cost: its own partial VGG forward and backward up to its
    deepest tap, next to the fused plan's of compute_perceptual_loss.  The term always looks at the full-resolution images:
    the image pyramid of compute_perceptual_loss(scales=...) does not reach it."""
    import style_transfer as _st
    if not isinstance(model, _vgg.Vgg19Features):
        raise TypeError("compute_swd_loss needs the st3d VGG returned by utils.get_vgg()")
    if not torch.is_tensor(current_imgs) or not torch.is_tensor(style_imgs):
        raise TypeError("current_imgs and style_imgs must be tensors")
    if not current_imgs.is_cuda or not style_imgs.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    layers = _st.check_swd_layers(layers)
    if current_imgs.dim() != 4 or current_imgs.shape[1] != 3 or style_imgs.dim() != 4 or style_imgs.shape[1] != 3:
        raise ValueError("current_imgs and style_imgs must be (B,3,S,S)")
    B, S = current_imgs.shape[0], current_imgs.shape[2]
    if style_imgs.shape[0] not in (1, B):
        raise ValueError(f"style_imgs must hold 1 or {B} images, got {style_imgs.shape[0]}")
    masks = check_style_masks(masks, B, S)
    if isinstance(directions, dict):
        if set(directions) != set(layers) or not all(torch.is_tensor(v) for v in directions.values()):
            raise ValueError("directions handed in must be one (K,C) tensor per layer")
    else:
        directions = _st.swd_draw(layers, _st.check_swd_directions(directions), generator, current_imgs.device)
    return _st._swd_term(current_imgs, style_imgs, model, layers, masks, batch_denom, directions)


class _FusedLossFn(torch.autograd.Function):
    """A loss whose HIP call returns the value and its gradient together: backward only scales."""

    @staticmethod
    def forward(ctx, x, op, *extra):
        loss, grad = op(x.detach(), *extra, want_grad=x.requires_grad)
        ctx.grad, ctx.n_extra = grad, len(extra)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.grad * grad_out if ctx.grad is not None else None
        return (g, None) + (None,) * ctx.n_extra


def _on_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    return t.to(torch.float32)


def _texture_values(mesh):
    """what the texture regularisers read: the map of a TexturesUV, the (V,3) colours of a TexturesVertex, the (F,R,R,3)
    texels of a TexturesAtlas"""
    if isinstance(mesh.textures, _render.TexturesVertex):
        return mesh.textures.verts_features_packed()
    if isinstance(mesh.textures, _render.TexturesAtlas):
        return mesh.textures.atlas_packed()
    return mesh.textures.maps_padded()


def rgb_range_loss(mesh):
    """Sum of the texture map's (or the vertex colours') excursions outside [0,1] (reference losses.py:48-51; every call
    site in the reference is commented out).  One fused launch: value + sign gradient."""
    tex = _on_gpu(_texture_values(mesh))
    return _FusedLossFn.apply(tex, _ops.range_loss)


def compute_tv_loss(images, masks):
    """Masked anisotropic L1 total variation / sum(masks) (reference losses.py:55-65; call sites commented out
    there too).  Value and d/d images from one fused pass.  Handed a mesh with per-vertex colours in the images' place
    (total variation of the texture itself): ValueError -- vertex colours lie on no grid; nor do the blocks of a TexturesAtlas."""
    if isinstance(getattr(images, "textures", None), _render.TexturesVertex):
        raise ValueError("compute_tv_loss: a TexturesVertex mesh has per-vertex colours, which lie on no pixel grid; total "
                         "variation is defined for images (and texture maps) only")
    if isinstance(getattr(images, "textures", None), _render.TexturesAtlas):
        raise ValueError("compute_tv_loss: a TexturesAtlas mesh has per-face texel blocks, which lie on no pixel grid; total "
                         "variation is defined for images (and texture maps) only")
    return _FusedLossFn.apply(_on_gpu(images), _ops.tv_loss, _on_gpu(masks).detach())


def compute_laplacian_loss(current_imgs, content_imgs, pools=(4,), *, batch_denom=None):
    """The Laplacian content term (Li, Xu, Nie and Chua, "Laplacian-Steered Neural Style Transfer", 2017; st3d.lap) of
    ``current_imgs`` (B,C,H,W) against ``content_imgs`` of the same shape: for every pool side p of ``pools`` (strictly
    increasing, from 1, 2, 4, 8, 16, each dividing H and W with pooled sides >= 2) the mean over (batch, channel, pooled pixel)
    of (D(pool_p(current)) - D(pool_p(content)))^2, D the 5-point Laplacian with a replicate border, every channel on its
    own; the terms are added in ascending p.  The targets D(pool_p(content)) carry no gradient and are cached on the content
    tensor's identity and version.  ``batch_denom`` is the global batch when the views are sharded.  Value and
    d/d current_imgs come from one fused pass per pool side."""
    if not torch.is_tensor(current_imgs) or not torch.is_tensor(content_imgs):
        raise TypeError("current_imgs and content_imgs must be tensors")
    if current_imgs.dim() != 4 or tuple(content_imgs.shape) != tuple(current_imgs.shape):
        raise ValueError(f"current_imgs and content_imgs must be (B,C,H,W) tensors of one shape, got {tuple(current_imgs.shape)} "
                         f"and {tuple(content_imgs.shape)}")
    pools = _lap.check_pools(pools, tuple(current_imgs.shape[2:]))
    _on_gpu(content_imgs)
    targets = [_lap.lap_target_cached(content_imgs, p) for p in pools]
    return _FusedLossFn.apply(_on_gpu(current_imgs), _lap_op, targets, pools, batch_denom)


def _lap_op(x, targets, pools, batch_denom, want_grad=True):
    return _lap.lap_term(x, targets, pools, batch_denom, want_grad)


def texture_l2_loss(mesh, original_map):
    """mean((texture - original)^2): the "l2 regularization w.r.t. the original texture" idea of the reference's
    notes.txt:39 (not implemented there).  A TexturesVertex mesh: its colours against the original (V,3) colours; a
    TexturesAtlas mesh: its texels against the original (F,R,R,3) atlas."""
    tex = _on_gpu(_texture_values(mesh))
    return _FusedLossFn.apply(tex, _l2_to, _on_gpu(original_map).detach())


def _l2_to(x, ref, want_grad=True):
    if not want_grad:
        return _ops.sqdiff_sum(x, ref.reshape(x.shape), scale=1.0 / x.numel()), None
    loss, diff = _ops.sqdiff_sum(x, ref.reshape(x.shape), scale=1.0 / x.numel(), want_diff=True)
    return loss, diff * (2.0 / x.numel())


class _SilhouetteLossFn(torch.autograd.Function):
    """verts -> scale * sum (alpha - target)^2 over this call's views: project, general raster, then ONE fused launch that
    reduces the loss and writes d loss / d dists (alpha never reaches memory).  backward: raster backward of the stored
    grad_dists and the projection backward, scaled by the incoming scalar."""

    @staticmethod
    def forward(ctx, verts, faces_i32, R, T, target, S, K, blur, clip, sigma, cull, persp, z_clip, scale):
        v = verts.detach().to(torch.float32).contiguous()
        ndc = _ops.project_verts(v, R, T)
        p2f, _zbuf, _bary, dists, slots = _ops.raster_soft_fwd(ndc, faces_i32, S, K, blur, clip, cull, persp, z_clip)
        loss, gd = _ops.silhouette_loss(p2f, dists, target, sigma, scale, want_grad=verts.requires_grad)
        ctx.saved = (gd, p2f, slots, v, ndc, faces_i32, R, T, clip, persp, z_clip)
        ctx.verts_shape = verts.shape
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        gd, p2f, slots, v, ndc, faces_i32, R, T, clip, persp, z_clip = ctx.saved
        gverts = None
        if gd is not None and ctx.needs_input_grad[0]:
            gndc = _ops.raster_soft_bwd((None, None, gd), p2f, ndc, faces_i32, clip, persp, slots, z_clip)
            gverts = (_ops.project_verts_bwd(v, R, T, gndc) * grad_out).reshape(ctx.verts_shape)
        return (gverts,) + (None,) * 13


class _SilhouetteRasterLossFn(torch.autograd.Function):
    """The same loss on the silhouette rasteriser (csrc/silraster.hip) at faces_per_pixel K = 1..64: project, ONE raster pass
    from the face records to the loss (no fragments, alpha never reaches memory), backward from the saved per-pixel state
    (keep, the cut, alpha - target: 16 bytes per pixel whatever K is) to the vertices.  Projected vertices and face records
    are recomputed in the backward rather than kept."""

    @staticmethod
    def forward(ctx, verts, faces_i32, R, T, target, K, blur, clip, sigma, cull, persp, z_clip, scale):
        v = verts.detach().to(torch.float32).contiguous()
        ndc = _ops.project_verts(v, R, T)
        loss, state = _ops.silraster_loss(ndc, faces_i32, target, K, blur, sigma, scale, clip, cull, persp, z_clip)
        ctx.saved = (state if verts.requires_grad else None, v, faces_i32, R, T)
        ctx.settings = (blur, clip, sigma, cull, persp, z_clip, scale)
        ctx.verts_shape = verts.shape
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        state, v, faces_i32, R, T = ctx.saved
        blur, clip, sigma, cull, persp, z_clip, scale = ctx.settings
        gverts = None
        if state is not None and ctx.needs_input_grad[0]:
            ndc = _ops.project_verts(v, R, T)
            gndc = _ops.silraster_bwd(state, ndc, faces_i32, blur, sigma, None, 2.0 * scale, clip, cull, persp, z_clip)
            gverts = (_ops.project_verts_bwd(v, R, T, gndc) * grad_out).reshape(ctx.verts_shape)
        return (gverts,) + (None,) * 12


SILHOUETTE_FACES_PER_PIXEL = 8
SILHOUETTE_RASTER_MAX_FACES_PER_PIXEL = _ops.SILRASTER_MAX_FACES_PER_PIXEL      # 64


def check_silhouette_faces_per_pixel(faces_per_pixel):
    """None (the general rasteriser at K = 8) or an integer 1..64 (the silhouette rasteriser at that K); else ValueError"""
    if faces_per_pixel is None:
        return None
    k = faces_per_pixel
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SILHOUETTE_RASTER_MAX_FACES_PER_PIXEL:
        raise ValueError(f"faces_per_pixel must be None or an integer in 1..{SILHOUETTE_RASTER_MAX_FACES_PER_PIXEL}, "
                         f"got {faces_per_pixel!r}")
    return k


def silhouette_blur_radius(sigma):
    """PyTorch3D's silhouette-fitting tutorial: blur_radius = log(1 / 1e-4 - 1) * sigma (faces whose sigmoid falls below
    1e-4 are not rasterised)."""
    return math.log(1.0 / 1e-4 - 1.0) * float(sigma)


def compute_silhouette_loss(renderer_or_settings, mesh, cameras, target_masks, sigma=1e-4, batch_denom=None,
                            faces_per_pixel=None):
    """mean over views and pixels of (alpha - target)^2, alpha = SoftSilhouetteShader's (sigmoid_alpha_blend with
    BlendParams(sigma)): the image-space term that holds the OUTLINE when the vertices move.  target_masks (n,1,S,S), e.g.
    the 0/1 coverage of the content renders.  The silhouette pass takes image size, culling, perspective correction and the
    clipping depth from the renderer (or RasterizationSettings) given and rasterises with faces_per_pixel = 8 -- the
    kernels' maximum; PyTorch3D's tutorial uses 50 -- and blur_radius = log(1 / 1e-4 - 1) * sigma, the tutorial's rule.
    batch_denom: the GLOBAL batch the mean divides by when the views are sharded over ranks (default: this call's views).
    The mesh needs no textures.  Gradients flow to the vertices only.
    faces_per_pixel: None = the path above, bit for bit.  An integer 1..64 (PyTorch3D's tutorial: 50) = the silhouette
    rasteriser (csrc/silraster.hip) at that K: same semantics -- at K = 8 the same alpha and loss bit for bit --, no
    fragments in memory, 16 bytes per pixel kept for the backward.  Anything else: ValueError."""
    faces_per_pixel = check_silhouette_faces_per_pixel(faces_per_pixel)
    rs = getattr(getattr(renderer_or_settings, "rasterizer", None), "raster_settings", renderer_or_settings)
    if not isinstance(rs, _render.RasterizationSettings):
        raise TypeError("compute_silhouette_loss takes a MeshRenderer or RasterizationSettings")
    if not float(sigma) > 0.0:
        raise ValueError("sigma must be positive")
    verts = mesh.verts_packed()
    if not verts.is_cuda or not target_masks.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    R, T = _render.join_cameras(cameras)
    n, S = R.shape[0], rs.image_size
    if target_masks.numel() != n * S * S:
        raise ValueError(f"target_masks must be ({n},1,{S},{S}), got {tuple(target_masks.shape)}")
    scale = 1.0 / (float(S) * float(S) * float(batch_denom if batch_denom is not None else n))
    with _ops.trace("silhouette_loss"):
        if faces_per_pixel is not None:
            return _SilhouetteRasterLossFn.apply(verts, mesh.faces_i32(), R.to(verts.device), T.to(verts.device),
                                                 target_masks.detach().to(torch.float32).reshape(n, 1, S, S), faces_per_pixel,
                                                 silhouette_blur_radius(sigma), True, float(sigma), rs.cull_backfaces,
                                                 rs.perspective_correct, rs.z_clip, scale)
        return _SilhouetteLossFn.apply(verts, mesh.faces_i32(), R.to(verts.device), T.to(verts.device),
                                       target_masks.detach().to(torch.float32), S, SILHOUETTE_FACES_PER_PIXEL,
                                       silhouette_blur_radius(sigma), True, float(sigma), rs.cull_backfaces,
                                       rs.perspective_correct, rs.z_clip, scale)


class _MaskedMseFn(torch.autograd.Function):
    """F.mse_loss(rendered*masks, target*masks) (reference :71-75) as one fused reduction."""

    @staticmethod
    def forward(ctx, rendered, masks, target):
        loss, grad = _ops.masked_mse(rendered.detach(), target.detach(), masks.detach(), want_grad=rendered.requires_grad)
        ctx.grad = grad
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        return (ctx.grad * grad_out if ctx.grad is not None else None), None, None


def _masked_mse(rendered, masks, target_rendered, batch_denom=None):
    if not rendered.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    loss = _MaskedMseFn.apply(rendered, masks, target_rendered)
    if batch_denom is not None and batch_denom != rendered.shape[0]:
        # views sharded over ranks: the mean over this rank's views becomes its share of the mean over the whole batch
        loss = loss * (rendered.shape[0] / float(batch_denom))
    return loss


def _mesh_terms(verts, target_verts, mesh, weights):
    """The four view-independent regularisers both approaches add for 'mesh'/'both'
    (reference losses.py:84-87,93-96,112-115,121-124), same weights-dict keys."""
    return _mesh_losses.mesh_terms(verts, target_verts, mesh, weights)      # one fused forward+gradient call


def compute_first_approach_loss(rendered, masks, target_rendered, verts, target_verts, mesh, weights, opt_type, *,
                                batch_denom=None):
    # 'texture' ignores main_loss_weight (reference :75); an unknown opt_type leaves `loss` unbound and
    # raises UnboundLocalError at the return, as the reference does (:98).
    # batch_denom (views sharded over ranks): only the IMAGE term is a mean over views and is scaled to this rank's
    # share of the global batch; the mesh terms are view-independent and already enter with 1/world per rank.
    if opt_type == 'texture':
        loss = _masked_mse(rendered, masks, target_rendered, batch_denom)
    elif opt_type in ('mesh', 'both'):
        loss = weights['main_loss_weight'] * _masked_mse(rendered, masks, target_rendered, batch_denom)
        loss = loss + _mesh_terms(verts, target_verts, mesh, weights)
    return loss


def compute_second_approach_loss(current, content, style, model, style_weight, content_weight, verts, target_verts, mesh,
                                 weights, opt_type, *, batch_denom=None, style_masks=None, style_scales=(1,),
                                 style_scale_weights=None):
    # style_scales / style_scale_weights: compute_perceptual_loss's scales / scale_weights (the multi-scale loss)
    if opt_type in ('texture', 'mesh', 'both'):
        perceptual = compute_perceptual_loss(current, content, style, model, style_weight=style_weight,
                                             content_weight=content_weight, batch_denom=batch_denom, style_masks=style_masks,
                                             scales=style_scales, scale_weights=style_scale_weights)
    if opt_type == 'texture':
        loss = perceptual                                   # no main_loss_weight here (reference :103-104)
    elif opt_type in ('mesh', 'both'):
        loss = weights['main_loss_weight'] * perceptual + _mesh_terms(verts, target_verts, mesh, weights)
    return loss
