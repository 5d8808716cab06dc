"""Drop-in for the reference's ``style_transfer.py`` (same names, signatures, defaults and
return values: reference style_transfer.py:10,31,38) running on libst3d (MI355X / gfx950).

  get_features   one fused VGG forward through the plan (13 MFMA conv launches) instead of
                 37 module calls; taps are the POST-ReLU activations, exactly what the
                 reference's in-place ReLU leaves in its feature dict
  gram_matrix    split-K fp32-MFMA Gram with an autograd backward
  style_transfer targets once, then per step ONE call into the fused forward/loss/backward
                 plan and ONE fused Adam launch on the pixels (reference :59-83 builds and
                 tears down an autograd graph per step)
"""
import torch
import torch.optim as optim  # noqa: F401  (star-import surface of the reference module)
from tqdm import tqdm

from st3d import lap as _lap
from st3d import ops as _ops
from st3d import optim as _st3d_optim
from st3d import vgg as _vgg

# Check if CUDA is available
device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

_DEFAULT_LAYERS = {
    '0': 'conv1_1',
    '5': 'conv2_1',
    '10': 'conv3_1',
    '19': 'conv4_1',
    '21': 'conv4_2',  # Content layer
    '28': 'conv5_1'
}


def _fused_ok(image, model):
    return (isinstance(model, _vgg.Vgg19Features) and image.is_cuda and image.dim() == 4 and image.shape[1] == 3
            and image.shape[2] == image.shape[3] and image.shape[2] >= 16)


class _FeaturesFn(torch.autograd.Function):
    """Differentiable taps: forward = the fused plan forward, backward = the plan's input-gradient chain seeded with the
    gradients the caller's loss sends into the taps (st3d_plan_backward).  The plan keeps the activations the backward
    needs; if another forward has used its buffers since (``plan.generation``), the forward is redone first."""

    @staticmethod
    def forward(ctx, image, model, modules):
        plan = model.plan(image.shape[0], image.shape[2])
        upto = max(modules)
        plan.forward(image, upto=upto)
        ctx.plan, ctx.modules, ctx.upto, ctx.generation = plan, modules, upto, plan.generation
        ctx.save_for_backward(image)
        return tuple(plan.activation(m).clone() for m in modules)

    @staticmethod
    def backward(ctx, *grads):
        plan = ctx.plan
        (image,) = ctx.saved_tensors
        if plan.generation != ctx.generation:
            plan.forward(image, upto=ctx.upto)
        given = {m: g for m, g in zip(ctx.modules, grads) if g is not None}
        return plan.backward(given, ctx.upto), None, None


# Extract features using VGG19
def get_features(image, model, layers=None):
    if layers is None:
        layers = _DEFAULT_LAYERS
    if _fused_ok(image, model):
        want = {int(k): v for k, v in layers.items() if k in model._modules}
        features = {}
        if want:
            modules = tuple(int(name) for name in model._modules if int(name) in want)     # module order, as the reference fills it
            if image.requires_grad and torch.is_grad_enabled():
                # the reference's own loop body (style_transfer.py:61-83) back-propagates through these
                outs = _FeaturesFn.apply(image, model, modules)
            else:
                plan = model.plan(image.shape[0], image.shape[2])
                plan.forward(image, upto=max(want))
                outs = tuple(plan.activation(m).clone() for m in modules)
            for m, t in zip(modules, outs):
                features[want[m]] = t
        return features
    if isinstance(model, _vgg.Vgg19Features) and image.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("differentiable get_features on the st3d VGG needs square (B,3,S,S) GPU images, S >= 16")
    # any other model: the reference's generic walk (each module is whatever the caller built)
    features = {}
    x = image
    for name, layer in model._modules.items():
        x = layer(x)
        if name in layers:
            features[layers[name]] = x
    return features


class _GramFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tensor):
        t = tensor.detach().to(torch.float32).contiguous()
        ctx.save_for_backward(t)
        return _ops.gram_fwd(t)

    @staticmethod
    def backward(ctx, grad_gram):
        (t,) = ctx.saved_tensors
        D = (grad_gram + grad_gram.transpose(1, 2)).contiguous()       # dF = (dG + dG^T) F
        return _ops.gram_bwd(D, t, 1.0)


# Calculate Gram matrix for style representation
def gram_matrix(tensor):
    batch_size, d, h, w = tensor.size()
    if not tensor.is_cuda:
        raise RuntimeError("st3d gram_matrix runs on the GPU (libst3d); got a CPU tensor -- there is no CPU fallback")
    return _GramFn.apply(tensor)


class _GuidedGramFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tensor, q):
        t = tensor.detach().to(torch.float32).contiguous()
        ctx.save_for_backward(t, q)
        return _ops.gram_fwd(t, q=q)

    @staticmethod
    def backward(ctx, grad_gram):
        t, q = ctx.saved_tensors
        D = (grad_gram + grad_gram.transpose(1, 2)).contiguous()       # dF = q o ((dG + dG^T) (q o F))
        return _ops.gram_bwd(D, t, 1.0, q=q), None


def guided_gram_matrix(tensor, mask):
    """The Gram of ``tensor`` (B,C,H,W) taken over the guided region (Gatys et al. 2017): ``mask`` (B,1,S,S) or (B,S,S) in
    [0,1] is brought to H x H by 2x2 averages (S / H one of 1, 2, 4, 8, 16) and normalised to mean 1 over the image, and
    G^ = sum_p w[p] F[:,p] F[:,p]^T.  Gradient to ``tensor``; the mask is a constant."""
    batch_size, d, h, w = tensor.size()
    if not tensor.is_cuda:
        raise RuntimeError("st3d guided_gram_matrix runs on the GPU (libst3d); got a CPU tensor -- there is no CPU fallback")
    planes, _ = _ops.guidance_build(mask)
    for q in planes:
        if q.shape[0] == batch_size and q.shape[1] == h and q.shape[2] == w:
            return _GuidedGramFn.apply(tensor, q)
    raise ValueError(f"features of {h} x {w} are no style-tap resolution of a mask of side {planes[0].shape[1]} "
                     f"(sides {[int(p.shape[1]) for p in planes]})")


# ---------------------------------------------------------------------------- style regions (csrc/regions.hip)
REGION_STYLE_TAPS = {k: v for k, v in _DEFAULT_LAYERS.items() if v != 'conv4_2'}       # the five style taps, in module order
REGION_CONTENT_TAP = 'conv4_2'


def region_style_norm(C, H, W, batch_denom):
    """the plan's normalisation of a style layer: the reference's 1 / (d h w) per layer under the mean over the batch and
    the Gram's C x C entries"""
    return 1.0 / (batch_denom * C * C) / (float(C) * C * H * W)


def region_grams(taps, planes):
    """taps: the five style taps (B,C_l,H_l,H_l); planes[r][l] of regions.region_planes -> G^[r][l] (B,C_l,C_l): the R x 5
    guided Grams, one launch pair per region (st3d_gram_fwd_multi_weighted takes up to 8 items; a region's five are the
    plan's own shape of call)."""
    return [_ops.gram_fwd_multi(list(taps), qs=list(planes[r])) for r in range(len(planes))]


_REGION_MASKED = {}         # key -> ((sums, targets): held, so the key's addresses stay theirs; the masked targets)
_REGION_MASKED_ENTRIES = 8  # the alternating view batches of a run


def _region_masked_targets(sums, targets, B):
    """T[r][l] (B,C,C): region r's target Gram for the views in which the region is visible at level l (Sigma_l > 0), zeros
    for the others -- there G^ is exactly 0 (q = 0), so D = G^ - T = 0: the (view, region, tap) adds exactly nothing to the
    value and, q being 0, nothing to the gradient.  Kept for as long as the same planes and targets come back (a
    texture-only run builds them once per view batch)."""
    key = (sums.data_ptr(), sums._version, tuple(sums.shape), id(targets))
    hit = _REGION_MASKED.get(key)
    if hit is not None and hit[0][0] is sums and hit[0][1] is targets:
        return hit[1]
    seen = sums > 0                                         # (R,5,B)
    masked = [[torch.where(seen[r, l][:, None, None], A.expand(B, -1, -1), torch.zeros((), dtype=A.dtype, device=A.device))
               .contiguous() for l, A in enumerate(targets[r])] for r in range(len(targets))]
    while len(_REGION_MASKED) >= _REGION_MASKED_ENTRIES:
        _REGION_MASKED.pop(next(iter(_REGION_MASKED)))
    _REGION_MASKED[key] = ((sums, targets), masked)
    return masked


class _RegionLossFn(torch.autograd.Function):
    """(five style taps [, the content tap]) -> content_weight x content + style_weight x sum_r lambda_r sum_l norm_l
    |G^_{r,l} - A_{r,l}|^2.  Forward: the R x 5 guided Grams, one launch pair per region, the ordered loss sums (st3d_sqdiff_sum_multi,
    eight items a launch, content first, then r ascending and l ascending inside: the items are folded into their slots
    in that order in fp32), and, when a gradient is wanted, per tap R calls of the accumulating st3d_gram_bwd_weighted in
    ascending r.  Backward only scales.  -> (total, parts (3,) [total, content, style])."""

    @staticmethod
    def forward(ctx, setup, *taps):
        planes, masked, lambdas, bd, style_weight, content_weight, content_target = setup
        want = any(t.requires_grad for t in taps)
        feats = [t.detach().to(torch.float32).contiguous() for t in taps]
        style_taps, content_tap = feats[:5], (feats[5] if len(feats) > 5 else None)
        R, B = len(planes), style_taps[0].shape[0]
        grams = region_grams(style_taps, planes)
        items, norms = [], []
        if content_tap is not None:
            items.append((content_tap, content_target, 1.0 / (bd * content_tap[0].numel()), 1, want))
        for r in range(R):
            for l, t in enumerate(style_taps):
                C, H, W = t.shape[1], t.shape[2], t.shape[3]
                norms.append(region_style_norm(C, H, W, bd))
                items.append((grams[r][l], masked[r][l], lambdas[r] * norms[-1], 2, want))
        out, diffs = None, []
        for first in range(0, len(items), 8):
            last = first + 8 >= len(items)
            out, d = _ops.sqdiff_sum_multi(items[first:first + 8], first == 0, last, style_weight, content_weight, out=out)
            diffs += d
        grads = [None] * len(feats)
        if want:
            if content_tap is not None:
                grads[5] = diffs[0] * (2.0 * content_weight / (bd * content_tap[0].numel()))
                diffs = diffs[1:]
            for l, t in enumerate(style_taps):
                g = None
                for r in range(R):          # ascending r: the first call writes, the others accumulate
                    coef = 4.0 * style_weight * lambdas[r] * norms[r * 5 + l]
                    g = _ops.gram_bwd(diffs[r * 5 + l], t, coef, out=g, q=planes[r][l])
                grads[l] = g
        ctx.grads = grads
        ctx.grams = grams
        parts = out.clone()
        ctx.mark_non_differentiable(parts)
        return out[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_out, _grad_parts):
        return (None,) + tuple(g * grad_out if g is not None and need else None
                               for g, need in zip(ctx.grads, ctx.needs_input_grad[1:]))


def check_region_weights(region_weights, R):
    """None (all 1) or R finite numbers >= 0 -> tuple of R floats; else ValueError"""
    if region_weights is None:
        return (1.0,) * R
    try:
        w = tuple(float(x) for x in region_weights)
    except (TypeError, ValueError):
        raise ValueError(f"region weights must be numbers, got {region_weights!r}") from None
    if len(w) != R:
        raise ValueError(f"{len(w)} region weights for {R} regions: one per region")
    if not all(x >= 0.0 and x != float("inf") for x in w):
        raise ValueError(f"region weights must be finite and >= 0, got {w!r}")
    return w


def _region_check(features, planes, sums, targets, region_weights, batch_denom):
    for name in REGION_STYLE_TAPS.values():
        if name not in features or not torch.is_tensor(features[name]) or features[name].dim() != 4:
            raise ValueError(f"features must hold the tap {name} as (B,C,H,W); get_features gives them")
    taps = [features[name] for name in REGION_STYLE_TAPS.values()]
    if not taps[0].is_cuda:
        raise RuntimeError("st3d region_style_loss runs on the GPU (libst3d); got CPU tensors -- there is no CPU fallback")
    R, B = len(planes), taps[0].shape[0]
    if not 1 <= R <= 8 or len(targets) != R or any(len(p) != 5 for p in planes) or any(len(t) != 5 for t in targets):
        raise ValueError("planes and targets must hold five entries for each of the same 1..8 regions")
    if tuple(sums.shape) != (R, 5, B):
        raise ValueError(f"sums must be ({R},5,{B}) -- the planes of these {B} views --, got {tuple(sums.shape)}")
    for l, t in enumerate(taps):
        if tuple(planes[0][l].shape) != (B, t.shape[2], t.shape[3]):
            raise ValueError(f"the planes of level {l} are {tuple(planes[0][l].shape)}, the tap {tuple(t.shape)}")
        if tuple(targets[0][l].shape) != (1, t.shape[1], t.shape[1]):
            raise ValueError(f"the target of level {l} must be (1,{t.shape[1]},{t.shape[1]}), got {tuple(targets[0][l].shape)}")
    if batch_denom is not None and not (isinstance(batch_denom, int) and not isinstance(batch_denom, bool) and batch_denom >= 1):
        raise ValueError(f"batch_denom must be a positive integer, got {batch_denom!r}")
    return taps, check_region_weights(region_weights, R), int(batch_denom or B)


def region_style_loss(features, planes, sums, targets, region_weights=None, batch_denom=None):
    """The style term over R mesh regions (Gatys et al. 2017, spatial control with one style per region):
        sum_r lambda_r sum_l norm_l sum_b | G^_{r,l,b} - A_{r,l} |^2,   G^ = sum_p q_r[p]^2 F[:,p] F[:,p]^T,
    ``features`` the taps of ``get_features`` over the current images, ``planes`` / ``sums`` of st3d.regions.region_planes
    for the same views, ``targets`` of st3d.regions.region_targets, norm_l the plan's (the reference's layer weights and
    1 / (d h w); the mean over ``batch_denom``, default B).  For one region that holds every face this is the style term
    ``compute_perceptual_loss(style_masks=coverage)`` defines.  A (view, region, tap) whose Sigma_l is 0 -- the region is not
    visible in that view, or vanished at that level -- adds exactly 0 to the value and to the gradient.  The sum runs in
    ascending r in fp32 in a fixed order: two runs are bit-equal.  Gradient to ``features`` only."""
    taps, lambdas, bd = _region_check(features, planes, sums, targets, region_weights, batch_denom)
    masked = _region_masked_targets(sums, targets, taps[0].shape[0])
    return _RegionLossFn.apply((planes, masked, lambdas, bd, 1.0, 0.0, None), *taps)[0]


# ---------------------------------------------------------------------------- NNFM style loss (csrc/nnfm.hip)
NNFM_LAYERS = ('conv2_1', 'conv3_1', 'conv4_1', 'conv4_2', 'conv5_1')       # names of _DEFAULT_LAYERS the term may tap
_NNFM_MASK_RATIOS = (1, 2, 4, 8, 16)


class NnfmStyle:
    """The unit-norm copy of a style tap (Bs,C,Hs,Ws), made once per style image by ``nnfm_style``."""

    def __init__(self, hat):
        self.hat = hat


def nnfm_style(style_features):
    """style tap (Bs,C,Hs,Ws) -> NnfmStyle: every position's vector over its norm (a zero vector stays zero)."""
    if not torch.is_tensor(style_features):
        raise TypeError("style_features must be a tensor (Bs,C,Hs,Ws)")
    if not style_features.is_cuda:
        raise RuntimeError("st3d nnfm_style runs on the GPU (libst3d); got a CPU tensor -- there is no CPU fallback")
    hat, _ = _ops.nnfm_normalise(style_features.detach())
    return NnfmStyle(hat)


def nnfm_pool_mask(mask, B, H, W):
    """mask (B,1,S,S') | (B,S,S') in [0,1] -> position weights (B,H,W): successive 2x2 averages, S / H = S' / W one of
    1, 2, 4, 8, 16.  Plain torch pooling (not the hot path); a constant of the gradient."""
    if not torch.is_tensor(mask):
        raise TypeError("mask must be a tensor (B,1,S,S) or (B,S,S)")
    m = mask.detach().to(torch.float32)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3 or m.shape[0] != B:
        raise ValueError(f"mask must be ({B},1,S,S) or ({B},S,S), got {tuple(mask.shape)}")
    S, S2 = int(m.shape[1]), int(m.shape[2])
    if S % H or S2 % W or S // H != S2 // W or S // H not in _NNFM_MASK_RATIOS:
        raise ValueError(f"a mask of {S} x {S2} does not reduce to features of {H} x {W} by a factor of {_NNFM_MASK_RATIOS}")
    m = m[:, None]
    for _ in range((S // H).bit_length() - 1):
        m = torch.nn.functional.avg_pool2d(m, 2)
    return m[:, 0].contiguous()


class _NnfmFn(torch.autograd.Function):
    """One tap: forward = ops.nnfm_normalise (the queries), ops.nnfm_search, ops.nnfm_sum; backward = ops.nnfm_bwd, one
    launch.  Indices and weights are constants; the style gets no gradient."""

    @staticmethod
    def forward(ctx, features, style_hat, weights, batch_denom):
        f = features.detach().to(torch.float32).contiguous()
        normalised = _ops.nnfm_normalise(f)
        idx, dist = _ops.nnfm_search(f, style_hat, weights, normalised=normalised)
        loss, wsum = _ops.nnfm_sum(dist, weights, batch_denom)
        ctx.saved = (f, style_hat, idx, dist, wsum, weights, batch_denom)
        ctx.idx, ctx.dist = idx, dist
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        f, style_hat, idx, dist, wsum, weights, batch_denom = ctx.saved
        grad = None
        if ctx.needs_input_grad[0]:
            grad = _ops.nnfm_bwd(f, style_hat, idx, dist, wsum, weights, batch_denom, grad_out)
        return grad, None, None, None


def nnfm_loss(features, style_features, mask=None, batch_denom=None):
    """The nearest-neighbour feature matching loss of ARF (Zhang et al., ECCV 2022) over one tap: every position of
    ``features`` (B,C,H,W) looks up its nearest position of ``style_features`` ((Bs,C,Hs,Ws), Bs 1 or B, any resolution; a
    tensor or the ``nnfm_style`` of one) by cosine distance, and the loss is the mean distance per image, summed over the
    images and divided by ``batch_denom`` (default B).  ``mask`` (B,1,S,S) | (B,S,S) in [0,1] weights the positions
    (``nnfm_pool_mask``); positions of weight 0 are not searched and receive an exact zero gradient.  A zero feature vector
    has distance 1 and gradient 0 (ARF adds 1e-8 to the norm).  Gradient to ``features`` only."""
    if not torch.is_tensor(features):
        raise TypeError("features must be a tensor (B,C,H,W)")
    if not features.is_cuda:
        raise RuntimeError("st3d nnfm_loss runs on the GPU (libst3d); got a CPU tensor -- there is no CPU fallback")
    if features.dim() != 4:
        raise ValueError(f"features must be (B,C,H,W), got {tuple(features.shape)}")
    if batch_denom is not None and not (isinstance(batch_denom, int) and not isinstance(batch_denom, bool) and batch_denom >= 1):
        raise ValueError(f"batch_denom must be a positive integer, got {batch_denom!r}")
    style = style_features if isinstance(style_features, NnfmStyle) else nnfm_style(style_features)
    B, C, H, W = features.shape
    if style.hat.dim() != 4 or style.hat.shape[1] != C or style.hat.shape[0] not in (1, B):
        raise ValueError(f"style_features must be (1 or {B},{C},Hs,Ws), got {tuple(style.hat.shape)}")
    weights = nnfm_pool_mask(mask, B, H, W) if mask is not None else None
    return _NnfmFn.apply(features, style.hat, weights, batch_denom)


def check_nnfm_layers(layers):
    """a non-empty sequence of distinct names from NNFM_LAYERS -> the tuple; else ValueError"""
    if isinstance(layers, str):
        layers = tuple(s for s in layers.split(',') if s)
    layers = tuple(layers)
    if not layers or len(set(layers)) != len(layers) or any(name not in NNFM_LAYERS for name in layers):
        raise ValueError(f"nnfm layers must be distinct names from {','.join(NNFM_LAYERS)}, got {layers!r}")
    return layers


def _nnfm_tap_map(layers):
    return {k: v for k, v in _DEFAULT_LAYERS.items() if v in layers}


def _nnfm_style_taps(style_imgs, model, layers):
    """{layer: NnfmStyle} of the style image(s), cached on the model under the tensor's identity and version (as the plan
    caches the style Grams): the style VGG forward and its normalisation run once per style, not once per step.  One image
    expanded over the batch is one style (Bs = 1)."""
    key = (style_imgs.data_ptr(), style_imgs._version, tuple(style_imgs.shape), tuple(style_imgs.stride()), layers)
    cache = getattr(model, "_nnfm_style_cache", None)
    if cache is not None and cache[0] == key and cache[1].data_ptr() == style_imgs.data_ptr():
        return cache[2]
    s = style_imgs.detach()
    if s.shape[0] > 1 and s.stride(0) == 0:
        s = s[:1]
    with torch.no_grad():
        feats = get_features(s.to(torch.float32).contiguous(), model, _nnfm_tap_map(layers))
        taps = {name: nnfm_style(feats[name]) for name in layers}
    model._nnfm_style_cache = (key, style_imgs, taps)
    return taps


def _nnfm_term(current_imgs, style_imgs, model, layers, masks, batch_denom):
    taps = _nnfm_style_taps(style_imgs, model, layers)
    feats = get_features(current_imgs, model, _nnfm_tap_map(layers))
    total = None
    for name in layers:
        term = nnfm_loss(feats[name], taps[name], mask=masks, batch_denom=batch_denom)
        total = term if total is None else total + term
    return total


# ---------------------------------------------------------------------------- sliced Wasserstein style loss (csrc/swd.hip)
SWD_LAYERS = tuple(_DEFAULT_LAYERS.values())                                # every tap may carry the term
SWD_DEFAULT_LAYERS = ('conv2_1', 'conv3_1', 'conv4_1', 'conv5_1')           # conv1_1 at 512^2 is 64 rows of 262 144 positions per view
_SWD_CHANNELS = {'conv1_1': 64, 'conv2_1': 128, 'conv3_1': 256, 'conv4_1': 512, 'conv4_2': 512, 'conv5_1': 512}


def swd_directions(K, C, generator=None, device=None):
    """(K,C) fp32 unit rows: a normal draw from ``generator`` (on the generator's device, so a CPU generator gives the same
    directions on every rank and device) over its norm, moved to ``device``.  Plain torch; a constant of the gradient."""
    for n, what in ((K, "K"), (C, "C")):
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= _ops.SWD_MAX_CHANNELS:
            raise ValueError(f"{what} must be an integer in 1..{_ops.SWD_MAX_CHANNELS}, got {n!r}")
    where = generator.device if generator is not None else (device if device is not None else "cpu")
    v = torch.randn((K, C), generator=generator, dtype=torch.float32, device=where)
    v = v / v.norm(dim=1, keepdim=True)
    return v.to(device) if device is not None else v


class _SwdFn(torch.autograd.Function):
    """One tap: forward = ops.swd_project -> ops.swd_sort of the render tap and of the style tap with the same directions,
    ops.swd_loss; backward = ops.swd_bwd, then ops.swd_project with the transposed directions.  The permutation, the
    directions and the weights are constants; the style gets no gradient."""

    @staticmethod
    def forward(ctx, features, style_features, directions, weights, batch_denom):
        f = features.detach().to(torch.float32).contiguous()
        v = directions.detach().to(torch.float32).contiguous()
        proj = _ops.swd_project(f, v)
        rows, perm, count = _ops.swd_sort(proj, weights)
        tsorted, _, _ = _ops.swd_sort(_ops.swd_project(style_features.detach(), v), None, want_perm=False)
        loss = _ops.swd_loss(rows, count, tsorted, batch_denom)
        ctx.saved = (rows, perm, count, tsorted, v, batch_denom, tuple(f.shape))
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        rows, perm, count, tsorted, v, batch_denom, shape = ctx.saved
        grad = None
        if ctx.needs_input_grad[0]:
            gproj = _ops.swd_bwd(rows, perm, count, tsorted, batch_denom, grad_out)
            grad = _ops.swd_project(gproj, v.t().contiguous()).reshape(shape)
        return grad, None, None, None, None


def swd_loss(features, style_features, directions, mask=None, batch_denom=None):
    """The sliced Wasserstein loss of Heitz et al. (CVPR 2021) over one tap: ``features`` (B,C,H,W) and ``style_features``
    ((Bs,C,Hs,Ws), Bs 1 or B, any resolution) are projected onto the unit rows of ``directions`` (K,C), every projected row is
    sorted, and the loss is the mean over directions and positions of the squared difference between a render's sorted row
    and the style's, resampled to as many samples by nearest rank; the per-image means are summed and divided by
    ``batch_denom`` (default B).  ``mask`` (B,1,S,S) | (B,S,S) in [0,1] selects the positions (``nnfm_pool_mask``): a position
    takes part iff its pooled weight is > 0, unweighted; the others receive an exact zero gradient.  Gradient to
    ``features`` only."""
    if not torch.is_tensor(features):
        raise TypeError("features must be a tensor (B,C,H,W)")
    if not torch.is_tensor(style_features) or not torch.is_tensor(directions):
        raise TypeError("style_features must be a tensor (Bs,C,Hs,Ws) and directions a tensor (K,C)")
    if not features.is_cuda:
        raise RuntimeError("st3d swd_loss runs on the GPU (libst3d); got a CPU tensor -- there is no CPU fallback")
    if features.dim() != 4:
        raise ValueError(f"features must be (B,C,H,W), got {tuple(features.shape)}")
    if batch_denom is not None and not (isinstance(batch_denom, int) and not isinstance(batch_denom, bool) and batch_denom >= 1):
        raise ValueError(f"batch_denom must be a positive integer, got {batch_denom!r}")
    B, C, H, W = features.shape
    if style_features.dim() != 4 or style_features.shape[1] != C or style_features.shape[0] not in (1, B):
        raise ValueError(f"style_features must be (1 or {B},{C},Hs,Ws), got {tuple(style_features.shape)}")
    if directions.dim() != 2 or directions.shape[1] != C or not 1 <= directions.shape[0] <= _ops.SWD_MAX_CHANNELS:
        raise ValueError(f"directions must be (1..{_ops.SWD_MAX_CHANNELS},{C}), got {tuple(directions.shape)}")
    weights = nnfm_pool_mask(mask, B, H, W) if mask is not None else None
    return _SwdFn.apply(features, style_features, directions, weights, batch_denom)


def check_swd_layers(layers):
    """a non-empty sequence of distinct names from SWD_LAYERS -> the tuple; else ValueError"""
    if isinstance(layers, str):
        layers = tuple(s for s in layers.split(',') if s)
    layers = tuple(layers)
    if not layers or len(set(layers)) != len(layers) or any(name not in SWD_LAYERS for name in layers):
        raise ValueError(f"swd layers must be distinct names from {','.join(SWD_LAYERS)}, got {layers!r}")
    return layers


def check_swd_directions(K):
    """0 (as many directions as the tap has channels) or 1..512 -> K; else ValueError"""
    if isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= _ops.SWD_MAX_CHANNELS:
        raise ValueError(f"swd directions must be 0 (= the channels of each tap) or 1..{_ops.SWD_MAX_CHANNELS}, got {K!r}")
    return K


def swd_draw(layers, K, generator, device=None):
    """{layer: directions} for one step, drawn from ``generator`` in the order of ``layers`` (K = 0: as many as the tap has
    channels).  The draw does not look at any image, so a rank without views makes it too and stays in step."""
    return {name: swd_directions(K or _SWD_CHANNELS[name], _SWD_CHANNELS[name], generator, device) for name in layers}


def _swd_tap_map(layers):
    return {k: v for k, v in _DEFAULT_LAYERS.items() if v in layers}


def _swd_style_taps(style_imgs, model, layers):
    """{layer: the style tap (Bs,C,Hs,Ws)}, cached on the model under the tensor's identity and version as
    ``_nnfm_style_taps`` does: the style VGG forward runs once per style.  Its projection and sort follow the directions
    and are redone with every draw."""
    key = (style_imgs.data_ptr(), style_imgs._version, tuple(style_imgs.shape), tuple(style_imgs.stride()), layers)
    cache = getattr(model, "_swd_style_cache", None)
    if cache is not None and cache[0] == key and cache[1].data_ptr() == style_imgs.data_ptr():
        return cache[2]
    s = style_imgs.detach()
    if s.shape[0] > 1 and s.stride(0) == 0:
        s = s[:1]
    with torch.no_grad():
        feats = get_features(s.to(torch.float32).contiguous(), model, _swd_tap_map(layers))
        taps = {name: feats[name].detach() for name in layers}
    model._swd_style_cache = (key, style_imgs, taps)
    return taps


def _swd_term(current_imgs, style_imgs, model, layers, masks, batch_denom, directions):
    """``directions``: {layer: (K,C)} of this step (``swd_draw``)"""
    taps = _swd_style_taps(style_imgs, model, layers)
    feats = get_features(current_imgs, model, _swd_tap_map(layers))
    total = None
    for name in layers:
        term = swd_loss(feats[name], taps[name], directions[name].to(feats[name].device), mask=masks, batch_denom=batch_denom)
        total = term if total is None else total + term
    return total


def check_lap_pools(pools, side=None):
    """the pool sides of the Laplacian content term: a non-empty, strictly increasing sequence from (1, 2, 4, 8, 16), each
    dividing ``side`` (an int or (H, W)) with a pooled side >= 2; -> a tuple of int, else ValueError"""
    return _lap.check_pools(pools, side)


def laplacian_targets(content_imgs, pools):
    """[D(pool_p(content)) for p in pools] without gradient, cached on the content tensor's identity and version
    (st3d.lap.lap_target_cached): the targets of the Laplacian content term, computed once per content batch"""
    return [_lap.lap_target_cached(content_imgs, p) for p in pools]


def style_transfer(initial_optimized_imgs, content_imgs, style_imgs, model, steps=2000, style_weight=1e6, content_weight=1, lr=0.003,
                   style_masks=None, nnfm_weight=0.0, nnfm_layers=('conv3_1',), swd_weight=0.0, swd_layers=SWD_DEFAULT_LAYERS,
                   swd_directions=0, swd_seed=0, style_scales=(1,), style_scale_weights=None, color='rgb', lap_weight=0.0,
                   lap_pools=(4,)):
    # style_masks (B,1,S,S) | (B,S,S) in [0,1], e.g. the coverage of the renders being stylised: the guided style loss --
    # each tap's Gram of the optimised images is taken over the masked region only (default None: the reference's loss)
    # nnfm_weight > 0: every step adds nnfm_weight x the NNFM term over nnfm_layers (its own partial VGG forward and backward
    # next to the fused plan's) to the plan's gradient before Adam; style_masks serves both terms.  0: today's loop.
    nnfm_weight = float(nnfm_weight)
    if not (nnfm_weight >= 0.0 and nnfm_weight != float("inf")):
        raise ValueError("nnfm_weight must be finite and >= 0")
    if nnfm_weight:
        nnfm_layers = check_nnfm_layers(nnfm_layers)
    # swd_weight > 0: every step adds swd_weight x the sliced Wasserstein term over swd_layers in the same way; its directions
    # (swd_directions per tap, 0 = as many as the tap has channels) are redrawn every step from one generator seeded with
    # swd_seed, so two calls with the same seed take the same steps.  0: nothing of it runs.
    swd_weight = float(swd_weight)
    if not (swd_weight >= 0.0 and swd_weight != float("inf")):
        raise ValueError("swd_weight must be finite and >= 0")
    if swd_weight:
        swd_layers = check_swd_layers(swd_layers)
        swd_k = check_swd_directions(swd_directions)
        if isinstance(swd_seed, bool) or not isinstance(swd_seed, int):
            raise ValueError(f"swd_seed must be an integer, got {swd_seed!r}")
        swd_generator = torch.Generator().manual_seed(swd_seed)
    # style_scales / style_scale_weights: the multi-scale loss (st3d.imgpyr; losses.compute_perceptual_loss(scales=...)) --
    # every step adds w_f x the pyramid's transpose of the gradient of the fused loss at side S / f, f in {2, 4}, to the
    # plan's gradient before Adam, in ascending f.  The NNFM and SWD terms stay at full resolution.  (1,): today's loop.
    multi_scale = not (isinstance(style_scales, tuple) and style_scales == (1,) and style_scale_weights is None)
    if multi_scale:
        from st3d import imgpyr as _imgpyr
        style_scales, style_scale_weights = _imgpyr.check_scales(style_scales, style_scale_weights,
                                                                 initial_optimized_imgs.shape[2])

    # color='luminance' (Gatys et al. 2017, section 5.2; st3d.color): content and style are replaced by their luminance once;
    # every step ONE luma_fwd of the optimised pixels is what the plan(s) and the NNFM / SWD terms see, and each term's
    # gradient comes back through luma_bwd before it is added; the result is the optimised luminance under the content's
    # chroma (color.recombine).  'rgb': today's loop, nothing of it runs.
    if color not in ('rgb', 'luminance'):
        raise ValueError(f"color must be 'rgb' or 'luminance', got {color!r}")
    luminance = color == 'luminance'
    # lap_weight > 0: every step adds lap_weight x the gradient of the Laplacian content term over lap_pools
    # (losses.compute_laplacian_loss; one fused pass per pool side, targets set once) before Adam.  Under 'luminance' the
    # term compares the luminance images.  0: nothing of it runs.
    lap_weight = float(lap_weight)
    if not (lap_weight >= 0.0 and lap_weight != float("inf")):
        raise ValueError("lap_weight must be finite and >= 0")
    if lap_weight:
        lap_pools = check_lap_pools(lap_pools, tuple(initial_optimized_imgs.shape[2:]))

    # Ensure content_imgs and style_imgs are batched tensors
    assert initial_optimized_imgs.shape[0] == content_imgs.shape[0] == style_imgs.shape[0]
    if not isinstance(model, _vgg.Vgg19Features):
        raise TypeError("style_transfer needs the st3d VGG returned by utils.get_vgg()")
    if luminance:
        from st3d import color as _color
        rgb_content = content_imgs.to(device).detach()
        with torch.no_grad():
            content_imgs = _color.luma_fwd(rgb_content.to(torch.float32))
            one_style = style_imgs.shape[0] > 1 and style_imgs.stride(0) == 0      # one image expanded stays one image expanded
            style_src = (style_imgs[:1] if one_style else style_imgs).to(device).detach().to(torch.float32)
            style_imgs = _color.luma_fwd(style_src)
            if one_style:
                style_imgs = style_imgs.expand(content_imgs.shape[0], -1, -1, -1)

    B, S = initial_optimized_imgs.shape[0], initial_optimized_imgs.shape[2]
    full_weight = 1.0 if not multi_scale else dict(zip(style_scales, style_scale_weights)).get(1, 0.0)
    plan = model.plan(B, S) if full_weight else None
    if style_masks is not None:
        if not torch.is_tensor(style_masks) or tuple(style_masks.shape) not in ((B, 1, S, S), (B, S, S)):
            raise ValueError(f"style_masks must be ({B},1,{S},{S}) or ({B},{S},{S})")
        style_masks = style_masks.detach().to(device=device, dtype=torch.float32)

    # content conv4_2 features and style Grams: computed once (reference :44-51)
    if plan is not None:
        plan.set_content(content_imgs.to(device), force=True)
        plan.set_style(style_imgs.to(device), B, force=True)
    coarse = []             # (f, w_f, the plan of side S / f, the masks reduced by f): targets set once, here
    if multi_scale:
        with torch.no_grad():
            for f, w in zip(style_scales, style_scale_weights):
                if f == 1 or w == 0.0:
                    continue
                p = model.plan(B, S // f)
                p.set_content(_imgpyr.reduce(content_imgs.to(device).detach(), f), force=True)
                p.set_style(_imgpyr.reduce(style_imgs.to(device).detach().contiguous(), f), B, force=True)
                coarse.append((f, w, p, _imgpyr.reduce(style_masks.reshape(B, 1, S, S), f) if style_masks is not None else None))
    nnfm_style_imgs = style_imgs.to(device) if nnfm_weight else None      # one tensor for the run: its taps are cached on it
    swd_style_imgs = style_imgs.to(device) if swd_weight else None
    lap_targets = laplacian_targets(content_imgs.to(device), lap_pools) if lap_weight else None

    # Initialize target images  --> the ones to optimize
    optimized_imgs = initial_optimized_imgs.clone().detach().to(device).contiguous().requires_grad_(True)

    # Define optimizer (fused HIP Adam; pixels are not sharded, so no gradient all-reduce)
    optimizer = _st3d_optim.Adam([optimized_imgs], lr=lr, reduce_grads=False)

    back = _color.luma_bwd if luminance else (lambda g: g)      # how a term's gradient reaches the pixels

    for step in tqdm(range(steps), desc="2D Style Transfer"):
        grad = None
        seen = optimized_imgs       # what the terms see: the pixels themselves, or one luminance image a step for all of them
        if luminance:
            seen = _color.luma_fwd(optimized_imgs.detach()).requires_grad_(bool(nnfm_weight or swd_weight))
        if plan is not None:
            _, grad = plan.loss(seen, style_weight, content_weight, style_mask=style_masks)
            grad = back(grad)
            if full_weight != 1.0:
                grad = grad * full_weight
        for f, w, p, m in coarse:
            _, g = p.loss(_imgpyr.reduce(seen.detach(), f), style_weight, content_weight, style_mask=m)
            while g.shape[2] < S:
                g = _ops.pyr_down_bwd(g)
            g = back(g)
            g = g * w if w != 1.0 else g
            grad = g if grad is None else grad + g
        if grad is None:        # every scale has weight 0
            grad = torch.zeros_like(optimized_imgs)
        if nnfm_weight:
            # the term forwards through the same plan: taken after the fused loss has delivered its gradient
            term = _nnfm_term(seen, nnfm_style_imgs, model, nnfm_layers, style_masks, None)
            (extra,) = torch.autograd.grad(term, seen)
            grad = grad + nnfm_weight * back(extra)
        if swd_weight:
            term = _swd_term(seen, swd_style_imgs, model, swd_layers, style_masks, None,
                             swd_draw(swd_layers, swd_k, swd_generator, device))
            (extra,) = torch.autograd.grad(term, seen)
            grad = grad + swd_weight * back(extra)
        if lap_weight:
            _, extra = _lap.lap_term(seen.detach(), lap_targets, lap_pools)
            grad = grad + lap_weight * back(extra)
        optimized_imgs.grad = grad
        optimizer.step()

    if luminance:
        return _color.recombine(optimized_imgs, rgb_content)
    return optimized_imgs
