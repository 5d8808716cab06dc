"""Image pyramid for the multi-scale style loss: the perceptual terms look at the render and at copies of it
reduced by 2 and by 4, so that VGG's receptive fields, fixed in pixels, also cover the large shapes of the style image
(Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style Transfer"; the multi-resolution loss of Heitz et al. 2021).

    y = pyr_down(x)                 # (B,C,H,W) -> (B,C,H/2,W/2), differentiable
    y = reduce(x, f)                # f in {1, 2, 4}: f = 4 is two steps, f = 1 is x itself
    m = reduce_need(need, f)        # the need mask (st3d.render.tag_need) under the same steps
    y = reduced_cached(t, f)        # the reduced copy of a tensor that does not change: the same object every call

One step is the separable tent filter [1 3 3 1] / 8 centred on every 2 x 2 block (csrc/imgpyr.hip): the filter of an
anti-aliased bilinear resize by 1/2.  Its backward is the exact transpose written as a gather -- fixed order, no atomics, two
runs give the same bits.  A coarse pixel is needed iff any pixel of its footprint is, so a gradient a coarse plan computed at
its needed pixels only arrives unchanged at the needed fine pixels.  tests/_imgpyrref.py restates all three in numpy.
"""
import ctypes
from collections import OrderedDict

import torch

from ._lib import call, dptr, stream_ptr

F32, U8 = torch.float32, torch.uint8
FACTORS = (1, 2, 4)
CACHE_ENTRIES = 8       # reduced content batches and styles kept: a run cycles through ceil(n_views / batch) content batches
MAX_SIDE = 32768


# ---------------------------------------------------------------------------- the device wrappers (also st3d.ops.pyr_down_*)
def pyr_down_tile():
    """(rows, columns) of fine pixels one workgroup of the pyramid kernels owns: halos cross tile borders there"""
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    call("st3d_pyr_down_tile", ctypes.byref(h), ctypes.byref(w))
    return h.value, w.value


def _sides(shape, what, coarse=False):
    H, W = int(shape[-2]), int(shape[-1])
    if coarse:
        H, W = 2 * H, 2 * W
    if H < 2 or W < 2 or H % 2 or W % 2 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: a pyramid step takes even sides in 2...{MAX_SIDE}, got {tuple(shape)}")
    return H, W


def pyr_down_fwd(x):
    """(B,C,H,W) float32, H and W even -> (B,C,H/2,W/2): the separable [1 3 3 1] / 8 filter centred on every 2 x 2 block,
    replicate border, roundings as include/st3d.h states them"""
    if x.dim() != 4 or x.shape[0] * x.shape[1] < 1:
        raise ValueError(f"pyr_down_fwd takes a non-empty (B,C,H,W) tensor, got {tuple(x.shape)}")
    H, W = _sides(x.shape, "pyr_down_fwd")
    B, C = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((B, C, H // 2, W // 2), dtype=F32, device=x.device)
    call("st3d_pyr_down_fwd", dptr(x.contiguous(), F32), B * C, H, W, dptr(out), stream_ptr())
    return out


def pyr_down_bwd(grad_out):
    """(B,C,H/2,W/2) float32 -> (B,C,H,W): the exact transpose of pyr_down_fwd, a gather in a fixed order (no atomics)"""
    if grad_out.dim() != 4 or grad_out.shape[0] * grad_out.shape[1] < 1:
        raise ValueError(f"pyr_down_bwd takes a non-empty (B,C,H/2,W/2) tensor, got {tuple(grad_out.shape)}")
    H, W = _sides(grad_out.shape, "pyr_down_bwd", coarse=True)
    B, C = int(grad_out.shape[0]), int(grad_out.shape[1])
    out = torch.empty((B, C, H, W), dtype=F32, device=grad_out.device)
    call("st3d_pyr_down_bwd", dptr(grad_out.contiguous(), F32), B * C, H, W, dptr(out), stream_ptr())
    return out


def pyr_down_need(need):
    """(B,H,W) uint8 -> (B,H/2,W/2) uint8: 1 where any pixel of the coarse pixel's clamped 4 x 4 footprint is non-zero"""
    if need.dim() != 3 or need.shape[0] < 1 or need.dtype != U8:
        raise ValueError(f"pyr_down_need takes a non-empty (B,H,W) uint8 tensor, got {need.dtype} {tuple(need.shape)}")
    H, W = _sides(need.shape, "pyr_down_need")
    B = int(need.shape[0])
    out = torch.empty((B, H // 2, W // 2), dtype=U8, device=need.device)
    call("st3d_pyr_down_need", dptr(need.contiguous(), U8), B, H, W, dptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------------------- autograd, the steps, the cache
class _PyrDownFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return pyr_down_fwd(x.detach().to(torch.float32).contiguous())

    @staticmethod
    def backward(ctx, grad_out):
        return pyr_down_bwd(grad_out.detach().to(torch.float32).contiguous())


def pyr_down(x):
    """(B,C,H,W) on the GPU, H and W even -> (B,C,H/2,W/2); gradient to ``x`` through the transpose"""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("pyr_down takes a (B,C,H,W) tensor")
    return _PyrDownFn.apply(x)


def check_factor(f):
    if isinstance(f, bool) or not isinstance(f, int) or f not in FACTORS:
        raise ValueError(f"a pyramid factor must be one of {FACTORS}, got {f!r}")
    return f


MIN_PLAN_SIDE = 32      # the smallest side a coarse plan is built for


def check_scales(scales, weights=None, side=None):
    """``scales``: a non-empty, strictly increasing sequence from FACTORS; ``weights``: None (all 1) or one finite weight >= 0
    per scale; ``side``: the image side the scales reduce, divisible by every factor with side / f >= MIN_PLAN_SIDE.
    -> (scales, weights) as tuples of int and float; else ValueError.  Pure host logic."""
    try:
        scales = tuple(scales)
    except TypeError:
        raise ValueError(f"scales must be a sequence of factors from {FACTORS}, got {scales!r}")
    if not scales:
        raise ValueError("scales must name at least one factor")
    for f in scales:
        check_factor(f)
    if any(b <= a for a, b in zip(scales, scales[1:])):
        raise ValueError(f"scales must be strictly increasing, got {scales!r}")
    if weights is None:
        weights = (1.0,) * len(scales)
    else:
        try:
            weights = tuple(float(w) for w in weights)
        except (TypeError, ValueError):
            raise ValueError(f"scale weights must be numbers, got {weights!r}")
        if len(weights) != len(scales):
            raise ValueError(f"{len(scales)} scale(s) need as many weights, got {len(weights)}")
        if any(not (w >= 0.0 and w != float("inf")) for w in weights):
            raise ValueError(f"scale weights must be finite and >= 0, got {weights!r}")
    if side is not None:
        side = int(side)
        for f in scales:
            if side % f or side // f < MIN_PLAN_SIDE:
                raise ValueError(f"an image side of {side} does not reduce by {f}: it must be divisible by the factor and "
                                 f"leave a side >= {MIN_PLAN_SIDE}")
    return scales, weights


def reduce(x, f):
    """``x`` (B,C,H,W) reduced by ``f``: 1 returns ``x`` itself, 2 is one step, 4 is two"""
    f = check_factor(f)
    while f > 1:
        x = pyr_down(x)
        f //= 2
    return x


def reduce_need(mask, f):
    """a need mask (B,H,W) uint8 under the steps of ``reduce``: a coarse pixel is needed iff any pixel of its footprint is"""
    f = check_factor(f)
    while f > 1:
        mask = pyr_down_need(mask)
        f //= 2
    return mask


_CACHE = OrderedDict()      # key -> (the source tensor, its reduced copy), oldest first


def _key(t, f):
    return (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, f)


def reduced_cached(t, f):
    """``reduce(t, f)`` without gradient for a tensor that does not change from step to step (content renders, the style
    image).  The SAME reduced tensor comes back while ``t`` is unmodified, so the coarse plan's own target caches
    (PerceptualPlan.set_content / set_style) keep hitting.  Keyed as PerceptualPlan._same is: the source is held, so its
    address cannot be handed to another tensor while the entry lives, and compared by address and version.  One image
    expanded over the batch stays one image expanded.  At most CACHE_ENTRIES entries, oldest out."""
    f = check_factor(f)
    if f == 1:
        return t
    k = _key(t, f)
    hit = _CACHE.get(k)
    if hit is not None and hit[0].data_ptr() == t.data_ptr():
        _CACHE.move_to_end(k)
        return hit[1]
    with torch.no_grad():
        src = t.detach()
        if src.dim() == 4 and src.shape[0] > 1 and src.stride(0) == 0:
            out = reduce(src[:1], f).expand(src.shape[0], -1, -1, -1)
        else:
            out = reduce(src, f)
    while len(_CACHE) >= CACHE_ENTRIES:
        _CACHE.popitem(last=False)
    _CACHE[k] = (t, out)
    return out


def clear_cache():
    _CACHE.clear()
