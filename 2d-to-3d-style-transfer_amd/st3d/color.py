"""Colour control for the style terms ("Colour preservation"): section 5 of Gatys et al. 2017, "Controlling
Perceptual Factors in Neural Style Transfer" -- the strokes of the style without its palette.

    y = luma(x)                          # (B,3,H,W) -> (B,3,H,W), three equal planes of Rec. 601 luminance, differentiable
    y = luma_cached(t)                   # the same without gradient for a tensor that does not change: the same object every call
    s = color_stats(images, masks)       # {'n', 'mean' (3,), 'cov' (3,3)} of the (masked) pixels, fp64 on the host
    A, b = match_matrix(src, dst)        # the affine map that gives src's pixels dst's mean and covariance
    out = recolor(images, A, b)          # that map applied (csrc/color.hip)
    out = recombine(optimised, original) # the luminance of one under the chroma of the other
    style = match_style(style, content_images, content_masks)               # section 5.1: colour matching
    style = match_style_luminance(style, content_images, content_masks)     # section 5.2: the style's luminance, matched

Colour matching recolours the style image once so that its pixel mean and covariance equal the content's; everything
downstream is unchanged.  Luminance-only transfer shows the loss the luminance of render, content and style; at the end the
optimised luminance is recombined with the content's chroma.  The arithmetic of the kernels is stated in include/st3d.h and
restated in numpy by tests/_colorref.py; all of it is per pixel and in a fixed order, two runs give the same bits.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from ._lib import call, dptr, load, stream_ptr

F32, F64, U8 = torch.float32, torch.float64, torch.uint8
LUMA_WEIGHTS = (np.float32(0.299), np.float32(0.587), np.float32(0.114))       # Rec. 601, as the kernels hold them
EIG_FLOOR = 1e-8        # eigenvalues (variances) below it are raised to it: a flat image has no palette to stretch
CACHE_ENTRIES = 8       # as st3d.imgpyr; a run with more view batches asks for more (reserve_cache)
MODES = ("off", "match", "luminance")


# ---------------------------------------------------------------------------- the device wrappers (also st3d.ops.*)
def color_stats_chunk():
    """the pixels one workgroup of color_stats owns: the sums change their association at multiples of it"""
    return int(load().st3d_color_stats_chunk())


def _planar(x, what):
    if not torch.is_tensor(x) or x.dim() not in (3, 4) or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError(f"{what} takes a non-empty (B,3,H,W) or (B,3,P) tensor, got {tuple(getattr(x, 'shape', ()))}")
    B = int(x.shape[0])
    return B, x.numel() // (3 * B)


def _stream(name, x, other=None):
    B, P = _planar(x, name)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=F32, device=x.device)
    if other is None:
        call(name, dptr(x, F32), B, P, dptr(out), stream_ptr())
    else:
        if tuple(other.shape) != tuple(x.shape):
            raise ValueError(f"{name}: the two images must have one shape, got {tuple(x.shape)} and {tuple(other.shape)}")
        call(name, dptr(x, F32), dptr(other.contiguous(), F32), B, P, dptr(out), stream_ptr())
    return out


def luma_fwd(x):
    """(B,3,H,W) | (B,3,P) float32 -> the same shape: every channel plane holds Y = fmaf(W2, b, fmaf(W1, g, W0 * r))"""
    return _stream("st3d_luma_fwd", x)


def luma_bwd(g):
    """the exact transpose of luma_fwd: s = (g0 + g1) + g2, out_c = W_c * s"""
    return _stream("st3d_luma_bwd", g)


def luma_recombine(opt, orig):
    """d = Y(opt) - Y(orig), out_c = orig_c + d: the luminance of ``opt`` under the chroma (YIQ's I and Q) of ``orig``"""
    return _stream("st3d_luma_recombine", opt, orig)


def color_affine(x, A, b, clamp=True):
    """out_c = fmaf(A[c][2], x2, fmaf(A[c][1], x1, fmaf(A[c][0], x0, b_c))), then clamped to [0,1] (NaN stays) if ``clamp``.
    ``A`` (3,3) and ``b`` (3,) are host values, rounded to fp32 once."""
    B, P = _planar(x, "color_affine")
    A = np.asarray(A, dtype=np.float64).reshape(3, 3).astype(np.float32)
    b = np.asarray(b, dtype=np.float64).reshape(3).astype(np.float32)
    ab = np.ascontiguousarray(np.concatenate([A.reshape(9), b]))       # 12 host floats: the kernel takes them by value
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=F32, device=x.device)
    call("st3d_color_affine", dptr(x, F32), ctypes.c_void_p(ab.ctypes.data), ctypes.c_void_p(ab.ctypes.data + 36), 1 if clamp else 0, B, P,
         dptr(out), stream_ptr())
    return out


def color_sums(x, mask=None):
    """(B,3,H,W) | (B,3,P) float32, mask (B,H,W) | (B,1,H,W) | (B,P) uint8 / bool or None -> (10,) float64 on the device: the
    count of the pixels whose mask byte is non-zero, their three sums x_c and six sums x_c x_d (c <= d), fp64 in a fixed
    two-stage order"""
    B, P = _planar(x, "color_stats")
    x = x.contiguous()
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(U8)
        if mask.dtype != U8 or mask.numel() != B * P or mask.shape[0] != B or mask.device != x.device:
            raise ValueError(f"color_stats: the mask must hold one uint8 per pixel ({B} x {P}), got {mask.dtype} {tuple(mask.shape)}")
        mask = mask.contiguous()
    chunks = -(-P // color_stats_chunk())
    partials = torch.empty((B * chunks * 10,), dtype=F64, device=x.device)
    out = torch.empty((10,), dtype=F64, device=x.device)
    call("st3d_color_stats", dptr(x, F32), dptr(mask), B, P, dptr(partials), dptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------------------- autograd and the cache
def _fmaf(a, b, c):
    """fmaf on three fp32 scalars, correctly rounded: the exact fp64 product, the sum rounded to odd (TwoSum's error says
    whether and whither to move off an even last bit), then one rounding to fp32 (tests/_colorref.py has the argument)"""
    p, c = np.float64(a) * np.float64(b), np.float64(c)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    if np.isfinite(e) and e != 0 and not (np.array(s).view(np.int64) & 1):
        s = np.nextafter(s, np.inf if e > 0 else -np.inf)
    return np.float32(s)


def luma_of_color(c):
    """the numpy-fp32 restatement of Y for one colour (3 floats): what luma_fwd writes where the image holds ``c``"""
    r, g, b = (np.float32(v) for v in c)
    return float(_fmaf(LUMA_WEIGHTS[2], b, _fmaf(LUMA_WEIGHTS[1], g, np.float32(LUMA_WEIGHTS[0] * r))))


class _LumaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return luma_fwd(x.detach().to(F32).contiguous())

    @staticmethod
    def backward(ctx, grad_out):
        return luma_bwd(grad_out.detach().to(F32).contiguous())


def luma(x):
    """(B,3,H,W) on the GPU -> (B,3,H,W) luminance planes, gradient to ``x`` through the transpose (luma_bwd).

    The output CARRIES THE TAGS of ``x``'s producer (st3d.render.tag_need, tag_flat, FragmentCache epochs), so a loss that
    is handed ``luma(render)`` skips what it skips for the render itself:
      * need: the same tensor object.  The op is per pixel: its backward reads its incoming gradient at pixel p only to
        write its own output gradient at p, and the render's backward reads that at covered pixels only -- so whatever
        produces the gradient of ``luma(x)`` is read at exactly the render's covered pixels.
      * epoch: unchanged (it names the need tensor, which is the same object, so epoch_of's identity check still holds).
      * flat: the tagged colour c becomes (y, y, y), y = Y(c) in the kernel's roundings: every uncovered pixel of ``x``
        holds c bit for bit, so every uncovered pixel of the output holds y.  A hint only: the device compares the pixels.
    A tensor without tags gives a tensor without tags."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("luma takes a (B,3,H,W) tensor")
    from . import render as _render      # (render imports ops, which re-exports this module's wrappers)
    out = _LumaFn.apply(x)
    if out.requires_grad:
        need = getattr(x, _render.NEED_TAG, None)
        if need is not None and _render.need_of(x) is not None:      # (a watched or leaf tensor hands nothing on)
            setattr(out, _render.NEED_TAG, need)
            epoch = getattr(x, _render.EPOCH_TAG, None)
            if epoch is not None:
                setattr(out, _render.EPOCH_TAG, epoch)
    flat = _render.flat_of(x)
    if flat is not None:
        y = luma_of_color(flat)
        setattr(out, _render.FLAT_TAG, (y, y, y))
    return out


_CACHE = OrderedDict()      # key -> (the source tensor, its luminance), oldest first


def _key(t):
    return (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype)


def _luma_nograd(src):
    return luma_fwd(src.to(F32).contiguous())


def luma_cached(t):
    """``luma(t)`` without gradient for a tensor that does not change from step to step (content renders, the style image).
    The SAME tensor comes back while ``t`` is unmodified, so PerceptualPlan.set_content / set_style keep hitting their
    identity caches and ``imgpyr.reduced_cached(luma_cached(content), f)`` composes.  Keyed as imgpyr.reduced_cached is:
    address, version, shape, stride; the source is held, so its address cannot be handed to another tensor while the entry
    lives.  One image expanded over the batch stays one image expanded.  At most CACHE_ENTRIES entries (8, or what
    reserve_cache asked for), oldest out; every entry holds its source and its luminance until then."""
    k = _key(t)
    hit = _CACHE.get(k)
    if hit is not None and hit[0].data_ptr() == t.data_ptr():
        _CACHE.move_to_end(k)
        return hit[1]
    with torch.no_grad():
        src = t.detach()
        if src.dim() == 4 and src.shape[0] > 1 and src.stride(0) == 0:
            out = _luma_nograd(src[:1]).expand(src.shape[0], -1, -1, -1)
        else:
            out = _luma_nograd(src)
    while len(_CACHE) >= CACHE_ENTRIES:
        _CACHE.popitem(last=False)
    _CACHE[k] = (t, out)
    return out


def clear_cache():
    _CACHE.clear()


def reserve_cache(entries):
    """make room for ``entries`` sources at once (never fewer than the default): a loop that cycles through more tensors than
    the cache holds would miss on every call, recompute every luminance and, with it, every target a plan keys on the
    returned tensor.  A run calls it with its number of view batches."""
    global CACHE_ENTRIES
    CACHE_ENTRIES = max(CACHE_ENTRIES, int(entries))


# ---------------------------------------------------------------------------- moments and the match (host, fp64)
def stats_from_sums(sums):
    """the 10 sums (count, sum x_c, sum x_c x_d for c <= d) -> {'n', 'mean' (3,), 'cov' (3,3)}: the population covariance
    S_cd / n - mu_c mu_d, fp64 numpy.  n == 0: ValueError."""
    s = np.asarray(sums, dtype=np.float64).reshape(10)
    n = s[0]
    if not n > 0:
        raise ValueError("color_stats: no pixel selected (the mask is empty)")
    mean = s[1:4] / n
    second = np.empty((3, 3), np.float64)
    for k, (c, d) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        second[c, d] = second[d, c] = s[4 + k] / n
    return {"n": int(n), "mean": mean, "cov": second - np.outer(mean, mean)}


def color_stats(images, masks=None):
    """(B,3,H,W) images [, (B,H,W) | (B,1,H,W) uint8 / bool masks] -> {'n', 'mean', 'cov'} of the selected pixels"""
    return stats_from_sums(color_sums(images, masks).cpu().numpy())


def _sym_power(cov, power):
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    w = np.maximum(w, EIG_FLOOR)
    return (v * w ** power) @ v.T


def match_matrix(src, dst):
    """-> (A (3,3), b (3,)) fp64 with A Sigma_src A^T = Sigma_dst and A mu_src + b = mu_dst:
    A = Sigma_dst^(1/2) Sigma_src^(-1/2), symmetric square roots by eigendecomposition (the "image analogies" variant
    Gatys et al. prefer), eigenvalues below EIG_FLOOR raised to it; b = mu_dst - A mu_src.  Pure host logic."""
    A = _sym_power(dst["cov"], 0.5) @ _sym_power(src["cov"], -0.5)
    b = np.asarray(dst["mean"], np.float64) - A @ np.asarray(src["mean"], np.float64)
    return A, b


def luma_match(src_stats, dst_stats):
    """the one-dimensional match on channel 0 of luminance images -> (k, b): k = sigma_dst / sigma_src with both variances
    floored at EIG_FLOOR, b = mu_dst - k mu_src"""
    vs = max(float(src_stats["cov"][0][0]), EIG_FLOOR)
    vd = max(float(dst_stats["cov"][0][0]), EIG_FLOOR)
    k = float(np.sqrt(vd) / np.sqrt(vs))
    return k, float(dst_stats["mean"][0]) - k * float(src_stats["mean"][0])


def recolor(images, A, b, clamp=True):
    """the affine map x -> A x + b on every pixel of (B,3,H,W) images, clamped to [0,1] unless ``clamp`` is False"""
    return color_affine(images, A, b, clamp)


def recombine(optimised, original):
    """(B,3,H,W), (B,3,H,W) -> (B,3,H,W): the luminance of ``optimised`` under the chroma of ``original`` (Gatys et al. 2017,
    section 5.2; luma_recombine)"""
    if optimised.dim() != 4 or optimised.shape[1] != 3 or tuple(original.shape) != tuple(optimised.shape):
        raise ValueError(f"recombine takes two (B,3,H,W) tensors of one shape, got {tuple(optimised.shape)} and "
                         f"{tuple(original.shape)}")
    return luma_recombine(optimised.detach().to(F32), original.detach().to(F32))


def recombine_texture(optimised, original):
    """``recombine`` for the channel-last colour carriers -- (1,T,T',3) maps, (V,3) vertex colours, (F,R,R,3) atlases: permuted
    to one planar (1,3,N) image, the kernel, and back.  Runs once per run."""
    if optimised.shape[-1] != 3 or tuple(original.shape) != tuple(optimised.shape) or optimised.numel() == 0:
        raise ValueError(f"recombine_texture takes two (...,3) tensors of one shape, got {tuple(optimised.shape)} and "
                         f"{tuple(original.shape)}")
    planar = lambda t: t.detach().to(F32).reshape(-1, 3).t().contiguous()[None]
    planes = luma_recombine(planar(optimised), planar(original))
    out = torch.empty(optimised.shape, dtype=F32, device=optimised.device)
    out.view(-1, 3).copy_(planes[0].t())
    return out


def match_style(style, content_images, content_masks=None, clamp=True):
    """section 5.1: ``style`` (1 | B,3,H,W) recoloured so that its pixel mean and covariance equal those of the (masked)
    pixels of ``content_images``; -> the new style image"""
    A, b = match_matrix(color_stats(style), color_stats(content_images, content_masks))
    return recolor(style, A, b, clamp)


def match_style_luminance(style, content_images, content_masks=None, clamp=True):
    """section 5.2: the luminance of ``style``, its mean and variance matched to those of the luminance of the (masked)
    pixels of ``content_images``; -> the new style image, three equal planes"""
    ys = luma_fwd(style.detach().to(F32))
    k, b = luma_match(color_stats(ys), color_stats(luma_fwd(content_images.detach().to(F32)), content_masks))
    return recolor(ys, np.eye(3) * k, np.full(3, b), clamp)
