"""The Laplacian content term ("Laplacian content loss"): Li, Xu, Nie and Chua 2017, "Laplacian-Steered Neural
Style Transfer" -- the render keeps the fine detail of the asset (eyes, panel lines, print) that the conv4_2 content term,
with its receptive field of about a hundred pixels, does not see.

    L = lap_fwd(x, p)                          # (B,C,H,W) -> (B,C,H/p,W/p): D(pool_p(x)), every channel on its own
    loss, grad = lap_loss(x, T, p, scale)      # fp32((sum (L - T)^2) * scale) and d loss / d x from one fused pass
    T = lap_target_cached(content, p)          # lap_fwd of a tensor that does not change: the same object every call
    pools = check_pools(pools, S)              # a strictly increasing sequence from POOLS that fits the image side S

pool_p is the p x p block average, D the 5-point Laplacian with a replicate border (csrc/lap.hip).  D is symmetric, so the
backward applies the same stencil to the residual and hands every pixel of a block the block's value: a gather in a fixed
order, no atomics, two runs give the same bits.  The arithmetic is stated in include/st3d.h and restated in numpy by
tests/_lapref.py.
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ._lib import call, dptr, load, stream_ptr

F32, F64 = torch.float32, torch.float64
POOLS = (1, 2, 4, 8, 16)
CACHE_ENTRIES = 8       # as st3d.imgpyr; a run with more view batches asks for more (reserve_cache)
MAX_SIDE = 32768


def check_pools(pools, S=None):
    """``pools``: a non-empty, strictly increasing sequence from POOLS; ``S``: the image side (or (H, W)) they pool, divisible
    by every pool side with a pooled side >= 2.  -> the pools as a tuple of int; else ValueError.  Pure host logic."""
    try:
        pools = tuple(pools)
    except TypeError:
        raise ValueError(f"pools must be a sequence of pool sides from {POOLS}, got {pools!r}")
    if not pools:
        raise ValueError("pools must name at least one pool side")
    for p in pools:
        if isinstance(p, bool) or not isinstance(p, int) or p not in POOLS:
            raise ValueError(f"a pool side must be one of {POOLS}, got {p!r}")
    if any(b <= a for a, b in zip(pools, pools[1:])):
        raise ValueError(f"pools must be strictly increasing, got {pools!r}")
    if S is not None:
        sides = (int(S),) if isinstance(S, int) else tuple(int(s) for s in S)
        for side in sides:
            for p in pools:
                if side % p or side // p < 2:
                    raise ValueError(f"an image side of {side} does not pool by {p}: it must be divisible by the pool side and "
                                     f"leave a pooled side >= 2")
    return pools


# ---------------------------------------------------------------------------- the device wrappers (also st3d.ops.lap_*)
def lap_tile(p):
    """(rows, columns) of fine pixels one workgroup of the kernels owns at pool side ``p``: halos cross tile borders there"""
    check_pools((p,))
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    call("st3d_lap_tile", int(p), ctypes.byref(h), ctypes.byref(w))
    return h.value, w.value


def _planes(x, p, what):
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[0] * x.shape[1] < 1:
        raise ValueError(f"{what} takes a non-empty (B,C,H,W) tensor, got {tuple(getattr(x, 'shape', ()))}")
    check_pools((p,))
    H, W = int(x.shape[2]), int(x.shape[3])
    if H % p or W % p or H // p < 2 or W // p < 2 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: a pool side of {p} takes sides it divides, pooled sides >= 2 and sides <= {MAX_SIDE}, got "
                         f"{tuple(x.shape)}")
    return int(x.shape[0]), int(x.shape[1]), H, W


def lap_fwd(x, p):
    """(B,C,H,W) float32 -> (B,C,H/p,W/p): D(pool_p(x)), roundings as include/st3d.h states them"""
    B, C, H, W = _planes(x, p, "lap_fwd")
    out = torch.empty((B, C, H // p, W // p), dtype=F32, device=x.device)
    call("st3d_lap_fwd", dptr(x.contiguous(), F32), B * C, H, W, int(p), dptr(out), stream_ptr())
    return out


def lap_loss(x, target, p, scale, want_grad=True):
    """x (B,C,H,W), target (B,C,H/p,W/p) float32, ``scale`` a host double -> (loss (1,) float32, grad (B,C,H,W) | None):
    loss = fp32(scale * sum r^2) with r = D(pool_p(x)) - target, squares and sum in fp64 in a fixed order;
    grad = fp32(2 scale / p^2) * D(r) spread over every block.  Three launches, two without the gradient."""
    B, C, H, W = _planes(x, p, "lap_loss")
    if tuple(target.shape) != (B, C, H // p, W // p):
        raise ValueError(f"lap_loss: images {tuple(x.shape)} at pool side {p} need a target {(B, C, H // p, W // p)}, got "
                         f"{tuple(target.shape)}")
    scale = float(scale)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise ValueError(f"lap_loss: the scale must be finite and >= 0, got {scale!r}")
    nbytes = int(load().st3d_lap_workspace_bytes(B * C, H, W, int(p)))
    ws = torch.empty(((nbytes + 7) // 8,), dtype=F64, device=x.device)
    out = torch.empty((1,), dtype=F32, device=x.device)
    g = torch.empty((B, C, H, W), dtype=F32, device=x.device) if want_grad else None
    call("st3d_lap_loss", dptr(x.contiguous(), F32), dptr(target.contiguous(), F32), B * C, H, W, int(p), scale, dptr(ws),
         ws.numel() * 8, dptr(out), dptr(g), stream_ptr())
    return out, g


# ---------------------------------------------------------------------------- the term and the cache
def term_scale(shape, p, batch_denom=None):
    """1 / (batch_denom C h w) as a host double: the mean over the pooled residuals, the batch taken as ``batch_denom``
    (None: the images' own batch)"""
    B, C, H, W = (int(s) for s in shape)
    bd = B if batch_denom is None else int(batch_denom)
    if bd < 1:
        raise ValueError(f"batch_denom must be >= 1, got {batch_denom!r}")
    return 1.0 / (float(bd) * C * (H // p) * (W // p))


def lap_term(x, targets, pools, batch_denom=None, want_grad=True):
    """the terms of ``pools`` against ``targets`` (one per pool), and their gradients, added in ascending pool side in
    fp32 -> (loss (1,), grad | None): what losses.compute_laplacian_loss hands to its autograd function"""
    loss = grad = None
    for p, T in zip(pools, targets):
        l, g = lap_loss(x, T, p, term_scale(x.shape, p, batch_denom), want_grad)
        loss = l if loss is None else loss + l
        if want_grad:
            grad = g if grad is None else grad + g
    return loss, grad


_CACHE = OrderedDict()      # key -> (the source tensor, its Laplacian target), oldest first


def _key(t, p):
    return (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, p)


def lap_target_cached(content, p):
    """``lap_fwd(content, p)`` without gradient for a tensor that does not change from step to step (the content renders).
    The SAME tensor comes back while ``content`` is unmodified.  Keyed as imgpyr.reduced_cached is: address, version, shape,
    stride; the source is held, so its address cannot be handed to another tensor while the entry lives.  At most
    CACHE_ENTRIES entries (8, or what reserve_cache asked for), oldest out."""
    check_pools((p,))
    k = _key(content, p)
    hit = _CACHE.get(k)
    if hit is not None and hit[0].data_ptr() == content.data_ptr():
        _CACHE.move_to_end(k)
        return hit[1]
    with torch.no_grad():
        out = lap_fwd(content.detach().to(F32).contiguous(), p)
    while len(_CACHE) >= CACHE_ENTRIES:
        _CACHE.popitem(last=False)
    _CACHE[k] = (content, out)
    return out


def clear_cache():
    _CACHE.clear()


def reserve_cache(entries):
    """make room for ``entries`` targets at once (never fewer than the default): a run calls it with its number of view
    batches times its number of pools, so that no step recomputes a target"""
    global CACHE_ENTRIES
    CACHE_ENTRIES = max(CACHE_ENTRIES, int(entries))
