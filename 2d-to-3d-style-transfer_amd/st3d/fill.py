"""Filling the texels no view moved: a pull-push fill of the texture map (Gortler et al. 1996).

A run moves only the texels some rendered pixel touches; the rest keep the loaded map's colours and show as unstyled speckle
from directions the run never used, and whatever lies outside the chart bleeds across the UV seams of a viewer that filters
the map.  The fill hands every such texel a colour interpolated from the texels that did move, from as far away as it has to
(coarse levels of an average pyramid fill the large holes, fine ones the small):

    filled, count = fill_unseen(texture, original)              # the whole map
    filled, count = fill_unseen(texture, original, domain)      # only where domain != 0

A gather with fixed-order sums and no float atomics: two runs give the same bits, and tests/_fillref.py restates the contract
in fp64.  The device wrapper of csrc/fill.hip lives here: push_pull.
"""
import torch

from . import _lib
from ._lib import call, dptr, stream_ptr

F32, U8, I32 = torch.float32, torch.uint8, torch.int32
MAX_SIDE = 16384


def _check_map(texture, name="texture"):
    if not torch.is_tensor(texture) or texture.dim() != 3 or texture.shape[2] != 3 or texture.dtype != F32:
        raise ValueError(f"{name} must be an (H, W, 3) float32 tensor")
    H, W = int(texture.shape[0]), int(texture.shape[1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"the sides of {name} must be in 1...{MAX_SIDE}, got {H} x {W}")
    return H, W


def _check_mask(mask, H, W, name):
    if not torch.is_tensor(mask) or tuple(mask.shape) != (H, W) or mask.dtype != U8:
        raise ValueError(f"{name} must be ({H}, {W}) uint8")


def moved_texels(texture, original):
    """texture, original (H,W,3) float32 -> (H,W) uint8: 1 where any channel differs in bits (the int32 views are compared, so
    -0 differs from 0 and a NaN equals itself).  Exact as "the texels the run moved": the fused Adam leaves a parameter
    whose gradient was always zero bit-identical."""
    H, W = _check_map(texture)
    if not torch.is_tensor(original) or tuple(original.shape) != (H, W, 3) or original.dtype != F32:
        raise ValueError(f"original must be ({H}, {W}, 3) float32 like texture")
    if original.device != texture.device:
        raise ValueError(f"texture is on {texture.device}, original on {original.device}")
    moved = torch.empty((H, W), dtype=U8, device=texture.device)
    moved.copy_((texture.contiguous().view(I32) != original.contiguous().view(I32)).any(-1))
    return moved


def push_pull(texture, valid, domain=None):
    """texture (H,W,3) float32, valid (H,W) uint8 (non-zero = a texel that knows its colour), domain (H,W) uint8 or None
    -> (filled (H,W,3), count: a 0-d int64 device tensor).  filled = texture bit for bit where valid, where domain is given
    and 0, or when no texel is valid; elsewhere the pull-push colour of st3d_fill_pushpull (include/st3d.h).  count = the
    texels that took it.  The workspace (about 16/3 bytes per texel) is allocated here."""
    H, W = _check_map(texture)
    _check_mask(valid, H, W, "valid")
    if domain is not None:
        _check_mask(domain, H, W, "domain")
    ws_bytes = _lib.load().st3d_fill_workspace_bytes(H, W)
    dev = texture.device
    ws = torch.empty((ws_bytes // 16, 4), dtype=F32, device=dev)
    out = torch.empty((H, W, 3), dtype=F32, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    call("st3d_fill_pushpull", dptr(texture, F32), dptr(valid, U8), dptr(domain, U8), H, W, dptr(ws), ws_bytes, dptr(out),
         dptr(count), stream_ptr())
    return out, count


def fill_unseen(texture, original, domain=None):
    """push_pull(texture, valid = moved_texels(texture, original), domain) -> (filled (H,W,3), count)"""
    return push_pull(texture, moved_texels(texture, original), domain)
