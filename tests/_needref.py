"""numpy restatement of the need propagation (csrc/need.hip): from the pixels at which the render backward reads the image
gradient to the units the bottom launches of the VGG backward have to compute.  Whole-array operations only -- dilate,
any-reduce over tiles, expand, 2x2 OR-pool -- where the device works tile by tile from index ranges."""
import numpy as np


def dilate(m):
    """OR over the 3x3 window, (n, H, W) bool"""
    n, H, W = m.shape
    p = np.zeros((n, H + 2, W + 2), bool)
    p[:, 1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[:, dy:dy + H, dx:dx + W]
    return out


def tile_geometry(H, W):
    """(rows, cols) of the F(4x4,3x3) kernel's output tiles: 4 x 64 where the row is a multiple of 64 pixels, else 8 x 32"""
    if H > 0 and W > 0 and H % 4 == 0 and W % 64 == 0:
        return 4, 64
    if H > 0 and W > 0 and H % 8 == 0 and W % 32 == 0:
        return 8, 32
    return None


def tiles_any(m, rows, cols):
    n, H, W = m.shape
    return m.reshape(n, H // rows, rows, W // cols, cols).any(axis=(2, 4))


def expand(t, rows, cols):
    return np.repeat(np.repeat(t, rows, axis=1), cols, axis=2)


def pool_or(m):
    return tiles_any(m, 2, 2)


def segments(mask):
    """(n, H, W) -> (n, H, W / 64) uint8: the 64-pixel row segments that touch dilate(mask, 1)"""
    return tiles_any(dilate(np.asarray(mask) != 0), 1, 64).astype(np.uint8)


def need_model(mask, levels=3):
    """mask (n, S, S) -> (seg (n, S, S/64) uint8, [ascending int32 tile lists]): level 1 = seg, level 2 = the conv1_2
    input-gradient tiles (S x S map), level 3 = the conv2_1 input-gradient tiles (S/2 x S/2 map)."""
    mask = np.asarray(mask) != 0
    n, S, _ = mask.shape
    seg = segments(mask)
    lists = []
    cover = expand(seg != 0, 1, 64)              # the pixels at which the relu1_1 pass reads its input gradient
    res = S
    for level in range(levels - 1):
        rows, cols = tile_geometry(res, res)
        t = tiles_any(cover, rows, cols)
        lists.append(np.flatnonzero(t.reshape(-1)).astype(np.int32))
        # this launch reads the 1-pixel-dilated patch of its output tiles; conv1_2's input arrives pooled
        cover = dilate(expand(t, rows, cols))
        if level == 0:
            cover = pool_or(cover)
            res //= 2
    return seg, lists


def tile_pixels(tile_ids, n, H, W):
    """(n, H, W) bool: the pixels of the listed tiles"""
    rows, cols = tile_geometry(H, W)
    t = np.zeros(n * (H // rows) * (W // cols), bool)
    t[np.asarray(tile_ids, np.int64)] = True
    return expand(t.reshape(n, H // rows, W // cols), rows, cols)
