"""numpy restatement of the per-block need propagation (csrc/need.hip, st3d_need_blocks_build).  An F(4x4,3x3) launch
computes each aligned 4x4 output block from that block's own 6x6 input patch, so with need_k the pixels at which the
output of list k's launch is needed:

    B_k      = block4(need_k)                                  the blocks the launch has to get right
    list k   = the tiles of the launch's geometry that hold a block of B_k
    need_k+1 = dilate(B_k, 1), clipped to the map, then the 2x2 OR where launch k un-pools its input

need_0 = dilate(mask, 1): the relu1_1 pass gathers 3x3 at mask pixels.  Whole-array operations on pixel maps only (the
device works on block bitmaps in LDS)."""
import numpy as np

import _needref as NR

LIST_NAMES = ("conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3")     # the input gradients, bottom up
LIST_SHIFT = (0, 1, 1, 2, 2, 2)                    # list k's map is (S >> shift)^2
LIST_UNPOOLS = (True, False, True, False, False, False)


def geometry(R, cols=None):
    """(rows, cols) of the tiles of an R x R map: the kernel's own choice, or the one asked for (64 / 32) where it fits"""
    if not cols:
        return NR.tile_geometry(R, R)
    if cols == 64 and R % 64 == 0:
        return 4, 64
    if cols == 32 and R % 32 == 0 and R % 8 == 0:
        return 8, 32
    return None


def n_lists(S):
    k = 0
    while k < len(LIST_NAMES) and S % 64 == 0 and geometry(S >> LIST_SHIFT[k]) is not None:
        k += 1
    return k


def block4(need):
    """the pixels of the aligned 4x4 blocks that hold a needed pixel"""
    return NR.expand(NR.tiles_any(need, 4, 4), 4, 4)


def erode_blocks(B):
    """(mutant) B without its outermost ring of blocks"""
    b = NR.tiles_any(B, 4, 4)
    return NR.expand(~NR.dilate(~b), 4, 4)


def need_blocks_model(mask, nlists=None, tile_cols=None, mutant=None):
    """mask (n, S, S) -> dict: seg (n, S, S/64) uint8; lists[k] ascending int32 tile numbers ((n * tiles_y + ty) * tiles_x +
    tx) in geometry tile_cols[k] (None / 0: the kernel's own); need[k] (n, R_k, R_k) bool = need_k; reads[k] = need_k+1 at the
    resolution launch k's input is stored at (pooled where it un-pools); geo[k] = (rows, cols); gram = the 64-pixel runs of the
    (S/2)^2 map (image * runs per image + run, ascending) that meet reads[1], the pixels at which the conv2_1 input gradient
    reads the gradient of relu2_1 (None where S/2 is no multiple of 64 or there are fewer than two lists).
    mutant: None, "shrink" (the blocks lose their outer ring before they are handed up) or "no_pool_or" (the pooled need is
    the top-left sample of each 2x2 window instead of its OR) -- both must fail the sufficiency check."""
    mask = np.asarray(mask) != 0
    n, S, _ = mask.shape
    nlists = n_lists(S) if nlists is None else nlists
    out = {"seg": NR.segments(mask), "lists": [], "need": [], "reads": [], "geo": []}
    need = NR.dilate(mask)
    for k in range(nlists):
        R = S >> LIST_SHIFT[k]
        assert need.shape == (n, R, R)
        rows, cols = geometry(R, tile_cols[k] if tile_cols else None)
        B = block4(need)
        out["need"].append(need)
        out["geo"].append((rows, cols))
        out["lists"].append(np.flatnonzero(NR.tiles_any(B, rows, cols).reshape(-1)).astype(np.int32))
        need = NR.dilate(erode_blocks(B) if mutant == "shrink" else B)
        if LIST_UNPOOLS[k]:
            need = need[:, ::2, ::2].copy() if mutant == "no_pool_or" else NR.pool_or(need)
        out["reads"].append(need)
    out["gram"] = None
    if nlists >= 2 and (S // 2) % 64 == 0:
        out["gram"] = np.flatnonzero(NR.tiles_any(out["reads"][1], 1, 64).reshape(-1)).astype(np.int32)
    return out


def tile_pixels(tile_ids, n, R, rows, cols):
    """(n, R, R) bool: the pixels of the listed tiles of a rows x cols geometry"""
    t = np.zeros(n * (R // rows) * (R // cols), bool)
    t[np.asarray(tile_ids, np.int64)] = True
    return NR.expand(t.reshape(n, R // rows, R // cols), rows, cols)
