"""numpy restatement of the kept lists (csrc/need.hip, st3d_kept_build): which output blocks of the forward launches conv1_2 ..
conv3_3 may differ between two calls of a geometry epoch.  M_0 is the coverage, the only pixels that may differ:

    conv1_1 (direct, per pixel)          X = dilate(M_0, 1)
    an F(4x4,3x3) launch with input X    K = block4(dilate(X, 1)): an aligned 4x4 output block comes, rounding included, from
                                         its own 6x6 input patch; the output map is K, its blocks taken whole
    through a fused 2x2 pool             the 2x2 OR
    list k                               the tiles (or strips, four per step, padded per image) that hold a block of K_k

Lists 0 .. 5 = conv1_2 (+pool), conv2_1, conv2_2 (+pool), conv3_1, conv3_2, conv3_3: the maps of the need lists
(tests/_needblocks_ref.py).  Whole-array operations on pixel maps only (the device works on block bitmaps in LDS)."""
import numpy as np

import _needblocks_ref as NB
import _needref as NR
import _needstrips_ref as NS

LIST_NAMES = NB.LIST_NAMES
LIST_SHIFT = NB.LIST_SHIFT
LIST_POOLS = (True, False, True, False, False, False)      # the launch pools in its epilogue


def kept_maps(cover, nlists=6, mutant=None):
    """cover (n, S, S) -> [K_k (n, R_k, R_k) bool].  mutant: None, "no_dilate" (a launch's blocks are block4(X)) or "pixel_pool"
    (what goes through the pool is dilate(X, 1) per pixel, not K's whole blocks) -- both must fail tests/test_kept_ref.py."""
    X = NR.dilate(np.asarray(cover) != 0)
    out = []
    for k in range(nlists):
        reach = X if mutant == "no_dilate" else NR.dilate(X)
        K = NB.block4(reach)
        out.append(K)
        X = K
        if LIST_POOLS[k]:
            X = NR.pool_or(reach if mutant == "pixel_pool" else K)
    return out


def kept_model(cover, nlists=6, tile_cols=None):
    """cover (n, S, S) -> dict: K[k]; lists[k] = ascending int32 tile numbers in geometry tile_cols[k] (None / 0: the kernel's
    own; 64 / 32), or for tile_cols[k] == 16 the strip entries (four per step, -1 = void); counts[k] = tiles or steps"""
    K = kept_maps(cover, nlists)
    out = {"K": K, "lists": [], "counts": []}
    for k, m in enumerate(K):
        cols = tile_cols[k] if tile_cols else None
        if cols == 16:
            e, c = NS.strip_list(m)
        else:
            rows, cols = NB.geometry(m.shape[1], cols)
            e = np.flatnonzero(NR.tiles_any(m, rows, cols).reshape(-1)).astype(np.int32)
            c = len(e)
        out["lists"].append(e)
        out["counts"].append(c)
    return out


def covers(n, S):
    """name -> (n, S, S) uint8: the masks of tests/_needstrips_ref.py (empty, full, corners, blob, an empty image between
    covered ones) and three covers of one or two pixels whose strip counts of list 3 (conv3_1) are 1, 2 and 3 mod 4 per image"""
    out = {k: v for k, v in NS.masks(n, S).items() if not k.startswith("mod")}
    want = {1, 2, 3}
    for corner in (0, 1):           # one pixel, then one pixel and the far corner
        for y in range(0, S // 2, 3):
            for x in range(0, S // 2, 5):
                if not want:
                    return out
                m = np.zeros((1, S, S), np.uint8)
                m[0, y, x] = 1
                m[0, -1, -1] = corner
                r = int(NS.strips_of(kept_maps(m, 4)[3]).sum()) % 4
                if r in want:
                    want.discard(r)
                    out["mod%d" % r] = np.repeat(m, n, axis=0)
    assert not want, want
    return out


# ---- a conv / ReLU / pool chain with the dependence structure of the kernels, exact in fp64
def conv3x3(x, w):
    """x (n, C, H, W), w (Co, C, 3, 3), zero padding"""
    n, C, H, W = x.shape
    xp = np.zeros((n, C, H + 2, W + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((n, w.shape[0], H, W), x.dtype)
    for dy in range(3):
        for dx in range(3):
            y += np.einsum("oc,nchw->nohw", w[:, :, dy, dx], xp[:, :, dy:dy + H, dx:dx + W])
    return y


def block_conv3x3(x, w):
    """conv3x3 plus, on every element of an aligned 4x4 output block, the sum of the block's whole 6x6 input patch (all
    channels, zero padding): what stands in here for the rounding of an F(4x4,3x3) block, which comes from the whole patch"""
    n, C, H, W = x.shape
    s = x.sum(axis=1)
    sp = np.zeros((n, H + 2, W + 2), x.dtype)
    sp[:, 1:-1, 1:-1] = s
    c = np.cumsum(np.cumsum(np.pad(sp, ((0, 0), (1, 0), (1, 0))), axis=1), axis=2)
    y0, x0 = np.arange(0, H, 4), np.arange(0, W, 4)
    patch = c[:, y0[:, None] + 6, x0[None, :] + 6] - c[:, y0[:, None], x0[None, :] + 6] - c[:, y0[:, None] + 6, x0[None, :]] + \
        c[:, y0[:, None], x0[None, :]]
    return conv3x3(x, w) + NR.expand(patch, 4, 4)[:, None]


def pool2x2(x):
    n, C, H, W = x.shape
    return x.reshape(n, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def chain(img, weights):
    """img (n, 3, S, S) fp64, weights: 7 arrays (conv1_1, conv1_2, conv2_1, conv2_2, conv3_1, conv3_2, conv3_3) -> the outputs of
    the six Winograd launches as stored (conv1_2 and conv2_2 pooled: their full-resolution output is never kept)"""
    x = np.maximum(conv3x3(img, weights[0]), 0)
    outs = []
    for k in range(6):
        x = np.maximum(block_conv3x3(x, weights[1 + k]), 0)
        full = x
        if LIST_POOLS[k]:
            x = pool2x2(x)
        outs.append((full, x))
    return outs
