"""numpy restatement of the flat-field lists (csrc/flat.hip): which output tiles of the forward launches of conv1_2,
conv2_1 and conv2_2 see anything but the field the background colour produces, and which tile stands for the others.
Whole-array operations (dilate, any-reduce over tiles, 2x2 OR-pool from tests/_needref.py) where the device works tile by
tile from index ranges of one pooled map."""
import numpy as np

import _needref as NR


def varying_pixels(imgs, color):
    """(n,3,S,S) float32, (3,) float32 -> (n,S,S) bool: the pixel differs from the colour in any channel, as bits"""
    bits = np.ascontiguousarray(imgs, np.float32).view(np.uint32)
    cbits = np.asarray(color, np.float32).view(np.uint32)
    return (bits != cbits[None, :, None, None]).any(axis=1)


def dilate_k(m, k):
    for _ in range(k):
        m = NR.dilate(m)
    return m


def block4(m):
    """the aligned 4x4 blocks that meet m"""
    return NR.expand(NR.tiles_any(m, 4, 4), 4, 4)


def tile_classes(n, TY, TX, D=2):
    """(n,TY,TX) int: the border signature (min(ty,D), min(TY-1-ty,D), min(tx,D), min(TX-1-tx,D)) as one number"""
    ty, tx = np.arange(TY)[:, None], np.arange(TX)[None, :]
    c = ((np.minimum(ty, D) * (D + 1) + np.minimum(TY - 1 - ty, D)) * (D + 1) + np.minimum(tx, D)) * (D + 1) + np.minimum(TX - 1 - tx, D)
    return np.broadcast_to(c[None], (n, TY, TX))


def list_and_map(vary, per_view=False):
    """vary (n,TY,TX) bool -> (ascending int32 list of varying tiles + one representative per class of the others, int32
    map tile -> representative, -1 for listed tiles).  per_view: the MUTANT that picks a representative in every view."""
    n, TY, TX = vary.shape
    cls = tile_classes(n, TY, TX).reshape(-1).copy()
    if per_view:
        cls += 1000 * np.repeat(np.arange(n), TY * TX)
    v = vary.reshape(-1)
    rep = np.full(v.size, -1, np.int32)
    for c in np.unique(cls[~v]):
        members = np.flatnonzero(~v & (cls == c))
        rep[members] = members[0]
    listed = v | (rep == np.arange(v.size))
    return np.flatnonzero(listed).astype(np.int32), np.where(listed, -1, rep).astype(np.int32)


def varying_tiles(imgs, color, conv_dilation=1):
    """-> [vary (n,TY,TX) bool] for conv1_2, conv2_1, conv2_2.  "Varying" = may differ from the flat field in any bit.  The
    direct conv1_1 maps V to dilate(V, 1); a Winograd conv rounds a whole 4x4 output block from its 6x6 patch, so it maps V
    to block4(dilate(V, 1)); a pool maps V to the 2x2 OR.  A tile (whole blocks) varies iff its input patch (tile +- 1,
    clipped) meets the V of its input = the tile meets dilate(V_in, 1).
    conv_dilation != 1 is the MUTANT with every conv's dilation off by one."""
    d = conv_dilation
    S = imgs.shape[-1]
    v_in = dilate_k(varying_pixels(imgs, color), d)          # behind conv1_1: the input of conv1_2
    out = []
    for launch in range(3):
        res = S if launch == 0 else S // 2
        rows, cols = NR.tile_geometry(res, res)
        reach = dilate_k(v_in, d)
        out.append(NR.tiles_any(reach, rows, cols))
        v_in = NR.pool_or(block4(reach)) if launch == 0 else block4(reach)
    return out


def flat_model(imgs, color, conv_dilation=1, per_view=False):
    """-> [(list, map, vary)] per launch"""
    return [list_and_map(v, per_view) + (v,) for v in varying_tiles(imgs, color, conv_dilation)]


def tiles_view(t, rows, cols):
    """(n,C,H,W) array or tensor -> (n * H/rows * W/cols, C, rows, cols): tile t of the launch's numbering first"""
    n, C, H, W = t.shape
    return t.reshape(n, C, H // rows, rows, W // cols, cols).transpose(0, 2, 4, 1, 3, 5).reshape(-1, C, rows, cols) \
        if isinstance(t, np.ndarray) else \
        t.reshape(n, C, H // rows, rows, W // cols, cols).permute(0, 2, 4, 1, 3, 5).reshape(-1, C, rows, cols)


def images(n, S, color, what, seed=0):
    """(n,3,S,S) float32 holding `color` except where `what` says otherwise"""
    rng = np.random.default_rng(seed + 31 * S + n)
    img = np.empty((n, 3, S, S), np.float32)
    img[:] = np.asarray(color, np.float32)[None, :, None, None]
    tex = rng.random((n, 3, S, S), dtype=np.float32)

    def put(m):
        img[:] = np.where(m[:, None], tex, img)
    m = np.zeros((n, S, S), bool)
    if what == "empty":
        pass
    elif what == "full":
        m[:] = True
    elif what == "one_pixel":
        m[n - 1, S // 2 + 1, S // 2 + 3] = True
    elif what == "one_channel":          # differs in the last channel only
        img[n - 1, 2, 9, S - 5] = tex[n - 1, 2, 9, S - 5]
    elif what == "corners":
        m[:, 0, 0] = m[:, 0, -1] = m[:, -1, 0] = m[:, -1, -1] = True
    elif what == "nan":                  # NaN is varying; so is the colour with its sign flipped
        img[0, 1, 20, 40] = np.nan
        img[n - 1, 0, S - 9, 7] = -img[n - 1, 0, S - 9, 7]
    elif what == "blobs":
        for i in range(n):
            for _ in range(2):
                h, w = rng.integers(1, S // 3, 2)
                y, x = rng.integers(0, S - h + 1), rng.integers(0, S - w + 1)
                m[i, y:y + h, x:x + w] = True
    elif what == "first_view_only":      # the other views are entirely flat: their tiles take view 0's representatives
        m[0, S // 4:S // 2, S // 4:S // 2] = True
    else:
        raise KeyError(what)
    put(m)
    return img


def rect_image(n, S, color, y0, y1, x0, x1, view=0):
    """flat except rows y0..y1, columns x0..x1 (inclusive) of one view, which hold color + 0.25"""
    img = images(n, S, color, "empty")
    img[view, :, y0:y1 + 1, x0:x1 + 1] += np.float32(0.25)
    return img


def rect_expected(S, y0, y1, x0, x1):
    """The varying tile ranges [(ty_a, ty_b, tx_a, tx_b)] of the three launches for rect_image, by interval arithmetic: a
    conv grows the rectangle by 1 (conv1_1 and conv1_2: by 2), a Winograd conv's output then snaps outward to whole 4x4
    blocks, the pool halves it."""
    snap = lambda a, b: (a // 4 * 4, b // 4 * 4 + 3)
    out = []
    ya, yb, xa, xb = max(y0 - 2, 0), min(y1 + 2, S - 1), max(x0 - 2, 0), min(x1 + 2, S - 1)
    rows, cols = NR.tile_geometry(S, S)
    out.append((ya // rows, yb // rows, xa // cols, xb // cols))
    Sh = S // 2
    (ya, yb), (xa, xb) = snap(ya, yb), snap(xa, xb)
    ya, yb, xa, xb = ya // 2, yb // 2, xa // 2, xb // 2
    rows, cols = NR.tile_geometry(Sh, Sh)
    for launch in (1, 2):
        ya, yb, xa, xb = max(ya - 1, 0), min(yb + 1, Sh - 1), max(xa - 1, 0), min(xb + 1, Sh - 1)
        out.append((ya // rows, yb // rows, xa // cols, xb // cols))
        (ya, yb), (xa, xb) = snap(ya, yb), snap(xa, xb)
    return out
