"""numpy restatement of the need lists per strip (csrc/need.hip, st3d_need_blocks_build with tile_cols = 16), on top of the
per-block model of tests/_needblocks_ref.py.  The F(4x4,3x3) kernel's strip geometry gives each of the four tile rows of a
workgroup step an origin of its own, so a list names strips of 1 x 4 blocks = 4 x 16 pixels, four entries to a step:

    strip    = (n * strips_y + sy) * strips_x + sx,  strips_y = R / 4, strips_x = R / 16
    list k   = the strips that hold a block of B_k, ascending within an image, every image padded with -1 to whole steps
    count k  = steps = sum over the images of ceil(strips / 4)

B_k and the need propagation are the per-block model's: they do not depend on the geometry."""
import numpy as np

import _needblocks_ref as NB
import _needref as NR

STRIP_ROWS, STRIP_COLS, STEP = 4, 16, 4


def strips_of(need):
    """need_k (n, R, R) bool -> (n, R/4, R/16) bool: the strips that hold a block of B_k = block4(need_k)"""
    return NR.tiles_any(NB.block4(need), STRIP_ROWS, STRIP_COLS)


def strip_list(need):
    """need_k -> (entries int32, four per step, -1 = void; steps)"""
    s = strips_of(need)
    n = s.shape[0]
    per_img = s.shape[1] * s.shape[2]
    out = []
    for i in range(n):
        ids = np.flatnonzero(s[i].reshape(-1)) + i * per_img
        out.append(ids)
        out.append(np.full((-len(ids)) % STEP, -1))
    e = np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
    assert len(e) % STEP == 0
    return e, len(e) // STEP


def need_strips_model(mask, nlists=None):
    """mask (n, S, S) -> dict: need[k] (n, R_k, R_k) bool = need_k, lists[k] = the entries, steps[k] = the counts"""
    m = NB.need_blocks_model(mask, nlists=nlists)
    out = {"need": m["need"], "seg": m["seg"], "lists": [], "steps": []}
    for need in m["need"]:
        e, c = strip_list(need)
        out["lists"].append(e)
        out["steps"].append(c)
    return out


def strip_pixels(entries, n, H, W):
    """(n, H, W) bool: the pixels of the listed strips (voids skipped)"""
    t = np.zeros(n * (H // STRIP_ROWS) * (W // STRIP_COLS), bool)
    e = np.asarray(entries, np.int64)
    t[e[e >= 0]] = True
    return NR.expand(t.reshape(n, H // STRIP_ROWS, W // STRIP_COLS), STRIP_ROWS, STRIP_COLS)


def masks(n, S):
    """name -> (n, S, S) uint8, n >= 3: empty, full, one pixel in each corner, a blob, one empty image between covered ones,
    and masks whose strip counts of list 0 are 1, 2 and 3 (mod 4) per image"""
    assert n >= 3 and S >= 64
    z = lambda: np.zeros((n, S, S), np.uint8)
    out = {"empty": z(), "full": np.ones((n, S, S), np.uint8)}
    c = z()
    c[:, 0, 0] = c[:, 0, -1] = c[:, -1, 0] = c[:, -1, -1] = 1
    out["corners"] = c
    b = z()
    b[0, 9:47, 21:70] = 1
    b[1, 60:S - 3, 5:40] = 7
    b[2, 30:33, S - 20:S] = 255
    out["blob"] = b
    g = z()
    g[0, 17:50, 40:90] = 1
    g[2, 70:100, 3:30] = 1
    out["empty_image_between"] = g
    # list 0: need_0 = the 3x3 window of the pixel.  (y, x) = (5, 5): one block, one strip; (5, 15): the window crosses into
    # the next strip of the row, two; both pixels: three
    for name, pix in (("mod1", [(5, 5)]), ("mod2", [(41, 15)]), ("mod3", [(5, 5), (41, 15)])):
        m = z()
        for y, x in pix:
            m[:, y, x] = 1
        out[name] = m
    return out
