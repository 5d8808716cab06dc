"""The contract of st3d_fill_pushpull (include/st3d.h) restated in numpy, in fp64 by default: the pull-push fill of a texture
map.  dtype=np.float32 runs the same operations in the same order in fp32.

    out, count, detail = push_pull(tex, valid, domain=None)

Level 0: w = valid ? 1 : 0, c = valid ? tex : 0 (a select).  Pull: level l + 1 has sides ceil(h/2), ceil(w/2); a coarse texel
sums the children that exist in the order (0,0), (0,1), (1,0), (1,1): W = sum w, C = sum w c, c' = C / W where W > 0 else 0, w'
= min(W, 1); down to 1 x 1.  Push, coarsest to finest: w >= 1 keeps c, any other takes w c + (1 - w) up, up = the 2x bilinear
upsample of the completed coarser level (taps i/2 - 1 (1/4), i/2 (3/4) for even i; (i-1)/2 (3/4), (i+1)/2 (1/4) for odd i;
clamped; the four products summed in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1)).  out = tex where valid, outside the domain
or when nothing is valid; the pushed level-0 colour elsewhere; count = the texels that took it."""
import numpy as np


def level_sides(H, W):
    """[(H, W), (ceil(H/2), ceil(W/2)), ..., (1, 1)]"""
    sides = [(int(H), int(W))]
    while sides[-1] != (1, 1):
        h, w = sides[-1]
        sides.append(((h + 1) // 2, (w + 1) // 2))
    return sides


def workspace_bytes(H, W):
    """one (rgb, w) float4 per texel of every level above the map, at least one; 0 outside 1...16384"""
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        return 0
    return 16 * max(1, sum(h * w for h, w in level_sides(H, W)[1:]))


def pull(c, w):
    """one level down: c (h,w,3), w (h,w) -> c' (ceil(h/2), ceil(w/2), 3), w'.  A child that does not exist is left out of
    the sums (here: it enters as w = 0, c = 0, which adds nothing)."""
    h, wd = w.shape
    hp, wp = (h + 1) // 2 * 2, (wd + 1) // 2 * 2
    cp = np.zeros((hp, wp, 3), c.dtype)
    wq = np.zeros((hp, wp), w.dtype)
    cp[:h, :wd], wq[:h, :wd] = c, w
    W = np.zeros((hp // 2, wp // 2), w.dtype)
    C = np.zeros((hp // 2, wp // 2, 3), c.dtype)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        wk, ck = wq[dy::2, dx::2], cp[dy::2, dx::2]
        W = W + wk
        C = C + wk[..., None] * ck
    has = W > 0
    out = np.where(has[..., None], C / np.where(has, W, 1)[..., None], 0).astype(c.dtype)
    return out, np.minimum(W, 1).astype(w.dtype)


def axis_taps(n_fine, n_coarse, dtype):
    i = np.arange(n_fine)
    odd = (i % 2) == 1
    i0 = np.where(odd, (i - 1) // 2, i // 2 - 1)
    i1 = np.where(odd, (i + 1) // 2, i // 2)
    a0 = np.where(odd, 0.75, 0.25).astype(dtype)
    a1 = np.where(odd, 0.25, 0.75).astype(dtype)
    return np.clip(i0, 0, n_coarse - 1), np.clip(i1, 0, n_coarse - 1), a0, a1


def push(c, w, coarse):
    """complete level (c, w) from the completed coarser colours `coarse` (hc,wc,3) -> colours (h,w,3)"""
    h, wd = w.shape
    hc, wc = coarse.shape[:2]
    y0, y1, b0, b1 = axis_taps(h, hc, c.dtype)
    x0, x1, a0, a1 = axis_taps(wd, wc, c.dtype)
    up = np.zeros_like(c)
    for ys, bs in ((y0, b0), (y1, b1)):
        for xs, as_ in ((x0, a0), (x1, a1)):
            up = up + (bs[:, None] * as_[None, :])[..., None] * coarse[ys][:, xs]
    one = np.ones((), c.dtype)
    mixed = w[..., None] * c + (one - w)[..., None] * up
    return np.where((w >= 1)[..., None], c, mixed)


def push_pull(tex, valid, domain=None, dtype=np.float64):
    """tex (H,W,3) float32, valid (H,W) (non-zero = valid), domain (H,W) or None -> (out (H,W,3) float32 with the pushed
    colours rounded to fp32, count, detail: 'take' (H,W) bool, 'filled' (H,W,3) in `dtype` -- the pushed level-0 colours --
    and 'weights': the w of every level)"""
    tex = np.asarray(tex)
    H, W = tex.shape[:2]
    ok = np.asarray(valid).reshape(H, W) != 0
    dom = np.ones((H, W), bool) if domain is None else np.asarray(domain).reshape(H, W) != 0
    c0 = np.where(ok[..., None], tex, 0).astype(dtype)
    w0 = ok.astype(dtype)
    cs, ws = [c0], [w0]
    while ws[-1].shape != (1, 1):
        c, w = pull(cs[-1], ws[-1])
        cs.append(c)
        ws.append(w)
    done = cs[-1]
    for l in range(len(cs) - 2, -1, -1):
        done = push(cs[l], ws[l], done)
    take = ~ok & dom & bool(ws[-1][0, 0] > 0)
    out = np.array(tex, np.float32, copy=True)
    out[take] = done[take].astype(np.float32)
    return out, int(take.sum()), {"take": take, "filled": done, "weights": ws}
