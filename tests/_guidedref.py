"""References for the guided style loss (csrc/guide.hip, the weighted Gram kernels of csrc/gram.hip).

  * `planes_ref`: the guidance planes in fp32 numpy, in the operation order include/st3d.h fixes:
        H_0 = S, H_{l+1} = H_l // 2;  a_0 = mask;
        a_{l+1}[y][x] = 0.25f * ((a_l[2y][2x] + a_l[2y][2x+1]) + (a_l[2y+1][2x] + a_l[2y+1][2x+1]));
        Sigma_l = sum a_l;  r_l = (float)(H_l^2) / Sigma_l (0 when Sigma_l is not > 0);  w_l = a_l r_l;  q_l = sqrtf(w_l)
    numpy's fp32 +, *, / and sqrt are the correctly rounded IEEE operations, as the device's.  Sigma is the fp64 sum rounded
    to fp32: for a 0/1 mask every a_l is a multiple of 4^-l and every partial sum k 4^-l with k <= 2^24, so ANY summation
    order gives exactly this value and q must match bit for bit; for a fractional mask it is the correctly rounded sum, and
    an fp32 tree over n terms is within a few u of it (q, which carries half of Sigma's relative error, within 2 ulp).
  * `weights64`, `guided_gram_ref`, `guided_bwd_ref`, `guided_tail_ref`: the fp64 restatement of
        G^_l = sum_p w_l[p] F[:,p] F[:,p]^T,   loss = losses.py:34-39 with G^ in place of G,
        dL/dF = style_coef_l q o (D_l (q o F)),  D_l = G^_l - S_l
    built on tests/_gramref.py (imported, not edited): the Gram of q o F with q = sqrt(w) in fp64, so that a mask of ones
    runs _gramref's own operations on the same numbers and reproduces `tail_ref` exactly.

The two mutants of tests/test_guided_ref.py live here as switches (`one_operand`, `level0_r`): never set by a GPU test."""
import numpy as np
import torch

import _convref as R
import _gramref as G
from _convref import _d

LEVELS = 5
f32 = np.float32


def sides(S):
    return [S >> l for l in range(LEVELS)]


def pyramid_ref(mask):
    """mask (n, S, S) | (n, 1, S, S) -> [a_0 .. a_4] fp32 numpy, (n, H_l, H_l)"""
    a = np.ascontiguousarray(np.asarray(mask, dtype=f32))
    if a.ndim == 4:
        a = a[:, 0]
    out = [a]
    for _ in range(LEVELS - 1):
        H = a.shape[1] // 2
        c = a[:, :2 * H, :2 * H]                      # floor: a trailing odd row / column is dropped
        a = f32(0.25) * ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2]))
        out.append(np.ascontiguousarray(a.astype(f32)))
    return out


def planes_ref(mask):
    """-> (q, sums): q[l] (n, H_l, H_l) fp32, sums (5, n) fp32"""
    qs, sums = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in pyramid_ref(mask):
            n, H = a.shape[0], a.shape[1]
            sigma = a.reshape(n, -1).astype(np.float64).sum(1).astype(f32)
            r = np.where(sigma > 0, f32(float(H * H)) / np.where(sigma > 0, sigma, f32(1)), f32(0)).astype(f32)
            w = (a * r[:, None, None]).astype(f32)
            qs.append(np.sqrt(w).astype(f32))
            sums.append(sigma)
    return qs, np.stack(sums)


def weights64(mask, level0_r=False):
    """the weights the fp64 references use: w_l = a_l H_l^2 / Sigma_l in fp64 on the fp32 pyramid (exact for 0/1 masks),
    0 for an image without coverage at that level -> [w_0 .. w_4] torch fp64 (n, H_l, H_l).
    level0_r (mutant): r taken from level 0 for all levels"""
    out, r0 = [], None
    for a in pyramid_ref(mask):
        a = torch.from_numpy(a).double()
        H = a.shape[1]
        sigma = a.sum((1, 2))
        r = torch.where(sigma > 0, float(H * H) / torch.where(sigma > 0, sigma, torch.ones_like(sigma)), torch.zeros_like(sigma))
        if r0 is None:
            r0 = r
        out.append(a * (r0 if level0_r else r)[:, None, None])
    return out


def guided_gram_ref(F, w, one_operand=False):
    """F (B, C, H, W), w (B, H, W) fp64 -> (G^, M): the Gram of q o F, M the weighted absolute sum sum_p w |F| |F|^T.
    one_operand (mutant): the weight's square root applied to one operand only"""
    q = _d(w).sqrt().reshape(w.shape[0], 1, -1)
    f = _d(F).flatten(2)
    if one_operand:
        x = f * q
        Gm = torch.bmm(x, f.transpose(1, 2))
        return Gm, torch.bmm(x.abs(), f.abs().transpose(1, 2))
    return G.gram_ref((f * q))


def guided_bwd_ref(D, F, w, coef, base=None, gated=False):
    """out = base + coef q o (D (q o F)), zero where gated and F <= 0 -- the gate is the sign of F itself, whatever q is: what
    arrived from the layers above (base) passes under q = 0 wherever the ReLU was open -> (out, M)"""
    q = _d(w).sqrt().reshape(w.shape[0], 1, *F.shape[2:])
    out, M = G.gram_bwd_ref(D, _d(F) * q, coef)
    out, M = out * q, M * q
    if base is not None:
        out, M = out + _d(base), M + _d(base).abs()
    if gated:
        open_ = (_d(F) > 0).double()
        out, M = out * open_, M * open_
    return out, M


def guided_tail_ref(acts, weights, content_act, style_grams, content_target, style_weight, content_weight, batch_denom=None,
                    gated=(), want_grads=True, one_operand=False):
    """_gramref.tail_ref with G^ in place of G for the current images: same dict.  weights: [w_0 .. w_4] of `weights64`"""
    n = acts[0].shape[0]
    bd = float(batch_denom or n)
    Gs, MG, D, sums, shapes, coefs, grads = [], [], [], [], [], [], []
    for l, (A, S, w) in enumerate(zip(acts, style_grams, weights)):
        g, m = guided_gram_ref(A, w, one_operand)
        s, d = G.sqdiff_ref(g, S)
        C, H = A.shape[1], A.shape[2]
        coef = 4.0 * style_weight * G.style_norm(C, H, bd)
        Gs.append(g); MG.append(m); D.append(d); sums.append(s); shapes.append((C, H)); coefs.append(coef)
        if want_grads:
            grads.append(guided_bwd_ref(d, A, w, coef, gated=l in gated)[0])
    csum, cd = G.sqdiff_ref(content_act, content_target)
    chw = content_act[0].numel()
    cc = 2.0 * content_weight / (bd * chw)
    return dict(loss=list(G.loss_triple(csum, chw, sums, shapes, bd, style_weight, content_weight)), D=D, G=Gs, MG=MG,
                grads=grads, content_grad=cc * cd, coef=coefs, cc=cc, style_sums=sums, content_sum=csum, shapes=shapes)


# ------------------------------------------------------------------------------------------------ bound
# A product of the weighted Gram carries, besides what _gramref's kappa counts for the unweighted chain:
#   q = sqrtf(fl(a fl(H^2 / Sigma))): a division, a multiplication and a square root.  The first two put (1 + d)^2 under
#       the root, which halves them: 1 u; the root's own rounding: 0.5 u.  Together <= 1.5 u per q (a_l and Sigma_l are exact
#       for a 0/1 mask).
#   each operand's fl(q F): 1 u.
# Two operands per product: 2 (1.5 + 1) = 5 u, so kappa_w = kappa + 5.  (Confirmed on the CPU emulation -- gram_fwd_emul on
# fl(q F) -- by tests/test_guided_ref.py, never from the kernels.)
KAPPA_EXTRA = 5.0


def kappa_w_fwd(B, C, HW, scale=1, white=False):
    return G.kappa_fwd(B, C, HW, scale, white) + KAPPA_EXTRA


def kappa_w_bwd(C):
    """the backward's product coef D (q F) q carries one q F (1 + 1.5 u) and the epilogue's q (1.5 u) and its product (1 u)"""
    return G.kappa_bwd(C) + KAPPA_EXTRA


# ------------------------------------------------------------------------------------------------ masks
def disc_mask(n, S, frac=0.5):
    """0/1 discs of different radii and centres: (n, 1, S, S) fp32 torch"""
    y, x = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = []
    for b in range(n):
        cy, cx, r = S * (0.45 + 0.1 * b), S * (0.55 - 0.07 * b), S * frac * (0.6 + 0.2 * b)
        out.append((((y - cy) ** 2 + (x - cx) ** 2) <= r * r).float())
    return torch.stack(out)[:, None]


# ------------------------------------------------------------------------------------------------ the image gradient
POOLS_BEHIND = {5: 2, 10: 7, 19: 16, 28: 25}         # conv module whose input is a pool's output -> the conv that feeds the pool


SIGMAS = 8.0


def image_grad_ref(acts, weights, tap_grads, tap_errs=None, algos=None):
    """The VGG backward in fp64 on GIVEN activations: acts {conv module: post-ReLU output (n, C, H, W)} for every conv up to
    the deepest tap, weights {conv module: (Cout, Cin, 3, 3)}, tap_grads {module: d loss / d (that post-ReLU output)}
    (ungated: the gate, the sign of the activation, is applied here, as every input-gradient launch does).  Pools are
    undone through the argmax of the given activations (first maximum, as the kernels and ATen).
    -> (d loss / d image, E, Es).  With tap_errs {module: per-element bound e of the error the tap gradient arrives with}
    two per-element bounds of an fp32 evaluation of the same chain come out, both first order, both built from the local
    bounds alone: e at the taps, one u of |g| for every addition of a tap, and at every conv kappa u M with
    M = conv^T(|g|, |W|) max-pooled over the output tile of the layer's kernel (tests/_convref.py; algos {module: 'direct' |
    'f2' | 'f4'}, default the loosest, F(4x4,3x3)).
      E   worst case: the local bounds pushed through |W|^T, the gates and the unpools.  Nothing an fp32 evaluation in this
          order does can exceed it -- and after thirteen layers of |W|^T, which has none of W^T's cancellation (a factor of
          about sqrt(9 C) per layer), it admits far more than any such evaluation does.  Kept as the backstop.
      Es  SIGMAS standard deviations of the probabilistic model of rounding-error analysis (Higham & Mary 2019): the local
          errors are independent, of mean zero, and each local BOUND is taken for the standard deviation (so every local
          term is over-stated); variances then travel through the squares of the same operators, Var_in = conv^T(Var_out,
          W^2), gates and unpools as for the values.  The model ignores the correlation between neighbouring outputs that
          share inputs; with weights of both signs these correlations have both signs.  SIGMAS = 8: for 10^5 elements the
          chance that a Gaussian leaves 8 sigma is 10^-10.  This is the bound that can see an error of one term."""
    g = E = V = None
    pooled_from = None
    for m in sorted(acts, reverse=True):
        a = _d(acts[m])
        if g is not None and pooled_from == m:
            _, idx = R.pool_argmax(a)
            g, E, V = (R.unpool(x, idx, a.shape[2], a.shape[3]) for x in (g, E, V))
        if m in tap_grads:
            t = _d(tap_grads[m])
            te = _d(tap_errs[m]) if tap_errs is not None else torch.zeros_like(t)
            if g is None:
                g, E, V = t, te, te * te
            else:
                add = G.U32 * (g + t).abs()
                g, E, V = g + t, E + te + add, V + te * te + add * add
        if g is None:
            continue
        gate = (a > 0).double()
        g, E, V = g * gate, E * gate, V * gate
        W = _d(weights[m])
        algo = (algos or {}).get(m, "f4")
        local = R.KAPPA[algo] * G.U32 * R.mag(R.mag_dgrad(g, W), algo)
        E = torch.nn.functional.conv_transpose2d(E, W.abs(), padding=1) + local
        V = torch.nn.functional.conv_transpose2d(V, W * W, padding=1) + local * local
        g = R.conv_dgrad(g, W)
        pooled_from = POOLS_BEHIND.get(m)
    return g, E, SIGMAS * V.sqrt()
