"""References for the style regions (csrc/regions.hip, st3d/regions.py, style_transfer.region_style_loss).

  * `one_hot`, `planes_ref`: region r's level-0 plane is 1 where pix_to_face >= 0 and labels[pix_to_face] == r; everything
    behind it is tests/_guidedref.py's `planes_ref` on that one-hot mask (imported, not edited), region by region.
  * `weights64`: _guidedref.weights64 per region.
  * `region_tail_ref`: the fp64 loss -- the sum over regions, in ascending r, of _guidedref's guided tail (its
    guided_gram_ref / guided_bwd_ref and _gramref's sqdiff_ref, style_norm and loss_triple), with the zero-Sigma rule: a
    (view, region, tap) whose Sigma_l is 0 has D = 0, so it adds nothing to the value and nothing to the gradient (the
    guided tail alone would add the constant |A|^2 there).
  * `fold32`: the value as the device folds it -- fp32 additions of the fp32-rounded terms in a fixed order."""
import numpy as np
import torch

import _gramref as G
import _guidedref as GR
from _convref import _d

f32 = np.float32


def one_hot(p2f, labels, R):
    """p2f (n,S,S) int, labels (F,) int -> (R, n, S, S) fp32 0/1"""
    p2f, labels = np.asarray(p2f), np.asarray(labels)
    lab = np.where(p2f >= 0, labels[np.clip(p2f, 0, len(labels) - 1)], -1)
    return np.stack([(lab == r).astype(f32) for r in range(R)])


def planes_ref(p2f, labels, R):
    """-> (q[r][l] (n,H_l,H_l) fp32, sums (R,5,n) fp32)"""
    qs, sums = [], []
    for m in one_hot(p2f, labels, R):
        q, s = GR.planes_ref(m)
        qs.append(q)
        sums.append(s)
    return qs, np.stack(sums)


def weights64(p2f, labels, R):
    """-> w[r][l] torch fp64 (n,H_l,H_l): _guidedref.weights64 of every one-hot mask"""
    return [GR.weights64(m) for m in one_hot(p2f, labels, R)]


def visible(w):
    """w[r][l] -> bool (R,5,n): Sigma_l > 0 (the weights of an image without the region at that level are all 0)"""
    return torch.stack([torch.stack([(x.flatten(1).sum(1) > 0) for x in wr]) for wr in w])


def region_tail_ref(acts, w, content_act, style_grams, content_target, style_weight, content_weight, batch_denom=None,
                    lambdas=None, want_grads=True, view_weights=None):
    """acts: the five tap activations (n,C,H,H); w[r][l] of `weights64`; style_grams[r][l] (1 | C,C ...) region r's target;
    view_weights (R,n) or None: a further 0/1 factor per (region, view), the switch the zero-rule test uses in place of
    invisibility.  -> dict(loss [total, content, style], terms (R,5) the scaled style terms, D[r][l], MG[r][l], grads[l]
    (summed over r in ascending r), M[l] the sum of the absolute terms of grads[l], content_grad, coef (R,5), cc)"""
    n, R = acts[0].shape[0], len(w)
    bd = float(batch_denom or n)
    lambdas = [1.0] * R if lambdas is None else [float(x) for x in lambdas]
    seen = visible(w)
    terms = np.zeros((R, 5))
    coefs = np.zeros((R, 5))
    Ds, MGs, grads, Ms = [], [], [None] * 5, [None] * 5
    for r in range(R):
        Ds.append([]); MGs.append([])
        for l, A in enumerate(acts):
            C, H = A.shape[1], A.shape[2]
            g, m = GR.guided_gram_ref(A, w[r][l])
            keep = seen[r, l].double()
            if view_weights is not None:
                keep = keep * _d(view_weights)[r]
            T = _d(style_grams[r][l]).reshape(1, C, C) * keep[:, None, None]
            g = g * keep[:, None, None]                     # (exactly 0 already where Sigma is 0)
            s, d = G.sqdiff_ref(g, T)
            norm = G.style_norm(C, H, bd)
            terms[r, l] = lambdas[r] * norm * s
            coefs[r, l] = 4.0 * style_weight * lambdas[r] * norm
            Ds[r].append(d); MGs[r].append(m)
            if want_grads:
                out, M = GR.guided_bwd_ref(d, A, w[r][l], coefs[r, l])
                grads[l] = out if grads[l] is None else grads[l] + out
                Ms[l] = M if Ms[l] is None else Ms[l] + M
    csum, cd = G.sqdiff_ref(content_act, content_target)
    chw = content_act[0].numel()
    cc = 2.0 * content_weight / (bd * chw)
    content = csum / (bd * chw)
    style = float(terms.sum())
    return dict(loss=[content_weight * content + style_weight * style, content, style], terms=terms, D=Ds, MG=MGs, grads=grads,
                M=Ms, content_grad=cc * cd, coef=coefs, cc=cc, content_sum=csum, seen=seen)


def fold32(terms):
    """fp32 sum of the fp32-rounded `terms` in the order given, as st3d_sqdiff_sum_multi folds its items into a slot"""
    acc = f32(0.0)
    for t in terms:
        acc = f32(acc + f32(t))
    return acc
