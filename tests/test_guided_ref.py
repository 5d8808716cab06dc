"""Checks of the guided style loss's references (CPU; tests/_guidedref.py):

  * the fp64 tail with G^ equals torch autograd of the written-out loss (<= 1e-12 relative);
  * a mask of ones reproduces _gramref.tail_ref exactly, and the fp32 planes are then all ones;
  * scaling the covered area leaves G^ of a spatially constant F unchanged (the normalisation's point);
  * an empty mask gives zero gradient and the constant loss ||S||^2 norm;
  * S = 24 (sides 24, 12, 6, 3, 1) with coverage only in the last row / column of the 3 x 3 level: level 4 has Sigma = 0
    while levels 0-3 do not -- the floor rule and the r = 0 branch;
  * two mutants are caught: the weight on one operand only, and r taken from level 0 for all levels;
  * the bound kappa_w = kappa + 5 holds for the fp32 CPU emulation of the kernels' order on weighted inputs."""
import numpy as np
import pytest
import torch

import _convref as R
import _gramref as G
import _guidedref as GR


@pytest.fixture(scope="module")
def taps():
    return G.tap_activations(G.style_images(64)[[0, 5, 2]])


def _written_out(leaves, weights, sg, cl, ctgt, sw, cw):
    content = torch.nn.functional.mse_loss(cl, ctgt)
    style = 0
    for f, s, w in zip(leaves, sg, weights):
        b, c, h, ww = f.shape
        x = f.reshape(b, c, h * ww)
        g = torch.bmm(x * w.reshape(b, 1, h * ww), x.transpose(1, 2))          # sum_p w[p] F[:,p] F[:,p]^T
        style = style + torch.nn.functional.mse_loss(g, s.expand_as(g)) / (c ** 2 * h ** 2)
    return cw * content + sw * style, content, style


def test_guided_tail_matches_fp64_autograd(taps):
    gen = torch.Generator().manual_seed(0)
    acts = [taps[m][:2].double() for m in G.STYLE_TAPS]
    cact = taps[G.CONTENT_TAP][:2].double()
    ctgt = G.near(cact, 0.1, gen)
    sw, cw = 1e6, 1.0
    weights = GR.weights64(GR.disc_mask(2, 64))
    sg = [G.gram_ref(taps[m][2:3])[0] for m in G.STYLE_TAPS]
    leaves = [a.clone().requires_grad_(True) for a in acts]
    cl = cact.clone().requires_grad_(True)
    total, content, style = _written_out(leaves, weights, sg, cl, ctgt, sw, cw)
    total.backward()
    t = GR.guided_tail_ref(acts, weights, cact, sg, ctgt, sw, cw)
    for got, want in zip(t["loss"], (total, content, style)):
        assert abs(got - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    for got, leaf in zip(t["grads"], leaves):
        assert torch.allclose(got, leaf.grad, rtol=0, atol=1e-12 * float(leaf.grad.abs().max()))
    assert torch.allclose(t["content_grad"], cl.grad, rtol=0, atol=1e-12 * float(cl.grad.abs().max()))
    # mutants: the weight on one operand only (a Gram of sqrt(w) F with F), r of level 0 at every level
    bad = GR.guided_tail_ref(acts, weights, cact, sg, ctgt, sw, cw, one_operand=True)
    assert abs(bad["loss"][2] - float(style.detach())) > 1e-3 * abs(float(style.detach()))


def test_r_of_level_0_for_all_levels_is_caught():
    """second mutant.  Where every side is even the 2x2 averages keep the mean and r_l = r_0 at every level: the mutant is
    invisible at S = 64 (asserted: a test at such a size alone would not see it).  At S = 24 the 1 x 1 level drops the
    third row and column of the 3 x 3 level, r_4 != r_0, and the mutant fails the comparison the autograd check makes."""
    same = GR.weights64(GR.disc_mask(2, 64), level0_r=True)
    assert all(torch.equal(x, y) for x, y in zip(same, GR.weights64(GR.disc_mask(2, 64))))
    mask = GR.disc_mask(2, 24)
    imgs = R.style_crops(24, 24, R.STYLES[:3])
    t24 = G.tap_activations(imgs)
    acts = [t24[m][:2].double() for m in G.STYLE_TAPS]
    cact = t24[G.CONTENT_TAP][:2].double()
    sg = [G.gram_ref(t24[m][2:3])[0] for m in G.STYLE_TAPS]
    good = GR.guided_tail_ref(acts, GR.weights64(mask), cact, sg, cact, 1e6, 1.0)
    leaves = [a.clone().requires_grad_(True) for a in acts]
    total, _, style = _written_out(leaves, GR.weights64(mask), sg, cact, cact, 1e6, 1.0)
    assert abs(good["loss"][2] - float(style.detach())) <= 1e-12 * float(style.detach())
    bad = GR.guided_tail_ref(acts, GR.weights64(mask, level0_r=True), cact, sg, cact, 1e6, 1.0)
    assert not abs(bad["loss"][2] - float(style.detach())) <= 1e-12 * float(style.detach())
    for l in range(4):
        assert torch.equal(bad["G"][l], good["G"][l])
    assert float((bad["G"][4] - good["G"][4]).abs().max()) > 1e-3 * float(good["G"][4].abs().max())


def test_mask_of_ones_is_the_unguided_tail(taps):
    gen = torch.Generator().manual_seed(1)
    acts = [taps[m][:2].double() for m in G.STYLE_TAPS]
    cact = taps[G.CONTENT_TAP][:2].double()
    ctgt = G.near(cact, 0.1, gen)
    sg = [G.gram_ref(taps[m][2:3])[0] for m in G.STYLE_TAPS]
    ones = torch.ones(2, 1, 64, 64)
    q, sums = GR.planes_ref(ones.numpy())
    for l, H in enumerate(GR.sides(64)):
        assert q[l].shape == (2, H, H) and (q[l] == 1).all() and (sums[l] == H * H).all()
    a = GR.guided_tail_ref(acts, GR.weights64(ones), cact, sg, ctgt, 1e6, 1.0, gated=(1, 2, 3, 4))
    b = G.tail_ref(acts, cact, sg, ctgt, 1e6, 1.0, gated=(1, 2, 3, 4))
    assert a["loss"] == b["loss"]
    for k in ("G", "D", "grads"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k


def test_constant_features_do_not_see_the_covered_area():
    """F constant over the pixels: G^ = (sum_p w) f f^T = H^2 f f^T whatever the mask covers"""
    f = torch.rand(1, 8, 1, 1, generator=torch.Generator().manual_seed(2)).double()
    got = []
    for frac in (0.2, 0.4, 0.8):
        w = GR.weights64(GR.disc_mask(1, 64, frac))
        assert abs(float(w[0].sum()) - 64 * 64) < 1e-9 * 64 * 64
        got.append([GR.guided_gram_ref(f.expand(1, 8, H, H), w[l])[0] for l, H in enumerate(GR.sides(64))])
    for other in got[1:]:
        for x, y, H in zip(got[0], other, GR.sides(64)):
            assert torch.allclose(x, y, rtol=1e-12, atol=0)
            assert torch.allclose(x[0], H * H * (f[0, :, 0, 0, None] * f[0, None, :, 0, 0]), rtol=1e-12, atol=0)


def test_empty_mask_gives_the_constant_loss_and_no_gradient(taps):
    acts = [taps[m][:1].double() for m in G.STYLE_TAPS]
    cact = taps[G.CONTENT_TAP][:1].double()
    sg = [G.gram_ref(taps[m][2:3])[0] for m in G.STYLE_TAPS]
    q, sums = GR.planes_ref(np.zeros((1, 1, 64, 64), np.float32))
    assert all((x == 0).all() for x in q) and (sums == 0).all()
    t = GR.guided_tail_ref(acts, GR.weights64(torch.zeros(1, 1, 64, 64)), cact, sg, cact, 1e6, 1.0)
    assert all(float(g.abs().max()) == 0 for g in t["grads"]) and all(float(g.abs().max()) == 0 for g in t["G"])
    want = sum(float((s * s).sum()) * G.style_norm(a.shape[1], a.shape[2], 1.0) for s, a in zip(sg, acts))
    assert t["loss"][1] == 0 and abs(t["loss"][2] - want) <= 1e-14 * want


def test_floor_rule_and_the_empty_level_at_24():
    """sides 24, 12, 6, 3, 1: the 1 x 1 level averages rows / columns 0..1 of the 3 x 3 level; coverage confined to its last
    row and column (mask rows / columns 16..23) leaves level 4 empty while levels 0..3 are not"""
    assert GR.sides(24) == [24, 12, 6, 3, 1]
    m = np.zeros((2, 1, 24, 24), np.float32)
    m[0, 0, 16:, :] = 1
    m[1, 0, 3:20, 17:23] = 1
    q, sums = GR.planes_ref(m)
    assert [x.shape[1] for x in q] == [24, 12, 6, 3, 1]
    assert (sums[:4] > 0).all() and (sums[4] == 0).all() and (q[4] == 0).all()
    assert (q[3][0, :2] == 0).all() and (q[3][0, 2] > 0).all() and (q[3][1, :, :2] == 0).all()
    for l, H in enumerate(GR.sides(24)[:4]):           # w has mean 1: sum q^2 = H^2 up to the roundings of q
        assert np.allclose((q[l].astype(np.float64) ** 2).reshape(2, -1).sum(1), H * H, rtol=1e-6)
    # a mask that reaches into rows 0..15 does populate level 4
    m[0, 0, 15, 3] = 1
    assert GR.planes_ref(m)[1][4, 0] > 0
    w = GR.weights64(m)
    assert float(w[4][1].abs().max()) == 0 and float(w[4][0].sum()) == 1.0


@pytest.mark.parametrize("S", [64, 128])
def test_emulation_meets_the_weighted_bound(S):
    """kappa_w = kappa + 5 on the fp32 emulation of the kernels' summation order fed with fl(q F): the seeded VGG's taps of
    two style images composited on white under a disc's coverage (the shapes and the family of the GPU test; the white
    surround has weight 0, so kappa is the general one, not the worst case of the white family); prints the worst
    err / (kappa_w u M)"""
    mask = GR.disc_mask(2, S)
    imgs = R.style_crops(S, S, R.STYLES[:2])
    imgs = imgs * mask + (1 - mask)
    taps_ = G.tap_activations(imgs)
    q, _ = GR.planes_ref(mask.numpy())
    w = GR.weights64(mask)
    worst = 0.0
    for l, m in enumerate(G.STYLE_TAPS):
        F = taps_[m]
        B, C, H = F.shape[0], F.shape[1], F.shape[2]
        ref, M = GR.guided_gram_ref(F, w[l])
        for b in range(B):
            qf = F[b].flatten(1) * torch.from_numpy(q[l][b]).reshape(1, -1)          # fp32 product: one rounding
            got = G.gram_fwd_emul(qf, B=B)
            kap = GR.kappa_w_fwd(B, C, H * H)
            ratio = float(((got.double() - ref[b]).abs() / (kap * G.U32 * M[b]).clamp_min(1e-300))[M[b] > 0].max())
            assert bool((got[M[b] == 0] == 0).all())
            worst = max(worst, ratio)
    print(f"\n  weighted Gram emulation at {S}^2: worst err / (kappa_w u M) = {worst:.3f}")
    assert worst <= 1.0


def test_image_grad_ref_is_the_fp64_autograd_of_the_vgg():
    """_guidedref.image_grad_ref (the hand-written fp64 VGG backward the GPU test compares the plan's image gradient with)
    against torch autograd through the seeded fp64 VGG, for gradients arriving at the six taps; S = 24 has odd sides"""
    from oracle import perceptual_ref as P
    model = P.make_vgg19_features(seed=0).double()
    weights = {m: model._modules[str(m)].weight.detach() for m in R.VGG_CONVS}
    gen = torch.Generator().manual_seed(7)
    for S in (24, 32):
        x = R.style_crops(S, S, R.STYLES[:2]).double().requires_grad_(True)
        acts, h = {}, x
        for name, layer in model._modules.items():
            if int(name) > 29:
                break
            h = layer(h) if not isinstance(layer, torch.nn.ReLU) else torch.relu(h)
            if int(name) - 1 in R.VGG_CONVS:          # the ReLU behind a conv: the post-ReLU tap
                acts[int(name) - 1] = h
        taps = {m: torch.randn(acts[m].shape, generator=gen, dtype=torch.float64) for m in G.STYLE_TAPS + (G.CONTENT_TAP,)}
        sum((acts[m] * t).sum() for m, t in taps.items()).backward()
        A = {m: a.detach() for m, a in acts.items()}
        got, E, Es = GR.image_grad_ref(A, weights, taps, {m: torch.zeros_like(t) for m, t in taps.items()},
                                       algos={m: "direct" for m in A})
        assert torch.allclose(got, x.grad, rtol=0, atol=1e-12 * float(x.grad.abs().max())), S
        assert bool((E > 0).any()) and bool((Es <= E * (1 + 1e-12)).all())
        # torch's own fp32 evaluation of the same chain (direct convolutions) sits inside both bounds; a wrong gate bit at
        # one relu1_1 element leaves the probabilistic one
        x32 = x.detach().float().requires_grad_(True)
        m32 = P.make_vgg19_features(seed=0)
        h, loss = x32, 0
        for name, layer in m32._modules.items():
            if int(name) > 29:
                break
            h = layer(h) if not isinstance(layer, torch.nn.ReLU) else torch.relu(h)
            if int(name) - 1 in taps:
                loss = loss + (h * taps[int(name) - 1].float()).sum()
        loss.backward()
        err = (x32.grad.double() - got).abs()
        # (fp32 activations differ from the fp64 ones in the last bits: compare where no gate sits on the edge -- the bound is
        # for a chain on GIVEN activations, so only the figure is printed)
        print(f"\n  S={S}: torch fp32 chain, worst err / probabilistic bound {float((err / Es.clamp_min(1e-300)).max()):.3f}, "
              f"/ worst-case bound {float((err / E.clamp_min(1e-300)).max()):.2e}")
        flip = A[0].clone()
        on = torch.nonzero(flip[0, 3] > 0)[0]
        flip[0, 3, on[0], on[1]] = 0.0                           # one gate of relu1_1 closed that was open
        bad = GR.image_grad_ref({**A, 0: flip}, weights, taps)[0]
        assert bool(((bad - got).abs() > Es).any()), "the probabilistic bound cannot see one wrong gate bit"
