"""The guided style loss on the GPU: the guidance planes (csrc/guide.hip), the weighted Gram forward / backward
(csrc/gram.hip), the weighted bottom pass (csrc/tap0.hip), the plan and the public doors, against tests/_guidedref.py.

  planes        0/1 masks (the cow's coverage, a disc, one pixel, empty, full): q and Sigma bitwise the numpy restatement;
                a fractional mask: q within 2 ulp, two runs bitwise equal
  exact         integer F in {0..3} and q in {0, 2}: every product and partial sum is an integer below 2^24, so G^, D and the
                weighted backward (plain, gated, accumulating) must EQUAL the integer reference; single == multi launches;
                the fused bottom pass (D only, gy only, both) x (plain, need-listed) against the unfused weighted route
  independence  F replaced by other finite values wherever q = 0: G^ unchanged, gfeat unchanged where q > 0, == 0 elsewhere
                (and, accumulating, what arrived from above passes there wherever the ReLU was open)
  real          the seeded VGG's taps of two style images at 64^2 and 128^2, composited on white under the cow's coverage:
                per element |got - ref| <= kappa_w u M, kappa_w = kappa + 5 (derived in _guidedref, confirmed on the CPU
                emulation by tests/test_guided_ref.py, never from these kernels); G^ == G^T bitwise
  plan          B = 2 at S = 16, 24, 64: loss triple and, element by element, the image gradient against the fp64 tail and the
                fp64 VGG backward on the plan's own activations, within derived bounds; bitwise: mask of ones == unguided, cleared ==
                never set, run to run, graph replay on == off, need mask and flat colour; NaN poisons; plan bytes
  api           guided_gram_matrix's autograd against fp64, compute_perceptual_loss(style_masks=...) on a render,
                second_approach.py / first_approach.py --style_mask object as child processes

`pytest -s` prints the worst err / (kappa_w u M) per shape."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _convref as R
import _gramref as G
import _guidedref as GR
import _scenes as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


_COW = {}


def cow_coverage(dev, S, n=2):
    """the 0/1 coverage of n renders of the cow at S x S: (n, 1, S, S) fp32 on the device"""
    if (S, n) not in _COW:
        import utils as U
        U.device = dev
        a = SC.load_asset("cow")
        Rm, T = SC.random_cameras(n, seed=3)
        mesh, renderer, cams = SC.device_scene(U, dev, a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"],
                                               SC.texture_at(a, 64), Rm, T, S)
        with torch.no_grad():
            _, masks = U.render_meshes(renderer, mesh, cams)
        m = masks.detach().float().contiguous()
        assert m.shape == (n, 1, S, S) and bool(((m == 0) | (m == 1)).all()) and 0 < float(m.sum()) < m.numel()
        _COW[(S, n)] = m
    return _COW[(S, n)]


# ================================================================================================ planes
@pytest.mark.parametrize("S", [16, 24, 64])
def test_planes_of_01_masks_are_bitwise_the_restatement(dev, ops, S):
    one = torch.zeros(2, 1, S, S)
    one[0, 0, S - 1, S - 3] = 1                       # one pixel (in the dropped row / column region of the odd levels at S = 24)
    one[1, 0, 5, 2] = 1
    last = torch.zeros(2, 1, S, S)                    # coverage in the last third only: at S = 24 level 4 is empty, levels 0-3 not
    last[0, 0, 2 * S // 3:, :] = 1
    last[1, 0, 3:S - 4, 2 * S // 3 + 1:S - 1] = 1
    masks = {"cow": cow_coverage(dev, S).cpu(), "disc": GR.disc_mask(2, S), "one pixel": one, "last third": last,
             "empty": torch.zeros(2, 1, S, S), "full": torch.ones(2, 1, S, S)}
    for name, m in masks.items():
        planes, sums = ops.guidance_build(m.to(dev))
        q, sg = GR.planes_ref(m.numpy())
        assert [tuple(p.shape) for p in planes] == [(2, H, H) for H in GR.sides(S)]
        assert np.array_equal(sums.cpu().numpy(), sg), (name, sums.cpu().numpy(), sg)
        for l, p in enumerate(planes):
            assert np.array_equal(p.cpu().numpy().view(np.int32), q[l].view(np.int32)), (name, S, l)
    if S == 24:
        assert (GR.planes_ref(last.numpy())[1][4] == 0).all() and (GR.planes_ref(last.numpy())[1][:4] > 0).all()
    # (n, S, S) is taken as well
    assert torch.equal(ops.guidance_build(masks["disc"][:, 0].to(dev))[0][2], ops.guidance_build(masks["disc"].to(dev))[0][2])


@pytest.mark.parametrize("S", [16, 24, 64])
def test_planes_of_a_fractional_mask(dev, ops, S):
    m = torch.rand(2, 1, S, S, generator=torch.Generator().manual_seed(S)) * GR.disc_mask(2, S)
    a, sa = ops.guidance_build(m.to(dev))
    b, sb = ops.guidance_build(m.to(dev))
    assert torch.equal(sa, sb) and all(torch.equal(x, y) for x, y in zip(a, b))
    q, sg = GR.planes_ref(m.numpy())
    for l, p in enumerate(a):
        got, ref = p.cpu().numpy(), q[l]
        ulp = np.spacing(np.abs(ref).astype(np.float32))
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2 * ulp), (S, l)
        assert np.array_equal(got == 0, ref == 0)


# ================================================================================================ exact operands
EXACT_SHAPES = [(2, 64, 64 * 64), (2, 128, 32 * 32), (1, 256, 16 * 16), (1, 512, 8 * 8), (1, 512, 4 * 4), (2, 64, 9), (1, 512, 1)]


def _int_feat(shape, gen, top=3):
    f = torch.randint(0, top + 1, shape, generator=gen)
    return (f * torch.randint(0, 2, shape, generator=gen)).float()


def _q02(B, HW, gen):
    """q in {0, 2}: a 0/1 plane with Sigma = HW / 4 (r = 4) where HW is a multiple of 4, any 0/1 pattern otherwise"""
    q = torch.zeros(B, HW)
    for b in range(B):
        k = HW // 4 if HW % 4 == 0 else (HW + 1) // 2
        q[b, torch.randperm(HW, generator=gen)[:k]] = 2.0
    return q


def test_exact_weighted_gram_forward_and_backward(dev, ops):
    gen = torch.Generator().manual_seed(21)
    feats, qs, wants = [], [], []
    for B, C, HW in EXACT_SHAPES:
        f, q = _int_feat((B, C, HW), gen), _q02(B, HW, gen)
        x = (f * q[:, None]).double()
        want = torch.bmm(x, x.transpose(1, 2))
        assert int(want.max()) < 1 << 24
        fd, qd = f.to(dev), q.to(dev)
        got = ops.gram_fwd(fd, q=qd)
        assert torch.equal(got.cpu().double(), want), ("gram_fwd weighted", B, C, HW)
        assert torch.equal(got, got.transpose(1, 2))
        feats.append(fd); qs.append(qd); wants.append(want)
        # D = G^ - S on the device
        S_ = torch.randint(0, 1 << 10, (1, C, C), generator=gen).float()
        _, D = ops.sqdiff_sum(got, S_.to(dev), 1.0, want_diff=True)
        assert torch.equal(D.cpu().double(), want - S_.double())
        # backward: coef q o (D (q o F)), integer D in [-8, 8], coef 2: |sum| <= 2 * 8 * 6 * 512 * 2 + 8 < 2^24
        Dm = torch.randint(-4, 5, (B, C, C), generator=gen)
        Ds = (Dm + Dm.transpose(1, 2)).float()
        base = torch.randint(-8, 9, (B, C, HW), generator=gen).float()
        for gated in ((False, True) if C % 32 == 0 else (False,)):
            Dd = (Ds if gated else Dm.float()).to(dev).contiguous()
            core = 2 * torch.bmm(Dd.cpu().double(), x) * q[:, None].double()
            open_ = (f > 0).double() if gated else 1.0             # the gate is the sign of F itself, whatever q is
            got = ops.gram_bwd(Dd, fd, 2.0, gated=gated, q=qd)
            assert torch.equal(got.cpu().double(), core * open_), ("gram_bwd weighted", gated, B, C, HW)
            got = ops.gram_bwd(Dd, fd, 2.0, out=base.to(dev), gated=gated, q=qd)
            assert torch.equal(got.cpu().double(), (core + base.double()) * open_), ("gram_bwd weighted accumulate", gated, B, C, HW)
    # all of them in one launch pair: the same bits
    multi = ops.gram_fwd_multi(feats, qs=qs)
    for g, want, shp in zip(multi, wants, EXACT_SHAPES):
        assert torch.equal(g.cpu().double(), want), ("gram_fwd_multi weighted", shp)


def test_weights_of_one_give_the_unweighted_bits(dev, ops):
    gen = torch.Generator().manual_seed(22)
    for B, C, HW in EXACT_SHAPES + [(2, 256, 24 * 24), (2, 128, 144)]:
        f = torch.rand(B, C, HW, generator=gen).to(dev)
        one = torch.ones(B, HW, device=dev)
        g = ops.gram_fwd(f)
        assert torch.equal(ops.gram_fwd(f, q=one), g), (B, C, HW)
        D = (g - g.mean()).contiguous()
        base = torch.randn(B, C, HW, generator=gen).to(dev)
        for gated in ((False, True) if C % 32 == 0 else (False,)):
            assert torch.equal(ops.gram_bwd(D, f, 0.37, gated=gated, q=one), ops.gram_bwd(D, f, 0.37, gated=gated)), (B, C, HW, gated)
            assert torch.equal(ops.gram_bwd(D, f, 0.37, out=base.clone(), gated=gated, q=one),
                               ops.gram_bwd(D, f, 0.37, out=base.clone(), gated=gated)), (B, C, HW, gated, "accumulate")
    feats = [torch.rand(2, C, HW, generator=gen).to(dev) for C, HW in ((64, 4096), (128, 1024), (256, 256), (512, 64), (512, 16))]
    ones = [torch.ones(2, f.shape[2], device=dev) for f in feats]
    for a, b in zip(ops.gram_fwd_multi(feats, qs=ones), ops.gram_fwd_multi(feats)):
        assert torch.equal(a, b)


# ================================================================================================ independence
def test_features_under_zero_weight_do_not_matter(dev, ops):
    gen = torch.Generator().manual_seed(23)
    for (B, C, H), S in (((2, 64, 64), 64), ((2, 128, 32), 64), ((2, 256, 6), 24), ((2, 512, 4), 64)):
        planes, _ = ops.guidance_build(cow_coverage(dev, S))
        q = next(p for p in planes if p.shape[1] == H)
        assert 0 < int((q == 0).sum()) < q.numel()
        f = torch.rand(B, C, H, H, generator=gen).to(dev)
        other = torch.where((q == 0)[:, None], (torch.rand(B, C, H, H, generator=gen) * 100 - 50).to(dev), f)
        assert not torch.equal(f, other)
        g = ops.gram_fwd(f, q=q)
        assert torch.equal(ops.gram_fwd(other, q=q), g), (B, C, H)
        assert torch.equal(ops.gram_fwd_multi([other], qs=[q])[0], g)
        D = (g - g.mean(dim=(1, 2), keepdim=True)).contiguous()
        D = (D + D.transpose(1, 2)).contiguous()
        for gated in (False, True):
            a = ops.gram_bwd(D, f, 1e-3, gated=gated, q=q)
            b = ops.gram_bwd(D, other, 1e-3, gated=gated, q=q)
            zero = (q == 0)[:, None].expand_as(a)
            assert torch.equal(a[~zero], b[~zero]) and bool((a[zero] == 0).all()) and bool((b[zero] == 0).all()), (B, C, H, gated)
            # accumulating: what arrived from above passes under q = 0 wherever the ReLU was open (the gate is F's sign)
            base = torch.randn(a.shape, generator=gen).to(dev)
            c = ops.gram_bwd(D, f, 1e-3, out=base.clone(), gated=gated, q=q)
            want = torch.where(f > 0, base, torch.zeros_like(base)) if gated else base
            assert torch.equal(c[zero], want[zero]), (B, C, H, gated, "accumulate under q = 0")


def test_nan_under_zero_weight_is_not_laundered(dev, ops):
    f = torch.rand(1, 64, 16, 16, generator=torch.Generator().manual_seed(24)).to(dev)
    m = torch.ones(1, 1, 16, 16, device=dev)
    m[0, 0, 3, 5] = 0
    q = ops.guidance_build(m)[0][0]
    assert float(q[0, 3, 5]) == 0
    f[0, 7, 3, 5] = float("nan")
    g = ops.gram_fwd(f, q=q)
    assert bool(torch.isnan(g[0, 7]).all()) and bool(torch.isnan(g[0, :, 7]).all())
    out = ops.gram_bwd(torch.ones(1, 64, 64, device=dev), f, 1.0, q=q)
    assert bool(torch.isnan(out[0, :, 3, 5]).all()) and bool(torch.isfinite(out[0, :, 0, 0]).all())


# ================================================================================================ real operands
@pytest.mark.parametrize("S", [64, 128])
def test_real_operands_meet_the_weighted_bound(dev, ops, S):
    """kappa_w = kappa + 5 (tests/_guidedref.py: q carries a division, a multiplication and a square root, <= 1.5 u; each
    operand's q F one more u; two operands per product: 5 u on top of the chain _gramref counts).  M is the weighted
    absolute sum.  The backward's D is G^(image) - G(other style image), its bound kappa_bwd + 5."""
    mask = cow_coverage(dev, S)
    m = mask.cpu()
    imgs = R.style_crops(S, S, R.STYLES[:2])
    taps = G.tap_activations(imgs * m + (1 - m))
    other = G.tap_activations(R.style_crops(S, S, R.STYLES[2:3]))
    planes, _ = ops.guidance_build(mask)
    w = GR.weights64(m)
    for l, mod in enumerate(G.STYLE_TAPS):
        F = taps[mod]
        B, C, H = F.shape[0], F.shape[1], F.shape[2]
        ref, M = GR.guided_gram_ref(F, w[l])
        got = ops.gram_fwd(F.to(dev), q=planes[l])
        assert torch.equal(got, got.transpose(1, 2))
        kap = GR.kappa_w_fwd(B, C, H * H)
        err = (got.cpu().double() - ref).abs()
        assert bool((err <= kap * G.U32 * M).all()), (S, l, float((err / (kap * G.U32 * M).clamp_min(1e-300)).max()))
        worst = float((err / (G.U32 * M).clamp_min(1e-300))[M > 0].max())
        print(f"\n  weighted gram_fwd S={S} tap {l} (C={C}, HW={H * H}): worst err/(u M) {worst:.2f} of kappa_w {kap:.1f}")
        multi = ops.gram_fwd_multi([F.to(dev)], qs=[planes[l]])[0]
        err = (multi.cpu().double() - ref).abs()
        assert bool((err <= GR.kappa_w_fwd(B, C, H * H, G.multi_scale(C, H * H)) * G.U32 * M).all()), (S, l, "multi")
        # backward
        D = (got.cpu().double() - G.gram_ref(other[mod])[0]).float()
        coef = 4.0 * 1e6 * G.style_norm(C, H, B)
        for gated in (False, True):
            bref, bM = GR.guided_bwd_ref(D, F, w[l], coef, gated=gated)
            bgot = ops.gram_bwd(D.to(dev).expand(B, -1, -1).contiguous(), F.to(dev), coef, gated=gated, q=planes[l]).cpu().double()
            kb = GR.kappa_w_bwd(C)
            berr = (bgot - bref).abs()
            assert bool((berr <= kb * G.U32 * bM).all()), (S, l, gated, float((berr / (kb * G.U32 * bM).clamp_min(1e-300)).max()))
            print(f"  weighted gram_bwd gated={gated}: worst err/(u M) {float((berr / (G.U32 * bM).clamp_min(1e-300))[bM > 0].max()):.2f} of {kb:.1f}")


# ================================================================================================ public API
def test_guided_gram_matrix_autograd(dev):
    import style_transfer as ST
    gen = torch.Generator().manual_seed(25)
    f = torch.rand(2, 64, 16, 16, generator=gen)
    m = GR.disc_mask(2, 16)
    Rw = torch.randn(2, 64, 64, generator=gen)
    leaf = f.to(dev).requires_grad_(True)
    g = ST.guided_gram_matrix(leaf, m.to(dev))
    (g * Rw.to(dev)).sum().backward()
    w = GR.weights64(m)[0]
    ref, M = GR.guided_gram_ref(f, w)
    assert bool(((g.detach().cpu().double() - ref).abs() <= GR.kappa_w_fwd(2, 64, 256) * G.U32 * M).all())
    D = (Rw + Rw.transpose(1, 2))
    bref, bM = GR.guided_bwd_ref(D, f, w, 1.0)
    # (D itself is an fp32 sum: one more rounding per entry)
    assert bool(((leaf.grad.cpu().double() - bref).abs() <= (GR.kappa_w_bwd(64) + 1) * G.U32 * bM).all())
    with pytest.raises(RuntimeError):
        ST.guided_gram_matrix(f, m)
    with pytest.raises(ValueError):
        ST.guided_gram_matrix(torch.rand(2, 64, 5, 5).to(dev), m.to(dev))


# ================================================================================================ the fused bottom pass
def test_exact_weighted_bottom_pass(dev, ops):
    """st3d_conv1_bwd_weighted at 64 x 64 on integers (F in {0..3}, w0 in {0, 4}, |D| <= 4, |gy| <= 8, weights in -2..2, coef 2:
    |t| <= 8 + 2 * 4 * 12 * 64, |gx| <= 64 * 9 * 2 * |t| < 2^24) for (D only, gy only, both) x (plain, need-listed), against
    the integer reference and against the unfused weighted route on the same integers (gram_bwd with q, then the gated
    conv1_1 input gradient)."""
    import _needref as NR
    gen = torch.Generator().manual_seed(26)
    N, H, W = 2, 64, 64
    f = _int_feat((N, 64, H, W), gen)
    gy = torch.randint(-8, 9, (N, 64, H, W), generator=gen).float()
    D = torch.randint(-4, 5, (N, 64, 64), generator=gen).float()
    w = torch.randint(-2, 3, (64, 3, 3, 3), generator=gen).float()
    q = _q02(N, H * W, gen).reshape(N, H, W)
    w0 = q * q
    _, wd = ops.conv3x3_pack(w.to(dev))
    need = (GR.disc_mask(N, H)[:, 0] > 0).to(torch.uint8).numpy()
    seg = torch.from_numpy(NR.segments(need)).to(dev)
    needd = torch.from_numpy(need).to(dev)
    px = (needd != 0)[:, None].expand(-1, 3, -1, -1)
    fd, w0d, qd = f.to(dev), w0.to(dev), q.to(dev)
    for g_, D_ in ((None, D), (gy, None), (gy, D)):
        t = torch.zeros(N, 64, H * W, dtype=torch.float64)
        if g_ is not None:
            t = t + g_.double().flatten(2)
        if D_ is not None:
            t = t + 2.0 * torch.bmm(D_.double(), (f * w0[:, None]).double().flatten(2))
        ref, _ = R.conv1_bwd_ref(t.reshape(N, 64, H, W), f, None, 0.0, w)          # the gate is F's own sign
        assert float(ref.abs().max()) < 1 << 24
        gd = None if g_ is None else g_.to(dev)
        Dd = None if D_ is None else D_.to(dev)
        got = ops.conv1_bwd_weighted(gd, fd, Dd, 2.0, wd, w0d)
        assert torch.equal(got.cpu().double(), ref), ("conv1_bwd_weighted", g_ is not None, D_ is not None)
        listed = ops.conv1_bwd_weighted(gd, fd, Dd, 2.0, wd, w0d, seg, needd)
        assert torch.equal(listed[px], got[px]) and bool((listed[~px] == 0).all())
        # unfused: t through the weighted Gram backward (q twice = w0 once on these integers), then gate + conv1_1^T
        tt = gd.clone() if gd is not None else torch.zeros_like(fd)
        if Dd is not None:
            tt = ops.gram_bwd(Dd, fd, 2.0, out=tt, q=qd)
        unf = ops.conv3x3_dgrad(tt, fd, wd, 3)
        assert torch.equal(unf, got), ("unfused route", g_ is not None, D_ is not None)
    one = torch.ones(N, H, W, device=dev)
    assert torch.equal(ops.conv1_bwd_weighted(gy.to(dev), fd, D.to(dev), 2.0, wd, one), ops.conv1_bwd(gy.to(dev), fd, D.to(dev), 2.0, wd))


# ================================================================================================ through the plan
SW, CW = 1e6, 1.0


@pytest.fixture(scope="module")
def vgg(dev):
    from st3d import vgg as V
    return V.get_vgg(seed=0, device=dev)


def _plan_case(vgg, dev, S, seed=0):
    """B = 2 at S: (plan, current images = two style crops composited on white under the cow's coverage, mask).  A plan of
    its own (not the model's cached one), closed by the test."""
    from st3d import vgg as V
    mask = cow_coverage(dev, S)
    m = mask.cpu()
    cur = (R.style_crops(S, S, R.STYLES[:2]) * m + (1 - m)).contiguous()
    gen = torch.Generator().manual_seed(50 + seed)
    content = (cur * (1.0 + 1e-2 * torch.randn(cur.shape, generator=gen))).clamp(0, 1)
    style = R.style_crops(S, S, R.STYLES[2:3])
    plan = V.PerceptualPlan(vgg, 2, S)
    plan.use_graph(False)
    plan.set_content(content.to(dev), force=True)
    plan.set_style(style.to(dev), 2, force=True)
    return plan, cur.to(dev), mask, (content, style)


def _loss(plan, cur, **kw):
    loss, grad = plan.loss(cur, SW, CW, want_grad=True, **kw)
    return loss.clone(), grad


@pytest.mark.parametrize("S", [16, 24, 64])
def test_plan_guided_loss_against_the_fp64_tail(vgg, dev, ops, S):
    """S = 64 reaches the fused bottom pass, S = 24 the direct-conv path with odd sides.  The loss triple against the fp64
    guided tail on the plan's OWN fp32 activations, within the bound tests/test_gpu_loss_tail.py (c) derives with the Gram's
    kappa extended to kappa_w = kappa + 5 for the current images (the style targets are plain Grams: kappa).
    The image gradient, element by element, against the fp64 VGG backward (_guidedref.image_grad_ref: checked against
    torch autograd on the CPU; no kernel of the library takes part) of the fp64 guided tail's tap gradients, on the plan's own
    activations (gates and pool argmax included).  The bound is derived, first order: every tap gradient arrives with
        |coef| (dD (w |F|) + kappa_w_bwd u |D| (w |F|))        (dD: the bound of D = G^ - S used for the loss above)
    and the content tap with 4 u of itself, and every conv adds kappa u M, M = conv^T(|g|, |W|), with the kappa and the tile
    of the kernel the plan really ran for that layer (read from the plan's launch records).  Two bounds are built from
    these local terms (_guidedref.image_grad_ref): the worst case, pushed through |W|^T -- a backstop, thirteen layers
    without cancellation make it astronomically loose -- and the probabilistic one, 8 standard deviations with every local
    bound taken for a standard deviation and variances pushed through W^2, which tests/test_guided_ref.py shows to hold
    torch's own fp32 chain at under a hundredth and to catch one wrong gate bit.  Both are asserted, element by element;
    exact zeros of a bound admit only exact zeros."""
    plan, cur, mask, (content, style) = _plan_case(vgg, dev, S)
    try:
        plan.forward(style.to(dev))
        sacts = [plan.activation(m)[:1].cpu().clone() for m in G.STYLE_TAPS]
        plan.forward(content.to(dev))
        ctgt = plan.activation(G.CONTENT_TAP).cpu().clone()
        loss, grad = _loss(plan, cur, style_mask=mask)
        acts_d = [plan.activation(m).clone() for m in G.STYLE_TAPS]
        acts = [a.cpu() for a in acts_d]
        cact = plan.activation(G.CONTENT_TAP).cpu().clone()
        assert [a.shape[2] for a in acts] == GR.sides(S)
        Sref = [G.gram_ref(a) for a in sacts]
        w = GR.weights64(mask.cpu())
        t = GR.guided_tail_ref(acts, w, cact, [s[0] for s in Sref], ctgt, SW, CW, 2.0, want_grads=False)
        sb, dDs = 0.0, []
        for l, a in enumerate(acts):
            C, H, HW = a.shape[1], a.shape[2], a[0, 0].numel()
            dG = GR.kappa_w_fwd(2, C, HW, G.multi_scale(C, HW), white=True) * R.U32 * t["MG"][l]
            dS = G.kappa_fwd(1, C, HW, G.multi_scale(C, HW), white=True) * R.U32 * Sref[l][1].expand_as(dG)
            dD = dG + dS + R.U32 * (t["D"][l].abs() + dG + dS)
            dDs.append(dD)
            sq = float((2 * t["D"][l].abs() * dD + dD * dD).sum())
            sb += G.style_norm(C, H, 2) * (sq + G.sqdiff_kappa(a.shape[0] * C * C) * R.U32 * (float((t["D"][l] ** 2).sum()) + sq))
        cb = G.sqdiff_kappa(cact.numel()) * R.U32 * t["loss"][1]
        bounds = [CW * cb + SW * sb + 3 * R.U32 * t["loss"][0], cb, sb]
        got = loss.cpu().double().tolist()
        for k, nm in enumerate(("total", "content", "style")):
            err = abs(got[k] - t["loss"][k])
            print(f"\n  guided plan S={S} {nm:8s} {got[k]:.6e} (fp64 {t['loss'][k]:.6e})  err {err:.3e}  bound {bounds[k]:.3e}")
            assert err <= bounds[k], (nm, got[k], t["loss"][k], bounds[k])
        # the unguided loss of the same images is another number: the guidance is in effect
        plain, _ = _loss(plan, cur)
        assert abs(float(plain[2]) - got[2]) > 1e-3 * got[2]
        # image gradient against the fp64 backward of the fp64 tap gradients
        from oracle import perceptual_ref as P
        model = P.make_vgg19_features(seed=0)
        weights = {m: model._modules[str(m)].weight.detach() for m in R.VGG_CONVS}
        plan.forward(cur)                                       # every conv's full-resolution output (the same bits)
        A = {m: plan.activation(m).cpu().clone() for m in R.VGG_CONVS}
        for l, m in enumerate(G.STYLE_TAPS):
            assert torch.equal(A[m], acts[l])
        tref = GR.guided_tail_ref(acts, w, cact, [s[0] for s in Sref], ctgt, SW, CW, 2.0)
        taps, errs = {}, {}
        for l, m in enumerate(G.STYLE_TAPS):
            a = acts[l]
            wf = (a.double() * w[l][:, None]).flatten(2)        # w |F| (post-ReLU: F >= 0)
            e = abs(tref["coef"][l]) * (torch.bmm(dDs[l], wf) + GR.kappa_w_bwd(a.shape[1]) * R.U32 * torch.bmm(tref["D"][l].abs() + dDs[l], wf))
            taps[m], errs[m] = tref["grads"][l], e.reshape(a.shape)
        taps[G.CONTENT_TAP], errs[G.CONTENT_TAP] = tref["content_grad"], 4 * R.U32 * tref["content_grad"].abs()
        # which kernel ran each input gradient: the plan's own launch records of one more (profiled) call
        plan.profile(True)
        plan.profile_launches()
        again = _loss(plan, cur, style_mask=mask)
        fam = {"convx_dgrad": "direct", "convx_dgrad_need": "direct", "conv_dgrad": "f2", "conv43_dgrad": "f4", "conv43_dgrad_need": "f4"}
        algos = {m: fam[f] for f, m, _ in plan.profile_launches() if f in fam}
        plan.profile(False)
        assert torch.equal(again[1], grad) and sorted(algos) == sorted(R.VGG_CONVS)
        want, E, Es = GR.image_grad_ref(A, weights, taps, errs, algos=algos)
        err = (grad.cpu().double() - want).abs()
        assert bool((err[E == 0] == 0).all())
        ratio = err / Es.clamp_min(1e-300)
        k = int(ratio.argmax())
        print(f"  guided plan S={S} image gradient against the fp64 backward ({' '.join(algos[m] for m in sorted(algos))}): worst err / "
              f"probabilistic bound {float(ratio.max()):.4f} (bound / max|ref| there {float(Es.flatten()[k] / want.abs().max()):.2e}), "
              f"err/max|ref| {float(err.max() / want.abs().max()):.2e}, worst err / worst-case bound {float((err / E.clamp_min(1e-300)).max()):.2e}")
        assert bool((err <= Es).all()) and bool((err <= E).all()), float(ratio.max())
    finally:
        plan.close()


@pytest.mark.parametrize("S", [16, 24, 64])
def test_plan_guidance_invariants_bitwise(vgg, dev, S):
    """a mask of ones == the unguided call; cleared == never set; two runs equal; graph replay on == off; features under
    zero weight do not matter is checked at the kernels -- here: the gradient of a guided call differs from the unguided."""
    plan, cur, mask, _ = _plan_case(vgg, dev, S, seed=1)
    try:
        base = _loss(plan, cur)
        ones = _loss(plan, cur, style_mask=torch.ones_like(mask))
        assert torch.equal(ones[0], base[0]) and torch.equal(ones[1], base[1])
        g1 = _loss(plan, cur, style_mask=mask)
        g2 = _loss(plan, cur, style_mask=mask)
        assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
        assert not torch.equal(g1[1], base[1]) and bool(torch.isfinite(g1[1]).all())
        cleared = _loss(plan, cur)
        assert torch.equal(cleared[0], base[0]) and torch.equal(cleared[1], base[1])
        # (n, S, S) masks are taken as well
        g3 = _loss(plan, cur, style_mask=mask[:, 0])
        assert torch.equal(g3[0], g1[0]) and torch.equal(g3[1], g1[1])
        # graph replay: first call warms, second captures, third replays
        plan.use_graph(True)
        for _ in range(3):
            gg = _loss(plan, cur, style_mask=mask)
            assert torch.equal(gg[0], g1[0]) and torch.equal(gg[1], g1[1])
        for _ in range(3):                                     # and back to unguided under replay: keyed on the guidance
            gb = _loss(plan, cur)
            assert torch.equal(gb[0], base[0]) and torch.equal(gb[1], base[1])
        other = cow_coverage(dev, S).flip(0).contiguous()      # another mask, same addresses inside the plan
        plan.use_graph(False)
        want = _loss(plan, cur, style_mask=other)
        plan.use_graph(True)
        for _ in range(3):
            gg = _loss(plan, cur, style_mask=other)
            assert torch.equal(gg[0], want[0]) and torch.equal(gg[1], want[1])
        plan.use_graph(False)
        # an empty mask for one image: its style term is the constant, its gradient the content term's alone
        half = mask.clone()
        half[1] = 0
        e = _loss(plan, cur, style_mask=half)
        c_only = plan.loss(cur, 0.0, CW, want_grad=True)[1]
        assert bool(torch.isfinite(e[1]).all()) and torch.allclose(e[1][1], c_only[1], rtol=1e-5, atol=1e-12)
    finally:
        plan.close()


def test_plan_guided_with_need_mask_and_flat_colour(vgg, dev):
    """S = 64: guided with the need mask and the flat colour is bitwise the guided call without them at needed pixels, 0
    elsewhere; the loss is the same bits"""
    S = 64
    plan, cur, mask, _ = _plan_case(vgg, dev, S, seed=2)
    try:
        need = (mask[:, 0] > 0).to(torch.uint8).contiguous()
        full = _loss(plan, cur, style_mask=mask)
        for kw in (dict(need_mask=need), dict(flat_color=(1.0, 1.0, 1.0)), dict(need_mask=need, flat_color=(1.0, 1.0, 1.0))):
            got = _loss(plan, cur, style_mask=mask, **kw)
            assert torch.equal(got[0], full[0]), kw
            if "need_mask" in kw:
                px = (need != 0)[:, None].expand(-1, 3, -1, -1)
                assert torch.equal(got[1][px], full[1][px]) and bool((got[1][~px] == 0).all()), kw
            else:
                assert torch.equal(got[1], full[1]), kw
    finally:
        plan.close()


def test_plan_guided_nan_and_state_and_bytes(vgg, dev):
    from st3d import _lib
    S = 64
    plan, cur, mask, _ = _plan_case(vgg, dev, S, seed=3)
    try:
        lib = _lib.load()
        before = plan.bytes()
        _loss(plan, cur, style_mask=mask)
        grown = plan.bytes() - before
        B = 2
        stated = 4 * (lib.st3d_guidance_floats(B, S) + B * S * S + 5 * B + lib.st3d_guidance_partials(B, S))
        assert 0 < grown <= stated, (grown, stated)
        assert lib.st3d_guidance_floats(B, S) == B * sum(h * h for h in GR.sides(S)) <= 1.34 * B * S * S
        assert grown < 64 * B * S * S * 4 / 16                     # nowhere near a scaled copy of relu1_1
        _loss(plan, cur, style_mask=mask)
        assert plan.bytes() - before == grown                      # allocated once
        # a NaN pixel poisons the result (under weight 0 as well: no laundering)
        bad = cur.clone()
        y, x = [int(v[0]) for v in torch.where(mask[0, 0] == 0)]
        bad[0, 1, y, x] = float("nan")
        loss, grad = _loss(plan, bad, style_mask=mask)
        assert bool(torch.isnan(loss[2])) and bool(torch.isnan(loss[0]))
        # a guidance for another n than the loss call's
        plan.set_style_guidance(mask[:1], 1)
        with pytest.raises(_lib.St3dError, match="guidance"):
            _lib.call("st3d_plan_loss", plan._h, _lib.dptr(cur), 2, 2, SW, CW, _lib.dptr(plan.loss_buf), None, _lib.stream_ptr())
        plan.set_style_guidance(None)
        with pytest.raises(_lib.St3dError):
            plan.loss(cur, SW, CW, style_mask=mask.cpu())
        with pytest.raises(_lib.St3dError):
            plan.loss(cur, SW, CW, style_mask=mask[:, :, :32])
    finally:
        plan.close()


# ================================================================================================ public API through a render
def test_compute_perceptual_loss_with_style_masks_on_a_render(dev):
    import losses as L
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    S, B = 64, 2
    a = SC.load_asset("cow")
    Rm, T = SC.random_cameras(B, seed=3)
    mesh0, renderer, cams = SC.device_scene(U, dev, a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], SC.texture_at(a, 64), Rm, T, S)
    vgg = U.get_vgg(seed=0)
    style = SC.style_at(1, S).to(dev).expand(B, -1, -1, -1)
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, mesh0, cams)
    out = U.setup_optimizations("texture", mesh0, 0.01)
    res = {}
    for name in ("none", "object", "ones"):
        mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
        cur, masks = U.render_meshes(renderer, mesh, cams)
        sm = {"none": None, "object": masks, "ones": torch.ones_like(masks)}[name]
        loss = L.compute_perceptual_loss(cur, content, style, vgg, style_masks=sm)
        out["optimizer"].zero_grad()
        loss.backward()
        res[name] = (float(loss.detach()), out["texture_map"].grad.clone())
    assert res["ones"][0] == res["none"][0] and torch.equal(res["ones"][1], res["none"][1])
    assert res["object"][0] != res["none"][0] and not torch.equal(res["object"][1], res["none"][1])
    assert bool(torch.isfinite(res["object"][1]).all()) and float(res["object"][1].abs().max()) > 0
    mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
    cur, masks = U.render_meshes(renderer, mesh, cams)
    with pytest.raises(RuntimeError):
        L.compute_perceptual_loss(cur, content, style, vgg, style_masks=masks.cpu())
    with pytest.raises(ValueError):
        L.compute_perceptual_loss(cur, content, style, vgg, style_masks=masks[:1])
    # the third door: 2D style transfer of the renders under their coverage runs and moves the covered pixels
    o = ST.style_transfer(content, content, style, vgg, steps=2, style_masks=masks)
    assert bool(torch.isfinite(o).all()) and not torch.equal(o.detach(), content)


# ================================================================================================ the scripts
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "2d-to-3d-style-transfer_amd")


def _child(script, argv, cwd):
    """a fresh child process under its own time limit"""
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(PKG, script)] + argv, cwd=cwd,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]


def _log_losses(path):
    return [float(line.split("Loss ")[1]) for line in open(os.path.join(path, "log.txt")).read().splitlines()[1:]]


def _cow_files(tmp, cow, golden_dir):
    from PIL import Image
    from st3d import io as stio
    tex = torch.from_numpy(cow["texture_u8"][::16, ::16].copy()).float() / 255
    obj = os.path.join(tmp, "cow.obj")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    style = os.path.join(tmp, "style.png")
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    return obj, style


@pytest.mark.parametrize("script,extra", [
    ("second_approach.py", ["--epochs", "3", "--save_every", "0"]),
    ("first_approach.py", ["--n_style_transfer_steps", "3", "--n_mse_steps", "3"]),
])
def test_scripts_with_style_mask_object(dev, cow, golden_dir, tmp_path, script, extra):
    """3 steps at size 64 with --style_mask object and with none: both finish and export, and the logged first loss differs
    (second approach: the perceptual loss itself; first approach: the targets phase A hands to phase B)"""
    tmp = str(tmp_path)
    obj, style = _cow_files(tmp, cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0"] + extra
    first = {}
    for mode in ("object", "none"):
        out = os.path.join(tmp, mode)
        _child(script, common + ["--output_path", out, "--style_mask", mode], tmp)
        losses = _log_losses(out)
        assert len(losses) == 3 and all(np.isfinite(losses))
        assert os.path.exists(os.path.join(out, "final.obj"))
        first[mode] = losses[0]
    assert first["object"] != first["none"], first
