"""Checks of the checker (CPU): tests/_gramref.py's fp64 references, its split restatement, its operand families, its
bounds and their sharpness.

  * the fp64 tail (Grams, squared-difference sums, loss triple, gradients leaving the taps) equals torch autograd of the
    reference's formula in fp64; `gram_split` reproduces the split counts gram.hip quotes for config 2;
  * the operand families look like the product: most Gram entries far below the maximum, many exact zeros;
  * the bounds are not tuned to the kernels: the fp32 emulation of their summation order meets them on every family
    (this re-measures _gramref.MEASURED_CPU), and so does torch's own fp32 bmm where its own error is below the bound
    (where it is not, on a few of the images composited on white, the figure is printed);
  * wrong results fail: seven small wrong changes of a passing fp32 result fail the per-element bound, and three of them
    pass the suite's older `err <= 2e-5 max|ref|` on the same data."""
import time

import pytest
import torch

import _convref as R
import _gramref as G

OLD = 2e-5                       # the suite's global criterion for the Gram kernels (tests/test_gpu_kernels.py)
WHITE = (4, 5, 6, 7)             # indices of the images composited on white in the 8-image sets


@pytest.fixture(scope="module")
def crops():
    c = R.style_crops(96, 256)
    return G.tap_activations(torch.cat([c, R.on_white(c)]))


@pytest.fixture(scope="module")
def full():
    """512^2: style1 and style3 plain, style4 and style5 on white (the forward of all eight is 4.5 s; the GPU module takes all)"""
    t0 = time.time()
    taps = G.tap_activations(G.style_images(512)[[0, 1, 6, 7]])
    print(f"\n  VGG forward of four 512^2 images: {time.time() - t0:.1f} s")
    return taps


@pytest.fixture(scope="module")
def odd():
    return G.tap_activations(G.style_images(90))


def test_tail_reference_matches_fp64_autograd():
    """the reference's formula (gram_matrix + mse_loss per layer / (C^2 H^2), mean-squared content term) differentiated
    by autograd in fp64 with respect to the tap activations"""
    taps = G.tap_activations(G.style_images(64)[[0, 5, 2]])
    gen = torch.Generator().manual_seed(0)
    acts = [taps[m][:2].double() for m in G.STYLE_TAPS]
    cact = taps[G.CONTENT_TAP][:2].double()
    ctgt = G.near(cact, 0.1, gen)
    sw, cw = 1e6, 1.0
    for style_n in (1, 2):
        sg = [G.gram_ref(taps[m][2:3] if style_n == 1 else G.near(taps[m][:2], 0.05, gen))[0] for m in G.STYLE_TAPS]
        leaves = [a.clone().requires_grad_(True) for a in acts]
        cl = cact.clone().requires_grad_(True)
        content = torch.nn.functional.mse_loss(cl, ctgt)
        style = 0
        for f, s in zip(leaves, sg):
            b, c, h, w = f.shape
            g = torch.bmm(f.reshape(b, c, h * w), f.reshape(b, c, h * w).transpose(1, 2))
            style = style + torch.nn.functional.mse_loss(g, s.expand_as(g)) / (c ** 2 * h ** 2)
        total = cw * content + sw * style
        total.backward()
        t = G.tail_ref(acts, cact, sg, ctgt, sw, cw)
        for got, want in zip(t["loss"], (total, content, style)):
            assert abs(got - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        for got, leaf in zip(t["grads"], leaves):
            assert torch.allclose(got, leaf.grad, rtol=0, atol=1e-12 * float(leaf.grad.abs().max()))
        assert torch.allclose(t["content_grad"], cl.grad, rtol=0, atol=1e-12 * float(cl.grad.abs().max()))
    # gated: the same, zero where the activation is zero; M dominates |ref| and vanishes behind a closed gate
    D = t["D"][2]
    ref, M = G.gram_bwd_ref(D, acts[2], 0.37, base=torch.ones_like(acts[2]), gated=True)
    assert bool((ref[acts[2] <= 0] == 0).all()) and bool((M[acts[2] <= 0] == 0).all()) and bool((M >= ref.abs() - 1e-12).all())


def test_gram_split_reproduces_the_quoted_tables():
    """gram.hip's comments for config 2 (B = 8 at 512^2): 256 channels at 128^2 take 32 splits, 512 at 64^2 16, 512 at 32^2 8;
    and the invariants of every split: whole 32-pixel chunks, the splits cover HW with none empty, at most 256"""
    assert G.gram_split(8, 256, 128 * 128)[0] == 32
    assert G.gram_split(8, 512, 64 * 64)[0] == 16
    assert G.gram_split(8, 512, 32 * 32)[0] == 8
    assert G.gram_split(8, 64, 1 << 18) == (128, 2048) and G.gram_split(1, 64, 1 << 20) == (256, 4096)
    for B in (1, 3, 8):
        for C in (64, 96, 128, 256, 320, 512):
            for HW in (1, 25, 31, 121, 484, 1024, 2025, 8100, 1 << 14, 1 << 18, 1 << 20):
                for scale in (1, 2):
                    ns, kper = G.gram_split(B, C, HW, scale)
                    assert 1 <= ns <= 256 and kper % 32 == 0 and ns * kper >= HW > (ns - 1) * kper, (B, C, HW, scale)


def test_operand_families_look_like_the_product(crops, full):
    """at least 40 % of every real Gram's entries below 1e-3 of its maximum and at least 5 % exact zeros (measured: 53-69 %
    and 10-27 %), so the families cannot silently degrade into uniform ones"""
    for name, taps in (("crops", crops), ("full", full)):
        for m in G.STYLE_TAPS:
            g, _ = G.gram_ref(taps[m])
            for i in range(g.shape[0]):
                small = float((g[i] < 1e-3 * g[i].max()).double().mean())
                zero = float((g[i] == 0).double().mean())
                assert small >= 0.40 and zero >= 0.05, (name, m, i, small, zero)
            assert float(taps[m].min()) >= 0.0
    gen = torch.Generator().manual_seed(1)
    sc = G.chscale(crops[10][:1], gen)
    ratio = sc.flatten(2).amax(2)[0] / crops[10][:1].flatten(2).amax(2)[0].clamp_min(1e-30)
    assert float(ratio[ratio > 0].max() / ratio[ratio > 0].min()) > 1e4


def _fwd_rows(rows, name, A, B, white_idx, scale=1, bmm=None):
    ref, M = G.gram_ref(A)
    C, HW = A.shape[1], A[0, 0].numel()
    n = G.fwd_chain(B, C, HW, scale)
    sub = list(range(3, C, C // 16)) if HW >= 1024 else list(range(C))      # a sample of 16 rows of the large layers (CPU time)
    for i in range(A.shape[0]):
        white = i in white_idx
        r = G.report(G.gram_fwd_emul(A[i], B, scale, rows=sub)[None], ref[i:i + 1, sub], M[i:i + 1, sub])
        rows.append(("fwd_white" if white else "fwd", n, r["ratio"]))
        kap = G.kappa_fwd(B, C, HW, scale, white)
        assert r["ratio"] <= kap, (name, C, HW, B, i, r, kap)
        if bmm is not None:
            f = A[i:i + 1].flatten(2)
            rb = G.report(torch.bmm(f, f.transpose(1, 2)), ref[i:i + 1], M[i:i + 1])
            bmm.append((name, C, HW, i, rb["ratio"], kap))


def test_emulation_meets_the_bounds(crops, full, odd):
    """the fp32 emulation of the kernels' summation order within kappa on every family; the worst err / (u M sqrt(n)) are
    _gramref.MEASURED_CPU.  torch's fp32 bmm is held to the same bound wherever its own figure allows, and printed
    where it does not (one running sum per entry: it is a different, longer chain)."""
    t0 = time.time()
    gen = torch.Generator().manual_seed(2)
    rows, bmm = [], []
    for m in G.STYLE_TAPS:
        _fwd_rows(rows, "full", full[m][[0, 3]], 8, (1,), bmm=bmm)
        _fwd_rows(rows, "full B=1", full[m][2:3], 1, (0,))
        _fwd_rows(rows, "full multi", full[m][1:3], 8, (1,), scale=2)
        _fwd_rows(rows, "crops", crops[m][[0, 2, 5, 7]], 8, (2, 3), bmm=bmm)
        _fwd_rows(rows, "crops B=3", crops[m][3:5], 3, (1,))
        _fwd_rows(rows, "odd", odd[m][[1, 3, 4, 6]], 1, (2, 3), bmm=bmm)
        _fwd_rows(rows, "chscale", G.chscale(crops[m][1:2], gen), 8, ())
        _fwd_rows(rows, "relu_shift", G.relu_shift(crops[m][:1].shape, gen), 1, ())
    big = G.tap_activations(G.mirror_tiled(R.style_crops(512, 512)[1])[None], upto=5)
    _fwd_rows(rows, "1024^2", big[0], 1, ())
    _fwd_rows(rows, "1024^2 white", R.vgg_activations(R.on_white(G.mirror_tiled(R.style_crops(512, 512)[2]))[None], upto=0)[0][3], 1, (0,))
    for C, HW in ((64, 1), (64, 31), (96, 484), (320, 121)):
        _fwd_rows(rows, "small", G.relu_shift((1, C, HW), gen), 1, ())
    # backward: far and near D on real and channel-scaled activations, with and without a base, gated and not
    for m in G.STYLE_TAPS:
        for taps, a, b in ((crops, 6, 2), (odd, 0, 5)):
            F = taps[m][a]
            C, H = F.shape[0], F.shape[1]
            ga = G.gram_ref(taps[m][[a, b]])[0]
            Ds = {"far": (ga[0] - ga[1]).float()}
            for eps in (1e-2, 1e-4):
                Ds[f"near{eps:g}"] = (ga[0] - G.gram_ref(G.near(F, eps, gen)[None])[0][0]).float()
            coef = 4.0 * 1e6 * G.style_norm(C, H, 8)
            for dname, D in Ds.items():
                for Fx in (F, G.chscale(F[None], gen)[0]):
                    base = None if dname == "far" else torch.randn(Fx.shape, generator=gen) * float(coef * (D.abs() @ Fx.flatten(1)).mean())
                    for gated in (False, True):
                        ref, M = G.gram_bwd_ref(D[None], Fx[None], coef, None if base is None else base[None], gated)
                        r = G.report(G.gram_bwd_emul(D, Fx, coef, base, gated)[None], ref, M)
                        rows.append(("bwd", G.bwd_chain(C), r["ratio"]))
                        assert r["ratio"] <= G.kappa_bwd(C), (m, dname, gated, r)
    fig = G.chain_figures(rows)
    for k, v in fig.items():
        if k == "fwd_white":
            print(f"  emulation worst err/(u M n) on white: {v:.3f} (documented {G.MEASURED_CPU[k]:g}; its bound is the worst case n + 2)")
            continue
        cst = {"fwd": G.C_FWD, "bwd": G.C_BWD}[k]
        # each constant is at most MARGIN x the documented CPU figure
        print(f"  emulation worst err/(u M sqrt n) {k}: {v:.3f} (documented {G.MEASURED_CPU[k]:g}, bound constant {cst:g})")
        assert cst <= G.MARGIN * G.MEASURED_CPU[k] * (1 + 1e-9)
    for name, C, HW, i, ratio, kap in bmm:
        if ratio > kap:
            print(f"  torch fp32 bmm exceeds the kernels' bound on {name} C={C} HW={HW} image {i}: {ratio:.1f} u > kappa {kap:.1f}")
    assert sum(ratio <= kap for *_, ratio, kap in bmm) >= 0.8 * len(bmm)
    print(f"  {len(rows)} (kernel, family, shape, image) rows in {time.time() - t0:.1f} s")


def _largest_group_passing_old(ref, mutate, sizes=(32, 8, 4, 1)):
    """the largest aligned row group (the quietest non-dead one of its size) whose mutant passes err <= OLD max|ref|"""
    for size in sizes:
        g0 = G.quiet_group(ref, size)
        bad = mutate(g0, size)
        if G.scale_close(bad, ref, OLD):
            return size, g0, bad
    return None, None, None


def test_wrong_results_fail_the_bound_and_three_pass_the_old_criterion(full, crops):
    """Seven slips applied to an fp32 result that meets its bound.  All must fail the per-element bound.  (a), (c) and (e)
    are shown to PASS err <= 2e-5 max|ref| on the same data, on the quietest non-dead channel group: measured on the real
    features no aligned 32- or 64-channel group is quiet (every one holds a channel within 0.15-0.95 of the loudest), so
    the group is the largest of 32 / 8 / 4 / 1 rows for which the old criterion passes, and the stale mirror block of (c)
    holds what a stale slab holds in a running optimisation -- the previous iterate's Gram, F (1 + eps randn): with
    eps = 3e-4 the block is off by 1e-5 of the maximum (old criterion: passes) and by hundreds of u of its own entries;
    with eps = 1e-3 (3.8e-5 of the maximum) and taken from a different STYLE image (0.07-1.1 of the maximum) both criteria
    see it.  All three variants must fail the per-element bound."""
    gen = torch.Generator().manual_seed(3)
    passed_old = {}
    # ---- forward, relu1_1 at 512^2 in a batch of 8 (the image on white) and relu4_1
    A1 = full[0][2]
    C, HW = A1.shape[0], A1[0].numel()
    ref, M = (t[0] for t in G.gram_ref(A1[None]))
    g32, slabs = G.gram_fwd_emul(A1, 8, return_slabs=True)
    kap = G.kappa_fwd(8, C, HW, white=True)
    assert G.report(g32, ref, M)["ratio"] <= kap
    ns, kper = G.gram_split(8, C, HW)
    f = A1.flatten(1)
    k0 = (ns // 2) * kper + kper - 32                       # (a) the last 32-pixel chunk of the middle split
    chunk = f[:, k0:k0 + 32] @ f[:, k0:k0 + 32].t()

    def drop_chunk(g0, size):
        bad = g32.clone()
        bad[g0:g0 + size] -= chunk[g0:g0 + size]
        return bad
    size, g0, bad = _largest_group_passing_old(ref, drop_chunk)
    assert size is not None and G.report(bad, ref, M)["ratio"] > kap
    assert G.report(drop_chunk(0, 64), ref, M)["ratio"] > kap
    passed_old["(a) dropped 32-pixel chunk"] = f"rows {g0}..{g0 + size - 1} of relu1_1: {G.report(bad, ref, M)['ratio']:.0f} u (kappa {kap:.0f})"
    g0 = G.quiet_group(ref, 32)                             # (b) one slab left out of the reduce
    bad = g32.clone()
    bad[g0:g0 + 32] = G.reduce_emul(slabs, leave_out=slabs.shape[0] // 2)[g0:g0 + 32]
    assert G.report(bad, ref, M)["ratio"] > kap
    sub = list(range(3, C, 4))
    bad = G.gram_fwd_emul(G.trunc_mantissa(A1, 10), 8, rows=sub)      # (d) operands cut to 10 mantissa bits
    assert G.report(bad, ref[sub], M[sub])["ratio"] > kap
    # (c) a stale 64 x 64 mirror block below the diagonal of a 128-tile, relu4_1
    A4 = full[19]
    C4, HW4 = A4.shape[1], A4[0, 0].numel()
    ref4, M4 = (t[2] for t in G.gram_ref(A4))
    kap4 = G.kappa_fwd(8, C4, HW4, white=True)
    blocks = [(128 * t + 64, 128 * t) for t in range(C4 // 128)]
    r0, c0 = min(blocks, key=lambda rc: float(ref4[rc[0]:rc[0] + 64, rc[1]:rc[1] + 64].max()) or float("inf"))
    band = list(range(r0, r0 + 64))                         # (the emulation of the block's 64 rows only: CPU time)
    g4 = torch.zeros(C4, C4)
    g4[band] = G.gram_fwd_emul(A4[2], 8, rows=band)
    full_ref4, ref4, M4 = ref4, ref4[band], M4[band]
    assert G.report(g4[band], ref4, M4)["ratio"] <= kap4
    for what, other in (("another style image", A4[0]), ("the previous iterate (1e-3)", G.near(A4[2], 1e-3, gen)),
                        ("the previous iterate (3e-4)", G.near(A4[2], 3e-4, gen))):
        bad = g4[band].clone()
        bad[:, c0:c0 + 64] = G.gram_fwd_emul(other, 8, rows=band)[:, c0:c0 + 64]
        rr = G.report(bad, ref4, M4)
        assert rr["ratio"] > kap4, what
        rr["glob"] = float((bad.double() - ref4).abs().max() / full_ref4.max())
        if rr["glob"] <= OLD:
            print(f"  (c) from {what}: err/max|ref| {rr['glob']:.1e}: only the per-element bound sees it")
            passed_old["(c) stale 64 x 64 mirror block"] = f"rows {r0}.., columns {c0}.. of relu4_1 from {what}: {rr['ratio']:.0f} u (kappa {kap4:.0f})"
        else:
            print(f"  (c) from {what}: err/max|ref| {rr['glob']:.1e}: both criteria see it")
    # ---- backward, relu3_1 of the 96 x 256 crops: D = G(style1) - G(style3), channel-scaled activations
    A3 = crops[10]
    C3, H3 = A3.shape[1], A3.shape[2]
    g3 = G.gram_ref(A3[:2])[0]
    D = (g3[0] - g3[1]).float()
    F3 = G.chscale(A3[:1], gen)[0]
    D = (D * (F3.flatten(1).amax(1) / A3[0].flatten(1).amax(1).clamp_min(1e-30))[:, None]).contiguous()     # rows follow their channel
    coef = 4.0 * 1e6 * G.style_norm(C3, H3, 8)
    kb = G.kappa_bwd(C3)
    refb, Mb = (t[0].flatten(1) for t in G.gram_bwd_ref(D[None], F3[None], coef, gated=True))
    outb = G.gram_bwd_emul(D, F3, coef, gated=True).flatten(1)
    assert G.report(outb, refb, Mb)["ratio"] <= kb
    ungated = G.gram_bwd_emul(D, F3, coef).flatten(1)
    f3 = F3.flatten(1)

    def shift_gates(g0, size):                              # (e) gate bits taken from the rows one 32-row block further down
        bad = outb.clone()
        src = (g0 + 32) % C3
        bad[g0:g0 + size] = torch.where(f3[src:src + size] > 0, ungated[g0:g0 + size], torch.zeros_like(ungated[g0:g0 + size]))
        return bad
    size, g0, bad = _largest_group_passing_old(refb, shift_gates)
    assert size is not None and G.report(bad, refb, Mb)["ratio"] > kb
    assert G.report(shift_gates(G.quiet_group(refb, 32), 32), refb, Mb)["ratio"] > kb
    passed_old["(e) gate bits of the neighbouring block"] = f"rows {g0}..{g0 + size - 1} of relu3_1"
    # (f) D^T for D through the ungated entry point, D not symmetric
    Dn = (D + 0.1 * D.abs().mean() * torch.randn(D.shape, generator=gen)).contiguous()
    reff, Mf = (t[0] for t in G.gram_bwd_ref(Dn[None], F3[None], coef))
    assert G.report(G.gram_bwd_emul(Dn, F3, coef), reff, Mf)["ratio"] <= kb
    assert G.report(G.gram_bwd_emul(Dn.t().contiguous(), F3, coef), reff, Mf)["ratio"] > kb
    # (g) coef folded twice into one 128-row x 64-pixel tile
    bad = ungated.clone()
    g0 = G.quiet_group(reff.flatten(1), 128)
    D2 = D.clone()
    D2[g0:g0 + 128] *= torch.tensor(coef, dtype=torch.float32)
    bad[g0:g0 + 128, :64] = G.gram_bwd_emul(D2, f3[:, :64], coef)[g0:g0 + 128]
    rg, Mg = (t[0].flatten(1) for t in G.gram_bwd_ref(D[None], F3[None], coef))
    assert G.report(ungated, rg, Mg)["ratio"] <= kb and G.report(bad, rg, Mg)["ratio"] > kb
    for k, v in passed_old.items():
        print(f"  passes err <= {OLD:g} max|ref| and fails the per-element bound: {k} -- {v}")
    assert len(passed_old) == 3, passed_old
