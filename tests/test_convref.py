"""Checks of the checker (CPU): tests/_convref.py's fp64 references, its per-element bounds and its operand families.

  * the fp64 references equal torch's conv2d / autograd in fp64 on every operand family;
  * the bounds are not tuned to our kernels: torch's own fp32 conv2d meets the direct bound, the fp32 Winograd emulations
    meet theirs, on every family (this re-measures _convref.MEASURED_CPU);
  * the bounds are sharp enough: small wrong changes of the fp64 result fail them, and one of them passes the older global
    criterion at 3e-5 on real activations -- the reason the per-element metric exists."""
import pytest
import torch
import torch.nn.functional as F

import _convref as R

LAYERS = R.VGG_CONVS          # conv1_1 .. conv5_1
CROP = (16, 32)               # per-layer crop of the 64 x 128 images' activations (top-left: the image border is in)
CO = 64                       # output channels per layer checked (the first 64 filters; the reduction is over all of Cin)


@pytest.fixture(scope="module")
def operands():
    """per layer: (input families, seeded / shifted weights, bias, gradient families) on CPU, built once"""
    imgs = R.style_crops(64, 128)
    pair = torch.stack([imgs[0], R.on_white(imgs[2])])
    acts = R.vgg_activations(pair)
    g = torch.Generator().manual_seed(0)
    out = {}
    for i in LAYERS:
        x, w, b, y = acts[i]
        x, y = x[..., :CROP[0], :CROP[1]], y[..., :CROP[0], :CROP[1]]
        fam = R.input_families(x, g) if w.shape[1] > 3 else {"img": x[0:1], "img_white": x[1:2]}
        out[i] = dict(x=fam, w={"seeded": w[:CO], "shifted": R.shifted(w)[:CO]}, b=b[:CO], g=R.grad_families(y[:, :CO], g))
    return out


def test_operand_families_look_like_the_product(operands):
    """images in [0, 1] with a white surround; post-ReLU activations with exact zeros; gated gradients mostly zero"""
    img = operands[0]["x"]
    assert 0.0 <= float(img["img"].min()) and float(img["img"].max()) <= 1.0
    assert float(img["img_white"][..., 0, 0].min()) == 1.0                  # corner: background
    for i in LAYERS[1:]:
        real = operands[i]["x"]["real"]
        assert float(real.min()) >= 0.0 and float((real == 0).double().mean()) > 0.05, i
        gf = operands[i]["g"]
        assert float((gf["gate"]["g"] == 0).double().mean()) > 0.2 and float((gf["unpool"]["g"] == 0).double().mean()) >= 0.75
    w = operands[7]["w"]
    assert float(w["seeded"].sum((1, 2, 3)).abs().mean()) < float(w["shifted"].sum((1, 2, 3)).abs().mean()) / 3


@pytest.mark.parametrize("i", LAYERS)
def test_fp64_references_match_torch_autograd(operands, i):
    op = operands[i]
    for wname, w in op["w"].items():
        wd, bd = w.double().requires_grad_(False), op["b"].double()
        for xf in op["x"].values():
            x = xf.double().requires_grad_(True)
            y = F.conv2d(x, wd, bd, padding=1)
            # the forward reference against an independent im2col product in fp64
            cols = F.unfold(xf.double(), 3, padding=1)                         # N, Cin*9, H*W
            yi = (wd.reshape(wd.shape[0], -1) @ cols + bd.view(1, -1, 1)).reshape(y.shape)
            assert torch.allclose(R.conv_fwd(xf, w, op["b"]), yi, rtol=0, atol=1e-12 * float(yi.abs().max()))
            gy = torch.randn(y.shape, dtype=torch.float64)
            gx = torch.autograd.grad(torch.relu(y), x, gy)[0]
            ref = R.conv_dgrad(gy * (y > 0), w)
            assert torch.allclose(ref, gx, rtol=0, atol=1e-12 * float(gx.abs().max())), (wname, i)
        if w.shape[1] == 3:
            continue
        # through the pool: the unpool family against autograd of relu -> max_pool2d (ATen's first-max argmax)
        d = op["g"]["unpool"]
        a = d["act"].double().requires_grad_(True)
        p = F.max_pool2d(a, 2, 2)
        ga = torch.autograd.grad(p, a, d["gp"].double() * (p > 0))[0]
        assert torch.equal(R.unpool(d["gp"].double() * (d["pooled"] > 0), d["idx"], *a.shape[-2:]), ga)
        # the producer-gated chain with the content term against autograd: the link's output is d/dz of
        # <g, conv(relu(z))> + coef/2 |relu(z) - target|^2 with out_gate = relu(z) (z != 0 everywhere: relu' is defined)
        if w.shape[1] != op["x"]["real"].shape[1]:
            continue
        og = op["x"]["real"].double()
        z = torch.where(og > 0, og, -0.5 - torch.rand(og.shape, dtype=torch.float64)).requires_grad_(True)
        tgt = torch.randn(og.shape, dtype=torch.float64)
        g = op["g"]["gate"]["g"].double()
        a = torch.relu(z)
        obj = (g * F.conv2d(a, wd, bd, padding=1)).sum() + 0.5 * 0.37 * ((a - tgt) ** 2).sum()
        dz = torch.autograd.grad(obj, z)[0]
        got = R.gate_chain(R.conv_dgrad(g, w), og, tgt, 0.37)
        assert torch.allclose(got, dz, rtol=0, atol=1e-12 * float(dz.abs().max())), (wname, i)


def test_conv1_bwd_reference_matches_autograd(operands):
    x = operands[0]["x"]["img_white"].double()
    w, b = operands[0]["w"]["shifted"].double(), operands[0]["b"].double()
    xx = x.clone().requires_grad_(True)
    Fm = torch.relu(F.conv2d(xx, w, b, padding=1))
    N, C, H, W = Fm.shape
    D = torch.randn(N, C, C, dtype=torch.float64)
    D = 0.5 * (D + D.transpose(1, 2))
    gy = torch.randn(Fm.shape, dtype=torch.float64)
    Ff = Fm.reshape(N, C, H * W)
    obj = (gy * Fm).sum() + 0.5 * 0.37 * torch.einsum("ncp,ncd,ndp->", Ff, D, Ff)
    gx = torch.autograd.grad(obj, xx)[0]
    ref, M = R.conv1_bwd_ref(gy, Fm.detach(), D, 0.37, w)
    assert torch.allclose(ref, gx, rtol=0, atol=1e-12 * float(gx.abs().max()))
    assert bool((M >= ref.abs() - 1e-12).all())


def test_fp32_cpu_results_meet_the_bounds(operands):
    """torch's fp32 conv2d (forward) / conv_transpose2d (input gradient) within KAPPA_DIRECT, the fp32 emulations of F(2x2,3x3)
    and F(4x4,3x3) within KAPPA_F2 / KAPPA_F4, on every family; the worst ratios are _convref.MEASURED_CPU"""
    worst = {"direct": 0.0, "f2": 0.0, "f4": 0.0}
    for i in LAYERS:
        op = operands[i]
        for wname, w in op["w"].items():
            Cin = w.shape[1]
            for fname, x in op["x"].items():
                ref, M = R.conv_fwd(x, w, op["b"]), R.mag_fwd(x, w, op["b"])
                got = {"direct": F.conv2d(x, w, op["b"], padding=1)}
                if Cin >= 64:
                    got["f2"] = R.wino_emul(x, w, op["b"], 2)
                    got["f4"] = R.wino_emul(x, w, op["b"], 4)
                for algo, y in got.items():
                    r = R.report(y, ref, R.mag(M, algo))
                    worst[algo] = max(worst[algo], r["ratio"])
                    assert r["ratio"] <= R.KAPPA[algo], (i, wname, fname, algo, r)
            for fname, d in op["g"].items():
                g = d["g"]
                ref, M = R.conv_dgrad(g, w), R.mag_dgrad(g, w)
                got = {"direct": F.conv_transpose2d(g, w, padding=1)}
                if Cin >= 64:
                    got["f2"] = R.wino_emul(g, R.dgrad_weights(w), None, 2)
                    got["f4"] = R.wino_emul(g, R.dgrad_weights(w), None, 4)
                for algo, y in got.items():
                    r = R.report(y, ref, R.mag(M, algo))
                    worst[algo] = max(worst[algo], r["ratio"])
                    assert r["ratio"] <= R.KAPPA[algo], (i, wname, fname, algo, r)
    for algo, v in worst.items():
        # each kappa is at most 4x the documented CPU figure; the re-measured figure depends a little on the host's oneDNN
        # blocking and is reported, not pinned
        print(f"  CPU fp32 worst err/(u M) {algo}: {v:.2f} (documented {R.MEASURED_CPU[algo]:g}, kappa {R.KAPPA[algo]:g})")
        assert R.KAPPA[algo] <= 4.0 * R.MEASURED_CPU[algo]


def _contribution(x, w, n, co, ci, y0, x0, h=1, wd=1):
    """the 3x3 contribution of input channels ci (a slice) to outputs (n, co, y0:y0+h, x0:x0+wd) in fp64"""
    return F.conv2d(R._d(x)[n:n + 1, ci], R._d(w)[co:co + 1, ci], padding=1)[0, 0, y0:y0 + h, x0:x0 + wd]


@pytest.mark.parametrize("i", [5, 7, 16])         # maps at least 16 x 32
def test_small_wrong_changes_fail_the_per_element_bound(operands, i):
    op = operands[i]
    w, b, x = op["w"]["seeded"], op["b"], op["x"]["real"]
    """Each change is applied to an fp32 result that meets its bound -- torch's fp32 conv2d for the direct bound, the
    F(4x4,3x3) emulation for the loosest bound -- so the bound tells it apart from fp32 rounding, not just from zero."""
    ref = R.conv_fwd(x, w, b)
    M = R.mag_fwd(x, w, b)
    M4 = R.mag(M, "f4")
    y32 = F.conv2d(x, w, b, padding=1).double()
    y43 = R.wino_emul(x, w, b, 4).double()
    assert R.within(y32, ref, M, R.KAPPA_DIRECT) and R.within(y43, ref, M4, R.KAPPA_F4)
    # one input channel's 3x3 contribution missing at a single output element (direct bound)
    per_ch = torch.stack([_contribution(x, w, 0, 5, slice(c, c + 1), 6, 9)[0, 0] for c in range(x.shape[1])])
    bad = y32.clone()
    bad[0, 5, 6, 9] -= per_ch[int(per_ch.abs().argmax())]           # (a channel that is not all zero there)
    assert not R.within(bad, ref, M, R.KAPPA_DIRECT)
    # one 4-channel k-step missing over one 4x4 tile (F(4x4,3x3) bound, the loosest)
    steps = [_contribution(x, w, 0, 9, slice(k, k + 4), 4, 8, 4, 4) for k in range(0, x.shape[1], 4)]
    bad = y43.clone()
    bad[0, 9, 4:8, 8:12] -= steps[int(torch.stack([s.abs().max() for s in steps]).argmax())]
    assert not R.within(bad, ref, M4, R.KAPPA_F4)
    # a last-lanes store error: column 31 of a 32-wide row written to column 30
    bad = y43.clone()
    bad[0, 17, 3, 30] = y43[0, 17, 3, 31]
    assert not R.within(bad, ref, M4, R.KAPPA_F4)
    # one 64-channel cout block scaled by (1 + 2^-10)
    bad = y43.clone()
    bad[:, 0:64] *= 1 + 2.0 ** -10
    assert not R.within(bad, ref, M4, R.KAPPA_F4)


def test_the_global_criterion_misses_what_the_per_element_bound_catches(operands):
    """On a real activation (conv3_x input on the image on white): one input channel's contribution dropped at the quietest
    output element passes err <= 3e-5 max|ref| (the older `_scale_close`) and fails the direct kernels' per-element bound"""
    op = operands[16]
    w, b, x = op["w"]["seeded"], op["b"], op["x"]["real_white"]
    ref, M = R.conv_fwd(x, w, b), R.mag_fwd(x, w, b)
    n, co, yy, xx = (int(v) for v in (M == M.min()).nonzero()[0])
    per_ch = torch.stack([_contribution(x, w, 0, co, slice(c, c + 1), yy, xx)[0, 0] for c in range(x.shape[1])])
    floor = R.KAPPA_DIRECT * R.U32 * float(M[n, co, yy, xx])
    big = per_ch.abs() > floor                     # the smallest single-channel contribution the bound resolves
    assert bool(big.any())
    c = int(torch.where(big, per_ch.abs(), torch.full_like(per_ch, float("inf"))).argmin())
    y32 = F.conv2d(x, w, b, padding=1).double()                      # an fp32 result that meets the bound
    assert R.within(y32, ref, M, R.KAPPA_DIRECT)
    bad = y32.clone()
    bad[0, co, yy, xx] -= per_ch[c]
    assert R.scale_close(bad, ref, 3e-5)
    assert not R.within(bad, ref, M, R.KAPPA_DIRECT)
