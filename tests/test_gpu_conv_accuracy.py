"""Every conv entry point of the plan on VGG's real operands, element by element against fp64 (tests/_convref.py).

Operands: the inputs of the seeded VGG's conv layers on two style-image crops (one composited onto white, as a rendered
view), relu(randn + 1), 1 + 1e-3 randn and randn inputs; the seeded weights and a variant with shifted filter means;
ReLU-gated, unpool-scattered, Gram-backward (coef D F) and channel-scaled output gradients, and dense randn ones.  Each
(kernel, family) asserts
  (a) |got - ref| <= kappa u M per element (_convref's table: kappa and M of the kernel's algorithm), and
  (b) the suite's global bound err <= rtol max|ref| on the same data (direct 2e-5, dgrad_unpool 5e-5, conv1_bwd 3e-5;
      Winograd 3e-5 forward, 5e-5 input gradient, 6e-5 through the unpool).
ReLU'd outputs are compared as they are (relu is 1-Lipschitz).  Fused pools stay bitwise the pool of the kernel's own
full-resolution output.  Then bitwise invariances: the F(4x4,3x3) schedule (slots, XCD numbering) and the batch (image n of
an N = 3 launch == the image alone).  `pytest -s` prints one line per (kernel, family): worst err/(u M) and err/max|ref|."""
import pytest
import torch

import _convref as R

pytestmark = pytest.mark.gpu

# (module index, Cin, Cout, crop).  LAYERS: the crops every kernel takes (W % 64 -> F(4x4) 4 x 64 steps, W % 32 -> 8 x 32
# steps); ODD: the odd maps of the direct-kernel plan at S = 90 (45, 22, 11, 5), on the layers a pool follows (and conv5_1).
# Activations of the 96 x 256 image crops: 96 x 256, 48 x 128, 24 x 64, 12 x 32, 6 x 16 per level.
LAYERS = [(2, 64, 64, (16, 64)),
          (5, 64, 128, (16, 64)),
          (7, 128, 128, (8, 64)),
          (10, 128, 256, (8, 64)),
          (16, 256, 256, (8, 64)),
          (19, 256, 512, (8, 32)),
          (25, 512, 512, (8, 32))]
ODD = [(2, 64, 64, (45, 45)), (7, 128, 128, (45, 45)), (16, 256, 256, (22, 22)), (25, 512, 512, (11, 11)), (28, 512, 512, (5, 5))]
# operand families per case (fp64 work: about 100 GFLOP for the module, counted by _convref.FP64_FLOPS)
FWD_FAMILIES = {False: (None, ("real_white", "flat")), True: (("real", "flat"), ("real_white",))}     # odd: (seeded, shifted)
DGRAD_FAMILIES = {False: (None, ("gate",)), True: (("unpool", "chscale"), ())}
# (module index, map) where conv3x3_fwd exceeds kappa_direct on the shifted-mean filters: test_direct_forward_sum_order
DIRECT_SHIFTED_EXCEEDS = {(10, (8, 64)), (16, (8, 64)), (16, (22, 22)), (19, (8, 32)),
                          (25, (8, 32)), (25, (11, 11)), (28, (5, 5))}
GLOB = {("direct", "fwd"): 2e-5, ("direct", "dgrad"): 2e-5, ("direct", "unpool"): 5e-5, ("direct", "conv1_bwd"): 3e-5,
        ("f2", "fwd"): 3e-5, ("f2", "dgrad"): 5e-5, ("f2", "unpool"): 6e-5, ("f4", "fwd"): 3e-5, ("f4", "dgrad"): 5e-5,
        ("f4", "unpool"): 5e-5}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@pytest.fixture(scope="module")
def images():
    """top-left 96 x 256 crops of style1 (plain) and style4 (on white); all four styles for conv1_1"""
    c = R.style_crops(96, 256)
    return dict(pair=torch.stack([c[0], R.on_white(c[2])]), all=torch.cat([c, R.on_white(c)]))


@pytest.fixture(scope="module")
def acts(images):
    return R.vgg_activations(images["pair"])


@pytest.fixture(scope="module", autouse=True)
def _fp64_budget():
    n0 = R.FP64_FLOPS[0]
    yield
    print(f"\n  fp64 convolution work of the module: {(R.FP64_FLOPS[0] - n0) / 1e9:.1f} GFLOP")


def _check(rows, got, ref, M, algo, what, name):
    r = R.report(got, ref, R.mag(R._d(M), algo))
    rows.append((name, r))
    print(f"  {name:58s} err/(uM) {r['ratio']:8.2f} (kappa {R.KAPPA[algo]:g})   err/max|ref| {r['glob']:.2e}")
    return r, r["ratio"] <= R.KAPPA[algo] and r["glob"] <= GLOB[(algo, what)]


def _assert_all(rows, oks):
    bad = [f"{n}: err/(uM) {r['ratio']:.1f} at {r['loc']}, err/max|ref| {r['glob']:.2e}" for (n, r), ok in zip(rows, oks) if not ok]
    assert not bad, "\n".join(bad)


def _crop(t, hw):
    return t[..., :hw[0], :hw[1]].contiguous()


def _fwd_families(acts, idx, hw, odd, gen):
    x, w, b, _ = acts[idx]
    fam = R.input_families(_crop(x, hw), gen)
    seeded, shifted = FWD_FAMILIES[odd]
    sets = [("seeded", w, {k: fam[k] for k in (seeded or fam)})]
    sets.append(("shifted", R.shifted(w), {k: fam[k] for k in shifted}))
    return b, sets


def _kernels_fwd(lib, Cin, Cout, H, W, odd):
    ks = ["direct"]
    if not odd and lib.st3d_wino_supported(Cin, Cout, H, W):
        ks.append("f2")
    if not odd and lib.st3d_wino43_supported(Cin, Cout, H, W):
        ks.append("f4")
    return ks


def _run_fwd(ops, dev, algo, x, wt, b, relu, pool=False):
    xd, bd, Cout = x.to(dev), b.to(dev), wt.shape[0]
    if algo == "direct":
        wf, _ = ops.conv3x3_pack(wt.to(dev))
        return ops.conv3x3_fwd(xd, wf, bd, Cout, relu=relu)
    if algo == "f2":
        uf, _ = ops.wino_pack(wt.to(dev))
        return ops.wino_fwd(xd, uf, bd, Cout, relu=relu, pool=pool)
    uf, _ = ops.wino43_pack(wt.to(dev))
    return ops.wino43_fwd(xd, uf, bd, Cout, relu=relu, pool=pool)


_FWD_REFS = {}


def _forward_case(ops, lib, dev, acts, idx, hw, odd, seed, only=None):
    gen = torch.Generator().manual_seed(seed)
    b, sets = _fwd_families(acts, idx, hw, odd, gen)
    exempt = (idx, tuple(hw)) in DIRECT_SHIFTED_EXCEEDS
    rows, oks = [], []
    for wname, wt, fam in sets:
        if only is not None and wname != only:
            continue
        Cout, Cin = wt.shape[:2]
        xs = torch.cat(list(fam.values()))
        key = (idx, tuple(hw), wname)
        if key not in _FWD_REFS:                  # (test_direct_forward_sum_order reuses the main cases' references)
            _FWD_REFS[key] = (R.conv_fwd(xs, wt, b), R.mag_fwd(xs, wt, b))
        ref, M = _FWD_REFS[key]
        for algo in _kernels_fwd(lib, Cin, Cout, hw[0], hw[1], odd):
            pre = _run_fwd(ops, dev, algo, xs, wt, b, relu=False).cpu()
            post = _run_fwd(ops, dev, algo, xs, wt, b, relu=True)
            for i, fname in enumerate(fam):
                for tag, got, rf in (("", pre[i:i + 1], ref[i:i + 1]), (" relu", post[i:i + 1].cpu(), ref[i:i + 1].clamp_min(0))):
                    r, ok = _check(rows, got, rf, M[i:i + 1], algo, "fwd", f"{algo} fwd{tag} {Cin}->{Cout} {hw} {wname}/{fname}")
                    if algo == "direct" and wname == "shifted" and exempt and only is None:
                        ok = r["glob"] <= GLOB[(algo, "fwd")]        # (a) fails here: test_direct_forward_sum_order
                    oks.append(ok)
            if algo != "direct":            # fused pool: bitwise the pool kernel on the kernel's own full-resolution output
                yf, pd, pidx = _run_fwd(ops, dev, algo, xs, wt, b, relu=True, pool=True)
                p2, i2 = ops.maxpool2x2(post)
                assert torch.equal(yf, post) and torch.equal(pd, p2) and torch.equal(pidx, i2), (algo, wname)
    _assert_all(rows, oks)


@pytest.mark.parametrize("idx,Cin,Cout,hw", LAYERS)
def test_forward_on_real_operands(ops, lib, dev, acts, idx, Cin, Cout, hw):
    """conv3x3_fwd (MFMA path), wino_fwd, wino43_fwd (+ fused pool) on the layer's input crop"""
    _forward_case(ops, lib, dev, acts, idx, hw, False, idx)


@pytest.mark.parametrize("idx,Cin,Cout,hw", ODD)
def test_forward_on_real_operands_odd_maps(ops, lib, dev, acts, idx, Cin, Cout, hw):
    """the direct kernel on the odd maps of the off-fast-path plan (S = 90: 45, 22, 11, 5)"""
    _forward_case(ops, lib, dev, acts, idx, hw, True, idx + 100)


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="finding: conv3x3_fwd sums K = 9 Cin terms in one fp32 accumulator (2 per MFMA), so on filters with "
                          "a non-zero mean and non-negative inputs its error grows like sqrt(K): up to 43 u M at Cin 512 "
                          "against kappa_direct 21 (torch's CPU conv2d: 5.3); globally <= 4.3e-6 of max|ref|")
@pytest.mark.parametrize("idx,hw", sorted(DIRECT_SHIFTED_EXCEEDS))
def test_direct_forward_sum_order(ops, lib, dev, acts, idx, hw):
    """(a) for the direct forward kernel on the shifted-mean filters where it does not hold (every other (layer, map)
    asserts it in the cases above; these assert (b))"""
    odd = (idx, hw) not in {(l[0], l[3]) for l in LAYERS}
    _forward_case(ops, lib, dev, acts, idx, hw, odd, idx + (100 if odd else 0), only="shifted")


def _dgrad_unpool_direct(ops, gp, pidx, pooled, wd, Cin, H, W):
    """st3d_conv3x3_dgrad_unpool at the full map size (odd H / W as in the plan: the wrapper assumes 2 Hp x 2 Wp)"""
    N, Cout = gp.shape[:2]
    gx = torch.empty((N, Cin, H, W), dtype=torch.float32, device=gp.device)
    ops.call("st3d_conv3x3_dgrad_unpool", ops.dptr(gp.contiguous(), ops.F32), ops.dptr(pidx, ops.U8), ops.dptr(pooled, ops.F32),
             ops.dptr(wd, ops.F32), ops.dptr(gx), N, Cin, Cout, H, W, ops.stream_ptr())
    return gx


def _dgrad_case(ops, lib, dev, acts, idx, hw, odd, seed):
    gen = torch.Generator().manual_seed(seed)
    x, w, _, y = acts[idx]
    Cout, Cin = w.shape[:2]
    H, W = hw
    fam = R.grad_families(_crop(y, hw), gen)
    xin = _crop(x, hw)                                   # the conv's own input: the next link's gate on the chain kernels
    tgt = torch.randn(xin.shape, generator=gen) * xin.std()
    coef = 0.37
    f2 = not odd and lib.st3d_wino_supported(Cout, Cin, H, W) == 1
    f4 = not odd and lib.st3d_wino43_supported(Cout, Cin, H, W) == 1
    rows, oks = [], []
    seeded, shifted = DGRAD_FAMILIES[odd]
    for wname, wt, names in (("seeded", w, list(seeded or fam)), ("shifted", R.shifted(w), list(shifted))):
        _, wd = ops.conv3x3_pack(wt.to(dev))
        if f2:
            _, ud = ops.wino_pack(wt.to(dev))
        if f4:
            _, u6 = ops.wino43_pack(wt.to(dev))
        for fname in names:
            d = fam[fname]
            g, a = d["g"], d["act"]
            n = 0 if a is None or a is fam["gate"]["act"] else 1
            og, tg = xin[n:n + 1], tgt[n:n + 1]
            ref, M = R.conv_dgrad(g, wt), R.mag_dgrad(g, wt)
            gd, ad = g.to(dev), (a.to(dev) if a is not None else None)
            tag = f"{Cout}->{Cin} {hw} {wname}/{fname}"
            res = [("direct", "dgrad", ops.conv3x3_dgrad(gd, ad, wd, Cin), ref, M)]
            if f2:
                res.append(("f2", "dgrad", ops.wino_dgrad(gd, ad, ud, Cin), ref, M))
                res.append(("f2", "dgrad", ops.wino_dgrad_chain(gd, ud, Cin), ref, M))
            if f4:
                res.append(("f4", "dgrad", ops.wino43_dgrad_chain(gd, u6, Cin), ref, M))
            if fname == "unpool":
                gp, pidx, pooled = d["gp"].to(dev), d["idx"].to(dev), d["pooled"].to(dev)
                res.append(("direct", "unpool", _dgrad_unpool_direct(ops, gp, pidx, pooled, wd, Cin, H, W), ref, M))
                if f2:
                    res.append(("f2", "unpool", ops.wino_dgrad_unpool(gp, pidx, pooled, ud, Cin), ref, M))
                    gpg = torch.where(pooled > 0, gp, torch.zeros_like(gp))
                    res.append(("f2", "unpool", ops.wino_dgrad_chain(gpg, ud, Cin, pool_idx=pidx), ref, M))
                if f4:
                    gpg = torch.where(pooled > 0, gp, torch.zeros_like(gp))
                    res.append(("f4", "unpool", ops.wino43_dgrad_chain(gpg, u6, Cin, pool_idx=pidx), ref, M))
            # the producer-gated chain: out_gate = the conv's input, plus the content term coef (out_gate - target)
            ogd, tgd = og.to(dev), tg.to(dev)
            ref_c = R.gate_chain(ref, og, tg, coef)
            open_ = (R._d(og) > 0).double()
            for algo, fn in (("f2", lambda: ops.wino_dgrad_chain(gd, ud, Cin, out_gate=ogd, add_target=tgd, add_coef=coef)) if f2 else (None, None),
                             ("f4", lambda: ops.wino43_dgrad_chain(gd, u6, Cin, out_gate=ogd, add_target=tgd, add_coef=coef)) if f4 else (None, None)):
                if algo is None:
                    continue
                # magnitude of the chain output: the conv's (tile-pooled) plus the content term's, zero behind a closed gate
                Mc = open_ * (R.mag(M, algo) + coef * (R._d(og).abs() + R._d(tg).abs()))
                r = R.report(fn(), ref_c, Mc)
                ok = r["ratio"] <= R.KAPPA[algo] and r["glob"] <= GLOB[(algo, "dgrad")]
                rows.append((f"{algo} chain+gate+content {tag}", r))
                oks.append(ok)
                print(f"  {algo + ' chain+gate+content ' + tag:58s} err/(uM) {r['ratio']:8.2f}   err/max|ref| {r['glob']:.2e}")
            for algo, what, got, rf, m in res:
                _, ok = _check(rows, got.cpu(), rf, m, algo, what, f"{algo} {what} {tag}")
                oks.append(ok)
    _assert_all(rows, oks)


@pytest.mark.parametrize("idx,Cin,Cout,hw", LAYERS)
def test_input_gradient_on_real_operands(ops, lib, dev, acts, idx, Cin, Cout, hw):
    """conv3x3_dgrad, conv3x3_dgrad_unpool, wino_dgrad / _unpool / _chain, wino43_dgrad_chain (plain, pool_idx, gate + content)"""
    _dgrad_case(ops, lib, dev, acts, idx, hw, False, idx + 200)


@pytest.mark.parametrize("idx,Cin,Cout,hw", ODD)
def test_input_gradient_on_real_operands_odd_maps(ops, lib, dev, acts, idx, Cin, Cout, hw):
    """conv3x3_dgrad and conv3x3_dgrad_unpool on the odd maps of the S = 90 plan (the pool floors: last row / column dropped)"""
    _dgrad_case(ops, lib, dev, acts, idx, hw, True, idx + 300)


@pytest.mark.parametrize("hw", [(32, 64), (45, 90)])
def test_conv1_1_on_images(ops, dev, images, hw):
    """conv1_1 (3 -> 64) on [0, 1] images and the same crops on white: the VALU forward / input-gradient kernels (W % 4 == 0)
    and the MFMA ones (W = 90), and st3d_conv1_bwd with the Gram term on the real relu1_1 features"""
    gen = torch.Generator().manual_seed(hw[1])
    x = _crop(images["all"], hw)
    acts1 = R.vgg_activations(x, upto=0)
    _, w, b, y = acts1[0]
    rows, oks = [], []
    for wname, wt in (("seeded", w), ("shifted", R.shifted(w))):
        wf, wd = ops.conv3x3_pack(wt.to(dev))
        ref, M = R.conv_fwd(x, wt, b), R.mag_fwd(x, wt, b)
        got = ops.conv3x3_fwd(x.to(dev), wf, b.to(dev), 64, relu=False).cpu()
        for i in range(x.shape[0]):
            oks.append(_check(rows, got[i:i + 1], ref[i:i + 1], M[i:i + 1], "direct", "fwd", f"direct fwd 3->64 {hw} {wname}/image{i}")[1])
        yw = R.conv_fwd(x, wt, b, relu=True).float()
        fam = R.grad_families(yw[[0, 4]], gen)
        for fname in ("gate", "unpool", "chscale", "randn"):
            g, a = fam[fname]["g"], fam[fname]["act"]
            ref, M = R.conv_dgrad(g, wt), R.mag_dgrad(g, wt)
            got = ops.conv3x3_dgrad(g.to(dev), a.to(dev) if a is not None else None, wd, 3).cpu()
            oks.append(_check(rows, got, ref, M, "direct", "dgrad", f"direct dgrad 64->3 {hw} {wname}/{fname}")[1])
        # st3d_conv1_bwd: gate(gy + coef D F) through conv1_1^T, F = the real relu1_1 of an image on white
        F_ = yw[4:5]
        C, HW = 64, hw[0] * hw[1]
        Dm = torch.randn(1, C, C, generator=gen, dtype=torch.float64)
        Dm = (0.5 * (Dm + Dm.transpose(1, 2)) / HW).float()
        gy = torch.randn(F_.shape, generator=gen) * 1e-2
        for has_g, has_d in ((True, True), (False, True), (True, False)):
            ref, M = R.conv1_bwd_ref(gy if has_g else None, F_, Dm if has_d else None, 50.0, wt)
            got = ops.conv1_bwd(gy.to(dev) if has_g else None, F_.to(dev), Dm.to(dev) if has_d else None, 50.0, wd).cpu()
            oks.append(_check(rows, got, ref, M, "direct", "conv1_bwd", f"conv1_bwd {hw} {wname} g={has_g} D={has_d}")[1])
    _assert_all(rows, oks)


@pytest.mark.parametrize("Cin", [192, 320])
@pytest.mark.parametrize("hw", [(8, 64), (8, 32)])
def test_wino43_ring_phase(ops, dev, monkeypatch, Cin, hw):
    """Cin 192 / 320 = 12 / 20 sixteen-channel stages per tile, multiples of the 3-deep ring: a workgroup that walks several
    tiles starts every one of them on the same ring slot (Cin 64 .. 512 never do).  The ring carries over from tile to tile
    only inside one persistent workgroup's walk, so ST3D_W43_SLOTS = 1 (one workgroup per cout tile walks every tile) and 4
    (ragged walks) -- at the default these small maps get one tile per workgroup.  Forward and chains reducing over Cin
    stages against fp64, per element."""
    gen = torch.Generator().manual_seed(Cin + hw[1])
    w = torch.randn(Cin, Cin, 3, 3, generator=gen) * (2.0 / (Cin * 9)) ** 0.5         # Cin -> Cin: both directions reduce over Cin
    b = torch.randn(Cin, generator=gen) * 0.05
    x = torch.cat([torch.relu(torch.randn(1, Cin, *hw, generator=gen) + 1.0), torch.randn(1, Cin, *hw, generator=gen)])
    g = torch.relu(torch.randn(2, Cin, *hw, generator=gen)) * torch.randn(2, Cin, *hw, generator=gen)
    gp = torch.randn(2, Cin, hw[0] // 2, hw[1] // 2, generator=gen)
    pidx = torch.randint(0, 4, gp.shape, generator=gen, dtype=torch.uint8)
    up = R.unpool(gp, pidx, *hw)
    refs = [("fwd", R.conv_fwd(x, w, b), R.mag_fwd(x, w, b)), ("dgrad", R.conv_dgrad(g, w), R.mag_dgrad(g, w)),
            ("unpool", R.conv_dgrad(up, w), R.mag_dgrad(up, w))]
    uf, ud = ops.wino43_pack(w.to(dev))
    rows, oks = [], []
    for slots in ("1", "4"):
        monkeypatch.setenv("ST3D_W43_SLOTS", slots)
        got = [ops.wino43_fwd(x.to(dev), uf, b.to(dev), Cin, relu=False), ops.wino43_dgrad_chain(g.to(dev), ud, Cin),
               ops.wino43_dgrad_chain(gp.to(dev), ud, Cin, pool_idx=pidx.to(dev))]
        for (what, ref, M), y in zip(refs, got):
            oks.append(_check(rows, y.cpu(), ref, M, "f4", what, f"f4 {what} {Cin}->{Cin} {hw} slots {slots}")[1])
    _assert_all(rows, oks)


def _schedule_operands(acts, src, hw):
    """real: (input, weights, bias, post-ReLU output) of VGG module src; an int >= 100: synthetic with Cin = Cout = src"""
    if src < 100:
        x, w, b, y = acts[src]
        return _crop(x, hw), w, b, _crop(y, hw)
    gen = torch.Generator().manual_seed(src)
    w = torch.randn(src, src, 3, 3, generator=gen) * (2.0 / (src * 9)) ** 0.5
    x = torch.relu(torch.randn(2, src, *hw, generator=gen) + 0.5)
    return x, w, torch.randn(src, generator=gen) * 0.05, torch.relu(torch.randn(2, src, *hw, generator=gen))


@pytest.mark.parametrize("src,hw", [(16, (16, 64)), (25, (8, 32)), (192, (8, 64)), (320, (16, 32))])
def test_wino43_schedule_is_bitwise_invariant(ops, dev, acts, monkeypatch, src, hw):
    """Which workgroup computes a tile must not change its arithmetic: forward and chain outputs are torch.equal across
    ST3D_W43_SLOTS in {default, 0, 1, 2, 3, 7, 1000} x ST3D_W43_XCD in {1, 0} (stale-ring or tile-boundary errors below any
    tolerance show here), on real conv3_x / conv4_x operands and at Cin 192 / 320 (stage counts that are multiples of the
    ring depth)."""
    x, w, b, y = _schedule_operands(acts, src, hw)
    Cout, Cin = w.shape[:2]
    uf, ud = ops.wino43_pack(w.to(dev))
    xd, bd = x.to(dev), b.to(dev)
    g = (torch.randn(y.shape, generator=torch.Generator().manual_seed(src)) * (y > 0)).to(dev)
    pooled, pidx = ops.maxpool2x2(y.to(dev))
    gp = torch.where(pooled > 0, torch.ones_like(pooled), torch.zeros_like(pooled)) * 0.5
    og = x.to(dev)

    def run():
        yf, pd, pi = ops.wino43_fwd(xd, uf, bd, Cout, relu=True, pool=True)
        return (ops.wino43_fwd(xd, uf, bd, Cout, relu=False), yf, pd, pi, ops.wino43_dgrad_chain(g, ud, Cin),
                ops.wino43_dgrad_chain(g, ud, Cin, out_gate=og), ops.wino43_dgrad_chain(gp, ud, Cin, pool_idx=pidx))
    monkeypatch.delenv("ST3D_W43_SLOTS", raising=False)
    monkeypatch.delenv("ST3D_W43_XCD", raising=False)
    base = run()
    for slots in ("", "0", "1", "2", "3", "7", "1000"):
        for xcd in ("1", "0"):
            if slots:
                monkeypatch.setenv("ST3D_W43_SLOTS", slots)
            else:
                monkeypatch.delenv("ST3D_W43_SLOTS", raising=False)
            monkeypatch.setenv("ST3D_W43_XCD", xcd)
            for k, (a, b_) in enumerate(zip(run(), base)):
                assert torch.equal(a, b_), (slots, xcd, k)


def test_batch_invariance(ops, lib, dev, acts):
    """Image n of an N = 3 launch is bitwise the image launched alone, for the direct kernel, F(2x2,3x3) and F(4x4,3x3),
    forward and input gradient.  (The launchers pick one kernel variant whatever N: the direct grid has N as its z
    dimension; wino4 and wino43 deal the same per-tile arithmetic to more workgroups, so the per-tile sums do not move.)"""
    x, w, b, y = acts[16]
    x = torch.cat([_crop(x, (16, 64)), torch.relu(torch.randn(1, 256, 16, 64, generator=torch.Generator().manual_seed(3)) + 1)])
    g = torch.cat([_crop(y, (16, 64)), torch.randn(1, 256, 16, 64, generator=torch.Generator().manual_seed(4))]) * 0.1
    xd, gd, bd = x.to(dev), g.to(dev), b.to(dev)
    wf, wd = ops.conv3x3_pack(w.to(dev))
    uf, ud = ops.wino_pack(w.to(dev))
    u6f, u6d = ops.wino43_pack(w.to(dev))
    launches = {"direct fwd": lambda t: ops.conv3x3_fwd(t, wf, bd, 256, relu=True),
                "direct dgrad": lambda t: ops.conv3x3_dgrad(t, None, wd, 256),
                "f2 fwd": lambda t: ops.wino_fwd(t, uf, bd, 256, relu=True),
                "f2 dgrad": lambda t: ops.wino_dgrad_chain(t, ud, 256),
                "f4 fwd": lambda t: ops.wino43_fwd(t, u6f, bd, 256, relu=True),
                "f4 dgrad": lambda t: ops.wino43_dgrad_chain(t, u6d, 256)}
    for name, fn in launches.items():
        src = xd if "fwd" in name else gd
        full = fn(src)
        for n in range(3):
            assert torch.equal(full[n:n + 1], fn(src[n:n + 1].contiguous())), (name, n)
