"""The style-loss tail -- Gram forward, squared-difference sums with D = G - S, Gram backward, content term, the fused
bottom of the backward -- on exact operands (bitwise) and on VGG's real operands (element by element against fp64,
tests/_gramref.py).

  (a) exact: integer-valued operands whose every partial sum is an integer below 2^24, so every fp32 summation order gives
      the same bits and the result must EQUAL the integer reference (exact in fp64): whatever is dropped, doubled or misaddressed shows,
      whatever its magnitude.  Every kernel body the launchers pick is reached: by shape, by the per-call switches
      (monkeypatch) and, for the switches a process reads once, in one fresh child process per setting.
  (b) real: the seeded VGG's tap activations of the committed style images (plain and on white) at the config shapes;
      per element |got - ref| <= kappa u M with kappa from the CPU emulation (never from these kernels), the suite's
      global bound unchanged on the same data, exact zeros for dead channels, G == G^T bitwise.
  (c) the near-converged tail composed (Gram -> sqdiff_sum_multi -> gram_bwd[_gated]) and through the plan, against
      the fp64 tail on the same fp32 activations, within bounds DERIVED from (b)'s per-element bounds.
  (d) invariances, bitwise: multi == single launches, sqdiff_sum_multi == folded sqdiff_sum launches, run to run, and
      independence of stale workspace contents (NaN and 1e30 in the recycled blocks).

`pytest -s` prints one line per (kernel, family, shape): worst err / (u M) with its location, and err / max|ref|."""
import os
import subprocess
import sys
import time

import pytest
import torch

import _convref as R
import _gramref as G

pytestmark = pytest.mark.gpu

GLOB = 2e-5                     # the suite's global bound for the Gram kernels (tests/test_gpu_kernels.py), unchanged
TAP_C = (64, 128, 256, 512, 512)
WORST = {}                      # kernel -> worst err / (u M) seen on the GPU (printed at the end; never used in a bound)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import _lib, ops as o
    if os.environ.get("ST3D_DIAG_LIB"):          # the same tests against another build of the library
        _lib.SO_PATH = os.path.abspath(os.environ["ST3D_DIAG_LIB"])
    return o


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@pytest.fixture(scope="module")
def full():
    """tap activations of the eight 512^2 images (style1, 3, 4, 5 plain, then the same on white)"""
    t0 = time.time()
    taps = G.tap_activations(G.style_images(512))
    print(f"\n  CPU VGG forward of eight 512^2 images: {time.time() - t0:.1f} s")
    return taps


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0, n0 = time.time(), G.FP64_FLOPS[0]
    yield
    print(f"\n  fp64 Gram work of the module: {(G.FP64_FLOPS[0] - n0) / 1e9:.0f} GFLOP; module wall time {time.time() - t0:.0f} s")
    for k, v in sorted(WORST.items()):
        print(f"  GPU worst err/(u M) {k}: {v:.2f}")


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


def _axpy(ops, a, b, coef, out=None, gated=False):
    acc = 1
    if out is None:
        out, acc = torch.empty_like(a), 0
    ops.call("st3d_axpy_diff_gated" if gated else "st3d_axpy_diff", ops.dptr(a), ops.dptr(b), a.numel(), float(coef), acc,
             ops.dptr(out), ops.stream_ptr())
    return out


# ================================================================================================ (a) exact operands
def _int_feat(shape, gen, top=3):
    """values in {0 .. top} with half the entries zeroed"""
    f = torch.randint(0, top + 1, shape, generator=gen)
    return (f * torch.randint(0, 2, shape, generator=gen)).float()


def _int_gram(f):
    x = f.flatten(2).double()                  # (integers below 2^53: exact, and BLAS-fast)
    return torch.bmm(x, x.transpose(1, 2))


FWD_SHAPES = ([(B, C, 1 << (18 - 2 * l)) for B in (1, 3, 8) for l, C in enumerate(TAP_C)] +
              [(1, 64, 1 << 20), (1, 128, 1 << 20)] +
              [(2, C, HW) for C, HW in zip(TAP_C, (8100, 2025, 484, 121, 25))] +
              [(2, 96, 484), (1, 320, 1024), (2, 320, 121), (2, 64, 1), (1, 128, 31), (1, 256, 31), (1, 512, 1)])


def _exact_fwd(ops, dev, shapes, multi):
    gen = torch.Generator().manual_seed(11)
    for B, C, HW in shapes:
        f = _int_feat((B, C, HW), gen, top=2 if HW >= 1 << 20 else 3)
        want = _int_gram(f)
        assert int(want.max()) < 1 << 24
        fd = f.to(dev)
        got = ops.gram_fwd_multi([fd])[0] if multi else ops.gram_fwd(fd)
        assert torch.equal(got.cpu().double(), want), ("gram_fwd_multi" if multi else "gram_fwd", B, C, HW)
        del fd, got


def test_exact_gram_forward(dev, ops, lib):
    for B, C, HW in FWD_SHAPES:           # the Python restatement of gram_split against the library's own
        assert lib.st3d_gram_workspace_bytes(B, C, HW) == G.gram_workspace_bytes(B, C, HW), (B, C, HW)
    _exact_fwd(ops, dev, FWD_SHAPES, multi=False)


@pytest.mark.parametrize("scale", [None, "1", "4"])
def test_exact_gram_forward_multi(dev, ops, monkeypatch, scale):
    """the five taps of a step in one launch (default scale 2, and ST3D_GRAM_MULTI_SCALE = 1 / 4), B = 1, 3, 8; items the
    fused kernel has no body for (odd maps, C = 96 / 320) ride along in the same call"""
    if scale is None:
        monkeypatch.delenv("ST3D_GRAM_MULTI_SCALE", raising=False)
    else:
        monkeypatch.setenv("ST3D_GRAM_MULTI_SCALE", scale)
    gen = torch.Generator().manual_seed(12)
    for B in (1, 3, 8):
        feats = [_int_feat((B, C, 1 << (18 - 2 * l)), gen) for l, C in enumerate(TAP_C)]
        extra = [_int_feat((B, 96, 484), gen), _int_feat((B, 64, 8100), gen)] if B == 3 else []
        got = ops.gram_fwd_multi([f.to(dev) for f in feats + extra])
        for f, g in zip(feats + extra, got):
            assert torch.equal(g.cpu().double(), _int_gram(f)), (B, tuple(f.shape))
    _exact_fwd(ops, dev, [(1, 64, 1 << 20), (2, 512, 25), (2, 64, 1), (1, 128, 31)], multi=True)


BWD_SHAPES = ([(B, C, 1 << (18 - 2 * l)) for B in (1, 3, 8) for l, C in enumerate(TAP_C)] +
              [(1, 64, 1 << 20)] + [(2, C, HW) for C, HW in zip(TAP_C, (8100, 2025, 484, 121, 25))] +
              [(2, 96, 484), (1, 320, 1024), (2, 320, 121), (2, 64, 1), (1, 128, 31), (1, 512, 1)])


def _exact_bwd(ops, dev, shapes, seed=13):
    """out = base + coef D F with integer F, D, base and coef = 2 (exact in every order: |sum| <= 2 * 4 * 3 * 512 + 8);
    the plain entry point with a NON-symmetric D, the gated one with a symmetric D, each with and without a base"""
    gen = torch.Generator().manual_seed(seed)
    for B, C, HW in shapes:
        f = _int_feat((B, C, HW), gen)
        base = torch.randint(-8, 9, (B, C, HW), generator=gen).float()
        D = torch.randint(-4, 5, (B, C, C), generator=gen)
        Ds = D + D.transpose(1, 2)
        fd, based = f.to(dev), base.to(dev)
        for gated in ((False, True) if C % 32 == 0 else (False,)):
            Dm = Ds if gated else D
            want = 2 * torch.bmm(Dm.double(), f.double())
            open_ = (f > 0).double() if gated else 1
            Dd = Dm.float().to(dev).contiguous()
            got = ops.gram_bwd(Dd, fd, 2.0, gated=gated)
            assert torch.equal(got.cpu().double(), want * open_), ("gram_bwd", gated, B, C, HW)
            got = ops.gram_bwd(Dd, fd, 2.0, out=based.clone(), gated=gated)
            assert torch.equal(got.cpu().double(), (want + base.double()) * open_), ("gram_bwd accumulate", gated, B, C, HW)
        del fd, based


def test_exact_gram_backward(dev, ops, monkeypatch):
    monkeypatch.delenv("ST3D_GRAM_BWD_MT", raising=False)
    _exact_bwd(ops, dev, BWD_SHAPES)


@pytest.mark.parametrize("mt", ["1", "2", "3", "4"])
def test_exact_gram_backward_forced_tiles(dev, ops, monkeypatch, mt):
    monkeypatch.setenv("ST3D_GRAM_BWD_MT", mt)
    _exact_bwd(ops, dev, [(1, 64, 1 << 14), (2, 128, 1 << 12), (3, 256, 1 << 10), (1, 512, 4096), (2, 512, 121), (2, 96, 484),
                          (1, 320, 1024), (1, 128, 31)])


def test_exact_sqdiff_axpy_and_conv1_bwd(dev, ops):
    gen = torch.Generator().manual_seed(14)
    # squared-difference sums: a, b in {-1, 0, 1}, scales 1, 2, 4, weights 1 and 2: every partial, every slot and the
    # weighted total are integers below 2^24
    items, want, wantD = [], [0, 0, 0], []
    for k, (n, nb, slot) in enumerate([(8 * 512 * 64, 8 * 512 * 64, 1), (8 * 64 * 64, 64 * 64, 2), (8 * 128 * 128, 128 * 128, 2),
                                       (3 * 256 * 256, 3 * 256 * 256, 2), (2 * 512 * 512, 512 * 512, 2), (500003, 500003, 2)]):
        a = torch.randint(-1, 2, (n,), generator=gen)
        b = torch.randint(-1, 2, (nb,), generator=gen)
        d = a - b.repeat(n // nb)
        scale = 2.0 ** (k % 3)
        items.append((a.float().to(dev), b.float().to(dev), scale, slot, k != 0))
        want[slot] += int((d * d).sum()) * scale
        wantD.append(d)
        one = ops.sqdiff_sum(items[-1][0], items[-1][1], scale, want_diff=True)
        assert float(one[0]) == int((d * d).sum()) * scale and torch.equal(one[1].cpu().long(), d), ("sqdiff_sum", k)
    out, diffs = ops.sqdiff_sum_multi(items, True, True, 2.0, 1.0)
    assert diffs[0] is None
    for d, w in zip(diffs[1:], wantD[1:]):
        assert torch.equal(d.cpu().long(), w)
    assert out.tolist() == [want[1] + 2.0 * want[2], want[1], want[2]] and want[1] + 2.0 * want[2] < 1 << 24
    out2, _ = ops.sqdiff_sum_multi(items[:2], False, False, 4.0, 0.5, out=torch.tensor([7.0, 1.0, 2.0], device=dev))
    s0 = int((wantD[0] ** 2).sum()) * items[0][2]
    s1 = int((wantD[1] ** 2).sum()) * items[1][2]
    assert out2.tolist() == [7.0, 1.0 + s0, 2.0 + s1]
    # content term
    for n in (1, 31, 8 * 512 * 64 * 64):
        a = _int_feat((n,), gen).to(dev)
        b = torch.randint(-3, 4, (n,), generator=gen).float().to(dev)
        g0 = torch.randint(-8, 9, (n,), generator=gen).float().to(dev)
        for gated in (False, True):
            gate = (a > 0).float() if gated else 1.0
            assert torch.equal(_axpy(ops, a, b, 0.5, gated=gated), 0.5 * (a - b) * gate), ("axpy_diff", gated, n)
            assert torch.equal(_axpy(ops, a, b, 0.5, out=g0.clone(), gated=gated), (g0 + 0.5 * (a - b)) * gate)
    # the fused bottom of the backward: st3d_conv3x3_pack is a pure re-layout of the weights (pack_kernel copies), so small
    # integer weights stay integers: |t| <= 8 + 2 * 4 * 3 * 64, |gx| <= 64 * 9 * 2 * |t| < 2^24
    for N, H, W in ((1, 512, 512), (3, 90, 90), (2, 5, 6), (1, 1, 2)):
        f = _int_feat((N, 64, H, W), gen)
        gy = torch.randint(-8, 9, (N, 64, H, W), generator=gen).float()
        D = torch.randint(-4, 5, (N, 64, 64), generator=gen).float()
        w = torch.randint(-2, 3, (64, 3, 3, 3), generator=gen).float()
        _, wd = ops.conv3x3_pack(w.to(dev))
        for g_, D_ in ((gy, D), (None, D), (gy, None)):
            ref, _ = R.conv1_bwd_ref(g_, f, D_, 2.0, w)
            assert float(ref.abs().max()) < 1 << 24
            got = ops.conv1_bwd(None if g_ is None else g_.to(dev), f.to(dev), None if D_ is None else D_.to(dev), 2.0, wd)
            assert torch.equal(got.cpu().double(), ref), ("conv1_bwd", N, H, W, g_ is not None, D_ is not None)


# the switches a process reads once: one fresh child per setting runs the exact checks above on a short shape list
_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import torch
import test_gpu_loss_tail as T
from st3d import _lib, ops
import os
if os.environ.get("ST3D_DIAG_LIB"):
    _lib.SO_PATH = os.path.abspath(os.environ["ST3D_DIAG_LIB"])
dev = torch.device("cuda:0")
fwd = [(1, 64, 1 << 18), (3, 128, 1 << 14), (8, 256, 1 << 12), (1, 512, 4096), (3, 512, 1024), (2, 64, 8100), (2, 320, 121), (1, 128, 31)]
T._exact_fwd(ops, dev, fwd, multi=False)
T._exact_fwd(ops, dev, fwd, multi=True)
feats = [T._int_feat((3, C, 1 << (14 - 2 * l)), torch.Generator().manual_seed(l)) for l, C in enumerate(T.TAP_C)]
for f, g in zip(feats, ops.gram_fwd_multi([f.to(dev) for f in feats])):
    assert torch.equal(g.cpu().double(), T._int_gram(f)), tuple(f.shape)
T._exact_bwd(ops, dev, [(1, 64, 1 << 14), (2, 128, 1 << 12), (3, 256, 1 << 10), (1, 512, 4096), (2, 512, 121), (2, 96, 484), (1, 128, 31)])
torch.cuda.synchronize()
print("child ok")
"""


def test_exact_under_the_once_per_process_switches():
    """ST3D_GRAM_FAST=0, ST3D_GRAM_DIAG_TRI=0, ST3D_GRAM_MULTI=0, ST3D_GRAM_MULTI_DEAL=1, ST3D_GRAM_BWD_SYM=0 and
    ST3D_GRAM_BWD_K64=1 are function-local statics: each gets a fresh child process, one at a time, each with its own
    time limit; the next one is not started after a failure"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    for setting in ("ST3D_GRAM_FAST=0", "ST3D_GRAM_DIAG_TRI=0", "ST3D_GRAM_MULTI=0", "ST3D_GRAM_MULTI_DEAL=1", "ST3D_GRAM_BWD_SYM=0",
                    "ST3D_GRAM_BWD_K64=1"):
        k, v = setting.split("=")
        env = dict(os.environ)
        env[k] = v
        p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "child ok" in p.stdout, f"{setting}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


# ================================================================================================ (b) real operands
def _check(rows, kernel, name, got, ref, M, kappa, glob=GLOB):
    r = G.report(got, ref, M)
    _note(kernel, r["ratio"])
    ok = r["ratio"] <= kappa and r["glob"] <= glob
    print(f"  {kernel:14s} {name:44s} err/(uM) {r['ratio']:8.2f} at {str(r['loc']):22s} (kappa {kappa:6.1f})   err/max|ref| {r['glob']:.2e}")
    if not ok:
        rows.append(f"{kernel} {name}: err/(uM) {r['ratio']:.1f} at {r['loc']} (kappa {kappa:.1f}), err/max|ref| {r['glob']:.2e}")
    return r


def _fwd_check(rows, ops, dev, name, A, white_idx, multi_scale=None):
    """one Gram launch of the batch A (n, C, H, W) against fp64, image by image (the white ones have their own kappa)"""
    B, C, HW = A.shape[0], A.shape[1], A[0, 0].numel()
    ref, M = G.gram_ref(A)
    Ad = A.to(dev)
    got = (ops.gram_fwd_multi([Ad])[0] if multi_scale else ops.gram_fwd(Ad)).cpu()
    assert torch.equal(got, got.transpose(1, 2)), (name, "G != G^T")
    assert bool((got[ref == 0] == 0).all()), (name, "a dead channel's entry is not an exact zero")
    for white in (False, True):
        idx = [i for i in range(B) if (i in white_idx) == white]
        if idx:
            _check(rows, "gram_fwd_multi" if multi_scale else "gram_fwd", f"{name} C={C} HW={HW} B={B}{' white' if white else ''}", got[idx],
                   ref[idx], M[idx], G.kappa_fwd(B, C, HW, G.multi_scale(C, HW, multi_scale) if multi_scale else 1, white))
    return got


def test_real_gram_forward(dev, ops, full, monkeypatch):
    monkeypatch.delenv("ST3D_GRAM_MULTI_SCALE", raising=False)
    rows = []
    gen = torch.Generator().manual_seed(21)
    white8 = (4, 5, 6, 7)
    for m in G.STYLE_TAPS:
        _fwd_check(rows, ops, dev, "real 512^2", full[m], white8)                                  # config 2: B = 8
        _fwd_check(rows, ops, dev, "real 512^2 (multi)", full[m], white8, multi_scale=2)
        _fwd_check(rows, ops, dev, "real 512^2", full[m][[1]], ())                          # B = 1: the style target's split
        _fwd_check(rows, ops, dev, "real 512^2", full[m][[6]], (0,))
        _fwd_check(rows, ops, dev, "real 512^2", full[m][[0, 5, 2]], (1,))                         # B = 3
        _fwd_check(rows, ops, dev, "chscale 512^2", G.chscale(full[m][[0, 3]], gen), ())
    c = R.style_crops(96, 256)
    crops = G.tap_activations(torch.cat([c, R.on_white(c)]))
    odd = G.tap_activations(G.style_images(90))
    for m in G.STYLE_TAPS:
        _fwd_check(rows, ops, dev, "real 96x256", crops[m], white8)
        _fwd_check(rows, ops, dev, "real S=90", odd[m], white8)
        _fwd_check(rows, ops, dev, "real S=90 (multi)", odd[m], white8, multi_scale=2)
        _fwd_check(rows, ops, dev, "relu(randn+1)", G.relu_shift(crops[m][:2].shape, gen), ())
    big = G.tap_activations(G.mirror_tiled(R.style_crops(512, 512)[1])[None], upto=5)               # config 3: HW = 2^20
    _fwd_check(rows, ops, dev, "real 1024^2", big[0], ())
    _fwd_check(rows, ops, dev, "real 1024^2", big[5], ())
    bigw = R.vgg_activations(R.on_white(G.mirror_tiled(R.style_crops(512, 512)[2]))[None], upto=0)[0][3]
    _fwd_check(rows, ops, dev, "real 1024^2", bigw, (0,))
    assert not rows, "\n".join(rows)


def _bwd_check(rows, ops, dev, name, D, A, coef, base, gated):
    ref, M = G.gram_bwd_ref(D, A, coef, base, gated)
    got = ops.gram_bwd(D.to(dev).contiguous(), A.to(dev), coef, out=None if base is None else base.to(dev).clone(), gated=gated).cpu()
    assert bool((got[M == 0] == 0).all()), (name, "an output with no terms (closed gate, dead rows) is not an exact zero")
    C = A.shape[1]
    return _check(rows, "gram_bwd_gated" if gated else "gram_bwd", f"{name} C={C} HW={A[0, 0].numel()} B={A.shape[0]}", got, ref, M,
                  G.kappa_bwd(C))


def test_real_gram_backward(dev, ops, full):
    """far D = G(image a) - G(image b) and near D = G(F) - G(F'), both Grams made by the kernel under test; plain entry
    point also with a dense non-symmetric D; with and without a base; real and channel-scaled activations"""
    rows = []
    gen = torch.Generator().manual_seed(22)
    for m in G.STYLE_TAPS:
        sel = [0, 6] if m == 0 else [0, 1, 6, 7]                      # relu1_1: two images (fp64 CPU cost)
        A = full[m][sel]
        C, H = A.shape[1], A.shape[2]
        coef = 4.0 * 1e6 * G.style_norm(C, H, 8)
        g = ops.gram_fwd(A.to(dev)).cpu()
        far = g - g.roll(1, 0)
        nearD = g - ops.gram_fwd(G.near(A, 1e-2, gen).to(dev)).cpu()
        base = torch.randn(A.shape, generator=gen) * float(coef * torch.bmm(far.abs(), A.flatten(2)).mean())
        for gated in (False, True):
            _bwd_check(rows, ops, dev, "far", far, A, coef, None, gated)
            _bwd_check(rows, ops, dev, "near 1e-2 + base", nearD, A, coef, base, gated)
        Ac = G.chscale(A[:2], gen)
        gc = ops.gram_fwd(Ac.to(dev)).cpu()
        _bwd_check(rows, ops, dev, "chscale far", gc - gc.roll(1, 0), Ac, coef * 1e-6, None, True)
        dense = torch.randn(2, C, C, generator=gen) * float(far.abs().mean())
        _bwd_check(rows, ops, dev, "dense non-symmetric D", dense, A[:2], coef, base[:2], False)
    odd = G.tap_activations(G.style_images(90)[[0, 5]])
    for m in G.STYLE_TAPS:
        A = odd[m]
        C, H = A.shape[1], A.shape[2]
        g = ops.gram_fwd(A.to(dev)).cpu()
        for gated in (False, True):
            _bwd_check(rows, ops, dev, "S=90 far", g - g.roll(1, 0), A, 4.0 * 1e6 * G.style_norm(C, H, 2), None, gated)
    assert not rows, "\n".join(rows)


def test_real_sqdiff_sums(dev, ops, full):
    """the six sums of a config-2 step on real Grams (style target broadcast) and the real content term: value within the
    derived bound sqdiff_kappa(n) u of itself, D == fl(a - b) bitwise"""
    gen = torch.Generator().manual_seed(23)
    sw, cw, bd = 1e6, 1.0, 8.0
    cact = full[G.CONTENT_TAP]
    ctgt = G.near(cact, 0.05, gen)
    chw = cact[0].numel()
    items = [(cact.to(dev), ctgt.to(dev), 1.0 / (bd * chw), 1, False)]
    want = [0.0, 0.0, 0.0]
    bound = [0.0, 0.0, 0.0]
    s, _ = G.sqdiff_ref(cact, ctgt, 1.0 / (bd * chw))
    want[1], bound[1] = s, G.sqdiff_kappa(cact.numel()) * R.U32 * s
    gs = []
    for m in G.STYLE_TAPS:
        A = full[m]
        g = ops.gram_fwd(A.to(dev))
        S = ops.gram_fwd(G.near(A[6:7], 1e-2, gen).to(dev))
        norm = G.style_norm(A.shape[1], A.shape[2], bd)
        items.append((g, S, norm, 2, True))
        s, d = G.sqdiff_ref(g.cpu(), S.cpu(), norm)
        want[2] += s
        bound[2] += G.sqdiff_kappa(g.numel()) * R.U32 * s
        gs.append((g, S))
    out, diffs = ops.sqdiff_sum_multi(items, True, True, sw, cw)
    out = out.cpu().double().tolist()
    for (g, S), d in zip(gs, diffs[1:]):
        assert torch.equal(d, g - S)
    want[0] = cw * want[1] + sw * want[2]
    bound[0] = cw * bound[1] + sw * bound[2] + 3 * R.U32 * want[0]
    for k, nm in enumerate(("total", "content", "style")):
        err = abs(out[k] - want[k])
        _note("sqdiff_multi", err / (R.U32 * want[k]))
        print(f"  sqdiff_sum_multi {nm:8s} {out[k]:.9e}  err {err / (R.U32 * want[k]):6.2f} u (bound {bound[k] / (R.U32 * want[k]):.1f} u)")
        assert err <= bound[k], (nm, out[k], want[k])


# ================================================================================================ (c) the composed tail
def _tail_gpu(ops, dev, acts, cact, style_grams, ctgt, sw, cw, bd, gated):
    """Gram -> sqdiff_sum_multi -> gram_bwd[_gated] / axpy_diff through ops, as plan_loss_enqueue chains them"""
    n = acts[0].shape[0]
    grams = ops.gram_fwd_multi(acts)
    chw = cact[0].numel()
    items = [(cact, ctgt, 1.0 / (bd * chw), 1, False)]
    coefs = []
    for A, g, S in zip(acts, grams, style_grams):
        norm = G.style_norm(A.shape[1], A.shape[2], bd)
        items.append((g, S, norm, 2, True))
        coefs.append(4.0 * sw * norm)
    loss, D = ops.sqdiff_sum_multi(items, True, True, sw, cw)
    grads = [ops.gram_bwd(d, A, c, gated=l in gated) for l, (d, A, c) in enumerate(zip(D[1:], acts, coefs))]
    cgrad = _axpy(ops, cact, ctgt, 2.0 * cw / (bd * chw))
    return loss, grams, D[1:], grads, cgrad


def _style_loss_bound(t, grams_gpu, S_gpu, Sref, kG, kS, bd):
    """|d style| <= sum_l norm_l (sum 2 |D| dD + dD^2 + kappa_sq u sum D_gpu^2), dD = kappa_G u M_G + kappa_S u M_S + u |D_gpu|
    (the Gram bounds of (b) pushed through D = G - S and the squares; everything in fp64)"""
    tot, dDs = 0.0, []
    for l, (g, S) in enumerate(zip(grams_gpu, S_gpu)):
        C, H = t["shapes"][l]
        Dg = g.cpu().double() - S.cpu().double()
        dD = R.U32 * (kG[l] * t["MG"][l] + kS[l] * Sref[l][1].expand_as(t["MG"][l]) + Dg.abs())
        tot += G.style_norm(C, H, bd) * float((2 * t["D"][l].abs() * dD + dD * dD).sum() + G.sqdiff_kappa(g.numel()) * R.U32 * (Dg * Dg).sum())
        dDs.append(dD)
    return tot, dDs


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
def test_near_converged_tail_composed(dev, ops, full, eps, monkeypatch):
    """current = the eight 512^2 images' activations, style = those of F' = relu(F (1 + eps randn)) of the first image on
    white: D is a small difference of large numbers.  Loss triple and the gradient leaving every tap against the fp64 tail
    on the same fp32 activations; the bounds are derived from the per-element Gram bounds, the observed error / bound is
    printed."""
    monkeypatch.delenv("ST3D_GRAM_MULTI_SCALE", raising=False)
    gen = torch.Generator().manual_seed(31)
    sw, cw, bd = 1e6, 1.0, 8.0
    sel = [6, 4, 5, 7, 6, 4, 5, 7]                           # eight views of white-surround images, as a render batch
    acts = [full[m][sel] for m in G.STYLE_TAPS]
    # every view close to ITS OWN target: per-image style Grams (style_batch == n) of the perturbed activations
    sacts = [G.near(a, eps, gen) for a in acts]
    cact = full[G.CONTENT_TAP][sel]
    ctgt = G.near(cact, eps, gen)
    gated = (1, 2, 3, 4)                                    # the plan gates every tap but relu1_1 (fused into conv1_bwd)
    S_gpu = ops.gram_fwd_multi([a.to(dev) for a in sacts])
    Sref = [G.gram_ref(a) for a in sacts]
    t = G.tail_ref(acts, cact, [s[0] for s in Sref], ctgt, sw, cw, bd, gated=gated, want_grads=False)
    dacts = [a.to(dev) for a in acts]
    loss, grams, D, grads, cgrad = _tail_gpu(ops, dev, dacts, cact.to(dev), S_gpu, ctgt.to(dev), sw, cw, bd, gated)
    kG = [G.kappa_fwd(8, a.shape[1], a[0, 0].numel(), 2, white=True) for a in acts]
    sb, dDs = _style_loss_bound(t, grams, S_gpu, Sref, kG, kG, bd)
    cb = G.sqdiff_kappa(cact.numel()) * R.U32 * t["loss"][1]
    bounds = [cw * cb + sw * sb + 3 * R.U32 * t["loss"][0], cb, sb]
    got = loss.cpu().double().tolist()
    for k, nm in enumerate(("total", "content", "style")):
        err = abs(got[k] - t["loss"][k])
        print(f"  near {eps:g} composed  {nm:8s} {got[k]:.6e} (fp64 {t['loss'][k]:.6e})  rel err {err / t['loss'][k]:.2e}  err/bound {err / bounds[k]:.3f}")
        assert err <= bounds[k], (nm, got[k], t["loss"][k], bounds[k])
    # gradients: |err| <= |coef| (dD |F|) + kappa_bwd u |coef| |D_gpu| |F|   (+ 1 u of coef's own rounding in kappa_bwd's + 2)
    for l, (A, gr) in enumerate(zip(acts, grads)):
        C = A.shape[1]
        worst = 0.0
        for i in range(0, 8, 2):                              # in pairs of images: fp64 memory
            s = slice(i, i + 2)
            ref, _ = G.gram_bwd_ref(t["D"][l][s], A[s], t["coef"][l], gated=l in gated)
            f = A[s].double().flatten(2)
            bnd = abs(t["coef"][l]) * (torch.bmm(dDs[l][s], f) + G.kappa_bwd(C) * R.U32 * torch.bmm(D[l][s].cpu().double().abs(), f))
            err = (gr[s].cpu().double() - ref).flatten(2).abs()
            assert bool((err[bnd == 0] == 0).all())
            worst = max(worst, float((err / bnd.clamp_min(1e-300)).max()))
        print(f"  near {eps:g} composed  gradient leaving tap {l} (C={C}): worst err/bound {worst:.3f}")
        assert worst <= 1.0, (l, worst)
    ref = t["content_grad"]
    assert float(((cgrad.cpu().double() - ref).abs() - 3 * R.U32 * ref.abs()).max()) <= 0
    # the bottom of the backward as the plan runs it: relu1_1's style gradient, gate and conv1_1^T in one pass (st3d_conv1_bwd)
    # on the kernel's own D, against _convref's reference and direct-conv bound (as tests/test_gpu_conv_accuracy.py does on crops)
    from oracle import perceptual_ref as P
    w = P.make_vgg19_features(seed=0)._modules["0"].weight.detach()
    _, wd = ops.conv3x3_pack(w.to(dev))
    gx = ops.conv1_bwd(None, dacts[0][:2].contiguous(), D[0][:2].contiguous(), t["coef"][0], wd).cpu()
    ref, M = R.conv1_bwd_ref(None, acts[0][:2], D[0][:2].cpu(), t["coef"][0], w)
    r = G.report(gx, ref, M)
    _note("conv1_bwd", r["ratio"])
    print(f"  near {eps:g} composed  conv1_bwd on D of relu1_1: err/(uM) {r['ratio']:.2f} at {r['loc']} (kappa {R.KAPPA_DIRECT:g})   err/max|ref| {r['glob']:.2e}")
    assert r["ratio"] <= R.KAPPA_DIRECT and r["glob"] <= 3e-5


@pytest.mark.parametrize("n", [1, 4])
def test_near_converged_tail_through_the_plan(dev, ops, n):
    """plan.set_style(noisy image), plan.loss(image) at S = 256: the fp64 tail is computed from the plan's OWN tap
    activations (read back), so the conv kernels' error stays out; only the loss triple is compared.  Then
    current == style bit for bit: with n == style_batch == 1 both Grams take the same splits and the style loss is
    EXACTLY 0; with n = 4 the style Gram is made at B = 1 and the current ones at B = 4 (other splits), so G - S is
    rounding noise within the derived bound: the floor a converged run sits on, printed relative to the content term."""
    from st3d import vgg as V
    S, sw, cw = 256, 1e6, 1.0
    gen = torch.Generator().manual_seed(41 + n)
    img = G.style_images(S)[[6, 4, 5, 7][:n]]
    style = (img[:1] * (1.0 + 1e-2 * torch.randn(img[:1].shape, generator=gen))).clamp(0, 1)
    content = (img * (1.0 + 1e-2 * torch.randn(img.shape, generator=gen))).clamp(0, 1)
    vgg = V.get_vgg(seed=0, device=dev)
    plan = vgg.plan(n, S)
    try:
        def taps_of(x):
            plan.forward(x.to(dev))
            return [plan.activation(m).cpu().clone() for m in G.STYLE_TAPS], plan.activation(G.CONTENT_TAP).cpu().clone()
        gnear = None
        same = img[:1].repeat(n, 1, 1, 1)
        for case, sty, cur, con in (("near", style, img, content), ("equal", img[:1], same, same)):
            sacts, _ = taps_of(sty)
            _, ctgt = taps_of(con)
            sd, cd, imd = sty.to(dev), con.to(dev), cur.to(dev)
            plan.set_content(cd, force=True)
            plan.set_style(sd, n, force=True)
            loss, grad = plan.loss(imd, sw, cw, want_grad=True)
            got = loss.cpu().double().tolist()
            acts = [plan.activation(m).cpu().clone() for m in G.STYLE_TAPS]
            cact = plan.activation(G.CONTENT_TAP).cpu().clone()
            Sref = [G.gram_ref(a) for a in sacts]
            t = G.tail_ref(acts, cact, [s[0] for s in Sref], ctgt, sw, cw, float(n), want_grads=False)
            # the plan does not expose its Grams: the bound is built on the reference D,
            # dD = dG + dS + u (|D| + dG + dS) with dG = kappa_G u M_G, dS = kappa_S u M_S
            sb = 0.0
            for l, a in enumerate(acts):
                C, H, HW = a.shape[1], a.shape[2], a[0, 0].numel()
                dG = G.kappa_fwd(n, C, HW, 2, white=True) * R.U32 * t["MG"][l]
                dS = G.kappa_fwd(1, C, HW, 2, white=True) * R.U32 * Sref[l][1].expand_as(dG)
                dD = dG + dS + R.U32 * (t["D"][l].abs() + dG + dS)
                sq = float((2 * t["D"][l].abs() * dD + dD * dD).sum())
                sb += G.style_norm(C, H, n) * (sq + G.sqdiff_kappa(a.shape[0] * C * C) * R.U32 * (float((t["D"][l] ** 2).sum()) + sq))
            cb = G.sqdiff_kappa(cact.numel()) * R.U32 * t["loss"][1]
            bounds = [cw * cb + sw * sb + 3 * R.U32 * t["loss"][0], cb, sb]
            for k, nm in enumerate(("total", "content", "style")):
                err = abs(got[k] - t["loss"][k])
                print(f"  plan n={n} {case:5s} {nm:8s} {got[k]:.6e} (fp64 {t['loss'][k]:.6e})  err {err:.3e}  bound {bounds[k]:.3e}")
                assert err <= bounds[k], (case, nm, got[k], t["loss"][k], bounds[k])
            gn = float(grad.double().norm())
            if case == "near":
                gnear = gn
            else:
                # current == style == content bit for bit: the fp64 tail is 0 (the style term up to fp64 rounding of two
                # differently batched fp64 products)
                assert t["loss"][1] == 0.0 and got[1] == 0.0 and t["loss"][2] < 1e-24
                print(f"  plan n={n} current == style: style loss x weight {sw * got[2]:.3e}, |grad| {gn:.3e}"
                      f" (1e-2 away: loss {near_total:.3e}, |grad| {gnear:.3e})")
                if n == 1:              # the same splits on both sides: every D is exactly 0
                    assert got == [0.0, 0.0, 0.0] and float(grad.abs().max()) == 0.0
            near_total = got[0]
    finally:
        plan.close()


# ================================================================================================ (d) invariances
def _poison(dev, value):
    """leave freed blocks full of `value` in the caching allocator, in the sizes the workspaces below ask for"""
    junk = [torch.full((n,), value, dtype=torch.float32, device=dev) for n in (1 << 26, 1 << 24, 1 << 22, 1 << 20, 1 << 18, 1 << 16, 1 << 13)]
    del junk


def test_invariances_and_stale_workspace(dev, ops, full, monkeypatch):
    """bitwise: gram_fwd_multi at scale 1 == gram_fwd per item on the real taps; the whole tail run to run; and no result
    depends on what the recycled workspace held (NaN, 1e30): the FAST multi-tile launch leaves the lower-left 64 x 64 of its
    diagonal tiles unwritten and the reduce must not read them; the same for the partials of the sqdiff launches"""
    feats = [full[m][[0, 5, 6]].to(dev) for m in G.STYLE_TAPS]
    monkeypatch.setenv("ST3D_GRAM_MULTI_SCALE", "1")
    single = [ops.gram_fwd(f) for f in feats]
    for f, gm, gs in zip(feats, ops.gram_fwd_multi(feats), single):
        assert torch.equal(gm, gs), tuple(f.shape)
    monkeypatch.delenv("ST3D_GRAM_MULTI_SCALE")
    multi = ops.gram_fwd_multi(feats)
    S = [g[2:3].clone() for g in multi]
    cact = full[G.CONTENT_TAP][[0, 5, 6]].to(dev)
    ctgt = (cact * 0.9).contiguous()

    def tail():
        return _tail_gpu(ops, dev, feats, cact, S, ctgt, 1e6, 1.0, 3.0, (1, 2, 3, 4))

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    loss, grams, D, grads, cgrad = tail()
    assert same(grams, multi)
    for value in (float("nan"), 1e30):
        _poison(dev, value)
        assert same([ops.gram_fwd(f) for f in feats], single), f"st3d_gram_fwd read stale workspace ({value})"
        _poison(dev, value)
        l2, g2, D2, gr2, cg2 = tail()
        assert torch.equal(l2, loss) and same(g2, grams) and same(D2, D) and same(gr2, grads) and torch.equal(cg2, cgrad), value
        _poison(dev, value)
        a, b = multi[3], S[3]
        one = ops.sqdiff_sum(a, b, 0.5)
        _poison(dev, value)
        assert torch.equal(ops.sqdiff_sum(a, b, 0.5), one) and bool(torch.isfinite(one).all())


def test_sqdiff_multi_is_the_folded_single_launches(dev, ops, full):
    """st3d_sqdiff_sum_multi == six st3d_sqdiff_sum launches folded in order into their slots, bitwise, for every
    (zero_first, combine) and a non-zero starting loss_out3; broadcast and per-image style targets"""
    gen = torch.Generator().manual_seed(51)
    sw, cw = 1e6, 0.75
    cact = full[G.CONTENT_TAP][[0, 6]].to(dev)
    items = [(cact, G.near(full[G.CONTENT_TAP][[0, 6]], 0.05, gen).to(dev), 1.0 / cact.numel(), 1, False)]
    for l, m in enumerate(G.STYLE_TAPS):
        g = ops.gram_fwd(full[m][[0, 6]].to(dev))
        S = ops.gram_fwd(G.near(full[m][[0, 6]], 1e-2, gen).to(dev))
        items.append((g, S[:1].contiguous() if l % 2 else S, G.style_norm(g.shape[1], full[m].shape[2], 2.0), 2, True))
    start = [3.0, 0.25, 1e-7]
    for zero_first in (False, True):
        for combine in (False, True):
            out, diffs = ops.sqdiff_sum_multi(items, zero_first, combine, sw, cw, out=torch.tensor(start, device=dev))
            slots = [torch.zeros(1, device=dev) if zero_first else torch.tensor([v], device=dev) for v in start]
            for (a, b, scale, slot, want), d in zip(items, diffs):
                parts = torch.empty((ops._lib.load().st3d_reduce_partials(),), dtype=torch.float32, device=dev)
                Dk = torch.empty_like(a) if want else None
                ops.call("st3d_sqdiff_sum", ops.dptr(a), ops.dptr(b), a.numel(), b.numel(), float(scale), ops.dptr(Dk), ops.dptr(parts),
                         ops.dptr(slots[slot]), ops.stream_ptr())
                assert (d is None and Dk is None) or torch.equal(d, Dk)
            want3 = [float(s) for s in slots]
            if combine:
                want3[0] = float(torch.tensor(cw) * slots[1].cpu() + torch.tensor(sw) * slots[2].cpu())
            assert out.cpu().tolist() == want3, (zero_first, combine, out.cpu().tolist(), want3)
