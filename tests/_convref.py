"""fp64 references, per-element error bounds, fp32 Winograd emulations and realistic operands for the conv kernels.

A kernel result `got` (fp32) of an operation with fp64 reference `ref` passes when, element by element,

    |got - ref| <= kappa * u * M,        u = 2^-24,

where M is the operation's magnitude at that element:

    algorithm      M                                                          kappa                 CPU fp32 measurement
    direct         |x| (*) |w| + |b|  (input gradient: conv^T(|g|, |w|))     KAPPA_DIRECT = 21     torch conv2d:   5.3
    F(2x2,3x3)     the direct M max-pooled over the 2x2 output tile           KAPPA_F2     = 30     emulation:      7.6
    F(4x4,3x3)     the direct M max-pooled over the 4x4 output tile           KAPPA_F4     = 368    emulation:      92

(tiles aligned to the origin, as the kernels tile: rounding leaks across the outputs a Winograd tile computes together).
Each kappa is the worst err/(u M) measured on the CPU over every operand family of tests/test_convref.py -- torch's own
fp32 conv2d for the direct bound, the fp32 emulations below for the Winograd bounds -- times a margin of at most 4
(tests/test_convref.py::test_fp32_cpu_results_meet_the_bounds re-measures them; oneDNN picks its blocking per CPU, so the
figures move a little from host to host).  M is summed over non-negative terms, so
its own fp32 rounding (relative K u) is far below anything the bound resolves; it is computed in fp64 all the same.

The unit-less global figure err / max|ref| (the suite's older `_scale_close` criterion) is reported next to it: it cannot
see an error confined to a region or a channel whose magnitude is 10^3 below the tensor's maximum, which is where real
activations put most of their outputs.

Operand families (seeded, CPU): the style images of tests/golden (values in [0, 1]) and the same crops composited onto a
white 1.0 background, the inputs of every conv layer of the seeded VGG (oracle.perceptual_ref) on those images, relu(randn
+ 1), the near-constant 1 + 1e-3 randn, the seeded weights and a variant with every filter's mean shifted by 0.5 std, and
gradients that are ReLU-gated, scattered through a 2x2 unpool, Gram-backward terms coef D F, or channel-scaled by
10^U(-3, 3)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24

# worst err/(u M) of the CPU fp32 results over every family of tests/test_convref.py, and the bounds derived from them
MEASURED_CPU = {"direct": 5.3, "f2": 7.6, "f4": 92.0}
KAPPA_DIRECT = 21.0
KAPPA_F2 = 30.0
KAPPA_F4 = 368.0
KAPPA = {"direct": KAPPA_DIRECT, "f2": KAPPA_F2, "f4": KAPPA_F4}
TILE = {"direct": 1, "f2": 2, "f4": 4}
FP64_FLOPS = [0]              # multiply-adds x 2 of the fp64 convolutions below (the suite's CPU budget)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STYLES = ("style1", "style3", "style4", "style5")
VGG_CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)        # module indices of conv1_1 .. conv5_1


# ------------------------------------------------------------------------------------------------ fp64 references
def _d(t):
    return t.detach().double().cpu()


def _count(x, w):
    FP64_FLOPS[0] += 2 * x.shape[0] * w.shape[0] * w.shape[1] * 9 * x.shape[2] * x.shape[3]


def conv_fwd(x, w, b=None, relu=False):
    _count(x, w)
    y = F.conv2d(_d(x), _d(w), None if b is None else _d(b), padding=1)
    return y.clamp_min(0) if relu else y


def conv_dgrad(g, w):
    """input gradient of conv3x3(pad 1) for the (already gated) output gradient g"""
    _count(g, w)
    return F.conv_transpose2d(_d(g), _d(w), padding=1)


def pool_argmax(y):
    """MaxPool2d(2,2) values and the kernels' argmax byte (dy << 1 | dx, first maximum in row-major order, as ATen)"""
    y = _d(y)
    p, i = F.max_pool2d(y, 2, 2, return_indices=True)
    W = y.shape[-1]
    return p, (((i // W) % 2) * 2 + (i % W) % 2).to(torch.uint8)


def unpool(gp, idx, H, W):
    """2x2 max-unpool of a pooled-resolution gradient through the argmax bytes (odd H / W: the last row / column gets none)"""
    gp, idx = _d(gp), idx.cpu().long()
    N, C, Hp, Wp = gp.shape
    up = torch.zeros(N, C, H, W, dtype=torch.float64)
    for k in range(4):
        up[:, :, (k >> 1):2 * Hp:2, (k & 1):2 * Wp:2] = gp * (idx == k).double()
    return up


def gate_chain(gx, out_gate, add_target=None, add_coef=0.0):
    """the producer-side output of a chain link: !(out_gate <= 0) ? gx + add_coef (out_gate - add_target) : 0"""
    og = _d(out_gate)
    v = gx if add_target is None else gx + add_coef * (og - _d(add_target))
    return torch.where(og > 0, v, torch.zeros_like(v))


def conv1_bwd_ref(gy, act, D, coef, w):
    """st3d_conv1_bwd: conv1_1^T((act > 0) (gy + coef D act)); gy or D may be None.  Returns (ref, direct M)."""
    a = _d(act)
    N, C, H, W = a.shape
    af = a.reshape(N, C, H * W)
    t = torch.zeros_like(af)
    m = torch.zeros_like(af)
    if gy is not None:
        t = t + _d(gy).reshape(N, C, H * W)
        m = m + _d(gy).abs().reshape(N, C, H * W)
    if D is not None:
        t = t + coef * torch.bmm(_d(D), af)
        m = m + abs(coef) * torch.bmm(_d(D).abs(), af.abs())
    gate = (af > 0).double()
    t, m = (t * gate).reshape(N, C, H, W), (m * gate).reshape(N, C, H, W)
    return conv_dgrad(t, w), mag_dgrad(m, w)


# ------------------------------------------------------------------------------------------------ magnitudes
def mag_fwd(x, w, b=None):
    _count(x, w)
    m = F.conv2d(_d(x).abs(), _d(w).abs(), padding=1)
    return m if b is None else m + _d(b).abs().view(1, -1, 1, 1)


def mag_dgrad(g, w):
    _count(g, w)
    return F.conv_transpose2d(_d(g).abs(), _d(w).abs(), padding=1)


def tile_max(M, t):
    """M max-pooled over the t x t output tiles (aligned to the origin) and broadcast back to every element of the tile"""
    if t == 1:
        return M
    H, W = M.shape[-2:]
    p = F.max_pool2d(M, t, t, ceil_mode=True)
    return p.repeat_interleave(t, 2).repeat_interleave(t, 3)[..., :H, :W].contiguous()


def mag(M, algo):
    return tile_max(M, TILE[algo])


# ------------------------------------------------------------------------------------------------ fp32 Winograd emulations
def _bt2(d0, d1, d2, d3):
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def _at2(m0, m1, m2, m3):
    return (m0 + m1) + m2, (m1 - m2) - m3


def _bt6(d0, d1, d2, d3, d4, d5):
    """B^T of wino43.hip (bt6), the same expressions"""
    p, q = d4 - 4.0 * d2, d3 - 4.0 * d1
    r, s = d4 - d2, 2.0 * (d3 - d1)
    return 4.0 * d0 + (d4 - 5.0 * d2), p + q, p - q, r + s, r - s, 4.0 * d1 + (d5 - 5.0 * d3)


def _at6(m0, m1, m2, m3, m4, m5):
    """A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1], summed as wino43.hip's epilogue (halves b 0..2, 3..5)"""
    s0, d0 = m1 + m2, m1 - m2
    s1, d1 = m3 + m4, m3 - m4
    return (m0 + s0) + s1, d0 + 2.0 * d1, s0 + 4.0 * s1, d0 + (8.0 * d1 + m5)


_G2 = torch.tensor([[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]], dtype=torch.float64)
_G4 = torch.tensor([[0.25, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                    [1 / 24, -1 / 12, 1 / 6], [0, 0, 1.0]], dtype=torch.float64)


def _apply(fn, t, dim):
    return torch.stack(fn(*t.unbind(dim)), dim)


def wino_emul(x, w, b=None, m=4, kstep=4):
    """fp32 CPU emulation of Winograd F(m x m, 3x3) conv3x3(pad 1) (m = 2: wino.hip, m = 4: wino43.hip): U = G g G^T in fp64
    rounded to fp32 (as the packs), V = B^T d B, the products and the channel sum (kstep channels per fp32 accumulation
    step, as the MFMA k-steps) and Y = A^T M A, all in fp32 torch ops.  Input gradient: x = the gated gradient and
    w = w.flip(2, 3).transpose(0, 1), as the dgrad packs."""
    x = x.detach().float().cpu()
    w = w.detach().double().cpu()
    N, C, H, W = x.shape
    Co = w.shape[0]
    t = m + 2
    ty, tx = -(-H // m), -(-W // m)
    xp = F.pad(x, (1, tx * m + 1 - W, 1, ty * m + 1 - H))
    d = xp.unfold(2, t, m).unfold(3, t, m)                          # N C ty tx t(row) t(col)
    bt, at, G = (_bt2, _at2, _G2) if m == 2 else (_bt6, _at6, _G4)
    V = _apply(bt, _apply(bt, d, 4), 5)                             # rows, then columns (the kernels' order)
    V = V.permute(4, 5, 1, 0, 2, 3).reshape(t * t, C, N * ty * tx)  # xi C P
    U = torch.einsum("ak,oikl,bl->abio", G, w, G).reshape(t * t, C, Co).float()     # xi C Co
    acc = torch.zeros(t * t, Co, N * ty * tx)
    for k in range(0, C, kstep):
        acc += torch.bmm(U[:, k:k + kstep].transpose(1, 2), V[:, k:k + kstep])
    Mt = acc.reshape(t, t, Co, N, ty, tx).permute(3, 2, 4, 5, 0, 1)  # N Co ty tx a b
    Y = _apply(at, _apply(at, Mt, 4), 5)                            # N Co ty tx m m
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, Co, ty * m, tx * m)[:, :, :H, :W]
    if b is not None:
        Y = Y + b.detach().float().cpu().view(1, -1, 1, 1)
    return Y.contiguous()


def dgrad_weights(w):
    return w.flip(2, 3).transpose(0, 1)


# ------------------------------------------------------------------------------------------------ criterion
def report(got, ref, M):
    """worst err / (u M) with its location (n, c, y, x), and the global err / max|ref|"""
    got, ref, M = _d(got), _d(ref), _d(M)
    err = (got - ref).abs()
    if torch.isnan(got).any():
        return dict(ratio=float("inf"), loc=tuple(torch.nonzero(torch.isnan(got))[0].tolist()), glob=float("inf"))
    r = torch.where(M > 0, err / (U32 * M.clamp_min(1e-300)), torch.where(err > 0, float("inf"), 0.0))
    i = int(torch.argmax(r))
    loc = tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))
    return dict(ratio=float(r.reshape(-1)[i]), loc=loc, glob=float(err.max() / (ref.abs().max() + 1e-300)))


def within(got, ref, M, kappa):
    return report(got, ref, M)["ratio"] <= kappa


def scale_close(got, ref, rtol):
    """the suite's older global criterion (test_gpu_kernels._scale_close) as a predicate"""
    got, ref = _d(got), _d(ref)
    return float((got - ref).abs().max()) <= rtol * (float(ref.abs().max()) + 1e-30)


# ------------------------------------------------------------------------------------------------ operands
def style_crops(H, W, names=STYLES):
    """top-left H x W crops of the committed style images, (len(names), 3, H, W) in [0, 1]"""
    out = []
    for nm in names:
        rgb = np.load(os.path.join(GOLDEN, f"assets_{nm}_512.npz"))["rgb_u8"][:H, :W]
        out.append(torch.from_numpy(rgb.astype(np.float32) / 255.0).permute(2, 0, 1))
    return torch.stack(out)


def on_white(img):
    """the crops composited onto a white 1.0 background, as a rendered view: an ellipse of image, white around it"""
    H, W = img.shape[-2:]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    inside = ((yy - 0.55 * H) / (0.42 * H)) ** 2 + ((xx - 0.5 * W) / (0.4 * W)) ** 2 <= 1.0
    return torch.where(inside, img, torch.ones_like(img))


def vgg_activations(images, upto=28):
    """fp32 CPU forward of the seeded VGG (oracle.perceptual_ref.make_vgg19_features(seed=0)) on `images`: for every conv
    module index i <= upto, (input, weight, bias, post-ReLU output)"""
    from oracle import perceptual_ref as P
    model = P.make_vgg19_features(seed=0)
    out, x = {}, images.float()
    with torch.no_grad():
        for name, layer in model._modules.items():
            i = int(name)
            if i > upto:
                break
            if isinstance(layer, torch.nn.Conv2d):
                y = torch.relu(F.conv2d(x, layer.weight, layer.bias, padding=1))
                out[i] = (x, layer.weight.detach().clone(), layer.bias.detach().clone(), y)
                x = y
            elif isinstance(layer, torch.nn.MaxPool2d):
                x = F.max_pool2d(x, 2, 2)
    return out


def shifted(w):
    """every filter's mean moved by 0.5 of its std (trained filters have sum(w) != 0; the seeded ones have sum(w) ~ 0)"""
    return w + 0.5 * w.std(dim=(1, 2, 3), keepdim=True)


def input_families(real, gen):
    """name -> (1, C, H, W) fp32: two real activations (or images: plain, on white), relu(randn + 1), 1 + 1e-3 randn, randn"""
    shape = (1,) + tuple(real.shape[1:])
    return {"real": real[0:1].clone(), "real_white": real[1:2].clone(),
            "relu_shift": torch.relu(torch.randn(shape, generator=gen) + 1.0),
            "flat": 1.0 + 1e-3 * torch.randn(shape, generator=gen),
            "randn": torch.randn(shape, generator=gen)}


def grad_families(act, gen):
    """Output gradients for a conv whose post-ReLU output on the two real images is `act` (2, C, H, W): name -> dict(g =
    the gated full-resolution gradient, and for "unpool" gp / idx / pooled: the pooled-resolution gradient, the argmax
    of the activation's own 2x2 pool and its values; g = unpool(gp gated by pooled > 0))."""
    act = act.float()
    C, H, W = act.shape[1:]
    a0, a1 = act[0:1], act[1:2]
    out = {"gate": dict(g=torch.randn(a0.shape, generator=gen) * (a0 > 0), act=a0)}
    pooled, idx = pool_argmax(a1)
    pooled = pooled.float()
    gp = torch.randn(pooled.shape, generator=gen)
    out["unpool"] = dict(g=unpool(gp * (pooled > 0), idx, H, W).float(), gp=gp, idx=idx, pooled=pooled, act=a1)
    Dm = torch.randn(C, C, generator=gen, dtype=torch.float64)
    Dm = (0.5 * (Dm + Dm.T) / (C * H * W)).float()                 # a Gram difference, normalised as the style loss
    coef = 2.0 * 1e3 / C
    gd = coef * torch.einsum("cd,ndp->ncp", Dm, a0.reshape(1, C, H * W)).reshape(a0.shape)
    out["gram"] = dict(g=gd * (a0 > 0), act=a0)
    sc = 10.0 ** (6.0 * torch.rand(1, C, 1, 1, generator=gen) - 3.0)
    out["chscale"] = dict(g=torch.randn(a1.shape, generator=gen) * sc * (a1 > 0), act=a1)
    out["randn"] = dict(g=torch.randn(a0.shape, generator=gen), act=None)
    return out
