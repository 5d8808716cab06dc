"""fp64 references, per-element bounds, fp32 emulations of the summation order and realistic operands for the style-loss
tail: the Gram forward (gram.hip), the squared-difference sums with D = G - S (loss.hip), the Gram backward coef D F
(gram.hip) and the loss triple / the gradients leaving the taps as the loss plan composes them (plan.hip).

As in tests/_convref.py a kernel result `got` (fp32) with fp64 reference `ref` passes when, element by element,

    |got - ref| <= kappa * u * M,        u = 2^-24,

with M the operation's magnitude at that element (sum of the absolute values of the terms; for post-ReLU features the
Gram's M is the Gram itself: no cancellation, every entry must be right to a few u of ITSELF, and an exact zero of the
reference -- a dead channel -- admits nothing but an exact zero).

kappa is a function of the LENGTH n of the longest chain of fp32 roundings an element goes through.  The fp32 MFMA
(v_mfma_f32_32x32x2_f32) is, bit for bit, a k-ordered chain of fmaf -- D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)): the
products are exact and every pixel (forward) or channel (backward) adds ONE rounding:

    kernel          chain length n                                            kappa(n)
    Gram forward    kper / KG + ceil(nslab / 4) + 1                           min(n + 2, C_FWD sqrt(n));  on white: n + 2
                    (one fmaf per pixel of a slab's K range, the reduce's
                    four interleaved sums over the slabs, the tree)
    Gram backward   C + 1   (one fmaf per channel, started from `base`)       min(n + 2, C_BWD sqrt(n))
    sqdiff sums     ceil(n_elem / (256 blocks)) + 14                           n   (derived, not measured: see sqdiff_kappa)

n + 2 is the worst case of the order itself (every rounding is at most u of a partial sum that, for M's non-negative
terms, never exceeds M; + 1 for coef folded into D, + 1 for the second-order terms): nothing that sums in this order can
exceed it, so kappa never asks for less than fp32 can give.  c sqrt(n) is what the order really does on operands whose
roundings fall on either side: c = MARGIN x the worst err / (u M sqrt(n)) that the fp32 CPU EMULATION of the kernels'
order (gram_fwd_emul, gram_bwd_emul below: same splits, same k-groups, same fmaf chain, same reduce tree) reaches over
the operand families of tests/test_gramref.py; MARGIN = 4 as in _convref.  tests/test_gramref.py::
test_emulation_meets_the_bounds re-measures them.

    measured on the CPU, worst over the families                              value      bound derived from it
    forward, plain images and synthetic families, err / (u M sqrt(n))         3.59       C_FWD = 14.3
    backward, err / (u M sqrt(n))                                             1.67       C_BWD = 6.6
    forward, images composited on white, err / (u M n)                        0.35       none: kappa = n + 2

The white surround is a run of tens of thousands of EQUAL terms; their roundings all point the same way, the error grows
with n, not sqrt(n), and reaches a third of the worst case (style3 on white, relu2_1, 2048-pixel splits: 367 u of 1043).
No sqrt law holds there and a constant fitted to it would be blind everywhere else, so that family gets the worst-case
bound of the order -- still three times below what one dropped 32-pixel chunk costs at HW = 2^18 (about 2000 u).
(An emulation that advances TWO pixels per fp32 addition, gram_fwd_emul(fma=False), is kept for comparison: it
under-states the white family four-fold -- 88 u where the fmaf chain and the hardware give 367.)

None of these numbers comes from the GPU kernels.  The GPU's own worst figures are printed by
tests/test_gpu_loss_tail.py and recorded in DESIGN.md; they appear in no bound.

Operand families (seeded, CPU): `real` = the seeded VGG's tap activations (relu1_1 .. relu5_1, and conv4_2 for the content
term) of the committed style images, plain and composited on white; `chscale` = real with every channel scaled by
10^U(-3, 3); `relu_shift` = relu(randn + 1); for D: `far` = G(image a) - G(image b), `near` = G(F) - G(F') with
F' = relu(F (1 + eps randn)), and a dense non-symmetric randn D for the ungated entry point."""
import torch

import _convref as R
from _convref import U32, _d

MARGIN = 4.0
# worst figures of the fmaf-chain emulations: err / (u M sqrt(n)) for "fwd" and "bwd", err / (u M n) for "fwd_white"
MEASURED_CPU = {"fwd": 3.59, "fwd_white": 0.35, "bwd": 1.67}
C_FWD = 14.3
C_BWD = 6.6

STYLE_TAPS = (0, 5, 10, 19, 28)          # module indices of relu1_1 .. relu5_1 (the conv whose post-ReLU output is the tap)
CONTENT_TAP = 21
FP64_FLOPS = [0]


# ------------------------------------------------------------------------------------------------ the kernels' split
def gram_kgroups(C, HW=32):
    """slabs per split: the single-tile layers (C = 64 / 128, whole 32-pixel chunks) split each chunk over 4 / 2 k-groups"""
    return (4 if C == 64 else 2) if C in (64, 128) and HW % 32 == 0 else 1


def gram_split(B, C, HW, scale=1):
    """(nsplit, kper) of gram.hip's gram_split, restated (own code; tests/test_gpu_loss_tail.py checks it against
    st3d_gram_workspace_bytes): workgroups aimed for per layer, at most 2048 x scale pixels and at least 128 per split,
    at most 256 splits, kper rounded up to whole 32-pixel chunks"""
    nt = C // 128 if C % 128 == 0 else (C + 63) // 64
    pairs = nt * (nt + 1) // 2
    target = (1280 if C >= 512 else 768 if C == 256 else 512 if C == 128 else 1024) // scale
    ns = (target + pairs * B - 1) // (pairs * B)
    ns = max(ns, (HW + 2048 * scale - 1) // (2048 * scale))
    ns = min(ns, (HW + 127) // 128, 256)
    ns = max(ns, 1)
    kp = (HW + ns - 1) // ns
    kp = (kp + 31) // 32 * 32
    return (HW + kp - 1) // kp, kp


def gram_workspace_bytes(B, C, HW):
    ns, _ = gram_split(B, C, HW)
    return B * ns * (4 if C == 64 else 2 if C == 128 else 1) * C * C * 4


def multi_scale(C, HW, scale=2):
    """the split scale st3d_gram_fwd_multi really uses for an item: its own (default 2) where the fused kernel has a body
    for the shape (whole tiles and 32-pixel chunks), 1 where the item runs through st3d_gram_fwd"""
    return scale if HW % 32 == 0 and (C == 64 or C % 128 == 0) else 1


def fwd_chain(B, C, HW, scale=1):
    ns, kper = gram_split(B, C, HW, scale)
    kg = gram_kgroups(C, HW)
    return kper // kg + (ns * kg + 3) // 4 + 1


def kappa_fwd(B, C, HW, scale=1, white=False):
    n = fwd_chain(B, C, HW, scale)
    return n + 2.0 if white else min(n + 2.0, C_FWD * n ** 0.5)


def bwd_chain(C):
    return C + 1


def kappa_bwd(C):
    n = bwd_chain(C)
    return min(n + 2.0, C_BWD * n ** 0.5)


def sqdiff_kappa(n_elem):
    """derived, rigorous: d = fl(a - b) and d d round once each (relative to d^2: 3 u), a thread then adds
    ceil(n / (256 blocks)) squares in a running fp32 sum, the wave tree adds 6 levels, the workgroup 2; the rest is
    fp64 until the product with `scale` (itself an fp32 rounding of the caller's double) is rounded to fp32 and added
    to the slot: + 3.  All terms are non-negative, so every partial sum is below the total."""
    blocks = min(1024, max(1, (n_elem + 255) // 256))
    return float(-(-n_elem // (256 * blocks)) + 8 + 3 + 3)


# ------------------------------------------------------------------------------------------------ fp64 references
def gram_ref(F):
    """F (B, C, ...) -> (G, M) fp64: G = F F^T, M = |F| |F|^T"""
    f = _d(F).flatten(2)
    FP64_FLOPS[0] += 2 * f.shape[0] * f.shape[1] ** 2 * f.shape[2]
    G = torch.bmm(f, f.transpose(1, 2))
    return G, (G if float(f.min()) >= 0 else torch.bmm(f.abs(), f.abs().transpose(1, 2)))


def gram_bwd_ref(D, F, coef, base=None, gated=False):
    """out = base + coef D F, zero where gated and F <= 0; -> (out, M), M = |base| + |coef| |D| |F| (0 behind a closed gate)"""
    f = _d(F)
    shp = f.shape
    f = f.flatten(2)
    d = _d(D).expand(f.shape[0], -1, -1)
    FP64_FLOPS[0] += 4 * f.shape[0] * f.shape[1] ** 2 * f.shape[2]
    out = coef * torch.bmm(d, f)
    M = abs(coef) * torch.bmm(d.abs(), f.abs())
    if base is not None:
        out, M = out + _d(base).flatten(2), M + _d(base).flatten(2).abs()
    if gated:
        open_ = (f > 0).double()
        out, M = out * open_, M * open_
    return out.reshape(shp), M.reshape(shp)


def sqdiff_ref(a, b, scale=1.0):
    """-> (scale * sum (a - b)^2, D = a - b) in fp64; b broadcast over the leading axis when it is shorter"""
    a, b = _d(a), _d(b)
    D = a - (b if b.shape == a.shape else b.reshape(-1).repeat(a.numel() // b.numel()).reshape(a.shape))
    return float(scale) * float((D * D).sum()), D


def style_norm(C, H, batch_denom):
    """plan.hip's `norm` of a style layer (the plan is square: H * H)"""
    return 1.0 / (batch_denom * C * C) / (float(C) * C * H * H)


def loss_triple(content_sum, chw, style_sums, shapes, batch_denom, style_weight, content_weight):
    """[total, content, style] as plan_loss_enqueue scales them: content_sum = sum (F - Ft)^2 over all images,
    style_sums[l] = sum (G_l - S_l)^2, shapes[l] = (C, H)"""
    content = content_sum / (batch_denom * chw)
    style = sum(s * style_norm(C, H, batch_denom) for s, (C, H) in zip(style_sums, shapes))
    return content_weight * content + style_weight * style, content, style


def tail_ref(acts, content_act, style_grams, content_target, style_weight, content_weight, batch_denom=None, gated=(),
             want_grads=True):
    """The whole tail in fp64.  acts: the five tap activations (n, C, H, H); style_grams: (1 | n, C, C) each.
    -> dict(loss = [total, content, style], D = [G - S], G, MG, grads = [coef_l D_l F_l] (gated where l in `gated`),
    content_grad = cc (F - Ft), coef, cc, style_sums, shapes)"""
    n = acts[0].shape[0]
    bd = float(batch_denom or n)
    G, MG, D, sums, shapes, coefs, grads = [], [], [], [], [], [], []
    for l, (A, S) in enumerate(zip(acts, style_grams)):
        g, m = gram_ref(A)
        s, d = sqdiff_ref(g, S)
        C, H = A.shape[1], A.shape[2]
        coef = 4.0 * style_weight * style_norm(C, H, bd)
        G.append(g); MG.append(m); D.append(d); sums.append(s); shapes.append((C, H)); coefs.append(coef)
        if want_grads:
            grads.append(gram_bwd_ref(d, A, coef, gated=l in gated)[0])
    csum, cd = sqdiff_ref(content_act, content_target)
    chw = content_act[0].numel()
    cc = 2.0 * content_weight / (bd * chw)
    return dict(loss=list(loss_triple(csum, chw, sums, shapes, bd, style_weight, content_weight)), D=D, G=G, MG=MG, grads=grads,
                content_grad=cc * cd, coef=coefs, cc=cc, style_sums=sums, content_sum=csum, shapes=shapes)


# ------------------------------------------------------------------------------------------------ fp32 emulations
def _fma(acc, a, b):
    """fl32(acc + a b) with the product exact, as fmaf: the product of two fp32 is exact in fp64, the fp64 sum is then
    rounded to fp32 (the double rounding this can commit is one part in 2^29 of the cases)"""
    return (acc.double() + a.double() * b.double()).float()


def gram_fwd_emul(F, B=1, scale=1, return_slabs=False, fma=True, rows=None):
    """fp32 CPU emulation of the Gram forward's summation order for ONE image F (C, HW) launched in a batch of B (the
    split depends on B): per split of kper pixels -- and per k-group of the 32-pixel chunks where the single-tile
    kernel runs -- a running fp32 accumulator advanced by one fmaf per pixel (the MFMA's documented numerics), then the
    reduce: four interleaved partial sums over the slabs in ascending order, (p0 + p1) + (p2 + p3).  rows: only these
    rows of G (a sample, for the large layers).  fma=False: two pixels per fp32 addition (kept for comparison)."""
    f = F.detach().float().cpu().flatten(1)
    C, HW = f.shape
    ns, kper = gram_split(B, C, HW, scale)
    kg = gram_kgroups(C, HW)
    x = torch.zeros(C, ns * kper)
    x[:, :HW] = f                                                  # (adding the zeros past the end changes no bit)
    x = x.reshape(C, ns, kper // 32, kg, 32 // kg).permute(1, 3, 0, 2, 4).reshape(ns * kg, C, kper // kg)
    xr = x if rows is None else x[:, rows]
    acc = torch.zeros(ns * kg, xr.shape[1], C)
    if fma:
        xd, xrd = x.double(), xr.double()
        for t in range(kper // kg):
            acc = (acc.double() + xrd[:, :, t, None] * xd[:, None, :, t]).float()
    else:
        for t in range(0, kper // kg, 2):
            acc += torch.bmm(xr[:, :, t:t + 2], x[:, :, t:t + 2].transpose(1, 2))
    G = reduce_emul(acc)
    return (G, acc) if return_slabs else G


def reduce_emul(slabs, leave_out=None):
    p = [torch.zeros_like(slabs[0]) for _ in range(4)]
    for k in range(slabs.shape[0]):
        if k != leave_out:
            p[k % 4] = p[k % 4] + slabs[k]
    return (p[0] + p[1]) + (p[2] + p[3])


def gram_bwd_emul(D, F, coef, base=None, gated=False):
    """fp32 emulation of the Gram backward for one image: coef folded into D first (one fp32 product per entry), the
    accumulator started from `base`, one fmaf per channel in ascending order, the gate at the store.  D may hold a
    subset of the rows."""
    f = F.detach().float().cpu()
    f = f.flatten(1)
    dc = (torch.tensor(coef, dtype=torch.float32) * D.detach().float().cpu()).double()
    acc = torch.zeros(dc.shape[0], f.shape[1]) if base is None else base.detach().float().cpu().flatten(1).clone()
    fd = f.double()
    for k in range(f.shape[0]):
        acc = (acc.double() + dc[:, k, None] * fd[None, k]).float()
    if gated:
        acc = torch.where(f > 0, acc, torch.zeros_like(acc))
    return acc.reshape(F.shape) if acc.shape == f.shape else acc


# ------------------------------------------------------------------------------------------------ criterion
report = R.report
scale_close = R.scale_close


def quiet_group(ref, size):
    """start of the aligned group of `size` rows of a 2-D |ref| whose maximum is the smallest non-zero one"""
    a = _d(ref).abs()
    n = a.shape[0] // size
    mx = a[:n * size].reshape(n, size, -1).amax((1, 2))
    mx = torch.where(mx > 0, mx, torch.full_like(mx, float("inf")))
    return int(torch.argmin(mx)) * size


# ------------------------------------------------------------------------------------------------ operands
def tap_activations(images, upto=28):
    """fp32 CPU forward of the seeded VGG, one image at a time (only the taps are kept): module index -> (n, C, H, W) for
    the style taps and the content tap reached by `upto`"""
    keep = [i for i in STYLE_TAPS + (CONTENT_TAP,) if i <= upto]
    out = {i: [] for i in keep}
    for img in images:
        a = R.vgg_activations(img[None], upto=upto)
        for i in keep:
            out[i].append(a[i][3])
    return {i: torch.cat(v) for i, v in out.items()}


def style_images(S=512, names=R.STYLES):
    """the committed style images at S x S (top-left crop), plain then on white: (2 len(names), 3, S, S)"""
    c = R.style_crops(S, S, names)
    return torch.cat([c, R.on_white(c)])


def mirror_tiled(img):
    """(3, H, W) -> (3, 2H, 2W): the image and its mirror images, so that the seams are continuous"""
    top = torch.cat([img, img.flip(2)], 2)
    return torch.cat([top, top.flip(1)], 1)


def chscale(F, gen):
    return F * 10.0 ** (6.0 * torch.rand((1, F.shape[1]) + (1,) * (F.dim() - 2), generator=gen) - 3.0)


def relu_shift(shape, gen):
    return torch.relu(torch.randn(shape, generator=gen) + 1.0)


def near(F, eps, gen):
    """F' = relu(F (1 + eps randn)): the activations of an image that has almost converged to F's"""
    return torch.relu(F * (1.0 + eps * torch.randn(F.shape, generator=gen)))


def trunc_mantissa(t, bits=10):
    """fp32 values with the mantissa cut to `bits` explicit bits (what a reduced-precision matrix instruction would read)"""
    i = t.detach().float().contiguous().view(torch.int32)
    return (i & ~((1 << (23 - bits)) - 1)).view(torch.float32)


def chain_figures(rows):
    """rows of (kind 'fwd' | 'fwd_white' | 'bwd', chain length n, worst err / (u M)) -> worst ratio / sqrt(n) per kind
    (ratio / n for 'fwd_white')"""
    out = {}
    for kind, n, ratio in rows:
        out[kind] = max(out.get(kind, 0.0), ratio / (n if kind == "fwd_white" else n ** 0.5))
    return out
