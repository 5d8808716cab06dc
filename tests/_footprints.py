"""Dependency footprints of the VGG / loss kernels: which outputs MAY change when one input element changes.

Every function returns a bool tensor of the output's shape.  tests/test_gpu_nonfinite.py plants a NaN / Inf at one input
element and requires every non-finite kernel output to lie inside the footprint, and every output outside it to equal the
clean launch bit for bit (each kernel sums in a fixed order).  tests/test_host_logic.py checks these functions against the
Jacobian sparsity of torch fp64 autograd, so the harness is right before it judges a kernel.

Winograd kernels mix a whole output tile through their transforms, so their footprint is every m x m output tile whose
(m + 2) x (m + 2) input patch -- rows m * ty - 1 .. m * ty + m -- holds the element.  Input gradients are convolutions of the
output gradient, so the same rules apply with the roles of the two tensors swapped."""
import torch


def _span(v, n, m):
    """Output index range [lo, hi) reached from input index v along an axis of length n: 3-tap neighbourhood (m = 1) or
    the m-wide Winograd tiles whose m + 2 patch holds v."""
    if m == 1:
        return max(v - 1, 0), min(v + 2, n)
    t_lo = max(-(-(v - m) // m), 0)            # smallest t with m t + m >= v
    t_hi = min((v + 1) // m, (n - 1) // m)     # largest t with m t - 1 <= v
    return t_lo * m, min((t_hi + 1) * m, n)


def conv3x3(out_shape, n, y, x, tile=1):
    """3x3 / pad 1 convolution (or its input gradient): input element (n, any c, y, x) -> outputs of image n, every
    channel, the 3x3 neighbourhood (tile = 1) or the Winograd tiles of size `tile` (2: F(2x2,3x3), 4: F(4x4,3x3))."""
    N, C, H, W = out_shape
    m = torch.zeros(out_shape, dtype=torch.bool)
    y0, y1 = _span(y, H, tile)
    x0, x1 = _span(x, W, tile)
    m[n, :, y0:y1, x0:x1] = True
    return m


def pool2x2(full_mask):
    """MaxPool2d(2, 2) (floor) of a full-resolution footprint: a pooled cell may change iff its window meets it."""
    N, C, H, W = full_mask.shape
    f = full_mask[:, :, : H // 2 * 2, : W // 2 * 2]
    return f.reshape(N, C, H // 2, 2, W // 2, 2).any(dim=5).any(dim=3)


def element(shape, *idx):
    m = torch.zeros(shape, dtype=torch.bool)
    m[idx] = True
    return m


def gram(B, C, n, c):
    """G[n] = F[n] F[n]^T: element F[n, c, p] -> row c and column c of image n's Gram."""
    m = torch.zeros((B, C, C), dtype=torch.bool)
    m[n, c, :] = True
    m[n, :, c] = True
    return m


def gram_bwd_feat(feat_shape, n, p):
    """out[n] = coef * D[n] F[n] (optionally gated by F): F[n, c, p] -> pixel p of every channel of image n."""
    B, C = feat_shape[:2]
    m = torch.zeros((B, C, feat_shape[2:].numel()), dtype=torch.bool)
    m[n, :, p] = True
    return m.reshape(feat_shape)


def gram_bwd_D(feat_shape, n, a):
    """out[n] = coef * D[n] F[n]: D[n, a, b] -> row a (channel a, every pixel) of image n."""
    m = torch.zeros(feat_shape, dtype=torch.bool)
    m[n, a] = True
    return m
