"""The dependency footprints of tests/_footprints.py against the Jacobian sparsity of torch fp64 autograd (no GPU): the
NaN / Inf tracer of tests/test_gpu_nonfinite.py judges the kernels by these sets, so they are checked first."""
import pytest
import torch
import torch.nn.functional as F

import _footprints as fp


def _support(fn, x, idx):
    """Outputs whose derivative with respect to input element idx is non-zero (one Jacobian column, fp64)."""
    x = x.clone().requires_grad_(True)
    y = fn(x)
    cols = []
    for k in range(y.numel()):
        g, = torch.autograd.grad(y.reshape(-1)[k], x, retain_graph=True)
        cols.append(g[idx] != 0)
    return torch.stack(cols).reshape(y.shape)


def _tiles(mask, m):
    """Close a footprint over m x m output tiles."""
    N, C, H, W = mask.shape
    t = mask.reshape(N, C, H // m, m, W // m, m).any(dim=5, keepdim=True).any(dim=3, keepdim=True)
    return t.expand(N, C, H // m, m, W // m, m).reshape(N, C, H, W)


@pytest.mark.parametrize("tile,H,W", [(1, 5, 7), (2, 6, 8), (4, 8, 12)])
def test_conv_footprint_is_the_jacobian_support(tile, H, W):
    """Direct conv: exactly the 3x3 neighbourhood x all output channels of the image; Winograd: exactly the output tiles
    that the neighbourhood touches.  Forward and input gradient (a convolution with the flipped, transposed filter)."""
    g = torch.Generator().manual_seed(tile)
    N, Cin, Cout = 2, 2, 3
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64)
    gy = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64)
    fwd = lambda t: F.conv2d(t, w, padding=1)                                  # noqa: E731
    dgrad = lambda t: F.conv_transpose2d(t, w, padding=1)                      # noqa: E731
    for fn, inp, cin in ((fwd, x, Cin), (dgrad, gy, Cout)):
        for n, c, y, xx in [(0, 0, 0, 0), (1, cin - 1, H - 1, W - 1), (1, 0, H // 2, 1), (0, cin - 1, 1, W - 2),
                            (0, 0, H - 2, W // 2)]:
            sup = _support(fn, inp, (n, c, y, xx))
            want = sup if tile == 1 else _tiles(sup, tile)
            assert torch.equal(fp.conv3x3(sup.shape, n, y, xx, tile), want), (tile, n, c, y, xx)


@pytest.mark.parametrize("H,W", [(6, 8), (5, 7)])
def test_pool_footprint_is_the_window(H, W):
    """The element planted as its window's maximum reaches exactly its pooled cell; the dropped odd row / column none."""
    g = torch.Generator().manual_seed(H)
    x = torch.rand(2, 3, H, W, generator=g, dtype=torch.float64)
    for n, c, y, xx in [(0, 0, 0, 0), (1, 2, H - 1, W - 1), (1, 1, 3, 2)]:
        xb = x.clone()
        xb[n, c, y, xx] = 5.0
        sup = _support(lambda t: F.max_pool2d(t, 2, 2), xb, (n, c, y, xx))
        assert torch.equal(fp.pool2x2(fp.element(x.shape, n, c, y, xx)), sup)
    # pooling a conv footprint: every window it meets
    m = fp.conv3x3((1, 1, H, W), 0, 2, 3)
    assert torch.equal(fp.pool2x2(m), F.max_pool2d(m.double(), 2, 2) > 0)


def test_gram_footprints_are_the_jacobian_support():
    g = torch.Generator().manual_seed(0)
    B, C, H, W = 2, 4, 3, 5
    f = torch.rand(B, C, H, W, generator=g, dtype=torch.float64) + 0.1
    D = torch.randn(B, C, C, generator=g, dtype=torch.float64)
    gram = lambda t: torch.bmm(t.flatten(2), t.flatten(2).transpose(1, 2))    # noqa: E731
    bwd_f = lambda t: torch.bmm(D, t.flatten(2)).reshape(B, C, H, W)          # noqa: E731
    bwd_d = lambda t: torch.bmm(t, f.flatten(2)).reshape(B, C, H, W)          # noqa: E731
    for n, c, p in [(0, 0, 0), (1, C - 1, H * W - 1), (1, 2, 7)]:
        y, x = divmod(p, W)
        assert torch.equal(fp.gram(B, C, n, c), _support(gram, f, (n, c, y, x)))
        assert torch.equal(fp.gram_bwd_feat(f.shape, n, p), _support(bwd_f, f, (n, c, y, x)))
        assert torch.equal(fp.gram_bwd_D(f.shape, n, c), _support(bwd_d, D, (n, c, (c + 1) % C)))
