"""Every wrapper of st3d/color.py and the five colour ops between guard zones (tests/_guarded.py): no write outside its
outputs, no output element left unwritten, and the same bits under both fill patterns and in a plain run -- on the shapes of
tests/test_gpu_color.py and inside one tagged loss call at S = 64."""
import numpy as np
import pytest
import torch

import _colorref as CR
import _guarded as G

pytestmark = pytest.mark.gpu
MODULES = ("st3d.ops", "st3d.color")
U32 = np.uint32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(t, want):
    return np.array_equal(t.cpu().numpy().view(U32), np.ascontiguousarray(want).view(U32))


def test_every_wrapper_between_guard_zones(dev):
    from st3d import color, ops
    chunk = ops.color_stats_chunk()
    rng = np.random.default_rng(31)
    for B, H, W in ((1, 1, 1), (2, 3, 5), (1, 7, 37), (2, 16, 16), (1, 33, 65), (1, 1, chunk + 1), (2, 1, 2 * chunk - 1)):
        P = H * W
        x, y = rng.random((B, 3, H, W), dtype=np.float32), rng.random((B, 3, H, W), dtype=np.float32)
        g = rng.standard_normal((B, 3, H, W)).astype(np.float32)
        m = (rng.random((B, H, W)) < 0.3).astype(np.uint8)
        m[0, 0, 0] = 1
        A, b = rng.standard_normal((3, 3)) * 0.7, rng.standard_normal(3) * 0.3
        d_x, d_y, d_g, d_m = _t(x, dev), _t(y, dev), _t(g, dev), _t(m, dev)
        flat = lambda a: a.reshape(B, 3, P)         # noqa: E731
        out = G.compare_ab(lambda: {"fwd": ops.luma_fwd(d_x), "bwd": ops.luma_bwd(d_g), "rec": ops.luma_recombine(d_x, d_y),
                                    "aff": ops.color_affine(d_x, A, b, clamp=False), "affc": ops.color_affine(d_x, A, b),
                                    "sums": ops.color_sums(d_x, d_m), "all": ops.color_sums(d_x, None)}, modules=MODULES)
        shape = (B, H, W)
        assert _eq(out["fwd"], CR.luma_fwd(flat(x)).reshape(x.shape)), shape
        assert _eq(out["bwd"], CR.luma_bwd(flat(g)).reshape(x.shape)), shape
        assert _eq(out["rec"], CR.recombine(flat(x), flat(y)).reshape(x.shape)), shape
        assert _eq(out["aff"], CR.affine(flat(x), A, b, False).reshape(x.shape)), shape
        assert _eq(out["affc"], CR.affine(flat(x), A, b, True).reshape(x.shape)), shape
        assert out["sums"][0].item() == int(m.sum()) and out["all"][0].item() == B * P
        np.testing.assert_allclose(out["sums"].cpu().numpy(), CR.moments(flat(x), m.reshape(B, P)), rtol=1e-12)

        def autograd():
            leaf = d_x.clone().requires_grad_(True)
            v = color.luma(leaf)
            v.backward(d_g)
            return {"y": v.detach(), "grad": leaf.grad}

        # (autograd may hand the leaf the backward's own buffer or a copy of it: the gradient is the case's own either way)
        out = G.compare_ab(autograd, modules=MODULES, own=lambda raw: (raw["grad"],))
        assert _eq(out["y"], CR.luma_fwd(flat(x)).reshape(x.shape)) and _eq(out["grad"], CR.luma_bwd(flat(g)).reshape(x.shape))

        def public():
            color.clear_cache()
            one = d_x[:1].expand(3, -1, -1, -1)
            return {"cached": color.luma_cached(d_x), "expanded": color.luma_cached(one), "recolor": color.recolor(d_x, A, b),
                    "recombine": color.recombine(d_x, d_y), "matched": color.match_style(d_x, d_y, d_m, clamp=False),
                    "matched_luma": color.match_style_luminance(d_x, d_y, d_m),
                    "texture": color.recombine_texture(d_x.permute(0, 2, 3, 1).contiguous(), d_y.permute(0, 2, 3, 1).contiguous())}

        out = G.compare_ab(public, modules=MODULES)
        assert _eq(out["cached"], CR.luma_fwd(flat(x)).reshape(x.shape)) and tuple(out["expanded"].shape) == (3, 3, H, W)
        assert _eq(out["recombine"], CR.recombine(flat(x), flat(y)).reshape(x.shape))
        planar = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2, 3).reshape(3, -1))[None]       # noqa: E731
        want = CR.recombine(planar(x), planar(y))[0].reshape(3, B, H, W).transpose(1, 0, 2, 3)
        assert _eq(out["texture"].permute(0, 3, 1, 2).contiguous(), want)
        assert torch.isfinite(out["matched"]).all() and torch.isfinite(out["matched_luma"]).all()
    color.clear_cache()


def test_a_tagged_loss_between_guard_zones(dev):
    """luma(render-like tensor) with a need tag and a flat tag inside compute_perceptual_loss at S = 64: the luminance buffers
    sit between guards; the loss and the gradient, which the plan and autograd allocate, are the case's own."""
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import color
    from st3d import render as R
    U.device = ST.device = L.device = dev
    vgg = U.get_vgg(seed=0)
    B, S = 2, 64
    gen = torch.Generator().manual_seed(9)
    x, c, s = (torch.rand(B, 3, S, S, generator=gen).to(dev) for _ in range(3))
    need = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
    need[:, 9:41, 13:50] = 1
    white = torch.ones_like(x)
    x = torch.where(need.bool()[:, None], x, white)             # the background holds the flat colour, as a render's does

    def loss(tagged):
        color.clear_cache()                                     # every run takes the luminance of the content afresh
        leaf = x.clone().requires_grad_(True)
        cur = leaf * 1.0
        if tagged:
            setattr(cur, R.NEED_TAG, need)
            R.tag_flat(cur, (1.0, 1.0, 1.0))
        y = color.luma(cur)
        assert (R.need_of(y) is need) == tagged and (R.flat_of(y) is not None) == tagged
        value = L.compute_perceptual_loss(y, color.luma_cached(c), color.luma_cached(s), vgg)
        value.backward()
        out = {"loss": value.detach(), "grad": leaf.grad}
        out["_own"] = tuple(out.values())
        return out

    outs = {}
    for tagged in (False, True):
        outs[tagged] = G.compare_ab(lambda: loss(tagged), modules=MODULES, own=lambda raw: raw["_own"])
        o = outs[tagged]
        assert torch.isfinite(o["loss"]) and torch.isfinite(o["grad"]).all() and bool((o["grad"] != 0).any())
    px = need.bool()[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(outs[True]["loss"], outs[False]["loss"]) and torch.equal(outs[True]["grad"][px], outs[False]["grad"][px])
    color.clear_cache()
