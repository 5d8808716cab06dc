"""Geometry epochs: what a texture-only run recomputes every step although it depends on the coverage alone.

The plan (st3d_plan_loss_keyed, PerceptualPlan.loss(epoch=...)): need lists and flat-field lists are built once per epoch,
the latter from the coverage; the three flat fills are launched only while the shallow buffers do not hold the epoch's
background already.  The renderer (st3d.render.FragmentCache): an unchanged batch of views is projected and rasterised
once per rasteriser.  Everything stays the same bits: a keyed plan is compared, call by call, with a second plan that is
always called without an epoch."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHITE = (1.0, 1.0, 1.0)
TEAL = (0.125, 0.5, 0.625)
S, B = 128, 3
A, EB = 11, 12            # two epoch ids
# what a loss call writes: every conv's output, or the pooled output where the pool is fused into the conv's launch
ACTS = (0, 4, 5, 9, 10, 12, 14, 18, 19, 21, 23, 27, 28)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_NET = {}


def _net():
    from st3d import vgg as V
    return _NET.get("net") or _NET.setdefault("net", V.get_vgg(device=torch.device("cuda:0"), seed=0))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cover(kind):
    """(B,S,S) bool.  A: a view with two blobs, an EMPTY view between covered ones, a view with a rectangle that touches two
    image borders.  B: a fully covered view, a thin rectangle off the tile grid, an empty last view."""
    m = np.zeros((B, S, S), bool)
    yy, xx = np.mgrid[0:S, 0:S]
    if kind == "A":
        m[0] = ((yy - 40) ** 2 + (xx - 50) ** 2 < 23 ** 2) | ((yy - 100) ** 2 + (xx - 97) ** 2 < 11 ** 2)
        m[2, 0:37, 90:S] = True
    else:
        m[0] = True
        m[1, 61:71, 5:99] = True
    return m


def _image(cov, color, seed):
    """the colour where nothing is covered, seeded texels in (0, 0.9) elsewhere (never the colour of either test)"""
    rng = np.random.default_rng(seed)
    img = np.broadcast_to(np.asarray(color, np.float32)[None, :, None, None], (B, 3, S, S)).copy()
    tex = (rng.random((B, 3, S, S), dtype=np.float32) * 0.9).astype(np.float32)
    sel = np.broadcast_to(cov[:, None], img.shape)
    img[sel] = tex[sel]
    return img


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Pair:
    """a plan that gets the epochs and a plan that never does, fed the same calls"""

    def __init__(self, dev):
        from st3d import vgg as V
        self.dev = dev
        self.keyed, self.plain = V.PerceptualPlan(_net(), B, S), V.PerceptualPlan(_net(), B, S)
        g = torch.Generator().manual_seed(77)
        self.content, self.content2 = (torch.rand((B, 3, S, S), generator=g).to(dev) for _ in range(2))
        self.style = torch.rand((1, 3, S, S), generator=g).to(dev).expand(B, -1, -1, -1)     # one style: calls of 2 images too
        for p in (self.keyed, self.plain):
            p.set_content(self.content, force=True)
            p.set_style(self.style, B, force=True)

    def close(self):
        self.keyed.close()
        self.plain.close()

    def step(self, what, img, cov, color, epoch, n=B):
        cur, mask = _dev(img[:n], self.dev), _dev(cov[:n].astype(np.uint8), self.dev)
        l1, g1 = self.keyed.loss(cur, 1e6, 1.0, batch_denom=B, need_mask=mask, flat_color=color, epoch=epoch)
        l0, g0 = self.plain.loss(cur, 1e6, 1.0, batch_denom=B, need_mask=mask, flat_color=color)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g0).all()), what
        assert _same(l1, l0), (what, l1, l0)
        assert _same(g1, g0), (what, "gradient: %d elements differ" % int((_bits(g1) != _bits(g0)).sum()))
        for m in ACTS:
            a1, a0 = self.keyed.activation(m, n), self.plain.activation(m, n)
            assert _same(a1, a0), (what, "activation of module %d: %d elements differ" % (m, int((_bits(a1) != _bits(a0)).sum())))
        return g0


@pytest.mark.parametrize("force", ["0", "1"])
def test_keyed_calls_give_the_bits_of_unkeyed_calls_along_a_sequence(monkeypatch, dev, force):
    """ST3D_NEED_FORCE=1: the upper need levels engage at this size too"""
    monkeypatch.setenv("ST3D_NEED_FORCE", force)
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK"):
        monkeypatch.delenv(k, raising=False)
    ca, cb = _cover("A"), _cover("B")
    x1, x2, y1 = _image(ca, WHITE, 1), _image(ca, WHITE, 2), _image(cb, WHITE, 3)
    pair = _Pair(dev)
    try:
        g = pair.step("A first", x1, ca, WHITE, A)
        assert float(g.abs().max()) > 0 and bool((g[1] == 0).all())         # (the empty view draws no gradient)
        pair.step("A, other texels", x2, ca, WHITE, A)
        pair.step("A, a third time", x1, ca, WHITE, A)
        pair.step("B", y1, cb, WHITE, EB)
        pair.step("B again", _image(cb, WHITE, 4), cb, WHITE, EB)
        pair.step("A again", x1, ca, WHITE, A)
        pair.step("A twice", x2, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):
            p.set_content(pair.content2, force=True)
        pair.step("A after set_content", x2, ca, WHITE, A)
        pair.step("A", x1, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):              # an unkeyed call on OTHER images and another coverage in between
            p.loss(_dev(y1, dev), 1e6, 1.0, need_mask=_dev(cb.astype(np.uint8), dev), flat_color=WHITE)
        pair.step("A after an unkeyed call", x1, ca, WHITE, A)
        for p in (pair.keyed, pair.plain):              # a full forward of noise in the same buffers
            p.forward(torch.rand((B, 3, S, S), device=dev), upto=9)
        pair.step("A after plan.forward", x2, ca, WHITE, A)
        pair.step("A, two images", x1, ca, WHITE, A, n=2)
        pair.step("A, three again", x1, ca, WHITE, A)
        pair.step("A in another colour", _image(ca, TEAL, 5), ca, TEAL, A)
        pair.step("A in that colour again", _image(ca, TEAL, 6), ca, TEAL, A)
        pair.step("A back in white", x1, ca, WHITE, A)
        for e in (21, 22, 23, 24):                      # more epochs than slots, then the first ones again
            pair.step("epoch %d" % e, y1 if e % 2 else x1, cb if e % 2 else ca, WHITE, e)
        pair.step("A after eviction", x2, ca, WHITE, A)
        pair.step("B after eviction", y1, cb, WHITE, EB)
    finally:
        pair.close()


def _counts(plan, one_forward=False):
    torch.cuda.synchronize()
    fams = [f for f, _, _ in plan.profile_launches()]
    if one_forward:
        assert fams.count("convx_fwd") + fams.count("convx_fwd_flat") == 1     # conv1_1: in full, or over its covered tiles
    return fams.count("flat_fill"), fams.count("elementwise"), fams.count("conv43_fwd_flat"), fams.count("convx_fwd_flat")


def test_the_skip_happens_and_only_then(monkeypatch, dev):
    """through plan.profile_launches(): the second consecutive call of an epoch launches no fill and builds no list (two
    `elementwise` brackets fewer: the need lists and the flat-field lists) and runs conv1_1 over its covered tiles; the call
    after anything that may have written the buffers fills again, runs conv1_1 in full, and builds lists only where the
    epoch's are gone"""
    from st3d import vgg as V
    from st3d import _lib
    monkeypatch.setenv("ST3D_NEED_FORCE", "1")
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK"):
        monkeypatch.delenv(k, raising=False)
    ca, cb = _cover("A"), _cover("B")
    xa, xb, xt = (_dev(_image(c, col, 9), dev) for c, col in ((ca, WHITE), (cb, WHITE), (ca, TEAL)))
    ma, mb = _dev(ca.astype(np.uint8), dev), _dev(cb.astype(np.uint8), dev)
    net = _net()
    plan = V.PerceptualPlan(net, B, S)
    g = torch.Generator().manual_seed(5)
    content = torch.rand((B, 3, S, S), generator=g).to(dev)
    style = torch.rand((1, 3, S, S), generator=g).to(dev).expand(B, -1, -1, -1)
    try:
        plan.set_content(content, force=True)
        plan.set_style(style, B, force=True)
        plan.profile(True)
        _counts(plan)

        def call(x, m, col, epoch, n=B):
            plan.loss(x[:n], 1e6, 1.0, batch_denom=B, need_mask=m[:n], flat_color=col, epoch=epoch)
            return _counts(plan, one_forward=True)

        fill0, elem0, listed0, c1 = call(xa, ma, WHITE, 0)
        assert (fill0, listed0, c1) == (3, 3, 0) and elem0 >= 3
        built, kept_fill, skipped = (3, elem0, 3, 0), (3, elem0 - 2, 3, 0), (0, elem0 - 2, 3, 1)
        assert call(xa, ma, WHITE, A) == built
        assert call(xa, ma, WHITE, A) == skipped
        assert call(xa, ma, WHITE, A) == skipped
        assert call(xb, mb, WHITE, EB) == built                 # another epoch: its own lists, and the fills
        assert call(xb, mb, WHITE, EB) == skipped
        assert call(xa, ma, WHITE, A) == kept_fill              # back: A's lists are still there, the buffers hold B's background
        assert call(xa, ma, WHITE, A) == skipped
        plan.set_content(content, force=True)
        _counts(plan)
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xa, ma, WHITE, A) == skipped
        plan.set_style(style, B, force=True)
        _counts(plan)
        assert call(xa, ma, WHITE, A) == kept_fill
        plan.forward(xb, upto=4)
        _counts(plan)
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xa, ma, WHITE, 0) == (fill0, elem0, listed0, 0)   # an unkeyed call
        assert call(xa, ma, WHITE, A) == kept_fill
        plan.loss(xa, 1e6, 1.0)                                  # an unlisted one
        _counts(plan)
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xa, ma, WHITE, A) == skipped
        assert call(xa, ma, WHITE, A, n=2) == built             # another n: other lists, other fills
        assert call(xa, ma, WHITE, A, n=2) == skipped
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xt, ma, TEAL, A) == kept_fill               # another colour
        assert call(xt, ma, TEAL, A) == skipped
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xa, ma, WHITE, A) == skipped
        net.load_state_dict(V.synthetic_state(0))               # st3d_vgg_set_conv (the same weights again)
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xa, ma, WHITE, A) == skipped
        # a failed call: a coverage pointer that is not 16-byte aligned is refused before any launch
        raw = torch.zeros((B * S * S + 16,), dtype=torch.uint8, device=dev)
        off = raw[1:1 + B * S * S].view(B, S, S)
        assert off.data_ptr() % 16 != 0
        with pytest.raises(_lib.St3dError):
            plan.loss(xa, 1e6, 1.0, batch_denom=B, need_mask=off, flat_color=WHITE, epoch=A)
        _counts(plan)
        assert call(xa, ma, WHITE, A) == kept_fill
        assert call(xa, ma, WHITE, A) == skipped
        # no gradient wanted: the coverage still serves the flat-field lists
        plan.loss(xa, 1e6, 1.0, batch_denom=B, want_grad=False, need_mask=ma, flat_color=WHITE, epoch=A)
        assert _counts(plan)[::3] == (0, 1)
        # ST3D_FLAT=0 is read by every call: the full forward writes the buffers
        monkeypatch.setenv("ST3D_FLAT", "0")
        assert call(xa, ma, WHITE, A)[::2] == (0, 0)
        monkeypatch.delenv("ST3D_FLAT")
        assert call(xa, ma, WHITE, A) == kept_fill
        plan.profile(False)
    finally:
        plan.close()


def test_epoch_zero_gives_the_recorded_launch_list(monkeypatch, dev):
    """loss(epoch=0) is st3d_plan_loss_flat: the launches tests/golden/plan_launches.json holds for the same call"""
    spec = importlib.util.spec_from_file_location("record_plan_launches", os.path.join(ROOT, "tools", "record_plan_launches.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(ROOT, "tests", "golden", "plan_launches.json")) as f:
        gold = json.load(f)
    for k in rec.SWITCHES + ("ST3D_NEED_FORCE", "ST3D_FLAT_CHECK"):
        monkeypatch.delenv(k, raising=False)
    from st3d import vgg as V
    n, size = 1, 128
    want = gold["launch_lists"][gold["cases"][rec.case_name(n, size, {})]["calls"]["loss_need_flat@n1"]["launches"]]
    (content, style_1, _sn, _cur, flat, mask), _g = rec._inputs(n, size, dev)
    plan = V.PerceptualPlan(V.Vgg19Features(rec._state(), device=dev), n, size)
    try:
        plan.set_content(content, force=True)
        plan.set_style(style_1, n, force=True)
        plan.profile(True)
        plan.profile_launches()
        for epoch in (0, 0, 7, 0):
            plan.loss(flat, 1e6, 1.0, need_mask=mask, flat_color=rec.COLOR, epoch=epoch)
            torch.cuda.synchronize()
            got = [[f, m] for f, m, _ in plan.profile_launches()]
            assert got == want, (epoch, got, want)      # (the first call of an epoch builds its lists in the same places)
    finally:
        plan.close()


@pytest.mark.parametrize("H,W", [(16, 128), (24, 192), (20, 320)])      # whole tiles; a partial tile column; a partial tile row
def test_conv1_skips_exactly_the_flagged_tiles(dev, H, W):
    """st3d_conv1_skip_build against its definition (no covered pixel in the 8 x 128 tile +- 1, clipped), and
    st3d_conv3x3_fwd_skip against st3d_conv3x3_fwd: computed tiles equal bits, skipped tiles keep what they held"""
    from st3d import _lib, ops
    from st3d._lib import dptr, stream_ptr
    N, C, TH, TW = 2, 64, 8, 128
    g = torch.Generator().manual_seed(H + W)
    wf, _ = ops.conv3x3_pack((torch.randn((C, 3, 3, 3), generator=g) * 0.2).to(dev))
    bias = (torch.randn((C,), generator=g) * 0.1).to(dev)
    x = torch.rand((N, 3, H, W), generator=g).to(dev)
    ref = ops.conv3x3_fwd(x, wf, bias, C, relu=True)
    ty, tx = -(-H // TH), -(-W // TW)
    assert _lib.load().st3d_conv1_skip_tiles(N, H, W) == N * ty * tx
    covers = {"empty": [], "corner": [(0, 0, 0)], "last": [(1, H - 1, W - 1)],
              "tile_border": [(0, TH, TW - 1)],         # just outside tile (0, 1) and (1, 0), inside (1, 0)'s row: four tiles see it
              "one_inside": [(1, 3, min(W - 1, TW + 2))], "all": None}
    for name, pts in covers.items():
        cov = np.ones((N, H, W), np.uint8) if pts is None else np.zeros((N, H, W), np.uint8)
        for n, y, xx in pts or []:
            cov[n, y, xx] = 1
        want = np.zeros((N, ty, tx), np.uint8)
        for n in range(N):
            for j in range(ty):
                for i in range(tx):
                    ya, yb, xa, xb = max(0, j * TH - 1), min(H - 1, j * TH + TH), max(0, i * TW - 1), min(W - 1, i * TW + TW)
                    want[n, j, i] = 0 if cov[n, ya:yb + 1, xa:xb + 1].any() else 1
        skip = torch.full((N * ty * tx + 8,), 7, dtype=torch.uint8, device=dev)
        ops.call("st3d_conv1_skip_build", dptr(_dev(cov, dev)), N, H, W, dptr(skip), stream_ptr())
        assert np.array_equal(skip[:N * ty * tx].cpu().numpy(), want.reshape(-1)), name
        assert bool((skip[N * ty * tx:] == 7).all()), (name, "bytes past the last tile were written")
        if name == "tile_border" and ty > 1 and tx > 1:
            assert want[0, :2, :2].sum() == 0 and want[0].sum() == ty * tx - 4
        y = torch.full((N, C, H, W), -777.0, device=dev)
        ops.call("st3d_conv3x3_fwd_skip", dptr(x), dptr(wf), dptr(bias), dptr(y), N, 3, C, H, W, 1, dptr(skip), stream_ptr())
        px = torch.from_numpy(np.repeat(np.repeat(want == 0, TH, axis=1), TW, axis=2)[:, :H, :W]).to(dev)[:, None].expand(-1, C, -1, -1)
        assert _same(y[px], ref[px]), (name, "computed tiles differ")
        assert bool((y[~px] == -777.0).all()), (name, "a skipped tile was written")
    # any other shape is refused, not run in full
    with pytest.raises(_lib.St3dError):
        ops.call("st3d_conv3x3_fwd_skip", dptr(ref), dptr(wf), dptr(bias), dptr(ref), N, C, C, H, W, 1, dptr(skip), stream_ptr())


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import numpy as np, torch
import test_gpu_epochs as T
dev = torch.device("cuda:0")
ca = T._cover("A")
x1, x2 = T._image(ca, T.WHITE, 1), T._image(ca, T.WHITE, 2)
pair = T._Pair(dev)
pair.step("first call of a fresh plan, keyed", x1, ca, T.WHITE, T.A)
pair.step("second", x2, ca, T.WHITE, T.A)
pair.close()
print("child ok")
"""


def test_a_fresh_poisoned_plan_whose_first_call_is_keyed():
    """ST3D_POISON_PLAN=1 (read once per process: a fresh child): every plan buffer starts as NaN / -1, so the first call of
    an epoch has to fill -- nothing of the poison may reach a result"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    env["ST3D_POISON_PLAN"] = "1"
    env["ST3D_NEED_FORCE"] = "1"
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


def test_keyed_calls_under_graph_replay_are_unkeyed_ones(monkeypatch, dev):
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK", "ST3D_NEED_FORCE"):
        monkeypatch.delenv(k, raising=False)
    ca = _cover("A")
    pair = _Pair(dev)
    try:
        pair.keyed.use_graph(True)
        for i in range(4):      # plain, captured, replayed, replayed
            pair.step("graph call %d" % i, _image(ca, WHITE, 30 + i), ca, WHITE, A)
        pair.keyed.use_graph(False)
        pair.step("after the graph", _image(ca, WHITE, 40), ca, WHITE, A)
        pair.step("and again", _image(ca, WHITE, 41), ca, WHITE, A)
    finally:
        pair.close()


# ------------------------------------------------------------------------------------------------ the premise, on renders
def _scene(dev, n_views=B, asset="cow", seed=0):
    import _scenes as SC
    import losses as L
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    a = SC.load_asset(asset)
    R, T = SC.random_cameras(n_views, seed=seed)
    mesh0, renderer, cams = SC.device_scene(U, dev, a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], SC.texture_at(a, S), R, T, S)
    return U, SC, a, mesh0, renderer, cams


def test_the_premise_holds_on_renders_and_a_background_coloured_texel_loses_nothing(monkeypatch, dev):
    """ST3D_FLAT_CHECK=1: every keyed call compares the pixels with the coverage and fails if a pixel outside it differs
    from the colour.  Renders of the public renderer pass; a covered pixel that holds the colour only lists a tile the pixel
    lists would have left out, and the results stay those of the unkeyed call; a coverage that misses a pixel is refused."""
    from st3d import _lib
    from st3d import render as RD
    from st3d import vgg as V
    monkeypatch.setenv("ST3D_FLAT_CHECK", "1")
    monkeypatch.setenv("ST3D_NEED_FORCE", "1")
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    U, SC, a, mesh0, renderer, cams = _scene(dev)
    out = U.setup_optimizations("texture", mesh0, 0.01)
    tex = out["texture_map"]
    keyed, plain = V.PerceptualPlan(_net(), B, S), V.PerceptualPlan(_net(), B, S)
    try:
        with torch.no_grad():
            content, _ = U.render_meshes(renderer, mesh0, cams)
        style = SC.style_at(1, S).to(dev).expand(B, -1, -1, -1).contiguous()
        for p in (keyed, plain):
            p.set_content(content, force=True)
            p.set_style(style, B, force=True)
        for i in range(3):
            with torch.no_grad():
                tex.add_(0.03 * torch.randn(tex.shape, generator=torch.Generator().manual_seed(i)).to(dev))
                if i == 2:
                    tex.fill_(1.0)          # every covered pixel holds the background colour: the pixel lists would be empty
            mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], tex, out["verts"], out["faces"])
            cur, cov = U.render_meshes(renderer, mesh, cams)
            need = RD.need_of(cur)
            epoch = RD.epoch_of(cur, need)
            assert need is not None and epoch != 0 and RD.flat_of(cur) == WHITE
            assert torch.equal(need.bool(), cov[:, 0] > 0)
            l1, g1 = keyed.loss(cur, 1e6, 1.0, need_mask=need, flat_color=WHITE, epoch=epoch)      # (checks the premise)
            l0, g0 = plain.loss(cur, 1e6, 1.0, need_mask=need, flat_color=WHITE)
            assert _same(l1, l0) and _same(g1, g0), i
            for m in ACTS:
                assert _same(keyed.activation(m, B), plain.activation(m, B)), (i, m)
        # a coverage that leaves out a pixel which differs from the colour: refused, not computed wrongly
        cur = cur.detach().clone()
        bad = need.clone()
        y, x = (int(v) for v in torch.nonzero(need[0])[0])
        cur[0, :, y, x] = 0.25
        bad[0, y, x] = 0
        with pytest.raises(_lib.St3dError):
            keyed.loss(cur, 1e6, 1.0, need_mask=bad, flat_color=WHITE, epoch=999)
    finally:
        keyed.close()
        plain.close()


# ------------------------------------------------------------------------------------------------ fragment reuse
def _count_calls(monkeypatch):
    from st3d import ops
    seen = []
    real = ops.call

    def spy(name, *a):
        seen.append(name)
        return real(name, *a)

    monkeypatch.setattr(ops, "call", spy)
    return seen


def _geometry_calls(seen):
    return [s for s in seen if s in ("st3d_project_verts", "st3d_raster_fwd")]


def test_fragments_of_an_unchanged_batch_are_reused(monkeypatch, dev):
    from st3d import render as RD
    U, SC, a, mesh0, renderer, cams = _scene(dev)
    out = U.setup_optimizations("texture", mesh0, 0.01)
    tex = out["texture_map"]
    seen = _count_calls(monkeypatch)

    def render(r=renderer, c=cams, verts=None):
        del seen[:]
        mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], tex, out["verts"] if verts is None else verts, out["faces"])
        cur, cov = U.render_meshes(r, mesh, c)
        return cur, cov, _geometry_calls(seen)

    cur1, cov1, calls1 = render()
    assert calls1 == ["st3d_project_verts", "st3d_raster_fwd"]
    need1 = RD.need_of(cur1)
    e1 = RD.epoch_of(cur1, need1)
    assert e1 != 0
    cur2, cov2, calls2 = render()
    assert calls2 == [] and _same(cur2, cur1) and _same(cov2, cov1)
    need2 = RD.need_of(cur2)
    assert need2 is need1 and RD.epoch_of(cur2, need2) == e1
    assert "st3d_shade_fwd" in seen
    # the backward of a reused render: the same texture gradient
    gimg = torch.randn(cur1.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    grads = []
    for cur in (cur1, cur2):
        tex.grad = None
        cur.backward(gimg)
        grads.append(tex.grad.clone())
    assert float(grads[0].abs().max()) > 0 and _same(grads[0], grads[1])
    # other texels, same geometry: reused, other pixels
    with torch.no_grad():
        tex.mul_(0.5)
    cur3, _, calls3 = render()
    assert calls3 == [] and not _same(cur3, cur1) and RD.epoch_of(cur3, RD.need_of(cur3)) == e1
    # a tampered coverage tensor no longer names its epoch
    need1[0, 0, 0] ^= 1
    assert RD.epoch_of(cur3, RD.need_of(cur3)) == 0
    cur3b, _, calls3b = render()            # ... and the next render makes a new one, under a new epoch
    need3b = RD.need_of(cur3b)
    e3b = RD.epoch_of(cur3b, need3b)
    assert calls3b == [] and e3b not in (0, e1) and need3b is not need1 and _same(cur3b, cur3)
    assert torch.equal(need3b[0, 0, 0] ^ 1, need1[0, 0, 0])
    # vertices changed in place: rasterised again, under a new epoch, and the pixels are the moved mesh's
    with torch.no_grad():
        out["verts"].mul_(0.9)
    cur4, _, calls4 = render()
    e4 = RD.epoch_of(cur4, RD.need_of(cur4))
    assert calls4 == ["st3d_project_verts", "st3d_raster_fwd"] and e4 not in (0, e1, e3b) and not _same(cur4, cur3)
    # R changed in place
    with torch.no_grad():
        cams.R.copy_(SC_cameras(SC, B, 5, dev)[0])
    cur5, _, calls5 = render()
    assert calls5 == ["st3d_project_verts", "st3d_raster_fwd"] and RD.epoch_of(cur5, RD.need_of(cur5)) not in (0, e1, e3b, e4)
    assert render()[2] == []
    # a new renderer starts empty
    _, _, _, _, renderer2, _ = _scene(dev)
    assert render(r=renderer2)[2] == ["st3d_project_verts", "st3d_raster_fwd"]
    # vertices that require a gradient never enter: every render rasterises, and carries no epoch
    v = out["verts"].detach().clone().requires_grad_(True)
    for _ in range(2):
        cur6, _, calls6 = render(verts=v)
        assert calls6 == ["st3d_project_verts", "st3d_raster_fwd"] and RD.epoch_of(cur6, RD.need_of(cur6)) == 0
    # a render without gradient (the content render) is reused as well and makes no coverage tensor
    with torch.no_grad():
        c1, _, k1 = render()
        assert k1 == [] and RD.need_of(c1) is None


def SC_cameras(SC, n, seed, dev):
    R, T = SC.random_cameras(n, seed=seed)
    return torch.as_tensor(R).to(dev), torch.as_tensor(T).to(dev)


def test_eviction_recomputes_and_never_hands_out_another_batch(monkeypatch, dev):
    from st3d import render as RD
    U, SC, a, mesh0, renderer, cams = _scene(dev)
    out = U.setup_optimizations("texture", mesh0, 0.01)
    n_batches = RD.FragmentCache.ENTRIES + 2
    batches = [RD.FoVPerspectiveCameras(*SC_cameras(SC, B, 10 + i, dev), device=dev) for i in range(n_batches)]
    seen = _count_calls(monkeypatch)

    def render(c):
        del seen[:]
        mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
        cur, _ = U.render_meshes(renderer, mesh, c)
        return cur.detach().clone(), RD.epoch_of(cur, RD.need_of(cur)), _geometry_calls(seen)

    first = [render(c) for c in batches]
    assert all(k == ["st3d_project_verts", "st3d_raster_fwd"] for _, _, k in first)
    assert len({e for _, e, _ in first}) == n_batches and len(renderer.rasterizer.fragment_cache) == RD.FragmentCache.ENTRIES
    for i in reversed(range(n_batches)):       # the newest are still there, the oldest were evicted; either way: the batch's own pixels
        cur, e, k = render(batches[i])
        assert _same(cur, first[i][0]), i
        if i >= 2:
            assert k == [] and e == first[i][1], i
        else:
            assert k == ["st3d_project_verts", "st3d_raster_fwd"] and e not in {x for _, x, _ in first}, i


def test_second_approach_steps_reuse_fragments_lists_and_background(monkeypatch, dev):
    """three second_approach steps through the public loop body against the same steps with every reuse defeated (a new
    renderer per step, so no epoch): the same losses and texture gradients, and from the second step on no fill"""
    import losses as L
    for k in ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK", "ST3D_NEED_FORCE", "ST3D_NEED_MASK"):
        monkeypatch.delenv(k, raising=False)
    weights = {"main_loss_weight": 3.0, "mesh_verts_weight": 1.0, "mesh_edge_loss_weight": 1.0,
               "mesh_laplacian_smoothing_weight": 1.0, "mesh_normal_consistency_weight": 1.0}
    results = {}
    for reuse in (False, True):
        U, SC, a, mesh0, renderer, cams = _scene(dev)
        net = _net()
        out = U.setup_optimizations("texture", mesh0, 0.01)
        tex = out["texture_map"]
        verts0 = torch.from_numpy(a["verts"]).to(dev)
        sty = SC.style_at(1, S).to(dev).expand(B, -1, -1, -1)
        with torch.no_grad():
            content, _ = U.render_meshes(renderer, mesh0, cams)
        plan = net.plan(B, S)
        steps = []
        for i in range(3):
            if not reuse:
                _, _, _, _, renderer, _ = _scene(dev)
            tex.grad = None
            mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], tex, out["verts"], out["faces"])
            cur, cov = U.render_meshes(renderer, mesh, cams)
            plan.profile(True)
            plan.profile_launches()
            loss = L.compute_second_approach_loss(cur, content, sty, net, 1e6, 1.0, out["verts"], verts0, mesh, weights, "texture")
            loss.backward()
            torch.cuda.synchronize()
            fills = [f for f, _, _ in plan.profile_launches()].count("flat_fill")
            plan.profile(False)
            steps.append((loss.detach().clone(), tex.grad.clone(), fills))
            with torch.no_grad():
                tex.sub_(0.01 * tex.grad.sign())
        results[reuse] = steps
    for i in range(3):
        assert _same(results[True][i][0], results[False][i][0]) and _same(results[True][i][1], results[False][i][1]), i
    assert [f for _, _, f in results[False]] == [3, 3, 3]
    assert [f for _, _, f in results[True]] == [3, 0, 0]
