"""csrc/swd.hip on the GPU against tests/_swdref.py, staged: the projection per element against fp64 within the bound of an
fp32 chain; the sort bit for bit against the restatement on the GPU's own projections at every size where its launch changes
shape; the loss and the gradient on the GPU's own sorted rows and permutation; determinism and NaN; and the public path
(swd_loss and compute_swd_loss through autograd, a descent on a tap tensor beside the same loop in fp64, style_transfer, one
short second_approach run with a checkpoint and a resume).

Measured on the MI355X (printed by the tests): projection error / bound 0.573, and all 1 944 744 values bit-equal to the
emulated fma chain; the sort bit-equal in all 80 cases (block 8192, 3 strided passes at N = 40 000); loss error / (2^-23 |L|)
0.368; every gproj element 0 ulp from the rounded fp64 value; tap gradient error / composed bound 0.00125; the descent goes
0.205766 -> 0.025759 on the GPU and in the fp64 restatement alike (ratio 0.1252), relative gap 5e-08 of the allowed 0.01.
The file runs in 5.7 s."""
import math
import os

import numpy as np
import pytest
import torch

import _swdref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SIZES = [1, 3, 64, 100, 256, 512]
TILE = 128                                                               # positions per workgroup of the projection kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------- 1. the projection
def test_projection_is_within_the_chain_bound_at_every_size(ops, dev):
    positions = [1, 31, 32, 33, TILE - 1, TILE, TILE + 1, 1000]
    cases = []
    for k, N in enumerate(positions + positions[:4]):                    # 12 cases: every Q and R twice, every N, B in {1, 3}
        cases.append((1 + 2 * (k % 2), SIZES[k % 6], SIZES[(k + 3 + k // 6) % 6], N))
    cases += [(3, 512, 512, TILE + 1), (1, 256, 100, 1000)]
    assert {c[1] for c in cases} == set(SIZES) == {c[2] for c in cases} and {c[3] for c in cases} == set(positions)
    rng = np.random.default_rng(0)
    worst, same = 0.0, [0, 0]
    for B, Q, Rr, N in cases:
        x, a = R.relu_like(rng, (B, Q, N)), R.unit_rows(rng, Rr, Q)
        out = ops.swd_project(_t(x, dev), _t(a, dev)).cpu().numpy()
        assert out.shape == (B, Rr, N)
        ref, bound = R.project(x, a), R.project_bound(x, a)
        err = np.abs(out.astype(F64) - ref)
        assert (err <= bound).all(), (B, Q, Rr, N, (err - bound).max())
        if (bound > 0).any():
            worst = max(worst, (err[bound > 0] / bound[bound > 0]).max())
        chain = R.project(x, a, F32)
        same = [same[0] + int((_bits(out) == _bits(chain)).sum()), same[1] + out.size]
    print("swd projection: largest error / bound = %.3g; %d of %d values bit-equal to the emulated fma chain" % (worst, *same))


def test_equal_columns_in_different_tiles_and_images_get_equal_bits(ops, dev):
    rng = np.random.default_rng(1)
    B, Q, Rr, N = 3, 100, 64, 3 * TILE + 5
    x, a = R.relu_like(rng, (B, Q, N)), R.unit_rows(rng, Rr, Q)
    spots = [(0, 0), (0, TILE - 1), (1, TILE), (1, 2 * TILE + 37), (2, 3 * TILE + 4), (2, 77)]
    for b, n in spots:
        x[b, :, n] = x[0, :, 0]
    x[1, :, 1:TILE] = 0                                                  # a flat stretch: zero features
    out = ops.swd_project(_t(x, dev), _t(a, dev)).cpu().numpy()
    for b, n in spots:
        assert _bits(out[b, :, n]).tolist() == _bits(out[0, :, 0]).tolist()
    assert (_bits(out[1, :, 1:TILE]) == 0).all()                         # +0, never -0


# ---------------------------------------------------------------------------- 2. the sort
def _hurtful_rows(rng, B, K, N, block):
    """(B,K,N) fp32: one pattern per row, in rotation"""
    specials = np.array([0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF],
                        np.uint32).view(F32)
    out = np.empty((B, K, N), F32)
    for row in range(B * K):
        kind = row % 6
        v = rng.standard_normal(N).astype(F32)
        if kind == 0:
            v[:] = F32(0.75)                                             # one value
        elif kind == 1:
            v = np.round(v * 4).astype(F32) / 4                          # many ties, and a run of equals over every boundary
            for t in range(block, N, block):
                v[max(t - 3, 0):t + 3] = F32(0.5)
        elif kind == 2:
            where = rng.integers(0, N, size=max(1, N // 4))
            v[where] = specials[rng.integers(0, len(specials), size=len(where))]
            v[0], v[N - 1] = specials[4], specials[0]
        elif kind == 3:
            v = np.sort(v)
        elif kind == 4:
            v = np.sort(v)[::-1].copy()
        out[row // K, row % K] = v
    return out


def _weights(rng, B, N):
    w = rng.random((B, N)).astype(F32) + F32(0.05)
    w[0, rng.permutation(N)[:(3 * N) // 10]] = 0
    if B > 1:
        w[1] = 0                                                         # no active position
        w[2] = 0
        w[2, N // 2] = 0.5                                               # a single one
    return w


def test_sort_equals_the_total_order_bit_for_bit(ops, dev):
    block, passes = ops.swd_geometry(40000)
    assert block >= 4 and passes >= 2                                    # several global passes at 40 000
    assert ops.swd_geometry(block)[1] == 0 and ops.swd_geometry(block + 1)[1] >= 1
    sizes = [1, 2, 3, block - 1, block, block + 1, 2 * block + 1, 3 * block + 17, 1000, 40000]
    rng = np.random.default_rng(2)
    done = 0
    for N in sizes:
        for K in (1, 5):
            for B in (1, 3):
                proj = _hurtful_rows(rng, B, K, N, block)
                for weighted in (False, True):
                    w = _weights(rng, B, N) if weighted else None
                    srt, perm, count = ops.swd_sort(_t(proj, dev), None if w is None else _t(w, dev))
                    rs, rp, rc = R.sort_rows(proj, w)
                    assert count.cpu().numpy().tolist() == rc.tolist(), (N, K, B, weighted)
                    assert np.array_equal(perm.cpu().numpy(), rp), (N, K, B, weighted)
                    assert np.array_equal(_bits(srt.cpu().numpy()), _bits(rs)), (N, K, B, weighted)
                    done += 1
    # the style side: no weights, no perm
    srt, perm, count = ops.swd_sort(_t(proj, dev), None, want_perm=False)
    assert perm is None and np.array_equal(_bits(srt.cpu().numpy()), _bits(R.sort_rows(proj)[0]))
    print("swd sort: %d cases bit-equal; block %d, %d global passes at N = 40000" % (done, block, passes))


# ---------------------------------------------------------------------------- 3. loss and gradient
def test_loss_and_gradient_on_the_gpus_own_rows(ops, dev):
    rng = np.random.default_rng(3)
    worst_l = worst_g = 0.0
    #        B  Bs K   N     M     weighted denom
    cases = [(1, 1, 1, 1, 4, False, None), (2, 1, 5, 300, 300, False, None), (3, 3, 16, 1000, 257, True, 7),
             (3, 1, 7, 129, 5000, True, None), (2, 2, 64, 4097, 4097, False, 5), (1, 1, 3, 4, 1, False, None)]
    seen = set()
    for B, Bs, K, N, M, weighted, denom in cases:
        proj, tproj = rng.standard_normal((B, K, N)).astype(F32), rng.standard_normal((Bs, K, M)).astype(F32) + F32(0.5)
        w = _weights(rng, B, N) if weighted else None
        srt, perm, count = ops.swd_sort(_t(proj, dev), None if w is None else _t(w, dev))
        tsorted, _, _ = ops.swd_sort(_t(tproj, dev), None, want_perm=False)
        s, p, c, ts = srt.cpu().numpy(), perm.cpu().numpy(), count.cpu().numpy(), tsorted.cpu().numpy()
        seen |= {"=" if n == M else ("<" if n < M else ">") for n in c if n}
        loss = float(ops.swd_loss(srt, count, tsorted, denom))
        ref = R.loss(s, c, ts, denom)
        assert abs(loss - ref) <= 2.0 ** -23 * abs(ref), (B, K, N, M, loss, ref)
        if ref:
            worst_l = max(worst_l, abs(loss - ref) / (2.0 ** -23 * abs(ref)))
        scale = 1.0 if denom is None else 0.375
        gout = None if denom is None else torch.tensor(scale, device=dev)
        g = ops.swd_bwd(srt, perm, count, tsorted, denom, gout).cpu().numpy()
        ref32 = R.grad_proj(s, p, c, ts, denom, scale).astype(F32)
        ulps = np.abs(g.astype(F64) - ref32.astype(F64)) / np.spacing(np.maximum(np.abs(ref32), np.finfo(F32).tiny)).astype(F64)
        assert (ulps <= 1).all(), (B, K, N, M, ulps.max())
        worst_g = max(worst_g, ulps.max())
        if w is not None:
            off = np.broadcast_to((~(w > 0))[:, None, :], g.shape)
            assert (_bits(g)[off] == 0).all()                            # an exact +0, not a small number, not -0
            assert (_bits(g[1]) == 0).all() and g[0].any() and np.count_nonzero(g[2]) <= K
        one = ops.swd_bwd(srt, perm, count, tsorted, denom, torch.ones((), device=dev)).cpu().numpy()
        none = ops.swd_bwd(srt, perm, count, tsorted, denom, None).cpu().numpy()
        assert one.tobytes() == none.tobytes()
    assert seen == {"=", "<", ">"}
    print("swd loss: largest error / (2^-23 |L|) = %.3g; gradient: largest distance from the rounded fp64 value = %.3g ulp"
          % (worst_l, worst_g))


# ---------------------------------------------------------------------------- 4. determinism and non-finite inputs
def test_two_runs_are_bit_equal_and_nan_stays_in_its_image(dev):
    import style_transfer as ST
    rng = np.random.default_rng(4)
    B, C, H, W, K = 2, 64, 20, 15, 48
    F, S = R.relu_like(rng, (B, C, H, W)), R.relu_like(rng, (1, C, 13, 17))
    F[0, 7, 3, 4] = np.nan
    V = _t(R.unit_rows(rng, K, C), dev)
    mask = torch.ones(B, H, W, device=dev)
    mask[:, :2] = 0
    runs = []
    for _ in range(2):
        x = _t(F, dev).requires_grad_(True)
        loss = ST.swd_loss(x, _t(S, dev), V, mask=mask)
        loss.backward()
        runs.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    loss, g = runs[0]
    assert np.isnan(loss) and np.isnan(g[0, :, 3, 4]).all()
    assert np.isfinite(g[1]).all() and g[1].any() and (_bits(g[:, :, :2]) == 0).all()


# ---------------------------------------------------------------------------- 5. the public path
@pytest.fixture(scope="module")
def world(dev):
    import losses as L
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    vgg = U.get_vgg(seed=0)
    g = torch.Generator().manual_seed(7)
    cur = torch.rand(2, 3, 32, 32, generator=g).to(dev)
    style = torch.rand(1, 3, 48, 48, generator=g).to(dev)
    return L, ST, vgg, cur, style


def _tap_reference(ops, F, S, V, w, denom):
    """fp64 loss and gradient at the tap on the GPU's own permutations with their bounds, the gradient's per element, composed of stage 1 (each projection
    within (C+1) 2^-24 sum |V F| of fp64), stage 3 (gproj within 1 ulp <= 2^-23 |g| of its fp64 value on the rows it was
    given) and stage 1 again for the back-projection, a chain of length K."""
    B, C, N = F.shape
    K, M = V.shape[0], S.shape[2]
    p, t = ops.swd_project(F, V), ops.swd_project(S, V)
    _, perm, count = ops.swd_sort(p, w)
    _, tperm, _ = ops.swd_sort(t)
    perm, tperm, count = perm.cpu().numpy().astype(np.int64), tperm.cpu().numpy().astype(np.int64), count.cpu().numpy()
    Fn, Sn, Vn = F.cpu().numpy(), S.cpu().numpy(), V.cpu().numpy()
    srt = np.take_along_axis(R.project(Fn, Vn), perm, axis=2)
    tsorted = np.take_along_axis(R.project(Sn, Vn), tperm, axis=2)
    e_s = np.take_along_axis(R.project_bound(Fn, Vn), perm, axis=2)
    e_t = np.take_along_axis(R.project_bound(Sn, Vn), tperm, axis=2)
    L = R.loss(srt, count, tsorted, denom)
    g = R.grad_proj(srt, perm, count, tsorted, denom)
    eg = np.zeros_like(g)
    inv = 1.0 / float(denom if denom is not None else B)
    lbound = 2.0 ** -23 * abs(L)                                          # the fp64 sum, rounded once
    for b in range(B):
        n = int(count[b])
        if n:
            j = R.quantile(n, M)
            e = e_s[b, :, :n] + e_t[0][:, j]                              # of each difference
            lbound += (inv / (K * n)) * (2 * np.abs(srt[b, :, :n] - tsorted[0][:, j]) * e + e * e).sum()
            np.put_along_axis(eg[b], perm[b, :, :n], (2.0 * inv / (K * n)) * e, axis=1)
    eg += 2.0 ** -23 * np.abs(g)
    Va = np.abs(Vn.astype(F64))
    bound = np.einsum("kc,bkn->bcn", Va, eg) + (K + 1) * 2.0 ** -24 * np.einsum("kc,bkn->bcn", Va, np.abs(g) + eg)
    return L, lbound, np.einsum("kc,bkn->bcn", Vn.astype(F64), g), bound


def test_swd_loss_and_compute_swd_loss_through_autograd(ops, dev, world):
    L, ST, vgg, cur, style = world
    layers = ("conv2_1", "conv3_1")
    mask = torch.zeros(2, 1, 32, 32, device=dev)
    mask[:, :, 4:28, 8:24] = 1
    taps = {v: k for k, v in ST._DEFAULT_LAYERS.items()}
    with torch.no_grad():
        fs = ST.get_features(style, vgg, {taps[n]: n for n in layers})
        fc = ST.get_features(cur, vgg, {taps[n]: n for n in layers})
    directions = ST.swd_draw(layers, 0, torch.Generator().manual_seed(11), dev)
    assert [tuple(directions[n].shape) for n in layers] == [(128, 128), (256, 256)]
    assert torch.allclose(directions["conv3_1"].norm(dim=1), torch.ones(256, device=dev), atol=1e-6)
    total, grads, worst = None, {}, 0.0
    for name in layers:
        f = fc[name].clone().requires_grad_(True)
        part = ST.swd_loss(f, fs[name], directions[name], mask=mask, batch_denom=4)
        part.backward()
        B, C, H, W = f.shape
        w = ST.nnfm_pool_mask(mask, B, H, W)
        ref_l, lbound, ref_g, bound = _tap_reference(ops, f.detach().reshape(B, C, H * W), fs[name].reshape(1, C, -1), directions[name],
                                             w.reshape(B, -1), 4)
        assert abs(float(part.detach()) - ref_l) <= lbound, (name, float(part.detach()), ref_l, lbound)
        err = np.abs(f.grad.cpu().numpy().reshape(B, C, -1).astype(F64) - ref_g)
        assert (err <= bound).all(), (name, (err - bound).max())
        assert not f.grad.cpu().numpy().reshape(B, C, -1)[np.broadcast_to((w.reshape(B, 1, -1) == 0).cpu().numpy(), err.shape)].any()
        worst = max(worst, (err[bound > 0] / bound[bound > 0]).max())
        total = part.detach() if total is None else total + part.detach()
        grads[int(taps[name])] = f.grad.clone()
    print("swd tap gradient: largest error / composed bound = %.3g" % worst)
    # compute_swd_loss is the sum of these, its directions drawn in the order of the layers, its gradient the plan's
    x = cur.clone().requires_grad_(True)
    loss = L.compute_swd_loss(x, style.expand(2, -1, -1, -1), vgg, layers, generator=torch.Generator().manual_seed(11),
                              masks=mask, batch_denom=4)
    loss.backward()
    assert _bits(loss.detach().cpu().numpy()) == _bits(total.cpu().numpy())
    plan = vgg.plan(2, 32)
    plan.forward(cur, upto=max(grads))
    assert torch.equal(x.grad, plan.backward(grads, max(grads))) and bool(x.grad.abs().sum() > 0)
    handed = L.compute_swd_loss(cur, style, vgg, layers, directions=directions, masks=mask, batch_denom=4)
    assert _bits(handed.cpu().numpy()) == _bits(total.cpu().numpy())


def test_descent_on_a_tap_follows_the_same_loop_in_fp64(dev):
    """Adam (lr 0.05, 30 steps) on a tap tensor of C = 16, N = 256 with about 30 % of the positions inactive against M = 200
    style positions, K = 16 directions redrawn every step and handed to both loops; the value on fixed directions before and
    after.  The end / start ratio on the GPU must be within 1 % of the ratio the fp64 restatement reaches in this test."""
    import style_transfer as ST
    rng = np.random.default_rng(5)
    B, C, H, W, M, K, steps, lr = 1, 16, 16, 16, 200, 16, 30, 0.05
    F0, S = R.relu_like(rng, (B, C, H * W)), R.relu_like(rng, (1, C, M)) * F32(1.5)
    w = (rng.random((B, H * W)) > 0.3).astype(F32)
    fixed = R.unit_rows(rng, 64, C)
    draws = [R.unit_rows(rng, K, C) for _ in range(steps)]
    # fp64 restatement
    x, m, v = F0.astype(F64), np.zeros((B, C, H * W)), np.zeros((B, C, H * W))
    start64 = R.term(x, S, fixed, w)[0]
    for t, V in enumerate(draws, 1):
        # the order is taken on the fp32 rounding of the projections, the values stay fp64
        p = np.einsum("kc,bcn->bkn", V.astype(F64), x)
        tp = np.einsum("kc,bcn->bkn", V.astype(F64), S.astype(F64))
        _, perm, count = R.sort_rows(p.astype(F32), w)
        srt = np.take_along_axis(p, perm.astype(np.int64), axis=2)
        g = np.einsum("kc,bkn->bcn", V.astype(F64), R.grad_proj(srt, perm, count, np.sort(tp, axis=2)))
        m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        x = x - lr * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + 1e-8)
    p = np.einsum("kc,bcn->bkn", fixed.astype(F64), x)
    _, perm, count = R.sort_rows(p.astype(F32), w)
    tp = np.sort(np.einsum("kc,bcn->bkn", fixed.astype(F64), S.astype(F64)), axis=2)
    end64 = R.loss(np.take_along_axis(p, perm.astype(np.int64), axis=2), count, tp)
    # the GPU
    xg = _t(F0.reshape(B, C, H, W), dev).requires_grad_(True)
    Sg, mask = _t(S.reshape(1, C, 10, 20), dev), _t(w.reshape(B, H, W), dev)
    opt = torch.optim.Adam([xg], lr=lr)
    with torch.no_grad():
        start = float(ST.swd_loss(xg, Sg, _t(fixed, dev), mask=mask))
    for V in draws:
        opt.zero_grad()
        ST.swd_loss(xg, Sg, _t(V, dev), mask=mask).backward()
        opt.step()
    with torch.no_grad():
        end = float(ST.swd_loss(xg, Sg, _t(fixed, dev), mask=mask))
    gap = abs(end / start - end64 / start64) / (end64 / start64)
    print("swd descent: GPU %.6f -> %.6f (ratio %.4f), fp64 %.6f -> %.6f (ratio %.4f), relative gap %.3g"
          % (start, end, end / start, start64, end64, end64 / start64, gap))
    assert end64 < 0.5 * start64                                         # the loop descends at all
    assert gap <= 0.01
    after = xg.detach().cpu().numpy().reshape(B, C, H * W)
    off = np.broadcast_to((w == 0)[:, None, :], after.shape)
    assert np.array_equal(_bits(after)[off], _bits(F0)[off]) and not np.array_equal(after[~off], F0[~off])


def test_style_transfer_with_the_term_is_reproducible_from_its_seed(dev, world):
    L, ST, vgg, cur, style32 = world
    style = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(8)).to(dev).expand(2, -1, -1, -1)
    kw = dict(steps=5, swd_weight=1.0, swd_layers=("conv2_1", "conv3_1"), swd_directions=32)
    a = ST.style_transfer(cur, cur, style, vgg, swd_seed=3, **kw)
    b = ST.style_transfer(cur, cur, style, vgg, swd_seed=3, **kw)
    c = ST.style_transfer(cur, cur, style, vgg, swd_seed=4, **kw)
    off = ST.style_transfer(cur, cur, style, vgg, steps=5)
    assert torch.isfinite(a).all() and torch.equal(a.detach(), b.detach())
    assert not torch.equal(a.detach(), c.detach()) and not torch.equal(a.detach(), off.detach())
    zero = ST.style_transfer(cur, cur, style, vgg, steps=5, swd_weight=0.0, swd_seed=9)
    assert torch.equal(off.detach(), zero.detach())                       # weight 0: today's loop, bit for bit
    alone = ST.style_transfer(cur, cur, style, vgg, steps=5, style_weight=0.0, content_weight=0.0, swd_weight=1.0)
    assert torch.isfinite(alone).all() and not torch.equal(alone.detach(), cur)


def _write_cow_assets(tmp, cow, golden_dir, tex_size=32):
    from PIL import Image
    from st3d import io as stio
    tex = torch.from_numpy(cow["texture_u8"][::1024 // tex_size, ::1024 // tex_size].copy()).float() / 255
    obj = os.path.join(tmp, "cow.obj")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    sty = np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]
    style = os.path.join(tmp, "style.png")
    Image.fromarray(sty).save(style)
    return obj, style


def test_second_approach_resumed_equals_uninterrupted(dev, cow, golden_dir, tmp_path, monkeypatch):
    import losses as L
    import second_approach as SA
    import st3d.cli as cli
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    finals, export = [], cli.Run.export
    monkeypatch.setattr(cli.Run, "export", lambda self, mesh: (finals.append(self.opt[self.texture_key].detach().clone()),
                                                               export(self, mesh))[1])
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0",
              "--swd_weight", "1", "--style_mask", "object", "--save_every", "0", "--epochs", "3"]
    full, part = str(tmp_path / "full"), str(tmp_path / "part")
    SA.main(common + ["--output_path", full, "--checkpoint_every", "2"])
    ck = os.path.join(full, "checkpoint.pt")
    blob = torch.load(ck, map_location="cpu", weights_only=True)
    assert blob["progress"] == 2 and blob["swd_generator_state"].dtype == torch.uint8
    SA.main(common + ["--output_path", part, "--resume", ck])            # epoch 2 only
    log = lambda d: [line.split("Loss ")[1] for line in open(os.path.join(d, "log.txt")).read().splitlines()[1:]]
    lf, lp = log(full), log(part)
    print("losses", lf, "resumed", lp)
    assert len(lf) == 3 and len(lp) == 1 and all(math.isfinite(float(v)) for v in lf) and lp[0] == lf[2]
    assert len(finals) == 2 and torch.equal(finals[0], finals[1])          # the final texture, bit for bit
    assert not torch.equal(finals[0].cpu(), blob[[k for k in ("texture_map",) if k in blob][0]])
    with pytest.raises(ValueError, match="swd_weight"):
        SA.main([a for a in common if a not in ("--swd_weight", "1")] + ["--output_path", str(tmp_path / "bad"), "--resume", ck])
