"""csrc/nnfm.hip on the GPU against tests/_nnfmref.py: the search at every size where the launch changes shape (index and
distance conditions against fp64 at every position), ties on both sides of every tile and run boundary, the mask, the ordered
loss, the gradient per element against fp64 on the GPU's own indices, determinism and NaN, and the public path
(compute_nnfm_loss, a pixel optimisation, style_transfer, one short second_approach run).

Measured on the MI355X (printed by the tests, largest over all cases): index slack / 2E(C) 0 (every index is the fp64 arg-max),
|d - (1 - sim64)| / E(C) 0.231 (0.067 at 4096^2 x 64, where indices and distance bits equal the fp32 restatement at all 4 096
positions), loss error / (2^-23 |L|) 0.37, gradient error / bound 0.37; 20 Adam steps on the pixels take the term from 0.0302
to 0.0144.  The file runs in 6.3 s."""
import math
import os

import numpy as np
import pytest
import torch

import _nnfmref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
BASE = [1, 31, 32, 33, 127, 128, 129, 257, 1000]
CHANNELS = [1, 3, 64, 100, 256, 512]


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


def _tap(a):
    """(B, C, N) -> (B, C, 1, N): a tap one row high"""
    return a[:, :, None, :]


def _search(ops, F, S, dev, w=None):
    hat, _ = ops.nnfm_normalise(_t(_tap(S), dev))
    idx, d = ops.nnfm_search(_t(_tap(F), dev), hat, None if w is None else _t(w, dev))
    return idx.cpu().numpy(), d.cpu().numpy()


def _check_against_fp64(F, S, idx, d):
    """the two conditions at every position of every image -> (largest index slack / 2E, largest distance error / E)"""
    B, C, N = F.shape
    M = S.shape[2]
    worst_i = worst_d = 0.0
    for b in range(B):
        fhat, n = R.normalise(F[b])
        shat, _ = R.normalise(S[b if S.shape[0] > 1 else 0])
        sim = R.sims(fhat, shat)
        zero = n == 0
        assert (idx[b][zero] == -1).all() and (d[b][zero] == 1).all()
        on = ~zero
        assert ((idx[b][on] >= 0) & (idx[b][on] < M)).all()
        rows = np.arange(N)[on]
        got = sim[rows, idx[b][on]]
        slack = sim[rows].max(axis=1) - got
        err = np.abs(d[b][on].astype(F64) - (1 - got))
        assert (slack <= 2 * R.E(C)).all(), (b, slack.max(), R.E(C))
        assert (err <= R.E(C)).all(), (b, err.max(), R.E(C))
        if on.any():
            worst_i, worst_d = max(worst_i, slack.max() / (2 * R.E(C))), max(worst_d, err.max() / R.E(C))
    return worst_i, worst_d


# ---------------------------------------------------------------------------- 1. the search
def _cases(ops):
    tq, ts, seg = ops.nnfm_geometry(1000, 1000, 64)
    sizes = sorted(set(BASE + [tq - 1, tq + 1, ts - 1, ts + 1, seg * ts + 1]))
    batches = [(1, 1), (3, 1), (3, 3)]
    cases = []
    for k, n in enumerate(sizes):                                       # every size once as N and once as M
        cases.append((n, sizes[(3 * k + 5) % len(sizes)], CHANNELS[k % 6]) + batches[k % 3])
        cases.append((sizes[(5 * k + 2) % len(sizes)], n, CHANNELS[(k + 3) % 6]) + batches[(k + 1) % 3])
    return cases, (tq, ts, seg)


def test_search_meets_both_conditions_at_every_size(ops, dev):
    cases, (tq, ts, seg) = _cases(ops)
    assert tq >= 1 and ts >= 1 and seg >= 1
    assert {c[0] for c in cases} == {c[1] for c in cases} and {c[2] for c in cases} == set(CHANNELS)
    assert {c[3:] for c in cases} == {(1, 1), (3, 1), (3, 3)}
    rng = np.random.default_rng(0)
    worst = [0.0, 0.0]
    for N, M, C, B, Bs in cases:
        F, S = R.relu_like(rng, (B, C, N)), R.relu_like(rng, (Bs, C, M))
        idx, d = _search(ops, F, S, dev)
        wi, wd = _check_against_fp64(F, S, idx, d)
        worst = [max(worst[0], wi), max(worst[1], wd)]
    print("nnfm search: largest index slack / 2E(C) = %.3g, largest distance error / E(C) = %.3g" % tuple(worst))


def test_search_at_4096_squared(ops, dev):
    rng = np.random.default_rng(1)
    F, S = R.relu_like(rng, (1, 64, 4096)), R.relu_like(rng, (1, 64, 4096))
    idx, d = _search(ops, F, S, dev)
    print("nnfm search 4096^2 x 64: index slack / 2E = %.3g, distance error / E = %.3g" % _check_against_fp64(F, S, idx, d))
    i32, d32 = R.search(F, S, dtype=F32)
    print("  indices equal to the fp32 restatement: %d of 4096, distances bit-equal: %d" %
          ((idx == i32).sum(), (_bits(d) == _bits(d32)).sum()))


# ---------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("N,M,C", [(200, 1025, 16), (8192, 8192, 16)])
def test_duplicates_on_both_sides_of_every_boundary_return_the_lower_index(ops, dev, N, M, C):
    tq, ts, seg = ops.nnfm_geometry(N, M, C)
    stiles = -(-M // ts)
    run = -(-stiles // seg) * ts
    if N == 8192:
        assert run >= 2 * ts and seg > 1                                 # a run spans several tiles here
    bounds = list(range(ts, M, ts))                                      # every tile boundary; every run boundary is one
    assert all(s * run in bounds for s in range(1, seg))
    rng = np.random.default_rng(2)
    F, S = R.relu_like(rng, (1, C, N)), R.relu_like(rng, (1, C, M))
    queries = rng.permutation(N)[:2 * len(bounds)] if N >= 2 * len(bounds) else rng.integers(0, N, 2 * len(bounds))
    queries = list(dict.fromkeys(int(q) for q in queries))               # distinct query positions, random tiles and lanes
    expect = {}
    for k, t in enumerate(bounds):
        if 2 * k + 1 >= len(queries):
            break
        # family A: one vector at t - 1 and t (the two sides of the boundary) -> t - 1
        v = R.relu_like(rng, (C,)) + F32(0.01)
        S[0, :, t - 1] = v
        S[0, :, t] = v
        F[0, :, queries[2 * k]] = v
        expect[queries[2 * k]] = t - 1
        # family B: one vector just behind the boundary and again in the last tile (another run when seg > 1) -> the first
        far = M - 1 - k if M - 1 - k > t + 2 else None
        if far is not None and t + 1 < M and far not in (t - 1, t) and far % ts not in (0, ts - 1):
            u = R.relu_like(rng, (C,)) + F32(0.01)
            S[0, :, t + 1] = u
            S[0, :, far] = u
            F[0, :, queries[2 * k + 1]] = u
            expect[queries[2 * k + 1]] = t + 1
    assert len(expect) >= min(len(bounds), len(queries) // 2)
    idx, d = _search(ops, F, S, dev)
    wrong = {q: (int(idx[0, q]), j) for q, j in expect.items() if idx[0, q] != j}
    assert not wrong, wrong
    assert all(abs(d[0, q]) <= R.E(C) for q in expect)


# ---------------------------------------------------------------------------- 3. the mask
def _masked_case(rng, tq):
    B, C, N, M = 3, 64, 3 * tq + 16, 300
    F, S = R.relu_like(rng, (B, C, N)), R.relu_like(rng, (1, C, M))
    w = rng.random((B, N)).astype(F32) + F32(0.05)
    w[0, tq:2 * tq] = 0                                                  # a whole inactive query tile
    w[0, [0, 5, tq - 1, 2 * tq, N - 1]] = 0                              # single inactive positions inside active tiles
    w[1] = 0                                                             # an all-zero image
    w[2, rng.permutation(N)[:N // 3]] = 0
    return F, S, w


def test_mask_inactive_positions_and_active_bits(ops, dev):
    tq, _, _ = ops.nnfm_geometry(400, 300, 64)
    F, S, w = _masked_case(np.random.default_rng(3), tq)
    idx, d = _search(ops, F, S, dev, w)
    full_idx, full_d = _search(ops, F, S, dev)
    off = w == 0
    assert (idx[off] == -1).all() and (_bits(d[off]) == 0).all()
    assert (idx[~off] == full_idx[~off]).all() and (_bits(d[~off]) == _bits(full_d[~off])).all()
    Ft, hat = _t(_tap(F), dev), ops.nnfm_normalise(_t(_tap(S), dev))[0]
    loss, wsum = ops.nnfm_sum(_t(d, dev), _t(w, dev))
    assert wsum.cpu().numpy()[1] == 0
    g = ops.nnfm_bwd(Ft, hat, _t(idx, dev), _t(d, dev), wsum, _t(w, dev)).cpu().numpy()[:, :, 0, :]
    assert (_bits(g.transpose(0, 2, 1)[off]) == 0).all()                 # exact zeros, not small numbers, not -0
    assert not g[1].any() and g[0].any() and g[2].any()
    # an all-zero image alone: loss 0, zero gradient
    loss1, wsum1 = ops.nnfm_sum(_t(d[1:2], dev), _t(w[1:2], dev))
    g1 = ops.nnfm_bwd(Ft[1:2].contiguous(), hat, _t(idx[1:2], dev), _t(d[1:2], dev), wsum1, _t(w[1:2], dev))
    assert float(loss1) == 0.0 and not g1.any()


# ---------------------------------------------------------------------------- 4. the loss
def test_loss_is_the_ordered_fp64_sum(ops, dev):
    rng = np.random.default_rng(4)
    worst = 0.0
    for B, N, weighted, denom in ((1, 1, False, None), (3, 1000, True, None), (2, 5000, True, 8), (3, 1025, False, 5)):
        d = rng.random((B, N)).astype(F32)
        w = None
        if weighted:
            w = rng.random((B, N)).astype(F32)
            w[0, ::2] = 0
            d[0, ::2] = 0
        loss, wsum = ops.nnfm_sum(_t(d, dev), None if w is None else _t(w, dev), denom)
        ref = R.loss(d, w, denom)
        assert abs(float(loss) - ref) <= 2.0 ** -23 * abs(ref)
        worst = max(worst, abs(float(loss) - ref) / (2.0 ** -23 * abs(ref)))
        ws = np.full(B, float(N)) if w is None else w.astype(F64).sum(axis=1)
        assert np.abs(wsum.cpu().numpy() - ws).max() <= 1e-12 * ws.max()
    print("nnfm loss: largest error / (2^-23 |L|) = %.3g" % worst)


# ---------------------------------------------------------------------------- 5. the gradient
def test_gradient_per_element_against_fp64_on_the_gpus_indices(ops, dev):
    rng = np.random.default_rng(5)
    tq, _, _ = ops.nnfm_geometry(400, 300, 64)
    worst = 0.0
    cases = [(2, 3, 33, 31, 1, None, False), (3, 64, 257, 129, 3, 7, True), (1, 512, 130, 257, 1, None, False),
             (3, 100, tq + 1, 1000, 1, 5, True), (2, 1, 64, 40, 2, None, False)]
    for B, C, N, M, Bs, denom, weighted in cases:
        F, S = R.relu_like(rng, (B, C, N)), R.relu_like(rng, (Bs, C, M))
        w = None
        if weighted:
            w = rng.random((B, N)).astype(F32)
            w[0, ::3] = 0
        idx, d = _search(ops, F, S, dev, w)
        hat = ops.nnfm_normalise(_t(_tap(S), dev))[0]
        wd = None if w is None else _t(w, dev)
        _, wsum = ops.nnfm_sum(_t(d, dev), wd, denom)
        scale = 1.0 if denom is None else 0.375
        gout = None if denom is None else torch.tensor(scale, device=dev)
        g = ops.nnfm_bwd(_t(_tap(F), dev), hat, _t(idx, dev), _t(d, dev), wsum, wd, denom, gout).cpu().numpy()[:, :, 0, :]
        ref, bound = scale * R.grad(F, S, idx, w, denom), scale * R.grad_bound(F, S, idx, w, denom)
        err = np.abs(g.astype(F64) - ref)
        assert (err <= bound).all(), (B, C, N, M, (err - bound).max())
        assert not g[np.broadcast_to((idx < 0)[:, None, :], g.shape)].any()
        worst = max(worst, (err[bound > 0] / bound[bound > 0]).max())
    print("nnfm gradient: largest error / bound = %.3g" % worst)


# ---------------------------------------------------------------------------- 6. determinism and NaN
def test_two_runs_are_bit_equal_and_nan_stays_where_it_is(ops, dev):
    rng = np.random.default_rng(6)
    B, C, N, M = 2, 64, 300, 400
    F, S = R.relu_like(rng, (B, C, N)), R.relu_like(rng, (1, C, M))
    F[0, 7, 150] = np.nan                                                # a NaN query
    S[0, 3, 0] = np.nan                                                  # NaN style vectors: the first, one inside, the last
    S[0, 9, 200] = np.nan
    S[0, 0, M - 1] = np.nan
    w = rng.random((B, N)).astype(F32) + F32(0.1)
    hat = ops.nnfm_normalise(_t(_tap(S), dev))[0]
    runs = []
    for _ in range(2):
        idx, d = ops.nnfm_search(_t(_tap(F), dev), hat, _t(w, dev))
        loss, wsum = ops.nnfm_sum(d, _t(w, dev))
        g = ops.nnfm_bwd(_t(_tap(F), dev), hat, idx, d, wsum, _t(w, dev))
        runs.append((idx.cpu().numpy(), d.cpu().numpy(), loss.cpu().numpy(), g.cpu().numpy()[:, :, 0, :]))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    idx, d, loss, g = runs[0]
    assert idx[0, 150] == 0 and np.isnan(d[0, 150])
    bad = np.zeros((B, N), bool)
    bad[0, 150] = True
    assert not np.isnan(d[~bad]).any() and not np.isin(idx[~bad], (0, 200, M - 1)).any()
    assert np.isnan(g[0, :, 150]).all() and not np.isnan(g[np.broadcast_to(~bad[:, None, :], g.shape)]).any()
    assert np.isnan(loss).all()                                          # the mean of image 0 holds the NaN distance


# ---------------------------------------------------------------------------- 7. the public path
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


def test_compute_nnfm_loss_is_the_ops_composition_and_its_gradient_the_plans(ops, dev, world):
    L, ST, vgg, cur, style = world
    layers = ("conv2_1", "conv3_1")
    mask = torch.zeros(2, 1, 32, 32, device=dev)
    mask[:, :, 4:28, 8:24] = 1
    x = cur.clone().requires_grad_(True)
    loss = L.compute_nnfm_loss(x, style.expand(2, -1, -1, -1), vgg, layers, masks=mask, batch_denom=4)
    loss.backward()
    # the same from the parts
    taps = {v: k for k, v in ST._DEFAULT_LAYERS.items()}
    with torch.no_grad():
        fs = ST.get_features(style, vgg, {taps[n]: n for n in layers})
        fc = ST.get_features(cur, vgg, {taps[n]: n for n in layers})
    total, grads = None, {}
    for name in layers:
        f = fc[name]
        hat = ops.nnfm_normalise(fs[name])[0]
        w = ST.nnfm_pool_mask(mask, 2, f.shape[2], f.shape[3])
        idx, d = ops.nnfm_search(f, hat, w)
        part, wsum = ops.nnfm_sum(d, w, 4)
        total = part[0] if total is None else total + part[0]
        grads[int(taps[name])] = ops.nnfm_bwd(f, hat, idx, d, wsum, w, 4, torch.ones((), device=dev))
    assert _bits(loss.detach().cpu().numpy()) == _bits(total.cpu().numpy())
    plan = vgg.plan(2, 32)
    plan.forward(cur, upto=max(grads))
    ref = plan.backward(grads, max(grads))
    assert torch.equal(x.grad, ref) and bool(x.grad.abs().sum() > 0)
    # one style image expanded over the batch is one style; a real batch of two equal styles gives the same value
    two = L.compute_nnfm_loss(cur, style.repeat(2, 1, 1, 1), vgg, layers, masks=mask, batch_denom=4)
    assert float(two) == pytest.approx(float(loss.detach()), rel=1e-5)


def test_adam_on_the_pixels_lowers_the_term(dev, world):
    L, ST, vgg, cur, style = world
    from st3d import optim as O
    x = cur.clone().requires_grad_(True)
    opt = O.Adam([x], lr=0.01, reduce_grads=False)
    values = []
    for _ in range(20):
        x.grad = None
        loss = L.compute_nnfm_loss(x, style, vgg)
        loss.backward()
        opt.step()
        values.append(float(loss.detach()))
    with torch.no_grad():
        values.append(float(L.compute_nnfm_loss(x.detach(), style, vgg)))      # after the last step
    print("nnfm alone, 20 Adam steps at S = 32: first %.6f last %.6f" % (values[0], values[-1]))
    assert all(math.isfinite(v) for v in values) and values[-1] < values[0]


def test_style_transfer_with_the_term_moves_the_image(dev, world):
    L, ST, vgg, cur, style32 = world
    style = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(8)).to(dev).expand(2, -1, -1, -1)
    plain = ST.style_transfer(cur, cur, style, vgg, steps=3, style_weight=0.0, content_weight=0.0)
    assert torch.equal(plain.detach(), cur)                               # nothing pulls: the image stays
    out = ST.style_transfer(cur, cur, style, vgg, steps=3, style_weight=0.0, content_weight=0.0, nnfm_weight=1.0)
    assert torch.isfinite(out).all() and not torch.equal(out.detach(), cur)
    off = ST.style_transfer(cur, cur, style, vgg, steps=3)
    zero = ST.style_transfer(cur, cur, style, vgg, steps=3, nnfm_weight=0.0, nnfm_layers=("conv3_1",))
    assert torch.equal(off.detach(), zero.detach())                       # weight 0: today's loop, bit for bit


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


def test_second_approach_with_the_term_alone_ends_finite_and_writes_its_artefacts(dev, cow, golden_dir, tmp_path):
    import losses as L
    import second_approach as SA
    import style_transfer as ST
    import utils as U
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    out = str(tmp_path / "out")
    SA.main(["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "2", "--batch_size", "2", "--epochs", "3",
             "--nnfm_weight", "1", "--style_mask", "object", "--style_weight", "0", "--seed", "0", "--save_every", "0",
             "--output_path", out])
    lines = open(os.path.join(out, "log.txt")).read().splitlines()
    values = [float(line.split("Loss ")[1]) for line in lines if "Loss " in line]
    print("second_approach, nnfm alone:", values)
    assert len(values) == 3 and all(math.isfinite(v) for v in values)
    assert os.path.exists(os.path.join(out, "final.obj")) and os.path.exists(os.path.join(out, "final_render", "view_0.png"))
