"""The numpy restatement of the vertex-path backward (tests/_vertexpath_ref.py) pinned on the CPU, before any GPU test relies
on it: its fp64 reading against the C oracle (K = 1) and against torch fp64 autograd of oracle/soft_ref.py (general path,
every flag combination tests/test_gpu_vertexpath_exact.py uses), the fixed-point scatter's properties, and how far the fp32
reading is from the fp64 one per element -- the reason the GPU test compares bits and not against fp64 under a tolerance.

Measured (fragments of the C oracle, upstream gradients standard normal):
  fp64 K = 1 restatement vs oracle/raster_ref.c:ref_raster_bwd: 0.0 on cow S = 17, 32, 48 and on the quad.
  fp64 general restatement vs autograd, largest |difference| / max |gradient| over the 14 cases: 1.9e-12
  (k2-nonpersp; 2.6e-13 cow from inside/n1, every other case <= 1.5e-14), no fragment excluded in any case.
  fp32 vs fp64, worst |difference| / sum |contribution| of an element: cow 17 1.2e-4, cow 32 4.0e-3, cow 48 6.9e-5,
  quad 16 5.6e-8, quad 48 3.0e-8, sub 24 8.0e-5."""
import functools

import numpy as np
import pytest

import _vertexpath_ref as VP

F32, F64 = np.float32, np.float64

# 100 x the largest fp64-restatement-vs-autograd difference measured over the cases (1.9e-12, see above)
AUTOGRAD_BOUND = 2e-10
# the CPU comparison of the near-plane scenes runs at S = 32: autograd's pixel centres are fp64, the kernels' fp32, and
# only where 1 / S is a power of two are the two the same numbers (at S = 40 they differ by 6e-8, which is no rounding of
# the arithmetic under test); the flag combinations are those of the GPU test
AUTOGRAD_S = 32


@functools.lru_cache(maxsize=None)
def _hard(name, S):
    from oracle import render_ref as rr
    verts, faces, R, T, _ = VP.scene(name)
    B = R.shape[0]
    ndc = np.stack([rr.project_verts(verts, R[b], T[b]) for b in range(B)])
    p2f = np.stack([rr.rasterize(ndc[b], faces, S, 0.0, 4)[0] for b in range(B)])
    return ndc, faces, p2f, VP.upstream((B, S, S, 3), S)


def _per_element(idx, val, n):
    out = np.zeros(n, F64)
    np.add.at(out, idx.ravel(), val.astype(F64).ravel())
    return out


@pytest.mark.parametrize("name,S", [("cow", 17), ("cow", 32), ("cow", 48), ("quad", 16)])
def test_fp64_hard_restatement_is_the_oracles_raster_backward(name, S):
    from oracle import render_ref as rr
    ndc, faces, p2f, g = _hard(name, S)
    B, V = ndc.shape[:2]
    idx, c9, where = VP.restate_hard(ndc, faces, p2f, g, F64)
    assert len(where) > 50
    got = _per_element(idx, c9, B * V * 3).reshape(B, V, 3)
    ref = np.stack([rr.raster_bwd(g[b], p2f[b], ndc[b], faces) for b in range(B)])
    worst = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name} S={S}: {len(where)} fragments, fp64 restatement vs oracle {worst:.3e} of the largest element")
    assert worst <= 1e-12


@pytest.mark.parametrize("case", list(VP.SOFT_CASES))
def test_fp64_soft_restatement_matches_autograd(case):
    import torch
    from oracle import render_ref as rr
    from oracle import soft_ref as SR
    sc, S, K, blur, clip, persp, zc = VP.SOFT_CASES[case]
    if zc is not None:
        S = AUTOGRAD_S
    verts, faces, R, T, ndc = VP.scene(sc)
    if ndc is None:
        ndc = np.stack([rr.project_verts(verts, R[b], T[b]) for b in range(R.shape[0])])
    B, V = ndc.shape[:2]
    outs = [rr.rasterize_k(ndc[b], faces, S, K, blur, clip, nthreads=4, perspective_correct=persp, z_clip=zc,
                           return_slots=zc is not None) for b in range(B)]
    p2f = np.stack([o[0] for o in outs])
    slots = np.stack([o[4] for o in outs]) if zc is not None else None
    gb, gz, gd = VP.upstream((B, S, S, K, 3), 1), VP.upstream((B, S, S, K), 2), VP.upstream((B, S, S, K), 3)
    idx, c9, where = VP.restate_soft(ndc, faces, p2f, (gb, gz, gd), clip, persp, slots, zc, F64)
    got = _per_element(idx, c9, B * V * 3).reshape(B, V, 3)
    fc = torch.from_numpy(faces).long()
    worst = 0.0
    for b in range(B):
        nd = torch.from_numpy(ndc[b]).double().requires_grad_(True)
        if zc is None:
            b64, z64, d64, m64 = SR.soft_geometry(nd, fc, torch.from_numpy(p2f[b]).long(), S, clip, perspective_correct=persp)
        else:
            b64, z64, d64, m64 = SR.clipped_geometry(nd, fc, torch.from_numpy(slots[b]).long(), S, clip, persp, zc)
        md = m64.double()
        ((b64 * torch.from_numpy(gb[b]).double() * md.unsqueeze(-1)).sum() + (z64 * torch.from_numpy(gz[b]).double() * md).sum()
         + (d64 * torch.from_numpy(gd[b]).double() * md).sum()).backward()
        ref = nd.grad.numpy()
        worst = max(worst, float(np.abs(got[b] - ref).max() / np.abs(ref).max()))
    print(f"{case}: {len(where)} fragments, 0 excluded, fp64 restatement vs autograd {worst:.3e} of the largest element")
    assert len(where) > 10
    assert worst <= AUTOGRAD_BOUND


def test_det_scatter_does_not_depend_on_the_order_of_its_input():
    rng = np.random.default_rng(0)
    n, m = 5000, 37
    idx = rng.integers(0, m, n)
    v = (rng.standard_normal(n) * np.exp2(rng.uniform(-20, 20, n))).astype(F32)
    ref = VP.det_scatter(idx, v, m)
    for seed in range(3):
        p = np.random.default_rng(seed + 1).permutation(n)
        assert np.array_equal(VP.det_scatter(idx[p], v[p], m).view(np.int32), ref.view(np.int32))


def test_det_scatter_is_within_one_ulp_of_the_rounded_exact_sum():
    import math
    rng = np.random.default_rng(1)
    n, m = 4000, 53
    idx = rng.integers(0, m, n)
    v = (rng.standard_normal(n) * np.exp2(rng.uniform(-20, 20, n))).astype(F32)
    got = VP.det_scatter(idx, v, m)
    exact = np.array([math.fsum(v[idx == j].astype(F64)) for j in range(m)])          # exactly rounded fp64 sums
    want = exact.astype(F32)
    ulp = np.spacing(np.abs(want)).astype(F64)
    assert (np.abs(got.astype(F64) - want.astype(F64)) <= ulp).all()


def test_det_scatter_refuses_a_bound_next_to_a_power_of_two():
    v = np.array([0.5, 0.25, 0.25 - 2.0 ** -20], F32)                # sum |v| = 1 - 2^-20, exactly
    assert float(np.abs(v.astype(F64)).sum()) == 1.0 - 2.0 ** -20
    with pytest.raises(VP.BoundNearPowerOfTwo):
        VP.det_scatter(np.array([0, 1, 1]), v, 2)
    out = VP.det_scatter(np.array([0, 1, 1]), (v * F32(1.25)).astype(F32), 2)       # the caller's remedy: rescale
    assert out[0] == F32(0.625)


@pytest.mark.parametrize("name,S", VP.HARD_CASES)
def test_fp32_restatement_is_far_from_fp64_per_element(name, S):
    """thousands of ulps between the fp32 and the fp64 reading of one element (cancellation inside each contribution, small
    face areas): a record of why the GPU is compared with the fp32 reading bit for bit and not with fp64 under a bound"""
    ndc, faces, p2f, g = _hard(name, S)
    n = ndc.shape[0] * ndc.shape[1] * 3
    idx, c64, _ = VP.restate_hard(ndc, faces, p2f, g, F64)
    _, c32, _ = VP.restate_hard(ndc, faces, p2f, g, F32)
    assert c32.dtype == F32 and c64.dtype == F64
    diff = np.abs(_per_element(idx, c32.astype(F64) - c64, n))
    sabs = _per_element(idx, np.abs(c64), n)
    m = sabs > 0
    worst = float((diff[m] / sabs[m]).max())
    print(f"{name} S={S}: worst |fp32 - fp64| / sum |c9| of an element {worst:.3e}")
    assert worst < 1e-2
