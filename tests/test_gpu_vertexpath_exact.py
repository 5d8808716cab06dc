"""The vertex-path backward on the GPU -- raster_bwd_kernel (csrc/raster.hip), raster_k_bwd_kernel / raster_k_frag_grad
(csrc/soft.hip), the fixed-point scatter (csrc/det.h) and project_verts_bwd_kernel -- against its fp32 restatement
(tests/_vertexpath_ref.py, pinned on the CPU by tests/test_vertexpath_ref.py) PER ELEMENT and without a tolerance: both
files are built without FMA contraction and with correctly rounded division, and the backward has only + - * /, comparisons,
fminf and fmaxf, so numpy's float32 reproduces every fragment's nine contributions bit for bit; the default scatter is
integer addition at a power-of-two scale, so the whole (B,V,3) result is reproduced bit for bit as well.  The norm tests of
test_gpu_kernels.py / test_gpu_vcol.py see none of: a wrong sign on one of a fragment's nine contributions, a face dropped
by a tile's LDS table, a fragment on the direct-to-global path with the wrong vertex index, a clipped sub-triangle that
hands its gradient to the wrong corner.

(a) one fragment at a time (float atomics, groups of fragments that share no vertex: every touched element is 0 + c, exact):
    names the fragment and the component that is wrong;
(b) fixed point (the default), dense upstream gradient: every element of the result equals det_scatter of the restated
    contributions bit for bit;
(c) float atomics, dense gradient: |got - sum| <= n 2^-24 sum|c| per element, n the number of nonzero terms of the element,
    sum and sum|c| the exact sums of the restated fp32 terms -- the textbook bound of an fp32 summation in any order (the
    LDS stage and the global stage are one summation tree); elements without a term are exactly 0;
(d) project_verts_bwd bit for bit.

Inputs are the GPU's own project_verts / rasteriser outputs (bit-pinned to the oracle elsewhere), copied to the host.
Scenes: cow B = 2, S = 17 / 32 / 48 (partial, 2 x 2, 3 x 3 tiles); quad S = 16 (256 lanes into two LDS entries), S = 48
(nine tiles add the same two faces through global atomics); sub = the cow subdivided twice, S = 24 (a face per pixel); the
general path at K = 1..4 with blur, clipped barycentrics, without perspective correction, through near-plane clipped
faces (z_clip = 0.5), and 'overflow': sub at S = 16, K = 8 -- more distinct faces in the single tile than the LDS table has
slots, so fragments take the direct-to-global branch."""
import numpy as np
import pytest
import torch

import _vertexpath_ref as VP

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SOFT_FACE_SLOTS = 512                   # kSoftFaceSlots of csrc/soft.hip
WHICH = ("all", "gb", "gz", "gd")       # the upstream gradients given to raster_soft_bwd; the others are None


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


_SCENES, _REFS = {}, {}


def _hard_scene(dev, ops, name, S):
    if (name, S) not in _SCENES:
        verts, faces, R, T, _ = VP.scene(name)
        d = dict(faces_np=faces, B=R.shape[0], V=verts.shape[0], S=S, K=None, verts_np=verts, R_np=R, T_np=T)
        d["faces"] = torch.from_numpy(faces).to(dev).contiguous()
        d["ndc"] = ops.project_verts(torch.from_numpy(verts).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev))
        d["p2f"] = ops.raster_fwd(d["ndc"], d["faces"], S)[0]
        d["ndc_np"], d["p2f_np"] = d["ndc"].cpu().numpy(), d["p2f"].cpu().numpy()
        d["g_np"] = (VP.upstream((d["B"], S, S, 3), S),)
        assert (d["p2f_np"] >= 0).sum() > 50
        _SCENES[(name, S)] = d
    return _SCENES[(name, S)]


def _soft_scene(dev, ops, case):
    if case not in _SCENES:
        sc, S, K, blur, clip, persp, zc = VP.SOFT_CASES[case]
        verts, faces, R, T, ndc = VP.scene(sc)
        d = dict(faces_np=faces, S=S, K=K, clip=clip, persp=persp, zc=zc)
        d["faces"] = torch.from_numpy(faces).to(dev).contiguous()
        if ndc is None:
            d["ndc"] = ops.project_verts(torch.from_numpy(verts).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev))
        else:
            d["ndc"] = torch.from_numpy(ndc).to(dev)
        d["B"], d["V"] = d["ndc"].shape[0], d["ndc"].shape[1]
        out = ops.raster_soft_fwd(d["ndc"], d["faces"], S, K, blur, clip, perspective_correct=persp, z_clip=zc)
        d["p2f"], d["slots"] = out[0], (out[4] if zc is not None else None)
        d["ndc_np"], d["p2f_np"] = d["ndc"].cpu().numpy(), d["p2f"].cpu().numpy()
        d["slots_np"] = d["slots"].cpu().numpy() if zc is not None else None
        B = d["B"]
        d["g_np"] = (VP.upstream((B, S, S, K, 3), 1), VP.upstream((B, S, S, K), 2), VP.upstream((B, S, S, K), 3))
        if zc is not None:
            assert (d["slots_np"] >= 0).sum() > 15
        if case == "overflow":      # more distinct faces in a tile than its LDS table holds: the direct-to-global branch runs
            p = d["p2f_np"]
            most = max(np.unique(t[t >= 0]).size for b in range(B) for y in range(0, S, 16) for x in range(0, S, 16)
                       for t in [p[b, y:y + 16, x:x + 16]])
            print(f"overflow: {most} distinct faces in a tile, table of {SOFT_FACE_SLOTS}")
            assert most > SOFT_FACE_SLOTS
        _SCENES[case] = d
    return _SCENES[case]


def _restate(d, grads):
    if d["K"] is None:
        return VP.restate_hard(d["ndc_np"], d["faces_np"], d["p2f_np"], grads[0], F32)
    return VP.restate_soft(d["ndc_np"], d["faces_np"], d["p2f_np"], grads, d["clip"], d["persp"], d["slots_np"], d["zc"], F32)


def _reference(key, d, which="all"):
    """The restated contributions of the dense upstream gradient and their fixed-point sum, computed once and left unchanged.
    det_scatter refuses a bound too close to a power of two (the kernel's fp32 bound could sit in the other binade): the
    upstream gradient is then rescaled by 1.25, at most twice -- a condition on the input, no tolerance."""
    if (key, which) not in _REFS:
        n = d["B"] * d["V"] * 3
        keep = {"all": (1, 1, 1), "gb": (1, 0, 0), "gz": (0, 1, 0), "gd": (0, 0, 1)}[which]
        for attempt in range(3):
            grads = tuple((g * F32(1.25) ** attempt).astype(F32) if k else None for g, k in zip(d["g_np"], keep))
            idx, c9, where = _restate(d, grads)
            assert c9.dtype == F32
            try:
                det = VP.det_scatter(idx.ravel(), c9.ravel(), n)
                break
            except VP.BoundNearPowerOfTwo:
                continue
        else:
            raise AssertionError("no usable bound after two rescalings")
        ref = dict(grads=grads, idx=idx, c9=c9, where=where, det=det, attempt=attempt)
        for v in (idx, c9, where, det):
            v.setflags(write=False)
        _REFS[(key, which)] = ref
    return _REFS[(key, which)]


def _launch(ops, dev, d, grads):
    """grads: numpy arrays or device tensors or None -> (B,V,3) numpy"""
    t = [None if g is None else (g if torch.is_tensor(g) else torch.from_numpy(g).to(dev)) for g in grads]
    if d["K"] is None:
        out = ops.raster_bwd(t[0], d["p2f"], d["ndc"], d["faces"])
    else:
        out = ops.raster_soft_bwd(tuple(t), d["p2f"], d["ndc"], d["faces"], d["clip"], perspective_correct=d["persp"],
                                  slots=d["slots"], z_clip=d["zc"])
    return out.cpu().numpy()


def _where(d, ref, j):
    """what element j of the flat (B,V,3) result is and which fragments deposit into it"""
    V = d["V"]
    hit = (ref["idx"] == j).any(axis=1)
    frs = [f"(view {b}, fragment {i}, face {f}, c9 entry {int(np.nonzero(row == j)[0][0])})"
           for (b, i, f), row in zip(ref["where"][hit][:6], ref["idx"][hit][:6])]
    return f"element (view {j // (3 * V)}, vertex {(j % (3 * V)) // 3}, component {j % 3}) <- {hit.sum()} fragments: " + ", ".join(frs)


def _assert_bits(d, ref, got, want, what):
    got, want = got.reshape(-1), want.reshape(-1)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    if bad.size:
        j = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ; first: got {got[j]!r} (0x{got.view(np.uint32)[j]:08x}), "
                             f"restated {want[j]!r} (0x{want.view(np.uint32)[j]:08x}); {_where(d, ref, j)}")


HARD_IDS = [f"{n}-{s}" for n, s in VP.HARD_CASES]


# ------------------------------------------------------------------------------------------------ (a) one fragment at a time
def _one_fragment_at_a_time(ops, dev, d, ref, what):
    B, S, K, n = d["B"], d["S"], d["K"], d["B"] * d["V"] * 3
    where, idx, c9 = ref["where"], ref["idx"], ref["c9"]
    assert len(where) == int((d["p2f_np"] >= 0).sum())                 # every fragment is restated, none skipped
    groups = VP.vertex_groups(where, d["faces_np"])
    assert sum(g.size for g in groups) == len(where)
    print(f"{what}: {len(where)} fragments in {len(groups)} groups (launches)")
    dense = [None if g is None else torch.from_numpy(g).to(dev) for g in ref["grads"]]
    per_view = S * S * (K or 1)
    for gi, grp in enumerate(groups):
        flat = torch.from_numpy(where[grp, 0] * per_view + where[grp, 1]).to(dev)
        masked = []
        for g in dense:
            m = torch.zeros_like(g)
            width = g.numel() // (B * per_view)
            m.view(B * per_view, width)[flat] = g.view(B * per_view, width)[flat]
            masked.append(m)
        got = _launch(ops, dev, d, masked).reshape(-1)
        want = np.zeros(n, F32)
        touched = idx[grp].ravel()
        assert np.unique(touched).size == touched.size
        want[touched] = c9[grp].ravel()
        assert not np.isnan(got).any()
        bad = np.nonzero(got != want)[0]                                # numeric ==: bit equality but for +0 / -0
        if bad.size:
            j = int(bad[0])
            raise AssertionError(f"{what}, group {gi}: {bad.size} elements differ; first: got {got[j]!r} (0x{got.view(np.uint32)[j]:08x}), "
                                 f"restated {want[j]!r} (0x{want.view(np.uint32)[j]:08x}); {_where(d, ref, j)}")


@pytest.mark.parametrize("S", [17, 32])
def test_hard_backward_one_fragment_at_a_time(dev, ops, monkeypatch, S):
    d = _hard_scene(dev, ops, "cow", S)
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    _one_fragment_at_a_time(ops, dev, d, _reference(("cow", S), d), f"cow S={S}")


@pytest.mark.parametrize("case", ["k4-clip", "cow from inside/p1", "cow from inside/n1"])
def test_soft_backward_one_fragment_at_a_time(dev, ops, monkeypatch, case):
    """about 20 launches each (cow from inside with K = 2 and blur would need 68: it is left to (b) and (c))"""
    d = _soft_scene(dev, ops, case)
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    _one_fragment_at_a_time(ops, dev, d, _reference(case, d), case)


# ------------------------------------------------------------------------------------------ (b) fixed point, bit for bit
@pytest.mark.parametrize("name,S", VP.HARD_CASES, ids=HARD_IDS)
def test_hard_backward_fixed_point_equals_the_restatement_bit_for_bit(dev, ops, name, S):
    assert ops.is_deterministic()
    d = _hard_scene(dev, ops, name, S)
    ref = _reference((name, S), d)
    got = _launch(ops, dev, d, ref["grads"])
    _assert_bits(d, ref, got, ref["det"], f"{name} S={S}")
    print(f"{name} S={S}: all {got.size} elements equal ({len(ref['where'])} fragments, {ref['attempt']} rescalings)")


@pytest.mark.parametrize("case", list(VP.SOFT_CASES))
def test_soft_backward_fixed_point_equals_the_restatement_bit_for_bit(dev, ops, case):
    assert ops.is_deterministic()
    d = _soft_scene(dev, ops, case)
    for which in WHICH:
        ref = _reference(case, d, which)
        got = _launch(ops, dev, d, ref["grads"])
        _assert_bits(d, ref, got, ref["det"], f"{case} [{which}]")
        print(f"{case} [{which}]: all {got.size} elements equal ({len(ref['where'])} fragments, {ref['attempt']} rescalings)")


# ------------------------------------------------------------------------------ (c) float atomics, summation-only bound
def _float_atomics_within_the_summation_bound(ops, dev, d, ref, what):
    got = _launch(ops, dev, d, ref["grads"]).reshape(-1)
    assert got.size == d["B"] * d["V"] * 3
    VP.assert_within_summation_bound(got, ref["idx"], ref["c9"], what, lambda j: _where(d, ref, j))


@pytest.mark.parametrize("name,S", VP.HARD_CASES, ids=HARD_IDS)
def test_hard_backward_float_atomics_within_the_summation_bound(dev, ops, monkeypatch, name, S):
    d = _hard_scene(dev, ops, name, S)
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    _float_atomics_within_the_summation_bound(ops, dev, d, _reference((name, S), d), f"{name} S={S}")


@pytest.mark.parametrize("case", list(VP.SOFT_CASES))
def test_soft_backward_float_atomics_within_the_summation_bound(dev, ops, monkeypatch, case):
    d = _soft_scene(dev, ops, case)
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    _float_atomics_within_the_summation_bound(ops, dev, d, _reference(case, d), case)


# ---------------------------------------------------------------------------------------------------- (d) projection backward
@pytest.mark.parametrize("V", [2930, 3])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_project_verts_bwd_equals_the_restatement_bit_for_bit(dev, ops, B, V):
    """upstream: the fixed-point raster backward of the cow at S = 17 under B cameras (dense over the visible vertices);
    V = 3: the three vertices of the face with the most fragments, with their rows of that gradient"""
    import _scenes
    import _vcolref as VC
    S = 17
    verts, faces = np.asarray(VC.cow()["verts"], F32), np.asarray(VC.cow()["faces"], np.int32)
    assert verts.shape[0] == 2930
    R, T = _scenes.random_cameras(B, 11)
    vd, fd = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    Rd, Td = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    ndc = ops.project_verts(vd, Rd, Td)
    p2f = ops.raster_fwd(ndc, fd, S)[0]
    gndc = ops.raster_bwd(torch.from_numpy(VP.upstream((B, S, S, 3), S)).to(dev), p2f, ndc, fd)
    if V == 3:
        covered = p2f[p2f >= 0].cpu().numpy()
        keep = torch.from_numpy(faces[np.bincount(covered).argmax()].astype(np.int64)).to(dev)
        vd, gndc, verts = vd[keep].contiguous(), gndc[:, keep].contiguous(), verts[keep.cpu().numpy()]
    g_np = gndc.cpu().numpy()
    assert g_np.shape == (B, V, 3) and np.count_nonzero(g_np) >= 9            # (views that do not see the face give zero rows)
    want = VP.project_verts_bwd_f32(verts, R, T, VP.INV_TAN_HALF_FOV, g_np)
    got = ops.project_verts_bwd(vd, Rd, Td, gndc)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # accumulate into a given gradient: the same tensor comes back, with the sum
    base = np.random.default_rng(B).standard_normal((V, 3)).astype(F32)
    want = VP.project_verts_bwd_f32(verts, R, T, VP.INV_TAN_HALF_FOV, g_np, out=base)
    out = torch.from_numpy(base.copy()).to(dev)
    back = ops.project_verts_bwd(vd, Rd, Td, gndc, out=out)
    assert back is out
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
