"""The numpy restatement of the texture-path backward (tests/_texpath_ref.py) pinned on the CPU, before any GPU test relies
on it.  Its fp64 reading must be the definitions the suite already has -- _mipref.shade_bwd (which at one level and
lambda = 0 is the plain kernel), _vcolref.shade_bwd, _atlasref.shade_bwd -- per element at 1e-12 of the largest element, on
the CPU oracle's fragments; its fp32 reading must be within the bar the existing GPU tests hold the kernels to (1e-5 of the
largest element), stated once, here; and its fp32 deposits, added in fp64, must be the C oracle's texture gradient.  k comes
from _mipref._blend in both precisions (_texpath_ref.blend_k).

The C oracle (oracle/raster_ref.c:ref_shade_bwd) is itself a mixed reading: k, g k and every deposit g k (wx wy) are fp32, the
sums are fp64, and its d/d(u,v) multiplies fp32 tap differences in fp64.  So the all-fp64 restatement is NOT the C oracle at
1e-12 (they differ by fp32 roundings, about 1e-7); what is exact is: the fp32 deposits summed in fp64 are the oracle's
texture gradient (measured 0.0 but for the order of the fp64 sums), and the oracle's grad_uv lies between the two readings
(asserted at the fp32 bar).

The mutation check at the end documents why the per-element tests exist: a restatement with the weights of two footprint
corners swapped on one fragment is caught by the per-element comparison on every scene, and on four of the ten it stays
inside 1e-5 of the largest element, the bar of the existing tests."""
import functools

import numpy as np
import pytest

import _atlasref as AT
import _mipref as M
import _scatter_scene as sc
import _texpath_ref as TP
import _vcolref as VC

F32, F64 = np.float32, np.float64
EXACT, BAR = 1e-12, 1e-5


def _stack(frags):
    return tuple(np.stack([f[i] for f in frags]) for i in range(4))


@functools.lru_cache(maxsize=None)
def _cow(S, T):
    """-> (frag (B,...), verts_uvs, faces_uvs, texture): the cow under _mipref.cameras(), the CPU oracle's fragments"""
    case = M.oracle_case(S, T)
    m = case["mesh"]
    return _stack(case["frags"]), m["verts_uvs"], m["faces_uvs"].astype(np.int32), case["tex"]


def _plain_scene(name):
    """-> (frag, verts_uvs, faces_uvs, texture, grad_rgb)"""
    kind, S, T = name
    if kind in ("scatter", "edge"):
        frag = sc.fragments() if kind == "scatter" else TP.edge_fragments()
        return frag, sc.VERTS_UVS, sc.FACES_UVS, sc.texture(T), sc.grad_rgb()
    frag, uvs, fuv, tex = _cow(S, T)
    if kind == "clamped":
        uvs = TP.clamped_uvs(uvs)
    return frag, uvs, fuv, tex, M.upstream(S)


PLAIN = [("cow", 17, 48), ("cow", 17, 64), ("cow", 32, 48), ("cow", 32, 64), ("scatter", 40, 4), ("scatter", 40, 64),
         ("scatter", 40, 1024), ("edge", 40, 64), ("clamped", 17, 64), ("clamped", 32, 64)]


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    scale = np.abs(ref).max()
    worst = np.abs(got - ref).max() / scale
    print(f"{what}: {worst:.3e} of the largest element (bound {rtol:.0e})")
    assert scale > 0 and worst <= rtol, what
    return worst


def _both(fn, frag):
    """the restatement in both precisions, k from _mipref._blend"""
    r64, r32 = fn(TP.blend_k(frag, F64), F64), fn(TP.blend_k(frag, F32), F32)
    assert r64["c"].dtype == F64 and r32["c"].dtype == F32
    return r64, r32


def _mip_definition(g64, frag, uvs, fuv, pyr, T, L, lam):
    B = frag[0].shape[0]
    gpyr = np.zeros(M.numel(T, L), F64)
    guv = []
    for b in range(B):
        fr = tuple(a[b] for a in frag)
        _, uv = M.shade_bwd(g64[b], fr, uvs, fuv, pyr, T, L, lam[b], F64, gpyr=gpyr)
        guv.append(uv)
    return gpyr, np.stack(guv)


def _gbary_of(guv, frag, uvs, fuv):
    """uv = sum_j b_j uv_j: gbary_j = gu u_j + gv v_j in fp64"""
    p2f = frag[0]
    t = np.asarray(uvs, F64)[np.asarray(fuv)[np.maximum(p2f, 0)]]                    # (B,S,S,3,2)
    out = guv[..., None, 0] * t[..., 0] + guv[..., None, 1] * t[..., 1]
    return np.where((p2f >= 0)[..., None], out, 0.0)


def _fp32_at_a_large_side(r32, r64, g, T):
    """T = 1024 (hand-made fragments, not the CPU oracle's): the fp32 reading is NOT within 1e-5 of the fp64 one, and no
    fp32 evaluation of uv_footprint can be.  u' = ((u 2 - 1) + 1) / 2 carries 0.75 * 2^-24 (half an ulp of gx < 1, half an
    ulp of a sum < 2, halved), ix = u' (T - 1) turns that into 0.75 ulp(T - 1) and adds half an ulp of its own; wx1 = ix - fx
    is exact.  So each weight is off by up to 1.25 ulp(T - 1), a corner's wx wy by up to 2.5 ulp(T - 1) = 1.5e-4 at T = 1024
    (ulp 2^-14), and a deposit g k (wx wy) by that times max |g| (k <= 1).  A texel of this scene takes one deposit (two
    where the lone pixel of view 1 repeats a pixel of view 2), so that, times the count, is the bound per element.
    Measured: 9.6e-5 of the largest element.  The existing GPU test of this scene compares
    with the C oracle, whose deposits are these fp32 values (0.0 apart, asserted by the caller)."""
    diff = np.abs(TP.scatter64(r32) - TP.scatter64(r64))
    i, _ = TP.deposits(r32)
    most = int(np.bincount(i).max())
    assert most <= 2
    bound = most * 2.5 * float(np.spacing(F32(T - 1))) * float(np.abs(g).max())
    print(f"fp32 texture gradient vs fp64 at T = {T}: {diff.max():.3e} absolute (bound {bound:.3e}), "
          f"{diff.max() / np.abs(TP.scatter64(r64)).max():.3e} of the largest element")
    assert diff.max() <= bound


# ---------------------------------------------------------------------------------------------------- plain and supersampled
@pytest.mark.parametrize("name", PLAIN, ids=lambda n: "%s%d-T%d" % n)
def test_plain_restatement_is_the_definition_and_the_oracle(name):
    from oracle import render_ref as rr
    frag, uvs, fuv, tex, g = _plain_scene(name)
    T = tex.shape[0]
    r64, r32 = _both(lambda k, dt: TP.restate_shade(g, frag, uvs, fuv, tex, k, dt), frag)
    print(f"{name}: {len(r64['where'])} fragments")
    assert len(r64["where"]) == int((frag[0] >= 0).sum()) > 50
    gtex, guv = _mip_definition(g.astype(F64), frag, uvs, fuv, tex.reshape(-1), T, 1, np.zeros(frag[0].shape, F32))
    _close(TP.scatter64(r64), gtex, EXACT, "fp64 texture gradient vs _mipref")
    _close(TP.dense(r64, "guv", frag), guv, EXACT, "fp64 grad_uv vs _mipref")
    _close(TP.dense(r64, "gbary", frag), _gbary_of(guv, frag, uvs, fuv), EXACT, "fp64 grad_bary vs the definition")
    if T <= 64:
        _close(TP.scatter64(r32), TP.scatter64(r64), BAR, "fp32 texture gradient vs fp64")
        _close(TP.dense(r32, "guv", frag), TP.dense(r64, "guv", frag), BAR, "fp32 grad_uv vs fp64")
        _close(TP.dense(r32, "gbary", frag), TP.dense(r64, "gbary", frag), BAR, "fp32 grad_bary vs fp64")
    else:
        _fp32_at_a_large_side(r32, r64, g, T)
    # the C oracle: fp32 deposits, fp64 sums; its grad_uv is a mixed reading (module docstring)
    otex, ouv = np.zeros((T, T, 3), F64), []
    for b in range(frag[0].shape[0]):
        _, uv = rr.shade_bwd(g[b], tuple(a[b] for a in frag), uvs, fuv, tex, otex, want_uv=True)
        ouv.append(uv)
    _close(TP.scatter64(r32), otex.reshape(-1), EXACT, "fp32 deposits summed in fp64 vs the C oracle's texture gradient")
    if T <= 64:             # (T = 1024: the fp32 footprint again, 6.4e-5)
        _close(np.stack(ouv), TP.dense(r64, "guv", frag), BAR, "the C oracle's grad_uv vs fp64")


@pytest.mark.parametrize("a", [2, 3])
def test_supersampled_restatement_is_the_plain_one_behind_the_box_filter(a):
    S, T = 12, 48
    frag, uvs, fuv, tex = _cow(a * S, T)
    g = M.upstream(S)
    r64, r32 = _both(lambda k, dt: TP.restate_shade(g, frag, uvs, fuv, tex, k, dt, a=a), frag)
    print(f"a = {a}: {len(r64['where'])} fragments")
    assert len(r64["where"]) > 50
    sub = np.repeat(np.repeat(g.astype(F64) / (a * a), a, axis=2), a, axis=3)            # box_down_bwd
    gtex, guv = _mip_definition(sub, frag, uvs, fuv, tex.reshape(-1), T, 1, np.zeros(frag[0].shape, F32))
    _close(TP.scatter64(r64), gtex, EXACT, "fp64 texture gradient vs _mipref behind the box filter")
    _close(TP.dense(r64, "guv", frag), guv, EXACT, "fp64 grad_uv")
    _close(TP.scatter64(r32), TP.scatter64(r64), BAR, "fp32 texture gradient vs fp64")
    _close(TP.dense(r32, "gbary", frag), TP.dense(r64, "gbary", frag), BAR, "fp32 grad_bary vs fp64")
    # the bound counts a pixel once if any of its sub-pixels holds a face
    block = (frag[0] >= 0).reshape(M.B, S, a, S, a).any(axis=(2, 4))
    assert r32["bound"] == float((np.abs(g.astype(F64)) * block[:, None]).sum()) < float(np.abs(g.astype(F64)).sum())


# ---------------------------------------------------------------------------------------------------------------------- mip
@pytest.mark.parametrize("case", [0, 4])
def test_mip_restatement_is_mipref(case):
    S, T, L = M.CASES[case]
    frag, uvs, fuv, tex = _cow(S, T)
    oc = M.oracle_case(S, T)
    g = M.upstream(S)
    lam = np.stack([M.lod(fr, oc["ndc"][b], oc["mesh"]["faces"], uvs, fuv, T, L) for b, fr in enumerate(oc["frags"])]).astype(F32)
    n, zero, frac, top = M.classes(lam, frag[0] >= 0, L)
    print(f"case {case}: covered {n}: lambda = 0 on {zero}, fractional on {frac}, clamped on {top}")
    assert zero >= 10 and frac >= 80
    pyr = M.pack(M.build(tex, L, F32))
    r64, r32 = _both(lambda k, dt: TP.restate_mip(g, frag, uvs, fuv, pyr, lam, T, L, k, dt), frag)
    gpyr, guv = _mip_definition(g.astype(F64), frag, uvs, fuv, pyr.astype(F64), T, L, lam)
    _close(TP.scatter64(r64), gpyr, EXACT, "fp64 per-level gradient vs _mipref")
    _close(TP.dense(r64, "guv", frag), guv, EXACT, "fp64 grad_uv vs _mipref")
    _close(TP.scatter64(r32), TP.scatter64(r64), BAR, "fp32 per-level gradient vs fp64")
    _close(TP.dense(r32, "guv", frag), TP.dense(r64, "guv", frag), BAR, "fp32 grad_uv vs fp64")
    _close(TP.dense(r32, "gbary", frag), TP.dense(r64, "gbary", frag), BAR, "fp32 grad_bary vs fp64")
    # the upper level's deposits exist exactly where lambda is fractional
    assert int(r32["valid"][:, 12:].any(axis=1).sum()) == frac


# ---------------------------------------------------------------------------------------------------- vertex colours, atlas
def _vc_scene(name):
    if name == "own":
        p2f, faces = sc.own_faces()
        frag = (p2f,) + sc.fragments()[1:]
        return frag, faces, sc.colours(3 * sc.S * sc.S), sc.grad_rgb()
    frag = _stack(VC.oracle_fragments(name)[0])
    faces = np.asarray(VC.cow()["faces"], np.int32)
    return frag, faces, VC.colours(VC.cow()["verts"].shape[0]), VC.upstream(name)


@pytest.mark.parametrize("name", [17, 32, "own"])
def test_vertex_colour_restatement_is_vcolref(name):
    frag, faces, col, g = _vc_scene(name)
    r64, r32 = _both(lambda k, dt: TP.restate_vc(g, frag, faces, col, k, dt), frag)
    gcol, gbary = np.zeros(col.shape, F64), []
    for b in range(frag[0].shape[0]):
        if (frag[0][b] >= 0).any():
            _, gb = VC.shade_bwd(g[b], tuple(a[b] for a in frag), faces, col, F64, gcol)
        else:
            gb = np.zeros(frag[0].shape[1:] + (3,), F64)
        gbary.append(gb)
    print(f"{name}: {len(r64['where'])} fragments")
    _close(TP.scatter64(r64), gcol.reshape(-1), EXACT, "fp64 colour gradient vs _vcolref")
    _close(TP.dense(r64, "gbary", frag), np.stack(gbary), EXACT, "fp64 grad_bary vs _vcolref")
    _close(TP.scatter64(r32), TP.scatter64(r64), BAR, "fp32 colour gradient vs fp64")
    _close(TP.dense(r32, "gbary", frag), TP.dense(r64, "gbary", frag), BAR, "fp32 grad_bary vs fp64")
    assert r32["bound"] >= np.abs(r32["c"].astype(F64)).reshape(len(r32["c"]), 3, 3).sum(axis=0).max()


@pytest.mark.parametrize("R", [1, 4, 7])
def test_atlas_restatement_is_atlasref(R):
    frag = _stack(VC.oracle_fragments(17)[0])
    F = VC.cow()["faces"].shape[0]
    g = VC.upstream(17)
    r64, r32 = _both(lambda k, dt: TP.restate_atlas(g, frag, R, F, k, dt), frag)
    ref = np.zeros((F, R, R, 3), F64)
    for b in range(frag[0].shape[0]):
        AT.shade_bwd(g[b], tuple(a[b] for a in frag), R, F, F64, ref)
    _close(TP.scatter64(r64), ref.reshape(-1), EXACT, "fp64 atlas gradient vs _atlasref")
    _close(TP.scatter64(r32), TP.scatter64(r64), BAR, "fp32 atlas gradient vs fp64")


# --------------------------------------------------------------------------------------------------------- the clamped scene
@pytest.mark.parametrize("S", [17, 32])
def test_the_clamped_scene_clamps_at_both_ends_of_u_and_v(S):
    T = 64
    frag, uvs, fuv, tex, g = _plain_scene(("clamped", S, T))
    r = TP.restate_shade(g, frag, uvs, fuv, tex, TP.blend_k(frag, F32), F32)
    counts = TP.clamp_counts(r, T)
    print(f"clamped cow S = {S}: (u low, u high, v low, v high, x1 == T, yf1 == T) = {counts} of {len(r['where'])} fragments")
    assert min(counts) >= TP.CLAMP_MIN
    # and the unclamped cow has none at the high end: the vx1 / vy1 masks are this scene's alone
    frag, uvs, fuv, tex, g = _plain_scene(("cow", S, T))
    plain = TP.clamp_counts(TP.restate_shade(g, frag, uvs, fuv, tex, TP.blend_k(frag, F32), F32), T)
    print(f"the cow as it is: {plain}")


# ------------------------------------------------------------------------------------------------------- the mutation check
# the scenes on which the least visible swap passes the old bar (measured: 4.6e-6, 5.2e-6, 9.4e-6 and 8.0e-7 of the largest
# element; on the others 4.6e-5 to 1.0e-3)
INSIDE_THE_OLD_BAR = {("cow", 17, 48), ("cow", 32, 48), ("cow", 32, 64), ("edge", 40, 64)}


def _swap_two_corners(r, n):
    """the deposits of fragment n with the weights of footprint corners 0 and 1 swapped: c = (g k) w, so the values swap"""
    c = r["c"].copy()
    c[n, 0:3], c[n, 3:6] = r["c"][n, 3:6], r["c"][n, 0:3]
    return dict(r, c=c)


@pytest.mark.parametrize("name", PLAIN, ids=lambda n: "%s%d-T%d" % n)
def test_a_swap_of_two_corner_weights_is_caught_per_element(name):
    """On every scene: the fragment whose swap moves the result least.  Per element the mutant differs from the restatement
    (what the bit-for-bit tests see: six elements, two texels by three channels); against the old bar, 1e-5 of the largest
    element, it passes on four of the ten scenes (INSIDE_THE_OLD_BAR)."""
    frag, uvs, fuv, tex, g = _plain_scene(name)
    r = TP.restate_shade(g, frag, uvs, fuv, tex, TP.blend_k(frag, F32), F32)
    ref = TP.scatter64(r)
    both = r["valid"][:, 0] & r["valid"][:, 3]
    move = np.abs(r["c"][:, 0:3].astype(F64) - r["c"][:, 3:6].astype(F64)).max(axis=1)
    move[~both | (move == 0)] = np.inf
    n = int(np.argmin(move))
    mutant = TP.scatter64(_swap_two_corners(r, n))
    differ = int((mutant.astype(F32) != ref.astype(F32)).sum())
    share = np.abs(mutant - ref).max() / np.abs(ref).max()
    print(f"{name}: fragment {tuple(r['where'][n])}: {differ} elements differ, {share:.3e} of the largest element "
          f"({'inside' if share <= BAR else 'outside'} the 1e-5 bar)")
    assert differ >= 2
    assert (share <= BAR) == (name in INSIDE_THE_OLD_BAR)
