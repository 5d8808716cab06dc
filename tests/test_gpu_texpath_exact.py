"""The texture-path backward on the GPU -- the K = 1 shading kernels that share csrc/shadek1.h and csrc/tilebins.h:
shade_bwd_kernel plain and supersampled (csrc/shade.hip), shade_mip_bwd_kernel (csrc/mipmap.hip), shade_vc_bwd_kernel
(csrc/vcolor.hip), shade_atlas_bwd_kernel (csrc/atlas.hip), with the fixed-point scatter of csrc/det.h -- against its fp32
restatement (tests/_texpath_ref.py, pinned on the CPU by tests/test_texpath_ref.py) PER ELEMENT and without a tolerance.
The files are built without FMA contraction and with correctly rounded division, and but for the blend factor k the backward
has only + - * /, comparisons and floorf, so numpy's float32 reproduces every deposit and every per-pixel output bit for
bit; the default scatter is integer addition at a power-of-two scale, so every scattered output is reproduced bit for bit
as well.  The norm tests (1e-5 / 1e-4 of the largest element) and the recorded "parent" bits see none of: a texel, vertex or
pixel far below the largest element that is entirely wrong, a dropped footprint corner of small weight, a border texel fed
from the wrong row of the vertical flip, a gv of the wrong sign where the texture is flat, a clamped footprint whose gu is
not zeroed (tests/test_texpath_ref.py shows a mutant that passes the old bar).

k = wnum / denom has expf, and the device's expf is not numpy's.  It is READ BACK from the GPU, exactly (probe_k): one launch
of ops.shade_bwd(want_uv=True) on the same pix_to_face / zbuf / dists with a UV table of zeros, T = 2, a texture that is zero
but for tex[T-1, 1, 0] = 1, and grad_rgb = (1, 0, 0).  Then u = v = 0 (every product b_j * 0 is a zero), gx = 0 * 2 - 1 = -1,
ix = ((-1 + 1) / 2) * 1 = 0: not clamped, x0 = yf0 = 0, wx1 = wy1 = 0, wx0 = wy0 = 1, all four taps exist, r0 = T - 1 = 1,
so t01 = tex[1][1] = (1, 0, 0) and the other taps are 0.  gk = (1 * k, 0 * k, 0 * k) = (k, 0, 0) and
    gix = ((0 + k * ((1 - 0) * 1 + (0 - 0) * 0)) + 0 * (...)) + 0 * (...) = k * (1 + 0) = k,    gu = gix * (float)(T - 1) = k * 1 = k:
grad_uv[..., 0] is the kernel's own k per pixel, bit for bit.  The vertex-colour kernel gives the same through grad_bary with
every colour (1, 0, 0) (gbary_j = (k * 1 + 0 * 0) + 0 * 0 = k); the two probes are asserted equal bit for bit.  The mip and
atlas kernels have no such output: they call the same blend_k1 from the same header under the same flags, and take the plain
probe.  The probed k is itself checked (d) against k evaluated in fp64 from the same fp32 dists / zbuf, in ulps.

(a) one fragment at a time (float atomics, groups of fragments that share no texel / vertex: every touched element is
    0 + c, exact): names the view, pixel, face, corner and channel that is wrong;
(b) fixed point (the default), dense upstream gradient: every element of every scattered output equals
    det_scatter(idx, c, bound=...) bit for bit, the bound restated per entry point; every per-pixel output (grad_uv,
    grad_bary) equals the restatement bit for bit on covered pixels and is +0.0 elsewhere; accumulation into a given
    gradient is base + v in fp32;
(c) float atomics, dense gradient: |got - sum| <= n 2^-24 sum|c| per element (_vertexpath_ref.assert_within_summation_bound);
(d) the probed k.

Inputs are the GPU's own fragments (bit-pinned to the oracle elsewhere), copied to the host.  Kernel x scene:
    plain     cow B = 2 S = 17 (ragged 2 x 2 tiles) and 32, T = 48 and 64; the hand-made scatter scene S = 40 (an empty view,
              a lone pixel, a full view) at T = 4 (hundreds of terms per LDS sum), 64, 1024 (1024 distinct keys in a tile);
              the same with dist > 0 at T = 64 (_texpath_ref.edge_fragments: the one scene on which k is not exactly 1);
              the clamped cow (UV table through _texpath_ref.clamped_uvs: cx / cy at both ends, x1 = T / yf1 = T) S = 17, 32
    ss        a = 2, 3 on S = 12 upstream (fragments at 24, 36), T = 48: g / 9 is a real rounding
    mip       _mipref.CASES[0] and [4] with the GPU's mip_lod plane, the packed per-level gradient (want_levels) -- and the
              folded grad_texture through mip_adjoint's restatement
    vc        cow S = 17, 32; _scatter_scene.own_faces(): 768 distinct vertices in one tile
    atlas     R = 1, 4, 7 on cow S = 17
(a) runs the plain kernel on cow S = 17 T = 64 (7 launches) and the clamped cow S = 17 (9), vertex colours on cow S = 17 (3):
whole views, nothing coarsened.

OUT OF SCOPE, and so still held only to the norm tests and the recorded bits: the lit variants (phong.h has powf and
normalisations) and the K > 1 soft path (an expf per layer) -- no numpy restatement reproduces their outputs to the bit."""
import numpy as np
import pytest
import torch

import _mipref as M
import _scatter_scene as sc
import _scenes
import _texpath_ref as TP
import _vcolref as VC
import _vertexpath_ref as VP

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64

# (d) the largest |k_gpu - k_fp64| in ulps of k, measured on MI355X outside the class that must be exactly 1; the bar is twice
# the measured value.  Over the rasterised scenes, the scatter scene and the quad: dist <= 0 there, so prob >= 1/2 and
# k = prob / (prob + 1e-10) rounds to 1.0f on EVERY fragment, whatever expf returns; the figure is 2e-10 / 2^-23, the distance
# of 1.0f from the fp64 value at prob = 1/2.
K_MEASURED_ULP = 0.001678
K_BAR_ULP = 2 * K_MEASURED_ULP
# Over ("edge",), dist / sigma in [0, 30), the only set with k != 1 (1269 of 1601 fragments): 23.35 ulp, above the 8 ulp that
# three expf and four roundings would explain.  The cause is the conditioning of exp, not the device's expf: x = dist / sigma
# is rounded to fp32 before expf, half an ulp of x near 30 is 2^-20, and exp turns that absolute error into a relative one:
# up to 16 ulp of exp(x), more with the rounding of 1e-4f itself (x 2.5e-9 |x|).  numpy's correctly rounded fp32 evaluation
# (_mipref._blend with np.float32) is the same 23.349 ulp from fp64, at the same fragment (x = 29.31, k = 1.86e-3).  What IS
# the device's expf is the distance of the probed k from that fp32 evaluation: held to the 8 ulp.
K_EDGE_MEASURED_ULP = 23.349
K_EDGE_BAR_ULP = 2 * K_EDGE_MEASURED_ULP
K_EXPF_BAR_ULP = 8.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)           # (a copy: the references are read-only arrays)


# ------------------------------------------------------------------------------------------------------------- fragment sets
_FRAGS, _CASES, _REFS = {}, {}, {}


def _frags(dev, ops, name):
    """name: ("cow", S) -- the GPU's own fragments of the cow under _mipref.cameras() --, ("quad", S) -- those of
    _vcolref.two_triangles(), for (d) -- or ("scatter",) / ("own",) / ("edge",): the hand-made ones -> dict(frag device tuple, frag_np,
    n_faces, + the cow's mesh tensors)"""
    if name not in _FRAGS:
        d = dict(name=name)
        if name[0] == "cow":
            m = _scenes.load_asset("cow")
            R, T = M.cameras()
            d["mesh"] = m
            d["faces"] = _t(m["faces"].astype(np.int32), dev)
            d["ndc"] = ops.project_verts(_t(m["verts"], dev), _t(R, dev), _t(T, dev))
            d["frag"] = ops.raster_fwd(d["ndc"], d["faces"], name[1])
            d["n_faces"] = m["faces"].shape[0]
        elif name[0] == "quad":
            verts, faces, R, T = VC.two_triangles()
            d["faces"] = _t(faces, dev)
            d["ndc"] = ops.project_verts(_t(verts, dev), _t(R, dev), _t(T, dev))
            d["frag"] = ops.raster_fwd(d["ndc"], d["faces"], name[1])
            d["n_faces"] = faces.shape[0]
        else:
            fr = TP.edge_fragments() if name[0] == "edge" else sc.fragments()
            if name[0] == "own":
                p2f, faces = sc.own_faces()
                fr = (p2f,) + fr[1:]
                d["faces_np"] = faces
            d["frag"] = tuple(_t(a, dev) for a in fr)
            d["n_faces"] = sc.S * sc.S if name[0] == "own" else 2
        d["frag_np"] = tuple(a.cpu().numpy() for a in d["frag"])
        d["covered"] = int((d["frag_np"][0] >= 0).sum())
        _FRAGS[name] = d
    return _FRAGS[name]


def probe_k(dev, ops, d):
    """the kernel's own k per pixel, (B,S,S) fp32, 0 where there is no face (module docstring)"""
    if "k" not in d:
        p2f = d["frag"][0]
        B, S, _ = p2f.shape
        uv0 = torch.zeros((1, 2), device=dev)
        fuv0 = torch.zeros((d["n_faces"], 3), dtype=torch.int32, device=dev)
        tex = torch.zeros((2, 2, 3), device=dev)
        tex[1, 1, 0] = 1.0
        g = torch.zeros((B, 3, S, S), device=dev)
        g[:, 0] = 1.0
        _, guv = ops.shade_bwd(g, d["frag"], uv0, fuv0, tex, want_uv=True, want_texture=False)
        k = guv[..., 0].cpu().numpy()
        assert not guv[..., 1].any()                                   # giy = k * ((0 - 0) * 1 + (0 - 1) * 0) = k * (0 + -0) = 0
        k.setflags(write=False)
        d["k"] = k
    return d["k"]


# --------------------------------------------------------------------------------------------------------------------- cases
PLAIN = ["cow17-T48", "cow17-T64", "cow32-T48", "cow32-T64", "scatter-T4", "scatter-T64", "scatter-T1024", "edge-T64",
         "clamped17-T64", "clamped32-T64"]
SS = ["ss2", "ss3"]
MIP = ["mip0", "mip4"]
VCOL = ["vc-cow17", "vc-cow32", "vc-own"]
ATLAS = ["atlas-R1", "atlas-R4", "atlas-R7"]
ALL = PLAIN + SS + MIP + VCOL + ATLAS
SS_S, SS_T = 12, 48


def _case(dev, ops, name):
    """-> dict: kind, fr (the fragment set), g_np (dense upstream), restate(g_np) -> the restatement, run(g, base=None) ->
    (scattered output flat numpy, {per-pixel outputs}), out_shape, and what the failure messages need"""
    if name in _CASES:
        return _CASES[name]
    c = dict(name=name)
    if name in PLAIN:
        scene, T = name.split("-T")
        T = int(T)
        if scene in ("scatter", "edge"):
            fr = _frags(dev, ops, (scene,))
            uvs_np, fuv_np, tex_np, g_np = sc.VERTS_UVS, sc.FACES_UVS, sc.texture(T), sc.grad_rgb()
        else:
            S = int(scene[-2:])
            fr = _frags(dev, ops, ("cow", S))
            m = fr["mesh"]
            uvs_np, fuv_np, tex_np, g_np = m["verts_uvs"], m["faces_uvs"].astype(np.int32), M.texture(T), M.upstream(S)
            if scene.startswith("clamped"):
                uvs_np = TP.clamped_uvs(uvs_np)
        uvs, fuv, tex = _t(uvs_np, dev), _t(fuv_np, dev), _t(tex_np, dev)
        c.update(kind="plain", T=T, out_shape=(T, T, 3), per_pixel=("guv", "gbary"))
        c["restate"] = lambda g: TP.restate_shade(g, fr["frag_np"], uvs_np, fuv_np, tex_np, probe_k(dev, ops, fr), F32)

        def run(g, base=None):
            gt, guv, gb = ops.shade_bwd(g, fr["frag"], uvs, fuv, tex, grad_texture=base, want_uv=True, want_bary=True)
            return gt, dict(guv=guv, gbary=gb)
    elif name in SS:
        a = int(name[2:])
        fr = _frags(dev, ops, ("cow", a * SS_S))
        m = fr["mesh"]
        uvs_np, fuv_np, tex_np, g_np = m["verts_uvs"], m["faces_uvs"].astype(np.int32), M.texture(SS_T), M.upstream(SS_S)
        uvs, fuv, tex = _t(uvs_np, dev), _t(fuv_np, dev), _t(tex_np, dev)
        c.update(kind="ss", T=SS_T, a=a, out_shape=(SS_T, SS_T, 3), per_pixel=("guv", "gbary"))
        c["restate"] = lambda g: TP.restate_shade(g, fr["frag_np"], uvs_np, fuv_np, tex_np, probe_k(dev, ops, fr), F32, a=a)

        def run(g, base=None):
            gt, guv, gb = ops.shade_ss_bwd(g, fr["frag"], uvs, fuv, tex, a, grad_texture=base, want_uv=True, want_bary=True)
            return gt, dict(guv=guv, gbary=gb)
    elif name in MIP:
        S, T, L = M.CASES[int(name[3:])]
        fr = _frags(dev, ops, ("cow", S))
        m = fr["mesh"]
        uvs_np, fuv_np, tex_np, g_np = m["verts_uvs"], m["faces_uvs"].astype(np.int32), M.texture(T), M.upstream(S)
        uvs, fuv, tex = _t(uvs_np, dev), _t(fuv_np, dev), _t(tex_np, dev)
        lod = ops.mip_lod(fr["frag"], fr["ndc"], fr["faces"], uvs, fuv, T, L)
        pyr = ops.mip_build(tex, L)
        lam_np, pyr_np = lod.cpu().numpy(), pyr.cpu().numpy()
        assert np.array_equal(pyr_np, M.pack(M.build(tex_np, L)))
        c.update(kind="mip", T=T, L=L, lam=lam_np, out_shape=(M.numel(T, L),), per_pixel=("guv", "gbary"))
        c["restate"] = lambda g: TP.restate_mip(g, fr["frag_np"], uvs_np, fuv_np, pyr_np, lam_np, T, L, probe_k(dev, ops, fr), F32)

        def run(g, base=None):
            gt, guv, gb, glev = ops.shade_mip_bwd(g, fr["frag"], uvs, fuv, pyr, lod, T, L, grad_texture=base, want_uv=True,
                                                  want_bary=True, want_levels=True)
            return glev, dict(guv=guv, gbary=gb, gtex=gt)
    elif name in VCOL:
        if name == "vc-own":
            fr = _frags(dev, ops, ("own",))
            faces_np, g_np = fr["faces_np"], sc.grad_rgb()
            col_np = sc.colours(3 * sc.S * sc.S)
        else:
            S = int(name[-2:])
            fr = _frags(dev, ops, ("cow", S))
            faces_np, g_np = fr["mesh"]["faces"].astype(np.int32), VC.upstream(S)
            col_np = VC.colours(fr["mesh"]["verts"].shape[0])
        faces, col = _t(faces_np, dev), _t(col_np, dev)
        c.update(kind="vc", faces_np=faces_np, out_shape=col_np.shape, per_pixel=("gbary",))
        c["restate"] = lambda g: TP.restate_vc(g, fr["frag_np"], faces_np, col_np, probe_k(dev, ops, fr), F32)

        def run(g, base=None):
            gc, gb = ops.shade_vc_bwd(g, fr["frag"], faces, col, grad_colours=base, want_bary=True)
            return gc, dict(gbary=gb)
    else:
        R = int(name.split("-R")[1])
        fr = _frags(dev, ops, ("cow", 17))
        F, g_np = fr["n_faces"], VC.upstream(17)
        c.update(kind="atlas", R=R, out_shape=(F, R, R, 3), per_pixel=())
        c["restate"] = lambda g: TP.restate_atlas(g, fr["frag_np"], R, F, probe_k(dev, ops, fr), F32)

        def run(g, base=None):
            return ops.shade_atlas_bwd(g, fr["frag"], R, F, grad_atlas=base), {}
    c.update(fr=fr, g_np=g_np, run=run)
    _CASES[name] = c
    return c


def _launch(dev, c, g, base=None):
    """-> (scattered output flat fp32 numpy, {name: numpy} per-pixel and other outputs)"""
    out, extra = c["run"](g if torch.is_tensor(g) else _t(g, dev), None if base is None else _t(base, dev))
    assert tuple(out.shape) == tuple(c["out_shape"])
    return out.cpu().numpy().reshape(-1), {k: v.cpu().numpy() for k, v in extra.items()}


def _reference(dev, ops, name):
    """The restated deposits of the dense upstream gradient and their fixed-point sum, computed once and left unchanged.
    det_scatter refuses a bound too close to a power of two (the kernel's fp32 bound could sit in the other binade): the
    upstream gradient is then rescaled by 1.25, at most twice -- a condition on the input, no tolerance."""
    if name not in _REFS:
        c = _case(dev, ops, name)
        for attempt in range(3):
            g = (c["g_np"] * F32(1.25) ** attempt).astype(F32)
            r = c["restate"](g)
            assert r["c"].dtype == F32 and len(r["where"]) == c["fr"]["covered"]          # every fragment is restated
            try:
                det = VP.det_scatter(*TP.deposits(r), r["n_out"], bound=r["bound"])
                break
            except VP.BoundNearPowerOfTwo:
                continue
        else:
            raise AssertionError("no usable bound after two rescalings")
        assert r["n_out"] == int(np.prod(c["out_shape"]))
        ref = dict(r, g=g, det=det, attempt=attempt)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[name] = ref
    return _REFS[name]


def _element(c, j):
    ch = j % 3
    t = j // 3
    if c["kind"] in ("plain", "ss"):
        return f"texel (row {t // c['T']}, column {t % c['T']}), channel {ch}"
    if c["kind"] == "mip":
        off = M.texel_offsets(c["T"], c["L"])
        l = int(np.searchsorted(off, t, side="right") - 1)
        n = c["T"] >> l
        return f"level {l} texel (row {(t - off[l]) // n}, column {(t - off[l]) % n}), channel {ch}"
    if c["kind"] == "vc":
        return f"vertex {t}, channel {ch}"
    R = c["R"]
    return f"atlas texel (face {t // (R * R)}, wy {t // R % R}, wx {t % R}), channel {ch}"


def _where(c, ref, j):
    """what element j of the flat scattered output is and which fragments deposit into it"""
    hit = ((ref["idx"] == j) & ref["valid"]).any(axis=1)
    side = c["fr"]["frag_np"][0].shape[1]
    frs = []
    for (b, i, f), row, ok in zip(ref["where"][hit][:6], ref["idx"][hit][:6], ref["valid"][hit][:6]):
        col = int(np.nonzero((row == j) & ok)[0][0])
        frs.append(f"(view {b}, pixel ({i // side}, {i % side}), face {f}, corner {col // 3}, channel {col % 3})")
    return f"{_element(c, j)} <- {int(hit.sum())} fragments: " + ", ".join(frs)


def _assert_bits(c, ref, got, want, what):
    got, want = np.ascontiguousarray(got, F32).reshape(-1), np.ascontiguousarray(want, F32).reshape(-1)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    if bad.size:
        j = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ; first: got {got[j]!r} (0x{got.view(np.uint32)[j]:08x}), "
                             f"restated {want[j]!r} (0x{want.view(np.uint32)[j]:08x}); {_where(c, ref, j)}")


def _assert_pixel_bits(c, ref, got, key, what):
    """a per-pixel output: the restatement on covered pixels, +0.0 elsewhere, bit for bit"""
    want = TP.dense(ref, key, c["fr"]["frag_np"])
    assert got.shape == want.shape and got.dtype == F32 and want.dtype == F32
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    if bad.size:
        b, y, x, j = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {key} differs on {len(bad)} values; first: view {b}, pixel ({y}, {x}), face "
                             f"{c['fr']['frag_np'][0][b, y, x]}, component {j}: got {got[b, y, x, j]!r} "
                             f"(0x{got.view(np.uint32)[b, y, x, j]:08x}), restated {want[b, y, x, j]!r} "
                             f"(0x{want.view(np.uint32)[b, y, x, j]:08x})")


# ------------------------------------------------------------------------------------------------ (a) one fragment at a time
@pytest.mark.parametrize("name", ["cow17-T64", "clamped17-T64", "vc-cow17"])
def test_one_fragment_at_a_time(dev, ops, monkeypatch, name):
    c, ref = _case(dev, ops, name), _reference(dev, ops, name)
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    groups = TP.disjoint_groups(ref)
    assert sum(g.size for g in groups) == len(ref["where"]) == c["fr"]["covered"]
    print(f"{name}: {len(ref['where'])} fragments in {len(groups)} groups (launches), whole views")
    assert len(groups) <= 30
    B, side = c["fr"]["frag_np"][0].shape[:2]
    dense = _t(ref["g"], dev)
    idx, cc, valid, where = ref["idx"], ref["c"], ref["valid"], ref["where"]
    for gi, grp in enumerate(groups):
        keep = torch.zeros((B, side * side), dtype=torch.bool, device=dev)
        keep[_t(where[grp, 0], dev), _t(where[grp, 1], dev)] = True
        masked = torch.where(keep.view(B, 1, side, side), dense, torch.zeros_like(dense))
        got, pix = _launch(dev, c, masked)
        want = np.zeros(ref["n_out"], F32)
        touched = idx[grp][valid[grp]]
        assert np.unique(touched).size == touched.size
        want[touched] = cc[grp][valid[grp]]
        assert not np.isnan(got).any()
        bad = np.nonzero(got != want)[0]                                # numeric ==: bit equality but for +0 / -0
        if bad.size:
            j = int(bad[0])
            raise AssertionError(f"{name}, group {gi}: {bad.size} elements differ; first: got {got[j]!r} (0x{got.view(np.uint32)[j]:08x}), "
                                 f"restated {want[j]!r} (0x{want.view(np.uint32)[j]:08x}); {_where(c, ref, j)}")
        flat = where[grp, 0] * side * side + where[grp, 1]
        for key in c["per_pixel"]:                                      # the group's own pixels see their dense upstream values
            g_px = pix[key].reshape(B * side * side, -1)[flat]
            assert np.array_equal(g_px.view(np.int32), ref[key][grp].view(np.int32)), (name, gi, key)


# ------------------------------------------------------------------------------------------ (b) fixed point, bit for bit
def _assert_scene(c, ref):
    """the scene holds what it is there for (asserted on the GPU's own fragments)"""
    name = c["name"]
    if name.startswith("clamped"):
        counts = TP.clamp_counts(ref, c["T"])
        print(f"{name}: clamped at (u low, u high, v low, v high) and x1 == T, yf1 == T: {counts}")
        assert min(counts) >= TP.CLAMP_MIN
    if c["kind"] == "mip":
        cov = c["fr"]["frag_np"][0] >= 0
        n, zero, frac, top = M.classes(c["lam"], cov, c["L"])
        print(f"{name}: covered {n}: lambda = 0 on {zero}, fractional on {frac}, clamped on {top}")
        assert zero >= 10 and frac >= 80
        if c["L"] <= 3:
            assert top >= 10
        assert not c["lam"][~cov].any()
    if name == "vc-own":
        p2f, faces = c["fr"]["frag_np"][0][2], c["faces_np"]
        assert np.unique(faces[p2f[:16, :16].ravel()]).size == 768
    if name == "scatter-T1024":
        p2f = c["fr"]["frag_np"][0][2]
        first = ref["where"][:, 0] == 2
        tile = first & (ref["where"][:, 1] // sc.S < 16) & (ref["where"][:, 1] % sc.S < 16)
        assert np.unique(ref["idx"][tile] // 3).size == 1024 and (p2f >= 0).all()
    if name == "scatter-T4":
        assert np.unique(ref["idx"][ref["valid"]] // 3).size == 16


@pytest.mark.parametrize("name", ALL)
def test_fixed_point_equals_the_restatement_bit_for_bit(dev, ops, name):
    assert ops.is_deterministic()
    c, ref = _case(dev, ops, name), _reference(dev, ops, name)
    _assert_scene(c, ref)
    got, pix = _launch(dev, c, ref["g"])
    _assert_bits(c, ref, got, ref["det"], name)
    for key in c["per_pixel"]:
        _assert_pixel_bits(c, ref, pix[key], key, name)
    # accumulation into a given gradient: base + v in fp32 (det_convert_kernel); the per-level gradient of the mip kernel
    # is overwritten, its fold (mip_adjoint, pinned bitwise by test_gpu_mip.py) is what accumulates
    shape = (c["T"], c["T"], 3) if c["kind"] == "mip" else c["out_shape"]
    base = np.random.default_rng(len(name)).standard_normal(shape).astype(F32)
    acc, pix = _launch(dev, c, ref["g"], base=base)
    if c["kind"] == "mip":
        _assert_bits(c, ref, acc, ref["det"], name + " (per-level, a gradient given)")
        fold = M.adjoint(M.unpack(ref["det"], c["T"], c["L"]))
        assert fold.dtype == F32
        assert np.array_equal(pix["gtex"].view(np.int32), (base + fold).view(np.int32)), name + ": folded grad_texture"
    else:
        _assert_bits(c, ref, acc, base.reshape(-1) + ref["det"], name + " (accumulated)")
    print(f"{name}: all {got.size} elements equal ({len(ref['where'])} fragments, {ref['attempt']} rescalings)")


# ------------------------------------------------------------------------------ (c) float atomics, summation-only bound
@pytest.mark.parametrize("name", ALL)
def test_float_atomics_within_the_summation_bound(dev, ops, monkeypatch, name):
    c, ref = _case(dev, ops, name), _reference(dev, ops, name)
    monkeypatch.setattr(ops, "_DETERMINISTIC", False)
    got, pix = _launch(dev, c, ref["g"])
    VP.assert_within_summation_bound(got, *TP.deposits(ref), name, lambda j: _where(c, ref, j))
    for key in c["per_pixel"]:                                          # the per-pixel outputs do not depend on the scatter
        _assert_pixel_bits(c, ref, pix[key], key, name + " (float atomics)")


# --------------------------------------------------------------------------------------------------------------- (d) k
# every fragment set of the cases above and the two-triangle quad that fills a 16-pixel view: on the cow (faces smaller than
# a pixel) and on the scatter scene dist / sigma stays in [-5, 0], so none of their pixels is in the class whose k must be
# exactly 1; most of the quad's are.  On all of these dist <= 0, prob >= 1/2 and k = prob / (prob + 1e-10) rounds to 1.0f
# whatever expf returns (0.0017 ulp = 2e-10 / 2^-23 from the fp64 value); only on ("edge",), where dist > 0, is k below 1.
FRAG_SETS = [("cow", 16), ("cow", 17), ("cow", 24), ("cow", 32), ("cow", 36), ("scatter",), ("own",), ("edge",), ("quad", 16)]


def test_the_probed_k(dev, ops):
    """every fragment set of the cases above and the quad: the vertex-colour probe equals the plain probe bit for bit; k == 1.0f exactly
    where dist / sigma <= -18 and z_inv >= 0.5 (1 + e rounds to 1 for e <= exp(-18) < 2^-25, expf(0) = 1, and delta = 1e-10
    vanishes in 1 + delta); elsewhere within K_BAR_ULP ulps (K_EDGE_BAR_ULP on the edge set) of k evaluated in fp64
    (_mipref._blend) from the same fp32 dists / zbuf, and everywhere within K_EXPF_BAR_ULP of its correctly rounded fp32
    evaluation"""
    assert {_case(dev, ops, n)["fr"]["name"] for n in ALL} | {("quad", 16)} == set(FRAG_SETS)
    worst, exact = 0.0, 0
    for name in FRAG_SETS:
        d = _frags(dev, ops, name)
        k = probe_k(dev, ops, d)
        p2f, zbuf, _, dists = d["frag_np"]
        cov = p2f >= 0
        B, S, _ = p2f.shape
        # the vertex-colour kernel's k
        faces = torch.zeros((d["n_faces"], 3), dtype=torch.int32, device=dev)
        col = torch.tensor([[1.0, 0.0, 0.0]], device=dev)
        g = torch.zeros((B, 3, S, S), device=dev)
        g[:, 0] = 1.0
        gb = ops.shade_vc_bwd(g, d["frag"], faces, col, want_colours=False, want_bary=True).cpu().numpy()
        for j in range(3):
            assert np.array_equal(gb[..., j].view(np.int32), k.view(np.int32)), (name, j)
        assert not k[~cov].any() and np.isfinite(k).all() and (k[cov] > 0).all() and (k <= 1).all()
        with np.errstate(all="ignore"):
            _, wnum, _, denom = M._blend(dists[cov], zbuf[cov], F64)
            x = (dists[cov] / F32(M.SIGMA)).astype(F32)
            z_inv = ((F32(M.ZFAR) - zbuf[cov]).astype(F32) / (F32(M.ZFAR) - F32(M.ZNEAR))).astype(F32)
        k64 = wnum / denom
        one = (x <= F32(-18.0)) & (z_inv >= F32(0.5))
        assert (k[cov][one] == F32(1.0)).all(), name
        exact += int(one.sum())
        rest = ~one
        ulp = np.spacing(k64.astype(F32)).astype(F64)
        ulps = np.abs(k[cov].astype(F64) - k64) / ulp
        w = float(ulps[rest].max()) if rest.any() else 0.0
        k32 = TP.blend_k(d["frag_np"], F32)[cov]                        # the correctly rounded fp32 evaluation
        e = float((np.abs(k[cov].astype(F64) - k32.astype(F64)) / ulp).max())
        print(f"{name}: {int(cov.sum())} fragments, {int((k[cov] != 1).sum())} with k != 1, in the class that must be 1: "
              f"{int(one.sum())}, elsewhere ({int(rest.sum())}) largest |k - k_fp64| = {w:.6f} ulp; from numpy's fp32 k {e:.3f} ulp")
        assert e <= K_EXPF_BAR_ULP, name
        if name == ("edge",):
            assert int((k[cov] != 1).sum()) > 1000
            worst_edge = w
        else:
            # dist <= 0: expf <= 1 (give or take its ulps), prob >= 1/2 less those, and 1e-10 is below half an ulp of it:
            # denom == wnum and k = wnum / wnum
            assert (dists[cov] <= 0).all() and (k[cov] == 1).all(), name
            worst = max(worst, w)
    print(f"k: largest error {worst:.6f} ulp (measured {K_MEASURED_ULP}, bar {K_BAR_ULP}); k == 1 exactly in its class on {exact} "
          f"fragments; on the edge set {worst_edge:.3f} ulp (measured {K_EDGE_MEASURED_ULP}, bar {K_EDGE_BAR_ULP})")
    assert exact >= 100
    assert K_BAR_ULP <= 2 * K_MEASURED_ULP * (1 + 1e-9) and K_EDGE_BAR_ULP <= 2 * K_EDGE_MEASURED_ULP * (1 + 1e-9)
    assert worst <= K_BAR_ULP and worst_edge <= K_EDGE_BAR_ULP
