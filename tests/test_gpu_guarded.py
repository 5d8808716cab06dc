"""Every device-launching wrapper of st3d.ops between guard zones (tests/_guarded.py): no write outside an output or a
workspace, no output element left unwritten, no scratch read before it is written.

Each case is a function run(ops, sc) -> dict of named output tensors.  It takes its inputs from the scene `sc` (seeded,
built with this module's own torch: outside the shim) and calls one wrapper, or a short chain where an op needs the
previous op's output.  Buffers the caller must provide (out=, grad_texture=, y=) are made by the case with defined
contents and named under "_own".  Every case runs three times -- plain, under Guarded(0xFF), under Guarded(0x01) -- and
  1. no guard byte changed;  2. every output is the shim's or the case's own;  3. A == B bit for bit;  4. plain == A.
Cases with atomics=True run once more with the float-atomic scatters (ops.set_deterministic(False)) and assertion 1 only.

Shapes: the smallest an entry point's own checks accept plus one that is no multiple of the kernel's tile (16 x 16 render
tiles, 4 x 16 strips, 8 x 32 tiles, 64 lanes, 256-thread blocks), from the tables the suite already has.

NOT_COVERED may hold only wrappers that launch nothing on the device, or that cannot run in one process on one GPU
(tests/test_guarded_host.py asserts the tables against st3d.ops).  UNSPECIFIED lists the regions the contract leaves open:
(wrapper, output name, function giving the specified part, the sentence that says so); assertions 3 and 4 compare that part."""
import numpy as np
import pytest
import torch

import _guarded as G

pytestmark = pytest.mark.gpu

RENDER = ("st3d.ops", "st3d.render")


class Case:
    def __init__(self, run, covers, atomics, modules):
        self.run, self.covers, self.atomics, self.modules = run, covers, atomics, modules


CASES = {}

NOT_COVERED = {
    "knn1_geometry": "a host-side query of the launch geometry: no kernel, no device memory",
    "nnfm_geometry": "a host-side query of the launch geometry: no kernel, no device memory",
    "swd_geometry": "a host-side query of the launch geometry: no kernel, no device memory",
    "device_info": "reads the device properties on the host: no kernel, no device memory",
}


def _upto(count_name):
    return lambda t, outs: t[:int(outs[count_name])]


UNSPECIFIED = [
    ("need_build", "lists[0]", _upto("counts[0]"),
     "ops.need_build: only the first `count` entries (a device int32 scalar) are meaningful."),
    ("need_build", "lists[1]", _upto("counts[1]"),
     "ops.need_build: only the first `count` entries (a device int32 scalar) are meaningful."),
] + [("flat_build", f"lists[{k}]", _upto(f"counts[{k}]"),
      "ops.flat_build: only the first `count` (device int32 scalar) list entries are meaningful.") for k in range(3)]


def _covered(t, outs):
    return t[outs["p2f"] >= 0]


def _ceil(v, m):
    return (v + m - 1) // m * m


GRAD_NP = ("include/st3d.h, st3d_shade_lit_bwd: grad_np is written at covered pixels only (pix_to_face >= 0): elsewhere it keeps "
           "what the buffer held.")
PACKS = ("include/st3d.h, st3d_conv3x3_pack: the floats behind a pack's own layout are neither written here nor read by any "
         "kernel.")
UNSPECIFIED += [(w, out, _covered, GRAD_NP) for w in ("shade_lit_bwd", "shade_ss_lit_bwd", "shade_soft_lit_bwd")
                for out in ("grad_np", "grad_np_alone")]
UNSPECIFIED += [("conv3x3_pack", "wf", lambda t, outs: t[:9 * _ceil(outs["w"].shape[1], 4) * _ceil(outs["w"].shape[0], 128)], PACKS),
                ("conv3x3_pack", "wd", lambda t, outs: t[:9 * _ceil(outs["w"].shape[0], 4) * _ceil(outs["w"].shape[1], 128)], PACKS)]


def case(name, covers, atomics=False, modules=G.DEFAULT_MODULES):
    covers = (covers,) if isinstance(covers, str) else tuple(covers)

    def deco(fn):
        assert name not in CASES, name
        CASES[name] = Case(fn, covers, atomics, modules)
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------------- the scene
class Scene:
    """Seeded inputs on the device, made once and read-only afterwards"""

    def __init__(self, dev, cow):
        self.dev, self.cow, self._memo = dev, cow, {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def t(self, a):
        a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return a.contiguous().to(self.dev)

    def randn(self, shape, seed, scale=1.0):
        return self.memo(("randn", tuple(shape), seed, scale),
                         lambda: self.t(torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale))

    def rand(self, shape, seed):
        return self.memo(("rand", tuple(shape), seed),
                         lambda: self.t(torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed))))

    def randint(self, hi, shape, seed, dtype=torch.uint8):
        return self.memo(("randint", hi, tuple(shape), seed, dtype),
                         lambda: self.t(torch.randint(0, hi, tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=dtype)))

    def fresh(self, shape, seed, scale=1.0):
        """a buffer of the case's own: new on every call, same contents"""
        return self.randn(shape, seed, scale).clone()

    # ---- meshes
    def mesh(self, name):
        def make():
            import _scatter_scene as SC
            import _vertexpath_ref as VP
            verts, faces, R, T, ndc = VP.scene(name)
            V = verts.shape[0] if verts is not None else ndc.shape[1]
            if name == "cow":
                uvs, fuv = self.cow["verts_uvs"], self.cow["faces_uvs"].astype(np.int32)
            else:
                uvs, fuv = 0.02 + 0.96 * SC.hash01(2 * V, 31).reshape(V, 2), np.asarray(faces, np.int32)
            m = dict(faces=self.t(np.asarray(faces, np.int32)), uvs=self.t(np.asarray(uvs, np.float32)), fuv=self.t(fuv), V=V,
                     F=int(faces.shape[0]))
            if verts is not None:
                m.update(verts=self.t(verts), R=self.t(np.asarray(R, np.float32)), T=self.t(np.asarray(T, np.float32)))
            else:
                m.update(verts=None, ndc=self.t(np.asarray(ndc, np.float32)))
            return m
        return self.memo(("mesh", name), make)

    def ndc(self, name):
        from st3d import ops
        m = self.mesh(name)
        return m["ndc"] if m["verts"] is None else self.memo(("ndc", name), lambda: ops.project_verts(m["verts"], m["R"], m["T"]))

    def hard(self, name, S=None):
        """-> dict(frag, uvs, fuv, faces, B, S, V, F[, ndc]) of a K = 1 scene"""
        def make():
            from st3d import ops
            if name == "scatter":
                import _scatter_scene as SC
                frag = tuple(self.t(a) for a in SC.fragments())
                return dict(frag=frag, uvs=self.t(SC.VERTS_UVS), fuv=self.t(SC.FACES_UVS), faces=self.t(SC.FACES_UVS), B=SC.B, S=SC.S,
                            V=4, F=2, ndc=None)
            m, ndc = self.mesh(name), self.ndc(name)
            frag = ops.raster_fwd(ndc, m["faces"], S)
            assert int((frag[0] >= 0).sum()) > 0
            return dict(frag=frag, uvs=m["uvs"], fuv=m["fuv"], faces=m["faces"], B=ndc.shape[0], S=S, V=m["V"], F=m["F"], ndc=ndc)
        return self.memo(("hard", name, S), make)

    def soft(self, key):
        """-> dict(frag (p2f, zbuf, bary, dists), slots | None, ...) of SOFT[key]"""
        def make():
            from st3d import ops
            name, S, K, blur, clip, persp, z_clip = SOFT[key]
            m, ndc = self.mesh(name), self.ndc(name)
            out = ops.raster_soft_fwd(ndc, m["faces"], S, K, blur, clip, False, persp, z_clip)
            assert int((out[0] >= 0).sum()) > 0
            return dict(frag=tuple(out[:4]), slots=out[4] if len(out) > 4 else None, uvs=m["uvs"], fuv=m["fuv"], faces=m["faces"],
                        B=ndc.shape[0], S=S, K=K, V=m["V"], F=m["F"], ndc=ndc, blur=blur, clip=clip, persp=persp, z_clip=z_clip)
        return self.memo(("soft", key), make)

    def tex(self, T):
        import _scatter_scene as SC
        return self.memo(("tex", T), lambda: self.t(SC.hash01(T * T * 3, 4 + T).reshape(T, T, 3)))

    def lit(self, name):
        """point lights on the cow (normals, incidence) / ambient light on the scatter scene"""
        def make():
            from st3d import render as R_
            if name == "scatter":
                import _scatter_scene as SC
                return SC._Lit(torch, self.dev)
            m = self.mesh(name)
            lights = R_.PointLights(location=((0.5, 1.0, 2.0),), device=self.dev)
            lighting = R_.lighting_of(lights, None, self.dev)
            lit = R_._lit_setup(lighting, m["verts"], m["verts"], m["faces"], m["R"], m["T"])
            lit._keep = lights
            return lit
        return self.memo(("lit", name), make)

    def topo(self, name):
        from st3d import mesh_losses as ML
        m = self.mesh(name)
        return self.memo(("topo", name), lambda: (ML.build_topology(m["faces"].long(), m["V"]),
                                                  ML.build_cot_topology(m["faces"].long(), m["V"])))

    def conv_w(self, Cout, Cin):
        return self.randn((Cout, Cin, 3, 3), 7 * Cout + Cin, (2.0 / (Cin * 9)) ** 0.5)

    def blobs(self, N, S, seed):
        """(N,S,S) uint8: a rectangle per image that ends off the tile grid, the second image empty"""
        def make():
            m = np.zeros((N, S, S), np.uint8)
            rng = np.random.default_rng(seed)
            for n in range(N):
                if n == 1:
                    continue
                y0, x0 = rng.integers(0, S // 2, 2)
                m[n, y0:y0 + S // 3 + 1, x0:x0 + S // 2 - 3] = 1
            return self.t(m)
        return self.memo(("blobs", N, S, seed), make)


# name -> (scene, S, K, blur, clip, persp, z_clip): cow at a ragged side, the overflow case of _vertexpath_ref.SOFT_CASES (more
# candidate faces than the per-tile list holds), a face through the near plane with clipping on
SOFT = {"cow17k4": ("cow", 17, 4, 3e-4, True, True, None),
        "cow17k1": ("cow", 17, 1, 0.0, False, True, None),
        "cow17k2n": ("cow", 17, 2, 0.0, False, False, None),
        "overflow": ("sub1", 16, 8, 1e-3, True, True, None),
        "near": ("one behind", 40, 2, 3e-3, True, True, 0.5)}
HARD = (("scatter", None), ("cow", 17), ("quad", 16))
BG = (0.2, 0.5, 0.9)


def _each(pairs):
    return [(f"{a}{'' if b is None else b}", a, b) for a, b in pairs]


# ================================================================================================== render: K = 1
@case("project_verts[cow]", "project_verts")
def _(ops, sc):
    m = sc.mesh("cow")
    return {"ndc": ops.project_verts(m["verts"], m["R"], m["T"])}


for _tag, _name, _S in _each(HARD[1:] + (("cow", 40), ("cow", 72), ("sub1", 16), ("sub", 24))):
    for _z in (None, 0.5):
        @case(f"raster_fwd[{_tag}{'' if _z is None else ',watch'}]", "raster_fwd")
        def _(ops, sc, name=_name, S=_S, z=_z):
            p2f, zbuf, bary, dists = ops.raster_fwd(sc.ndc(name), sc.mesh(name)["faces"], S, z_clip=z)
            ops.check_near_plane(block=True)
            return {"p2f": p2f, "zbuf": zbuf, "bary": bary, "dists": dists}

for _tag, _name, _S in _each(HARD):
    for _T in ((4, 64, 1024) if _name == "scatter" else (32,)):
        @case(f"shade_fwd[{_tag},T{_T}]", "shade_fwd")
        def _(ops, sc, name=_name, S=_S, T=_T):
            h = sc.hard(name, S)
            rgb, mask = ops.shade_fwd(h["frag"], h["uvs"], h["fuv"], sc.tex(T))
            return {"rgb": rgb, "mask": mask}

        @case(f"shade_bwd[{_tag},T{_T}]", "shade_bwd", atomics=True)
        def _(ops, sc, name=_name, S=_S, T=_T):
            h = sc.hard(name, S)
            gt, guv, gb = ops.shade_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 3), h["frag"], h["uvs"], h["fuv"], sc.tex(T),
                                        want_uv=True, want_bary=True)
            return {"grad_texture": gt, "grad_uv": guv, "grad_bary": gb}

    @case(f"shade_bwd[{_tag},own texture gradient]", "shade_bwd", atomics=True)
    def _(ops, sc, name=_name, S=_S):
        h = sc.hard(name, S)
        own = sc.fresh((32, 32, 3), 5)
        gt = ops.shade_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 3), h["frag"], h["uvs"], h["fuv"], sc.tex(32), grad_texture=own)
        return {"grad_texture": gt, "_own": [own]}

    @case(f"shade_bwd[{_tag},geometry only]", "shade_bwd")
    def _(ops, sc, name=_name, S=_S):
        h = sc.hard(name, S)
        none, gb = ops.shade_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 3), h["frag"], h["uvs"], h["fuv"], sc.tex(32),
                                 want_bary=True, want_texture=False)
        assert none is None
        return {"grad_bary": gb}

    @case(f"shade_vc[{_tag}]", ("shade_vc_fwd", "shade_vc_bwd"), atomics=True)
    def _(ops, sc, name=_name, S=_S):
        h = sc.hard(name, S)
        col = sc.rand((h["V"], 3), 7)
        rgb, mask = ops.shade_vc_fwd(h["frag"], h["faces"], col)
        gc, gb = ops.shade_vc_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 3), h["frag"], h["faces"], col, want_bary=True)
        own = sc.fresh((h["V"], 3), 8)
        gc2 = ops.shade_vc_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 3), h["frag"], h["faces"], col, grad_colours=own)
        gb2 = ops.shade_vc_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 3), h["frag"], h["faces"], col, want_colours=False, want_bary=True)
        return {"rgb": rgb, "mask": mask, "grad_colours": gc, "grad_bary": gb, "grad_colours_own": gc2, "grad_bary_alone": gb2,
                "_own": [own]}

    for _R in (1, 3):
        @case(f"shade_atlas[{_tag},R{_R}]", ("shade_atlas_fwd", "shade_atlas_bwd"), atomics=True)
        def _(ops, sc, name=_name, S=_S, R=_R):
            h = sc.hard(name, S)
            atlas = sc.rand((h["F"], R, R, 3), 9)
            rgb, mask = ops.shade_atlas_fwd(h["frag"], atlas)
            g = sc.randn((h["B"], 3, h["S"], h["S"]), 3)
            ga = ops.shade_atlas_bwd(g, h["frag"], R, h["F"])
            own = sc.fresh((h["F"], R, R, 3), 10)
            ga2 = ops.shade_atlas_bwd(g, h["frag"], R, h["F"], grad_atlas=own)
            return {"rgb": rgb, "mask": mask, "grad_atlas": ga, "grad_atlas_own": ga2, "_own": [own]}

for _tag, _name, _S in _each(HARD[1:]):
    @case(f"raster_bwd[{_tag}]", "raster_bwd", atomics=True)
    def _(ops, sc, name=_name, S=_S):
        h = sc.hard(name, S)
        return {"grad_ndc": ops.raster_bwd(sc.randn((h["B"], S, S, 3), 11), h["frag"][0], h["ndc"], h["faces"])}


@case("project_verts_bwd[cow]", "project_verts_bwd")
def _(ops, sc):
    m = sc.mesh("cow")
    g = sc.randn((2, m["V"], 3), 12)
    own = sc.fresh((m["V"], 3), 13)
    return {"grad_verts": ops.project_verts_bwd(m["verts"], m["R"], m["T"], g),
            "grad_verts_own": ops.project_verts_bwd(m["verts"], m["R"], m["T"], g, out=own), "_own": [own]}


# ---- supersampling: n = B C S^2 of 1, the vector path (S = 16, a = 2) and the scalar path (S = 17, a = 3)
for _B, _C, _S, _a in ((1, 1, 1, 1), (1, 1, 1, 2), (2, 3, 16, 2), (2, 3, 17, 3), (1, 1, 5, 4)):
    @case(f"box_down[B{_B},C{_C},S{_S},a{_a}]", ("box_down_fwd", "box_down_bwd"))
    def _(ops, sc, B=_B, C=_C, S=_S, a=_a):
        return {"down": ops.box_down_fwd(sc.randn((B, C, a * S, a * S), 14), a), "up": ops.box_down_bwd(sc.randn((B, C, S, S), 15), a)}

SS = (("scatter", None, 2), ("cow", 51, 3), ("quad", 32, 2), ("quad", 16, 4))
for _name, _SS, _a in SS:
    @case(f"shade_ss[{_name},a{_a}]", ("shade_ss_fwd", "shade_ss_bwd"), atomics=True)
    def _(ops, sc, name=_name, SS_=_SS, a=_a):
        h = sc.hard(name, SS_)
        S = h["S"] // a
        out = {}
        for T in ((4, 64) if name == "scatter" else (32,)):
            rgb, cov = ops.shade_ss_fwd(h["frag"], h["uvs"], h["fuv"], sc.tex(T), a)
            gt, guv, gb = ops.shade_ss_bwd(sc.randn((h["B"], 3, S, S), 16), h["frag"], h["uvs"], h["fuv"], sc.tex(T), a, want_uv=True,
                                           want_bary=True)
            out.update({f"rgb{T}": rgb, f"cov{T}": cov, f"grad_texture{T}": gt, f"grad_uv{T}": guv, f"grad_bary{T}": gb})
        return out


# ---- mip-mapped sampling: the (T, L) of tests/_mipref.CASES and the two smallest chains
for _T, _L in ((2, 1), (4, 2), (32, 3), (48, 3), (40, 4), (64, 2), (64, 6)):
    @case(f"mip_build_adjoint[T{_T},L{_L}]", ("mip_build", "mip_adjoint"))
    def _(ops, sc, T=_T, L=_L):
        P = ops.mip_numel(T, L)
        own_p, own_t = sc.fresh((P,), 17), sc.fresh((T, T, 3), 18)
        gp = sc.randn((P,), 19)
        return {"pyramid": ops.mip_build(sc.tex(T), L), "pyramid_own": ops.mip_build(sc.tex(T), L, out=own_p),
                "grad": ops.mip_adjoint(gp, T, L), "grad_own": ops.mip_adjoint(gp, T, L, out=own_t), "_own": [own_p, own_t]}

for _S, _T, _L in ((16, 32, 3), (17, 48, 3), (24, 64, 6)):
    @case(f"shade_mip[cow{_S},T{_T},L{_L}]", ("mip_lod", "shade_mip_fwd", "shade_mip_bwd", "mip_build"), atomics=True)
    def _(ops, sc, S=_S, T=_T, L=_L):
        h, m = sc.hard("cow", S), sc.mesh("cow")
        pyr = ops.mip_build(sc.tex(T), L)
        lod = ops.mip_lod(h["frag"], h["ndc"], m["faces"], h["uvs"], h["fuv"], T, L, 0.25)
        rgb, mask = ops.shade_mip_fwd(h["frag"], h["uvs"], h["fuv"], pyr, lod, T, L)
        gt, guv, gb, gl = ops.shade_mip_bwd(sc.randn((h["B"], 3, S, S), 20), h["frag"], h["uvs"], h["fuv"], pyr, lod, T, L, want_uv=True,
                                            want_bary=True, want_levels=True)
        return {"lod": lod, "rgb": rgb, "mask": mask, "grad_texture": gt, "grad_uv": guv, "grad_bary": gb, "grad_levels": gl}


@case("shade_mip[scatter,T4,L2,own texture gradient]", ("shade_mip_fwd", "shade_mip_bwd", "mip_build"), atomics=True)
def _(ops, sc):
    import _scatter_scene as SC
    h = sc.hard("scatter")
    T, L = 4, 2
    pyr, lod = ops.mip_build(sc.tex(T), L), sc.memo("lod42", lambda: sc.t(SC.lod_plane(L)))
    own = sc.fresh((T, T, 3), 21)
    rgb, mask = ops.shade_mip_fwd(h["frag"], h["uvs"], h["fuv"], pyr, lod, T, L)
    gt = ops.shade_mip_bwd(sc.randn((h["B"], 3, h["S"], h["S"]), 20), h["frag"], h["uvs"], h["fuv"], pyr, lod, T, L, grad_texture=own)
    return {"rgb": rgb, "mask": mask, "grad_texture": gt, "_own": [own]}


# ---- Phong lighting
@case("vertex_normals[cow]", ("vertex_normals", "vertex_normals_bwd"))
def _(ops, sc):
    from st3d import render as R_
    m = sc.mesh("cow")
    inc = R_.vertex_incidence(m["faces"], m["V"])
    n, u = ops.vertex_normals(m["verts"], m["faces"], inc)
    own, own2 = sc.fresh((m["V"], 3), 22), sc.fresh((m["V"], 3), 22)
    g = ops.vertex_normals_bwd(m["verts"], m["faces"], inc, u, sc.randn((m["V"], 3), 23), sc.randn((m["V"], 3), 24), own)
    g2 = ops.vertex_normals_bwd(m["verts"], m["faces"], inc, u, sc.randn((m["V"], 3), 23), None, own2)
    return {"normals": n, "unnormalised": u, "grad": g, "grad_without_positions": g2, "_own": [own, own2]}


for _name, _S in (("scatter", None), ("cow", 17)):
    @case(f"shade_lit[{_name}]", ("shade_lit_fwd", "shade_lit_bwd"), atomics=True)
    def _(ops, sc, name=_name, S=_S):
        h, lit = sc.hard(name, S), sc.lit(name)
        rgb, mask = ops.shade_lit_fwd(h["frag"], h["uvs"], h["fuv"], sc.tex(32), lit)
        g = sc.randn((h["B"], 3, h["S"], h["S"]), 25)
        gt, gb, gnp = ops.shade_lit_bwd(g, h["frag"], h["uvs"], h["fuv"], sc.tex(32), lit, want_texture=True, want_geometry=True)
        none, gb2, gnp2 = ops.shade_lit_bwd(g, h["frag"], h["uvs"], h["fuv"], sc.tex(32), lit, want_texture=False, want_geometry=True)
        return {"rgb": rgb, "mask": mask, "grad_texture": gt, "grad_bary": gb, "grad_np": gnp, "grad_bary_alone": gb2, "grad_np_alone": gnp2,
                "p2f": h["frag"][0], "_own": [h["frag"][0]]}

for _name, _SS, _a in (("scatter", None, 2), ("cow", 51, 3)):
    @case(f"shade_ss_lit[{_name},a{_a}]", ("shade_ss_lit_fwd", "shade_ss_lit_bwd"), atomics=True)
    def _(ops, sc, name=_name, SS_=_SS, a=_a):
        h, lit = sc.hard(name, SS_), sc.lit(name)
        S = h["S"] // a
        rgb, cov = ops.shade_ss_lit_fwd(h["frag"], h["uvs"], h["fuv"], sc.tex(32), lit, a)
        gt, gb, gnp = ops.shade_ss_lit_bwd(sc.randn((h["B"], 3, S, S), 26), h["frag"], h["uvs"], h["fuv"], sc.tex(32), lit, a,
                                           want_texture=True, want_geometry=True)
        return {"rgb": rgb, "cov": cov, "grad_texture": gt, "grad_bary": gb, "grad_np": gnp, "p2f": h["frag"][0], "_own": [h["frag"][0]]}


@case("shade_soft_lit[cow17k4]", ("shade_soft_lit_fwd", "shade_soft_lit_bwd"), atomics=True)
def _(ops, sc):
    s, lit = sc.soft("cow17k4"), sc.lit("cow")
    rgb, alpha = ops.shade_soft_lit_fwd(s["frag"], s["uvs"], s["fuv"], sc.tex(32), lit, 1e-4, 1e-4, BG)
    gt, geo, gnp = ops.shade_soft_lit_bwd(sc.randn((s["B"], 3, s["S"], s["S"]), 27), s["frag"], s["uvs"], s["fuv"], sc.tex(32), lit, 1e-4,
                                          1e-4, BG)
    return {"rgb": rgb, "alpha": alpha, "grad_texture": gt, "grad_geometry": geo, "grad_np": gnp, "p2f": s["frag"][0], "_own": [s["frag"][0]]}


@case("phong_scatter[cow17]", "phong_scatter", atomics=True)
def _(ops, sc):
    h, s = sc.hard("cow", 17), sc.soft("cow17k4")
    return {"k1": ops.phong_scatter(sc.randn((h["B"], 17, 17, 6), 28), h["frag"][0], h["frag"][2], h["faces"], h["V"]),
            "k4": ops.phong_scatter(sc.randn((s["B"], 17, 17, 4, 6), 29), s["frag"][0], s["frag"][2], s["faces"], s["V"])}


# ================================================================================================== render: K faces per pixel
for _key in SOFT:
    @case(f"raster_soft_fwd[{_key}]", "raster_soft_fwd")
    def _(ops, sc, key=_key):
        name, S, K, blur, clip, persp, z_clip = SOFT[key]
        out = ops.raster_soft_fwd(sc.ndc(name), sc.mesh(name)["faces"], S, K, blur, clip, False, persp, z_clip)
        return dict(zip(("p2f", "zbuf", "bary", "dists", "slots"), out))

    @case(f"shade_soft[{_key}]", ("shade_soft_fwd", "shade_soft_bwd"), atomics=True)
    def _(ops, sc, key=_key):
        s = sc.soft(key)
        g = sc.randn((s["B"], 3, s["S"], s["S"]), 30)
        rgb, alpha = ops.shade_soft_fwd(s["frag"], s["uvs"], s["fuv"], sc.tex(32), 1e-4, 1e-4, BG)
        gt, geo = ops.shade_soft_bwd(g, s["frag"], s["uvs"], s["fuv"], sc.tex(32), 1e-4, 1e-4, BG)
        gt2, none = ops.shade_soft_bwd(g, s["frag"], s["uvs"], s["fuv"], sc.tex(32), 1e-4, 1e-4, BG, want_geometry=False)
        none2, geo2 = ops.shade_soft_bwd(g, s["frag"], s["uvs"], s["fuv"], sc.tex(32), 1e-4, 1e-4, BG, want_texture=False)
        assert none is None and none2 is None
        return {"rgb": rgb, "alpha": alpha, "grad_texture": gt, "grad_geometry": geo, "grad_texture_alone": gt2, "grad_geometry_alone": geo2}

    @case(f"raster_soft_bwd[{_key}]", "raster_soft_bwd", atomics=True)
    def _(ops, sc, key=_key):
        s = sc.soft(key)
        B, S, K = s["B"], s["S"], s["K"]
        grads = (sc.randn((B, S, S, K, 3), 31), sc.randn((B, S, S, K), 32), sc.randn((B, S, S, K), 33))
        return {"grad_ndc": ops.raster_soft_bwd(grads, s["frag"][0], s["ndc"], s["faces"], s["clip"], s["persp"], s["slots"], s["z_clip"])}

    @case(f"silhouette[{_key}]", ("silhouette_fwd", "silhouette_bwd", "silhouette_loss"))
    def _(ops, sc, key=_key):
        s = sc.soft(key)
        B, S, K = s["B"], s["S"], s["K"]
        p2f, dists = s["frag"][0], s["frag"][3]
        ga, target = sc.randn((B, 1, S, S), 34), sc.rand((B, 1, S, S), 35)
        own = sc.fresh((B, S, S, K), 36)
        loss, gd = ops.silhouette_loss(p2f, dists, target, 1e-4, 0.5)
        loss2, none = ops.silhouette_loss(p2f, dists, target, 1e-4, 0.5, want_grad=False)
        return {"alpha": ops.silhouette_fwd(p2f, dists, 1e-4), "grad_dists": ops.silhouette_bwd(ga, p2f, dists, 1e-4),
                "grad_dists_own": ops.silhouette_bwd(ga, p2f, dists, 1e-4, out=own), "loss": loss, "loss_grad": gd, "loss_alone": loss2,
                "_own": [own]}

    for _K in (1, 64) if _key == "cow17k4" else (SOFT[_key][2],):
        @case(f"silraster[{_key},K{_K}]", ("silraster_fwd", "silraster_loss", "silraster_bwd"), atomics=True)
        def _(ops, sc, key=_key, K=_K):
            name, S, _k, blur, clip, persp, z_clip = SOFT[key]
            m, ndc = sc.mesh(name), sc.ndc(name)
            B = ndc.shape[0]
            kw = dict(clip_bary=clip, perspective_correct=persp, z_clip=0.5)
            alpha, state = ops.silraster_fwd(ndc, m["faces"], S, K, blur, 1e-4, **kw)
            loss, state4 = ops.silraster_loss(ndc, m["faces"], sc.rand((B, 1, S, S), 35), K, blur, 1e-4, 0.5, **kw)
            g = ops.silraster_bwd(state, ndc, m["faces"], blur, 1e-4, sc.randn((B, 1, S, S), 34), 1.0, **kw)
            g4 = ops.silraster_bwd(state4, ndc, m["faces"], blur, 1e-4, None, 1.0, **kw)
            return {"alpha": alpha, "state": state, "loss": loss, "state4": state4, "grad_ndc": g, "grad_ndc_of_loss": g4}


for _S in (1, 17, 33):          # 1, 289 and 1089 pixels per image: one thread, past one block, past four
    @case(f"apply_background[S{_S}]", "apply_background")
    def _(ops, sc, S=_S):
        img, mask = sc.rand((2, 3, S, S), 37), sc.memo(("bgmask", S), lambda: (sc.rand((2, 1, S, S), 38) > 0.5).float())
        return {"white": ops.apply_background(img, mask), "per_view": ops.apply_background(img, mask, sc.rand((2, 3, S, S), 39)),
                "shared": ops.apply_background(img, mask, sc.rand((1, 3, S, S), 40))}


# ================================================================================================== mesh losses
@case("mesh_reg[cow]", ("mesh_reg", "mesh_reg_ex"))
def _(ops, sc):
    m = sc.mesh("cow")
    topo, cot = sc.topo("cow")
    verts = sc.memo("cow moved", lambda: m["verts"] + 0.01 * sc.randn((m["V"], 3), 41))
    w = [0.7, 1.3, 0.9, 1.1]
    out = {}
    out["loss"], out["grad"] = ops.mesh_reg(verts, m["verts"], topo, w)
    out["loss_alone"], none = ops.mesh_reg(verts, m["verts"], topo, w, want_grad=False)
    out["uniform_loss"], out["uniform_grad"] = ops.mesh_reg_ex(verts, m["verts"], topo, None, w, "uniform", 0.0)
    out["cot_loss"], out["cot_grad"] = ops.mesh_reg_ex(verts, m["verts"], topo, cot, w, "cot", 0.0)
    out["cotcurv_loss"], out["cotcurv_grad"] = ops.mesh_reg_ex(verts, m["verts"], topo, cot, w, "cotcurv", 0.05)
    return out


def _clouds(sc, P1, P2):
    return sc.randn((P1, 3), 42 + P1), sc.randn((P2, 3), 43 + P2)


def _knn_sizes(ops):
    tile, _ = ops.knn1_geometry(257, 300)
    return ((1, 1), (257, tile + 1), (tile + 1, 1), (3, 40 * tile + 1))      # the last: several segments whatever the CU count


for _i in range(4):
    @case(f"chamfer[sizes {_i}]", ("knn1", "chamfer_sum", "chamfer_bwd"))
    def _(ops, sc, i=_i):
        P1, P2 = _knn_sizes(ops)[i]
        x, y = _clouds(sc, P1, P2)
        nn_x, d_x = ops.knn1(x, y)
        nn_y, d_y = ops.knn1(y, x)
        total = torch.full((1,), 0.25, device=sc.dev)
        ops.chamfer_sum(d_x, 1.0 / P1, total)
        ops.chamfer_sum(d_y, 1.0 / P2, total)
        s = torch.sort(nn_y, stable=True)
        own, own2, own3 = sc.fresh((P1, 3), 44), sc.fresh((P1, 3), 44), sc.fresh((P1, 3), 44)
        return {"nn_x": nn_x, "d_x": d_x, "nn_y": nn_y, "d_y": d_y, "sum": total,
                "grad": ops.chamfer_bwd(x, y, nn_x, s.indices.to(torch.int32), s.values, 0.5, 0.25, own),
                "grad_self": ops.chamfer_bwd(x, y, nn_x, None, None, 0.5, 0.0, own2),
                "grad_other": ops.chamfer_bwd(x, y, None, s.indices.to(torch.int32), s.values, 0.0, 0.25, own3),
                "_own": [total, own, own2, own3]}

for _n in (1, 257, 1025):
    @case(f"chamfer_sum[n{_n}]", "chamfer_sum")
    def _(ops, sc, n=_n):
        total = torch.full((1,), 0.25, device=sc.dev)
        return {"sum": ops.chamfer_sum(sc.rand((n,), 45), 0.5, total), "_own": [total]}

for _name, _N in (("cow", 1), ("cow", 257), ("quad", 1025)):
    @case(f"sample_points[{_name},N{_N}]", ("face_area_cdf", "sample_points_fwd", "sample_points_bwd"))
    def _(ops, sc, name=_name, N=_N):
        from st3d import render as R_
        m = sc.mesh(name)

        def uniforms():
            r = torch.rand((3, N), generator=torch.Generator().manual_seed(46))
            r[0] = torch.sort(r[0]).values
            return sc.t(r)
        r = sc.memo(("uniforms", N), uniforms)
        cdf = ops.face_area_cdf(m["verts"], m["faces"])
        points, face_idx = ops.sample_points_fwd(m["verts"], m["faces"], cdf, r)
        own = sc.fresh((m["V"], 3), 47)
        g = ops.sample_points_bwd(sc.randn((N, 3), 48), r, face_idx, m["F"], R_.vertex_incidence(m["faces"], m["V"]), own)
        return {"cdf": cdf, "points": points, "face_idx": face_idx, "grad": g, "_own": [own]}


# ================================================================================================== NNFM, sliced Wasserstein
def _nnfm_sizes(ops):
    tq, ts, _ = ops.nnfm_geometry(65, 65, 64)
    return ((1, 1, 1, 1, 1), (2, 2, 64, tq + 1, ts + 1), (2, 1, 64, 5, 2 * ts + 1), (1, 1, 512, tq + 1, 3),
            (1, 1, 64, 3, 40 * ts + 1))                                     # B, Bs, C, N, M; the last: several segments


for _i in range(5):
    @case(f"nnfm[sizes {_i}]", ("nnfm_normalise", "nnfm_search", "nnfm_sum", "nnfm_bwd"))
    def _(ops, sc, i=_i):
        B, Bs, C, N, M = _nnfm_sizes(ops)[i]
        feat, style = sc.randn((B, C, 1, N), 49), sc.randn((Bs, C, 1, M), 50)

        def weights():
            w = torch.rand((B, N), generator=torch.Generator().manual_seed(51))
            w[:, ::3] = 0.0
            if N > 1:
                w[B - 1, 1] = 1.0
            else:
                w[:] = 1.0
            return sc.t(w)
        w = sc.memo(("nnfm w", B, N), weights)
        fhat, fnorm = ops.nnfm_normalise(feat)
        none, snorm = ops.nnfm_normalise(style, want_hat=False)
        shat, _ = ops.nnfm_normalise(style)
        out = {"fhat": fhat, "fnorm": fnorm, "snorm": snorm, "shat": shat}
        for tag, ww in (("", None), ("_w", w)):
            idx, dist = ops.nnfm_search(feat, shat, ww)
            loss, wsum = ops.nnfm_sum(dist, ww)
            out.update({"idx" + tag: idx, "dist" + tag: dist, "loss" + tag: loss, "wsum" + tag: wsum,
                        "grad" + tag: ops.nnfm_bwd(feat, shat, idx, dist, wsum, ww, grad_out=sc.rand((1,), 52) if ww is not None else None)})
        return out


def _swd_sizes(ops):
    block, _ = ops.swd_geometry(1 << 16)
    return ((1, 1, 1, 1, 1, 1), (2, 2, 64, 33, 257, 300), (2, 1, 3, 2, block + 1, 2 * block + 1),
            (1, 1, 2, 3, 4 * block + 1, block - 1))                         # B, Bs, Q, R, N, M; the last: three strided passes


for _i in range(4):
    @case(f"swd[sizes {_i}]", ("swd_project", "swd_sort", "swd_loss", "swd_bwd"))
    def _(ops, sc, i=_i):
        B, Bs, Q, R, N, M = _swd_sizes(ops)[i]
        x, y, a = sc.randn((B, Q, N), 53), sc.randn((Bs, Q, M), 54), sc.randn((R, Q), 55)

        def weights():
            w = torch.rand((B, N), generator=torch.Generator().manual_seed(56))
            w[:, ::3] = 0.0
            w[:, 0] = 1.0
            return sc.t(w)
        w = sc.memo(("swd w", B, N), weights)
        proj, tproj = ops.swd_project(x, a), ops.swd_project(y, a)
        tsorted, none, tcount = ops.swd_sort(tproj, want_perm=False)
        out = {"proj": proj, "tproj": tproj, "tsorted": tsorted, "tcount": tcount}
        for tag, ww in (("", None), ("_w", w)):
            srt, perm, count = ops.swd_sort(proj, ww)
            out.update({"sorted" + tag: srt, "perm" + tag: perm, "count" + tag: count, "loss" + tag: ops.swd_loss(srt, count, tsorted),
                        "grad" + tag: ops.swd_bwd(srt, perm, count, tsorted, grad_out=sc.rand((1,), 57) if ww is not None else None)})
        return out


# ================================================================================================== conv / pool
CONV_SHAPES = [(2, 3, 64, 64, 64), (1, 64, 64, 48, 40), (2, 64, 128, 32, 32), (1, 128, 256, 24, 56), (1, 256, 256, 32, 32),
               (2, 512, 512, 16, 16), (1, 512, 512, 4, 4), (1, 3, 64, 33, 70)]        # test_gpu_kernels.CONV_CASES, H, W <= 70
WINO_SHAPES = [(2, 64, 64, 64, 64), (1, 64, 128, 32, 32), (1, 128, 256, 24, 56), (1, 256, 256, 32, 32), (2, 512, 512, 16, 16),
               (1, 512, 512, 4, 4), (1, 64, 64, 48, 40), (1, 128, 64, 10, 12)]        # test_gpu_kernels.WINO_CASES, H, W <= 70
WINO43_SHAPES = [(1, 64, 64, 4, 64), (2, 128, 64, 8, 64), (1, 64, 128, 8, 32), (2, 64, 64, 16, 32)]      # 4 x 64 and 8 x 32 tiles

for _N, _Cin, _Cout, _H, _W in CONV_SHAPES:
    @case(f"conv3x3[{_N},{_Cin},{_Cout},{_H},{_W}]", ("conv3x3_pack", "conv3x3_fwd", "conv3x3_dgrad", "maxpool2x2") +
          (("conv3x3_dgrad_unpool",) if _H % 2 == 0 and _W % 2 == 0 else ()))
    def _(ops, sc, N=_N, Cin=_Cin, Cout=_Cout, H=_H, W=_W):
        wf, wd = ops.conv3x3_pack(sc.conv_w(Cout, Cin))
        x, b, gy = sc.randn((N, Cin, H, W), 58), sc.randn((Cout,), 59, 0.1), sc.randn((N, Cout, H, W), 60)
        y = ops.conv3x3_fwd(x, wf, b, Cout, relu=True)
        out = {"w": sc.conv_w(Cout, Cin), "_own": [sc.conv_w(Cout, Cin)], "wf": wf, "wd": wd, "y": y, "y_linear": ops.conv3x3_fwd(x, wf, None, Cout, relu=False),
               "gx": ops.conv3x3_dgrad(gy, y, wd, Cin), "gx_ungated": ops.conv3x3_dgrad(gy, None, wd, Cin)}
        out["pooled"], out["pool_idx"] = ops.maxpool2x2(y)
        if H % 2 == 0 and W % 2 == 0:
            out["gx_unpool"] = ops.conv3x3_dgrad_unpool(sc.randn((N, Cout, H // 2, W // 2), 61), out["pool_idx"], out["pooled"], wd, Cin)
        return out

for _H, _W in ((7, 6), (2, 3), (12, 20)):
    @case(f"maxpool2x2[{_H},{_W}]", "maxpool2x2")
    def _(ops, sc, H=_H, W=_W):
        p, idx = ops.maxpool2x2(sc.randn((2, 5, H, W), 62))
        return {"pooled": p, "idx": idx, "pooled_alone": ops.maxpool2x2(sc.randn((2, 5, H, W), 62), want_idx=False)}

for _N, _H, _W in ((1, 1, 2), (2, 17, 22), (1, 3, 6), (1, 64, 64), (1, 33, 70)):
    @case(f"conv1_bwd[{_N},{_H},{_W}]", ("conv1_bwd", "conv1_bwd_weighted") + (("conv1_bwd_masked", "need_build") if _W % 64 == 0 else ()))
    def _(ops, sc, N=_N, H=_H, W=_W):
        _, wd = ops.conv3x3_pack(sc.conv_w(64, 3))
        act = sc.memo(("relu act", N, H, W), lambda: torch.relu(sc.randn((N, 64, H, W), 63)))
        gy, D, w0 = sc.randn((N, 64, H, W), 64), sc.randn((N, 64, 64), 65), sc.rand((N, H, W), 66)
        out = {"gx": ops.conv1_bwd(gy, act, D, 0.37, wd), "gx_gram_only": ops.conv1_bwd(None, act, D, 0.37, wd),
               "gx_gy_only": ops.conv1_bwd(gy, act, None, 0.37, wd), "gx_weighted": ops.conv1_bwd_weighted(gy, act, D, 0.37, wd, w0)}
        if W % 64 == 0:
            mask = sc.blobs(N, H, 67)
            seg, _lists = ops.need_build(mask, 1)
            out["gx_masked"] = ops.conv1_bwd_masked(gy, act, D, 0.37, wd, seg, mask)
            out["gx_weighted_masked"] = ops.conv1_bwd_weighted(gy, act, D, 0.37, wd, w0, seg, mask)
        return out

for _N, _Cin, _Cout, _H, _W in WINO_SHAPES:
    @case(f"wino[{_N},{_Cin},{_Cout},{_H},{_W}]", ("wino_pack", "wino_fwd", "wino_dgrad", "wino_dgrad_unpool", "wino_dgrad_chain"))
    def _(ops, sc, N=_N, Cin=_Cin, Cout=_Cout, H=_H, W=_W):
        uf, ud = ops.wino_pack(sc.conv_w(Cout, Cin))
        x, b, gy = sc.randn((N, Cin, H, W), 58), sc.randn((Cout,), 59, 0.1), sc.randn((N, Cout, H, W), 60)
        gp, og, tgt = sc.randn((N, Cout, H // 2, W // 2), 61), sc.randn((N, Cin, H, W), 68), sc.randn((N, Cin, H, W), 69)
        y, yp, idx = ops.wino_fwd(x, uf, b, Cout, relu=True, pool=True)
        none, yp2, idx2 = ops.wino_fwd(x, uf, b, Cout, relu=True, pool=True, keep_full=False)
        return {"uf": uf, "ud": ud, "y": y, "pooled": yp, "pool_idx": idx, "pooled_alone": yp2, "pool_idx_alone": idx2,
                "y_linear": ops.wino_fwd(x, uf, None, Cout, relu=False), "gx": ops.wino_dgrad(gy, y, ud, Cin),
                "gx_ungated": ops.wino_dgrad(gy, None, ud, Cin), "gx_unpool": ops.wino_dgrad_unpool(gp, idx, yp, ud, Cin),
                "chain": ops.wino_dgrad_chain(gy, ud, Cin, out_gate=og, add_target=tgt, add_coef=0.25),
                "chain_gated": ops.wino_dgrad_chain(gy, ud, Cin, act=y, out_gate=og),
                "chain_plain": ops.wino_dgrad_chain(gy, ud, Cin),
                "chain_unpool": ops.wino_dgrad_chain(gp, ud, Cin, pool_idx=idx, pooled=yp, out_gate=og)}

for _N, _Cin, _Cout, _H, _W in WINO43_SHAPES:
    @case(f"wino43[{_N},{_Cin},{_Cout},{_H},{_W}]", ("wino43_pack", "wino43_fwd", "wino43_dgrad_chain"))
    def _(ops, sc, N=_N, Cin=_Cin, Cout=_Cout, H=_H, W=_W):
        uf, ud = ops.wino43_pack(sc.conv_w(Cout, Cin))
        x, b, gy = sc.randn((N, Cin, H, W), 58), sc.randn((Cout,), 59, 0.1), sc.randn((N, Cout, H, W), 60)
        gp, og, tgt = sc.randn((N, Cout, H // 2, W // 2), 61), sc.randn((N, Cin, H, W), 68), sc.randn((N, Cin, H, W), 69)
        y, yp, idx = ops.wino43_fwd(x, uf, b, Cout, relu=True, pool=True)
        none, yp2, idx2 = ops.wino43_fwd(x, uf, b, Cout, relu=True, pool=True, keep_full=False)
        return {"uf": uf, "ud": ud, "y": y, "pooled": yp, "pool_idx": idx, "pooled_alone": yp2, "pool_idx_alone": idx2,
                "y_linear": ops.wino43_fwd(x, uf, None, Cout, relu=False), "chain_plain": ops.wino43_dgrad_chain(gy, ud, Cin),
                "chain": ops.wino43_dgrad_chain(gy, ud, Cin, out_gate=og, add_target=tgt, add_coef=0.25),
                "chain_unpool": ops.wino43_dgrad_chain(gp, ud, Cin, pool_idx=idx, out_gate=og)}


def _listed(sc, ids, total):
    lst = torch.full((total,), -1, dtype=torch.int32, device=sc.dev)
    lst[:len(ids)] = torch.tensor(ids, dtype=torch.int32, device=sc.dev)
    return lst, torch.tensor([len(ids)], dtype=torch.int32, device=sc.dev)


@case("wino43 listed tiles[2,64,64,8,64]", ("wino43_fwd_tiles", "wino43_dgrad_chain_tiles", "wino43_pack"))
def _(ops, sc):
    N, C, H, W = 2, 64, 8, 64
    uf, ud = ops.wino43_pack(sc.conv_w(C, C))
    x, b, gp = sc.randn((N, C, H, W), 58), sc.randn((C,), 59, 0.1), sc.randn((N, C, H // 2, W // 2), 61)
    pidx, og = sc.randint(4, (N, C, H // 2, W // 2), 70), sc.randn((N, C, H, W), 68)
    out, own = {}, []
    for tag, cols, total, ids in (("own", None, N * 2, [3, 0]), ("8x32", 32, N * 2, [1, 2, 3]), ("4x64", 64, N * 2, [2])):
        lst, cnt = _listed(sc, ids, total)
        y, yp, yi = sc.fresh((N, C, H, W), 71), sc.fresh((N, C, H // 2, W // 2), 72), sc.randint(256, (N, C, H // 2, W // 2), 73).clone()
        y2, g = sc.fresh((N, C, H, W), 71), sc.fresh((N, C, H, W), 74)
        ops.wino43_fwd_tiles(x, uf, b, C, lst, cnt[0], y=y, yp=yp, idx=yi, tile_cols=cols)
        ops.wino43_fwd_tiles(x, uf, b, C, lst, cnt[0], y=y2, relu=False, tile_cols=cols)
        ops.wino43_dgrad_chain_tiles(gp, ud, C, lst, cnt[0], g, pool_idx=pidx, out_gate=og, tile_cols=cols)
        out.update({f"y_{tag}": y, f"yp_{tag}": yp, f"idx_{tag}": yi, f"y_alone_{tag}": y2, f"gx_{tag}": g})
        own += [y, yp, yi, y2, g]
    out["_own"] = own
    return out


@case("wino43 listed strips[2,64,64,8,32]", ("wino43_fwd_strips", "wino43_dgrad_chain_tiles", "wino43_pack"))
def _(ops, sc):
    N, C, H, W = 2, 64, 8, 32
    uf, ud = ops.wino43_pack(sc.conv_w(C, C))
    x, b, gy, og = sc.randn((N, C, H, W), 58), sc.randn((C,), 59, 0.1), sc.randn((N, C, H, W), 60), sc.randn((N, C, H, W), 68)
    steps = [3, 0, -1, 1, 4, -1, -1, -1, -1, 6, 7, -1]            # strips (n * H/4 + sy) * W/16 + sx, four of one image per step
    lst = torch.full((16,), -1, dtype=torch.int32, device=sc.dev)
    lst[:len(steps)] = torch.tensor(steps, dtype=torch.int32, device=sc.dev)
    cnt = torch.tensor([3], dtype=torch.int32, device=sc.dev)
    y, g = sc.fresh((N, C, H, W), 71), sc.fresh((N, C, H, W), 74)
    ops.wino43_fwd_strips(x, uf, b, C, lst, cnt[0], y)
    ops.wino43_dgrad_chain_tiles(gy, ud, C, lst, cnt[0], g, out_gate=og, tile_cols=16)
    return {"y": y, "gx": g, "_own": [y, g]}


def _lists_out(seg, lists):
    return {"seg": seg, "lists": [l for l, _ in lists], "counts": [c for _, c in lists]}


for _N in (1, 3):
    @case(f"need_build[N{_N},S64]", "need_build")
    def _(ops, sc, N=_N):
        out = _lists_out(*ops.need_build(sc.blobs(N, 64, 75)))
        out["seg_alone"] = ops.need_build(sc.blobs(N, 64, 75), 1)[0]
        return out

    for _cols in (None, (16, 16, 16), (32, 0, 32)):
        @case(f"need_blocks_build[N{_N},S64,{_cols}]", "need_blocks_build")
        def _(ops, sc, N=_N, cols=_cols):
            return _lists_out(*ops.need_blocks_build(sc.blobs(N, 64, 75), tile_cols=list(cols) if cols else None))

        @case(f"kept_build[N{_N},S64,{_cols}]", "kept_build")
        def _(ops, sc, N=_N, cols=_cols):
            got = ops.kept_build(sc.blobs(N, 64, 76), first=0, tile_cols=list(cols) if cols else None)
            late = ops.kept_build(sc.blobs(N, 64, 76), first=2, tile_cols=list(cols) if cols else None)
            return {"lists": [got[k][0] for k in sorted(got)], "counts": [got[k][1] for k in sorted(got)],
                    "late_lists": [late[k][0] for k in sorted(late)], "late_counts": [late[k][1] for k in sorted(late)]}

    @case(f"flat_build[N{_N},S64]", "flat_build")
    def _(ops, sc, N=_N):
        def images():
            img = torch.ones((N, 3, 64, 64))
            on = sc.blobs(N, 64, 77).cpu().bool()[:, None].expand(-1, 3, -1, -1)
            return sc.t(torch.where(on, torch.rand((N, 3, 64, 64), generator=torch.Generator().manual_seed(78)), img))
        got = ops.flat_build(sc.memo(("flat images", N), images), torch.ones((3,), device=sc.dev))
        return {"lists": [g[0] for g in got], "counts": [g[1] for g in got], "maps": [g[2] for g in got]}


@case("need_blocks_build[N2,S128,gram runs]", ("need_blocks_build", "gram_bwd_gated_segs"))
def _(ops, sc):
    N, C, S = 2, 128, 128
    seg, lists, (glist, gcount) = ops.need_blocks_build(sc.blobs(N, S, 79), nlists=2, gram=True)
    feat = sc.memo("relu2_1 stand-in", lambda: torch.relu(sc.randn((N, C, S // 2, S // 2), 80)))
    D = sc.randn((N, C, C), 81)
    own, own2 = sc.fresh((N, C, S // 2, S // 2), 82), sc.fresh((N, C, S // 2, S // 2), 82)
    out = _lists_out(seg, lists)
    out.update({"gram_list": glist, "gram_count": gcount, "gfeat": ops.gram_bwd_gated_segs(D, feat, 0.37, glist, gcount, own),
                "gfeat_weighted": ops.gram_bwd_gated_segs(D, feat, 0.37, glist, gcount, own2, accumulate=True,
                                                          q=sc.rand((N, S // 2, S // 2), 83)), "_own": [own, own2]})
    return out


@case("flat_fill[3,16,8,64]", "flat_fill")
def _(ops, sc):
    N, C, H, W = 3, 16, 8, 64
    tile_map = torch.tensor([-1, 0, 0, -1, 3, 0], dtype=torch.int32, device=sc.dev)         # 4 x 64 tiles: two per image
    y, yp, yi = sc.fresh((N, C, H, W), 84), sc.fresh((N, C, H // 2, W // 2), 85), sc.randint(256, (N, C, H // 2, W // 2), 86).clone()
    y2, yp2 = sc.fresh((N, C, H, W), 84), sc.fresh((N, C, H // 2, W // 2), 85)
    ops.flat_fill(tile_map, y=y, yp=yp, idx=yi)
    ops.flat_fill(tile_map, y=y2)
    ops.flat_fill(tile_map, yp=yp2)
    return {"y": y, "yp": yp, "idx": yi, "y_alone": y2, "yp_alone": yp2, "_own": [y, yp, yi, y2, yp2]}


# ================================================================================================== Gram / losses / optimiser
for _B, _C, _H, _W in ((1, 64, 7, 9), (2, 512, 4, 4), (1, 32, 1, 1), (2, 128, 5, 13), (2, 64, 64, 64), (1, 128, 40, 40), (1, 64, 3, 3)):
    @case(f"gram[{_B},{_C},{_H},{_W}]", ("gram_fwd", "gram_bwd"))
    def _(ops, sc, B=_B, C=_C, H=_H, W=_W):
        feat = sc.memo(("gram feat", B, C, H, W), lambda: torch.relu(sc.randn((B, C, H, W), 87)))
        D, q = sc.randn((B, C, C), 88), sc.rand((B, H, W), 89)
        own, own2 = sc.fresh((B, C, H, W), 90), sc.fresh((B, C, H, W), 90)
        return {"gram": ops.gram_fwd(feat), "gram_weighted": ops.gram_fwd(feat, q), "bwd": ops.gram_bwd(D, feat, 0.37),
                "bwd_gated": ops.gram_bwd(D, feat, 0.37, gated=True), "bwd_weighted": ops.gram_bwd(D, feat, 0.37, gated=True, q=q),
                "bwd_own": ops.gram_bwd(D, feat, 0.37, out=own), "bwd_weighted_own": ops.gram_bwd(D, feat, 0.37, out=own2, q=q),
                "_own": [own, own2]}


@case("gram_fwd_multi", "gram_fwd_multi")
def _(ops, sc):
    feats = [sc.randn((2, 64, 7, 9), 91), sc.randn((2, 128, 4, 4), 92), sc.randn((2, 512, 4, 4), 93)]
    qs = [sc.rand((2, 7, 9), 94), sc.rand((2, 4, 4), 95), sc.rand((2, 4, 4), 96)]
    big = [sc.randn((2, 64, 64, 64), 115), sc.randn((2, 128, 32, 32), 116), sc.randn((2, 256, 16, 16), 117), sc.randn((2, 512, 8, 8), 118),
           sc.randn((2, 512, 4, 4), 93)]
    return {"grams": ops.gram_fwd_multi(feats), "weighted": ops.gram_fwd_multi(feats, qs), "one": ops.gram_fwd_multi(feats[:1]),
            "five taps": ops.gram_fwd_multi(big)}


for _S in (16, 17, 40):
    @case(f"guidance_build[S{_S}]", "guidance_build")
    def _(ops, sc, S=_S):
        planes, sums = ops.guidance_build(sc.rand((2, 1, S, S), 97))
        return {"planes": planes, "sums": sums}

for _n in (1, 257, 1025):
    @case(f"reductions[n{_n}]", ("sqdiff_sum", "sqdiff_sum_multi", "range_loss", "adam_step"))
    def _(ops, sc, n=_n):
        a, b, a3 = sc.randn((n,), 98), sc.randn((n,), 99), sc.randn((3, n), 100)
        s, D = ops.sqdiff_sum(a, b, 0.5, want_diff=True)
        s3, D3 = ops.sqdiff_sum(a3, b, 0.5, want_diff=True)
        multi, diffs = ops.sqdiff_sum_multi([(a, b, 0.5, 1, True), (a3, b, 2.0, 2, True), (b, a, 1.0, 2, False)], True, True, 3.0, 0.25)
        own = sc.fresh((3,), 101)
        multi2, _ = ops.sqdiff_sum_multi([(a, b, 0.5, 1, False)], False, False, 3.0, 0.25, out=own)
        rl, rg = ops.range_loss(sc.randn((n,), 102, 0.7))
        p, m, v = sc.fresh((n,), 103), sc.fresh((n,), 104, 0.1), sc.fresh((n,), 105).abs_()
        ops.adam_step(p, sc.randn((n,), 106), m, v, 3, 0.01)
        return {"sum": s, "diff": D, "sum_alone": ops.sqdiff_sum(a, b, 0.5), "sum_broadcast": s3, "diff_broadcast": D3, "multi": multi,
                "multi_diffs": diffs, "multi_own": multi2, "range": rl, "range_grad": rg, "range_alone": ops.range_loss(a, want_grad=False)[0],
                "p": p, "m": m, "v": v, "_own": [own, p, m, v]}

for _B, _C, _H, _W in ((1, 3, 1, 1), (2, 3, 17, 17), (1, 3, 5, 205)):       # 1, 289 and 1025 pixels per image
    @case(f"image losses[{_B},{_C},{_H},{_W}]", ("tv_loss", "masked_mse") if _H == _W else ("tv_loss",))
    def _(ops, sc, B=_B, C=_C, H=_H, W=_W):
        img, tgt = sc.rand((B, C, H, W), 107), sc.rand((B, C, H, W), 108)
        mask = sc.memo(("loss mask", B, H, W), lambda: (sc.rand((B, 1, H, W), 109) > 0.4).float())
        out = {}
        out["tv"], out["tv_grad"] = ops.tv_loss(img, mask)
        out["tv_alone"] = ops.tv_loss(img, mask, want_grad=False)[0]
        if H == W:
            out["mse"], out["mse_grad"] = ops.masked_mse(img, tgt, mask)
            out["mse_alone"] = ops.masked_mse(img, tgt, mask, want_grad=False)[0]
        return out

for _T, _L in ((1, 1), (24, 3), (17, 1), (40, 4)):
    @case(f"texpyr[T{_T},L{_L}]", ("texpyr_synth", "texpyr_adjoint"))
    def _(ops, sc, T=_T, L=_L):
        P = ops.texpyr_numel(T, L)
        own_t, own_p = sc.fresh((1, T, T, 3), 110), sc.fresh((P,), 111)
        params, grad = sc.randn((P,), 112), sc.randn((T, T, 3), 113)
        return {"texture": ops.texpyr_synth(params, T, L), "texture_own": ops.texpyr_synth(params, T, L, out=own_t),
                "grad": ops.texpyr_adjoint(grad, T, L), "grad_own": ops.texpyr_adjoint(grad, T, L, out=own_p), "_own": [own_t, own_p]}


# ================================================================================================== the renderer
def _render_case(sc, S, rs_kw, lights):
    """render_views forward and backward with the renderer's own buffers between guards as well; the gradients land in
    buffers of the case (.grad set beforehand: autograd accumulates into it in place)"""
    from st3d import render as R_
    m = sc.mesh("cow")
    verts = m["verts"].clone().requires_grad_(True)
    tex = sc.tex(32)[None].clone().requires_grad_(True)
    verts.grad, tex.grad = torch.zeros_like(verts), torch.zeros_like(tex)
    mesh = R_.Meshes(verts, m["faces"].long(), R_.TexturesUV(maps=tex, faces_uvs=m["fuv"].long()[None], verts_uvs=m["uvs"][None]))
    rs = R_.RasterizationSettings(image_size=S, **rs_kw)
    rgb, cov = R_.render_views(mesh, m["R"], m["T"], S, rs, None, lights(R_) if lights else None, None)
    (rgb * sc.randn((2, 3, S, S), 114)).sum().backward()
    return {"rgb": rgb.detach(), "coverage": cov.detach(), "grad_verts": verts.grad, "grad_texture": tex.grad,
            "_own": [verts.grad, tex.grad]}


@case("render_views[cow,B2,S17]", (), atomics=True, modules=RENDER)
def _(ops, sc):
    return _render_case(sc, 17, {}, None)


@case("render_views[cow,B2,S17,supersample 3,point lights]", (), atomics=True, modules=RENDER)
def _(ops, sc):
    return _render_case(sc, 17, {"supersample": 3}, lambda R_: sc.memo("render lights", lambda: R_.PointLights(location=((0.5, 1.0, 2.0),),
                                                                                                             device=sc.dev)))


# ================================================================================================== the test
@pytest.fixture(scope="module")
def sc(cow):
    assert torch.cuda.is_available()
    return Scene(torch.device("cuda:0"), cow)


@pytest.mark.parametrize("name", list(CASES))
def test_guarded(sc, name):
    from st3d import ops
    c = CASES[name]
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        spec = {out: part for wrapper, out, part, _ in UNSPECIFIED if wrapper in c.covers}
        own = lambda raw: raw.get("_own", ())          # noqa: E731
        G.compare_ab(lambda: c.run(ops, sc), modules=c.modules, own=own, specified=spec)
        if c.atomics:
            ops.set_deterministic(False)
            G.run_guarded(lambda: c.run(ops, sc), 0xFF, c.modules, own=lambda raw: list(G._flatten(raw).values()))
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):       # a device fault: every later launch would fail too
            pytest.exit(f"the device faulted in guarded case {name!r}: {e}", returncode=3)
        raise
    finally:
        ops.set_deterministic(was)
