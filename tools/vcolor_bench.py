#!/usr/bin/env python3
"""Cost of per-vertex colours (csrc/vcolor.hip, TexturesVertex, --texture_type vertex) next to the UV path, in one process,
at the config-2 shape (cow, 512^2, 8 views), medians of alternating windows:

  (a) kernels   shade_vc_fwd against shade_fwd, shade_vc_bwd against shade_bwd (colour / texture gradient alone) in both
                scatter modes, on the same fragments;
  (b) step      one second_approach-style texture step through the public API with a TexturesUV mesh and with a
                TexturesVertex mesh (colours = the map sampled at each vertex's UV).

Prints one JSON line and writes it to --out.

    python tools/vcolor_bench.py [--reps 50] [--rounds 7] [--steps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from silhouette_bench import _alternate, _summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="kernel calls per timing window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per candidate")
    ap.add_argument("--steps", type=int, default=5, help="optimisation steps per timing window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcolor_bench.json"))
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import cli, ops, render as R
    if not torch.cuda.is_available():
        raise SystemExit("vcolor_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    colours = cli.vertex_colors_from_map(verts.shape[0], faces, verts_uvs[0], faces_uvs[0], tex[0]).contiguous()
    line = {"shape": {"mesh": "cow", "size": S, "views": B, "verts": int(verts.shape[0]), "faces": int(faces.shape[0])}}
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    Rm, Tm = R.join_cameras(cameras)

    # (a) the kernels on the same fragments
    f32, fuv32 = faces.to(torch.int32).contiguous(), faces_uvs[0].to(torch.int32).contiguous()
    uvs, tmap = verts_uvs[0].contiguous(), tex[0].contiguous()
    frag = ops.raster_fwd(ops.project_verts(verts, Rm.to(dev), Tm.to(dev)), f32, S)
    g = torch.randn((B, 3, S, S), generator=torch.Generator().manual_seed(1)).to(dev)
    line["covered_share"] = round(float((frag[0] >= 0).float().mean()), 4)
    gtex, gcol = torch.zeros_like(tmap), torch.zeros_like(colours)

    def with_mode(det, fn):
        def run():
            ops.set_deterministic(det)
            fn()
        return run
    was = ops.is_deterministic()
    kernels = {
        "shade_fwd": lambda: ops.shade_fwd(frag, uvs, fuv32, tmap),
        "shade_vc_fwd": lambda: ops.shade_vc_fwd(frag, f32, colours),
        "shade_bwd_fixed_point": with_mode(True, lambda: ops.shade_bwd(g, frag, uvs, fuv32, tmap, grad_texture=gtex)),
        "shade_vc_bwd_fixed_point": with_mode(True, lambda: ops.shade_vc_bwd(g, frag, f32, colours, grad_colours=gcol)),
        "shade_bwd_float_atomics": with_mode(False, lambda: ops.shade_bwd(g, frag, uvs, fuv32, tmap, grad_texture=gtex)),
        "shade_vc_bwd_float_atomics": with_mode(False, lambda: ops.shade_vc_bwd(g, frag, f32, colours, grad_colours=gcol)),
        "shade_bwd_bary_too": with_mode(True, lambda: ops.shade_bwd(g, frag, uvs, fuv32, tmap, grad_texture=gtex, want_bary=True)),
        "shade_vc_bwd_bary_too": with_mode(True, lambda: ops.shade_vc_bwd(g, frag, f32, colours, grad_colours=gcol, want_bary=True)),
        "shade_vc_bwd_bary_alone": lambda: ops.shade_vc_bwd(g, frag, f32, colours, want_colours=False, want_bary=True),
    }
    line["kernels"] = {n: _summary(s) for n, s in _alternate(kernels, args.reps, args.rounds, args.warmup).items()}
    # the worst case for the LDS atomics: two triangles over the whole image, every lane of a tile deposits into the same
    # three or four entries (what a wave-level pre-reduction would be for)
    qv = torch.tensor([[-4.0, -4, 0], [5, -4, 0], [5, 4, 0], [-4, 4, 0]], device=dev)
    qf = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)
    qR, qT = torch.eye(3, device=dev).expand(B, 3, 3).contiguous(), torch.tensor([[0.0, 0, 3]], device=dev).expand(B, 3).contiguous()
    qfrag = ops.raster_fwd(ops.project_verts(qv, qR, qT), qf, S)
    qcol, qg = torch.rand(4, 3, device=dev), torch.zeros(4, 3, device=dev)
    large = {
        "quad_shade_vc_fwd": lambda: ops.shade_vc_fwd(qfrag, qf, qcol),
        "quad_shade_vc_bwd_fixed_point": with_mode(True, lambda: ops.shade_vc_bwd(g, qfrag, qf, qcol, grad_colours=qg)),
        "quad_shade_vc_bwd_float_atomics": with_mode(False, lambda: ops.shade_vc_bwd(g, qfrag, qf, qcol, grad_colours=qg)),
        "quad_shade_vc_bwd_bary_alone": lambda: ops.shade_vc_bwd(g, qfrag, qf, qcol, want_colours=False, want_bary=True),
    }
    line["large_faces"] = {"covered_share": round(float((qfrag[0] >= 0).float().mean()), 4)}
    line["large_faces"].update({n: _summary(s) for n, s in _alternate(large, args.reps, args.rounds, args.warmup).items()})
    ops.set_deterministic(was)
    line["deterministic"] = was

    # (b) one texture step through the public API
    vgg = U.get_vgg(seed=0)
    style = style_image.expand(B, -1, -1, -1)
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))

    def make_run(content_mesh, rebuild):
        with torch.no_grad():
            content, _ = U.render_meshes(renderer, content_mesh, cameras)
        out = U.setup_optimizations("texture", content_mesh, 0.01)

        def step():
            out["optimizer"].zero_grad()
            cur, _ = U.render_meshes(renderer, rebuild(out), cameras)
            loss = L.compute_perceptual_loss(cur, content, style, vgg, batch_denom=B)
            loss.backward()
            out["optimizer"].step()
        return step
    runs = {
        "textures_uv": make_run(U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces),
                                lambda o: U.build_mesh(o["verts_uvs"], o["faces_uvs"], o["texture_map"], o["verts"], o["faces"])),
        "textures_vertex": make_run(U.build_mesh_vertex(colours, verts, faces),
                                    lambda o: U.build_mesh_vertex(o["verts_features"], o["verts"], o["faces"])),
    }
    line["step"] = {n: _summary(s) for n, s in _alternate(runs, args.steps, args.rounds, args.warmup).items()}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
