#!/usr/bin/env python3
"""Cost of the per-face texel atlas (csrc/atlas.hip, TexturesAtlas, --texture_atlas) next to the UV and vertex-colour paths,
in one process, at the config-2 shape (cow, 512^2, 8 views), medians of alternating windows:

  (a) kernels   shade_atlas_fwd against shade_fwd, shade_atlas_bwd against shade_bwd (atlas / texture gradient alone) in
                both scatter modes, at R = 1 and R = 8, on the same fragments;
  (b) step      one second_approach-style texture step through the public API with a TexturesUV, a TexturesVertex and a
                TexturesAtlas (R = 8) mesh.

Prints one JSON line and writes it to --out.

    python tools/atlas_bench.py [--reps 50] [--rounds 7] [--steps 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atlas_bench.json"))
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import cli, ops, render as R
    if not torch.cuda.is_available():
        raise SystemExit("atlas_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    n_faces = int(faces.shape[0])
    atlases = {r: cli.atlas_from_map(r, verts_uvs[0], faces_uvs[0], tex[0]).contiguous() for r in (1, 8)}
    colours = cli.vertex_colors_from_map(verts.shape[0], faces, verts_uvs[0], faces_uvs[0], tex[0]).contiguous()
    line = {"shape": {"mesh": "cow", "size": S, "views": B, "verts": int(verts.shape[0]), "faces": n_faces}}
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    Rm, Tm = R.join_cameras(cameras)

    # (a) the kernels on the same fragments
    f32, fuv32 = faces.to(torch.int32).contiguous(), faces_uvs[0].to(torch.int32).contiguous()
    uvs, tmap = verts_uvs[0].contiguous(), tex[0].contiguous()
    frag = ops.raster_fwd(ops.project_verts(verts, Rm.to(dev), Tm.to(dev)), f32, S)
    g = torch.randn((B, 3, S, S), generator=torch.Generator().manual_seed(1)).to(dev)
    line["covered_share"] = round(float((frag[0] >= 0).float().mean()), 4)
    gtex = torch.zeros_like(tmap)
    gat = {r: torch.zeros_like(a) for r, a in atlases.items()}

    def with_mode(det, fn):
        def run():
            ops.set_deterministic(det)
            fn()
        return run
    was = ops.is_deterministic()
    kernels = {
        "shade_fwd": lambda: ops.shade_fwd(frag, uvs, fuv32, tmap),
        "shade_bwd_fixed_point": with_mode(True, lambda: ops.shade_bwd(g, frag, uvs, fuv32, tmap, grad_texture=gtex)),
        "shade_bwd_float_atomics": with_mode(False, lambda: ops.shade_bwd(g, frag, uvs, fuv32, tmap, grad_texture=gtex)),
    }
    for r in (1, 8):
        kernels[f"shade_atlas_fwd_R{r}"] = lambda r=r: ops.shade_atlas_fwd(frag, atlases[r])
        kernels[f"shade_atlas_bwd_fixed_point_R{r}"] = with_mode(
            True, lambda r=r: ops.shade_atlas_bwd(g, frag, r, n_faces, grad_atlas=gat[r]))
        kernels[f"shade_atlas_bwd_float_atomics_R{r}"] = with_mode(
            False, lambda r=r: ops.shade_atlas_bwd(g, frag, r, n_faces, grad_atlas=gat[r]))
    line["kernels"] = {n: _summary(s) for n, s in _alternate(kernels, args.reps, args.rounds, args.warmup).items()}
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
        "textures_atlas_R8": make_run(U.build_mesh_atlas(atlases[8], verts, faces),
                                      lambda o: U.build_mesh_atlas(o["atlas"], o["verts"], o["faces"])),
    }
    line["step"] = {n: _summary(s) for n, s in _alternate(runs, args.steps, args.rounds, args.warmup).items()}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
