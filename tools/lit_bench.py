#!/usr/bin/env python3
"""Cost of Phong lighting at the config-2 shape (cow, 512^2, 8 views, second_approach loop body): ms per optimisation step
with --lights ambient (today's unlit kernels), point and directional, for --target texture and both, plus per-kernel
times of the lit render kernels against their unlit counterparts.  Prints one JSON line.

    python tools/lit_bench.py [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]

import torch  # noqa: E402


def _timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops, render as R
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    vgg = U.get_vgg(seed=0)
    style = style_image.expand(B, -1, -1, -1)
    reg = {"main_loss_weight": 3.0, "mesh_verts_weight": 1.0, "mesh_edge_loss_weight": 1.0,
           "mesh_laplacian_smoothing_weight": 1.0, "mesh_normal_consistency_weight": 1.0}
    shading = {"ambient": (R.AmbientLights(device=dev), None),
               "point": (R.PointLights(location=((0.0, 1.0, 0.0),), device=dev), R.Materials(device=dev)),
               "directional": (R.DirectionalLights(direction=((0.0, 1.0, 0.0),), device=dev), R.Materials(device=dev))}
    line = {"shape": {"mesh": "cow", "size": S, "views": B}, "steps": args.steps, "ms_per_step": {}}
    for target in ("texture", "both"):
        for name, (lights, mats) in shading.items():
            renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev),
                                                       R.RasterizationSettings(image_size=S)),
                                      R.SoftPhongShader(device=dev, lights=lights, materials=mats))
            with torch.no_grad():
                content, _ = U.render_meshes(renderer, content_mesh, cameras)
            out = U.setup_optimizations(target, content_mesh, 0.01)

            def step():
                out["optimizer"].zero_grad()
                mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
                cur, masks = U.render_meshes(renderer, mesh, cameras)
                loss = L.compute_second_approach_loss(cur, content, style, vgg, 1e6, 1.0, out["verts"], verts, mesh, reg,
                                                      target, batch_denom=B)
                loss.backward()
                out["optimizer"].step()

            line["ms_per_step"][f"{target}/{name}"] = round(_timed(step, args.steps, args.warmup), 3)

    # per-kernel: the lit render kernels next to the unlit ones, on the same fragments
    R_, T_ = R.join_cameras(cameras)
    R_, T_ = R_.to(dev), T_.to(dev)
    v = verts.detach().float().contiguous()
    fi = content_mesh.faces_i32()
    uvs = verts_uvs.reshape(-1, 2).float().contiguous()
    fuv = content_mesh.textures.faces_uvs_i32()
    texm = tex.reshape(tex.shape[-3], tex.shape[-2], 3).float().contiguous()
    ndc = ops.project_verts(v, R_, T_)
    frag = ops.raster_fwd(ndc, fi, S)
    grad = torch.randn(B, 3, S, S, device=dev)
    lit = R._lit_setup(R.lighting_of(*shading["point"], dev), v, v, fi, R_, T_)
    inc = lit.incidence
    k = {}
    k["shade_fwd"] = _timed(lambda: ops.shade_fwd(frag, uvs, fuv, texm), 20)
    k["shade_lit_fwd"] = _timed(lambda: ops.shade_lit_fwd(frag, uvs, fuv, texm, lit), 20)
    k["shade_bwd_texture"] = _timed(lambda: ops.shade_bwd(grad, frag, uvs, fuv, texm), 20)
    k["shade_lit_bwd_texture"] = _timed(lambda: ops.shade_lit_bwd(grad, frag, uvs, fuv, texm, lit), 20)
    k["shade_bwd_both"] = _timed(lambda: ops.shade_bwd(grad, frag, uvs, fuv, texm, want_bary=True), 20)
    k["shade_lit_bwd_both"] = _timed(lambda: ops.shade_lit_bwd(grad, frag, uvs, fuv, texm, lit, want_geometry=True), 20)
    _, _, gnp = ops.shade_lit_bwd(grad, frag, uvs, fuv, texm, lit, want_texture=False, want_geometry=True)
    k["vertex_normals"] = _timed(lambda: ops.vertex_normals(v, fi, inc), 20)
    k["phong_scatter"] = _timed(lambda: ops.phong_scatter(gnp, frag[0], frag[2], fi, v.shape[0]), 20)
    s = ops.phong_scatter(gnp, frag[0], frag[2], fi, v.shape[0])
    gv = torch.zeros_like(v)
    k["vertex_normals_bwd"] = _timed(lambda: ops.vertex_normals_bwd(v, fi, inc, lit.unnormalised, s[1], s[0], gv), 20)
    line["kernel_ms"] = {n: round(t, 4) for n, t in k.items()}
    line["deterministic"] = ops.is_deterministic()
    ms = line["ms_per_step"]
    line["lit_minus_ambient_ms"] = {f"{t}/{n}": round(ms[f"{t}/{n}"] - ms[f"{t}/ambient"], 3)
                                    for t in ("texture", "both") for n in ("point", "directional")}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
