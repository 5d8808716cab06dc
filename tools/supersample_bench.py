#!/usr/bin/env python3
"""Cost and effect of supersampled rendering (csrc/shade.hip, RasterizationSettings(supersample=a), --supersample), in one
process, at the config-2 shape (cow, 512^2, 8 views, T = 512):

  (a) kernels   the fused forward (st3d_shade_ss_fwd) and the fused backward (st3d_shade_ss_bwd[_det], texture gradient)
                against the composition they replace (st3d_shade_fwd at a * S + st3d_box_down_fwd of rgb and mask;
                st3d_box_down_bwd + st3d_shade_bwd[_det] at a * S), a = 2 and, for the record, 3 and 4; HIP events, the
                candidates alternate inside every round; median and min-max over the rounds;
  (b) step      one second_approach-style texture step through the public API at a = 1, 2, 3, 4, in alternating windows;
  (c) quality   --quality_steps steps of that loop at a = 1 and a = 2: the share of texels that moved, and the final loss
                scored by an a = 1 and by an a = 2 render of the result.

Prints one JSON line and writes it to --out.

    python tools/supersample_bench.py [--reps 20] [--rounds 20] [--steps 5] [--quality_steps 200]
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
    ap.add_argument("--reps", type=int, default=20, help="kernel calls per timing window")
    ap.add_argument("--rounds", type=int, default=20, help="alternating windows per candidate")
    ap.add_argument("--steps", type=int, default=5, help="optimisation steps per timing window")
    ap.add_argument("--step_rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--quality_steps", type=int, default=200, help="0 = skip (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "supersample_bench.json"))
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops, render as R
    if not torch.cuda.is_available():
        raise SystemExit("supersample_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    line = {"deterministic": ops.is_deterministic(), "shape": {"mesh": "cow", "size": S, "views": B, "texture": S}}
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)

    # (a) the kernels, on the fragments of the config-2 views
    f32 = content_mesh.faces_i32()
    uvs = content_mesh.textures.verts_uvs_padded().reshape(-1, 2).contiguous()
    fuv = content_mesh.textures.faces_uvs_i32()
    t3 = tex.reshape(S, S, 3).contiguous()
    ndc = ops.project_verts(verts, cameras.R.to(dev), cameras.T.to(dev))
    g = torch.randn(B, 3, S, S, device=dev)
    kernels = {}
    for a in (2, 3, 4):
        frag = ops.raster_fwd(ndc, f32, a * S)

        def comp_fwd():
            hi, m = ops.shade_fwd(frag, uvs, fuv, t3)
            return ops.box_down_fwd(hi, a), ops.box_down_fwd(m, a)
        fns = {"fused_fwd": lambda: ops.shade_ss_fwd(frag, uvs, fuv, t3, a), "composition_fwd": comp_fwd,
               "fused_bwd": lambda: ops.shade_ss_bwd(g, frag, uvs, fuv, t3, a),
               "composition_bwd": lambda: ops.shade_bwd(ops.box_down_bwd(g, a), frag, uvs, fuv, t3),
               # the same candidate twice: what repeating one measurement gives
               "fused_fwd_again": lambda: ops.shade_ss_fwd(frag, uvs, fuv, t3, a),
               "fused_bwd_again": lambda: ops.shade_ss_bwd(g, frag, uvs, fuv, t3, a)}
        res = {n: _summary(s) for n, s in _alternate(fns, args.reps, args.rounds, args.warmup).items()}
        res["covered_share_of_sub_pixels"] = round(float((frag[0] >= 0).float().mean()), 4)
        kernels[f"a{a}"] = res
        del frag
    line["kernels"] = kernels

    # (b), (c): the second_approach texture step through the public API
    vgg = U.get_vgg(seed=0)
    style = style_image.expand(B, -1, -1, -1)

    def renderer(a):
        kw = {} if a == 1 else {"supersample": a}
        return R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S, **kw)),
                              R.SoftPhongShader(device=dev))

    def make_run(a):
        r = renderer(a)
        with torch.no_grad():
            content, _ = U.render_meshes(r, content_mesh, cameras)
        out = U.setup_optimizations("texture", content_mesh, 0.01)
        state = {"loss": None}

        def step():
            out["optimizer"].zero_grad()
            mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
            cur, _ = U.render_meshes(r, mesh, cameras)
            loss = L.compute_perceptual_loss(cur, content, style, vgg, batch_denom=B)
            loss.backward()
            out["optimizer"].step()
            state["loss"] = loss.detach()
        return step, out, state

    runs = {f"a{a}": make_run(a)[0] for a in (1, 2, 3, 4)}
    line["step"] = {n: _summary(s) for n, s in _alternate(runs, args.steps, args.step_rounds, args.warmup).items()}

    if args.quality_steps > 0:
        quality = {"steps": args.quality_steps}

        def score(texture_map, a):
            r = renderer(a)
            with torch.no_grad():
                content, _ = U.render_meshes(r, content_mesh, cameras)
                mesh = U.build_mesh(verts_uvs, faces_uvs, texture_map.detach(), verts, faces)
                cur, _ = U.render_meshes(r, mesh, cameras)
                return float(L.compute_perceptual_loss(cur, content, style, vgg, batch_denom=B))
        for a in (1, 2):
            step, out, state = make_run(a)
            for _ in range(args.quality_steps):
                step()
            moved = (out["texture_map"].detach() != tex).any(dim=-1)
            quality[f"a{a}"] = {"texels_moved_share": round(float(moved.float().mean()), 5), "last_training_loss": float(state["loss"]),
                                "final_loss_scored_at_a1": score(out["texture_map"], 1),
                                "final_loss_scored_at_a2": score(out["texture_map"], 2)}
        line["quality"] = quality
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
