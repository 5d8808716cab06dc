#!/usr/bin/env python3
"""Cost of the multi-scale style loss at the config-2 shape (cow, 512^2, 8 views, texture only, second_approach loop body):
ms per optimisation step with --style_scales 1, 1,2 and 1,2,4, the bytes each scale's plan holds, and one pyramid step
forward and transposed on (8,3,512,512) alone, next to the bytes they move.  The three settings are timed in turn, --rounds
times over, so that a drift of the machine shows up as spread and not as a difference.  Prints one JSON line.

    python tools/scales_bench.py [--steps 30] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--rounds", type=int, default=3)
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
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, content_mesh, cameras)
    settings = {"1": (1,), "1,2": (1, 2), "1,2,4": (1, 2, 4)}
    line = {"shape": {"mesh": "cow", "size": S, "views": B, "target": "texture"}, "steps": args.steps, "rounds": args.rounds,
            "ms_per_step": {k: [] for k in settings}}
    losses = {}
    for rnd in range(args.rounds):
        for name, scales in settings.items():
            out = U.setup_optimizations("texture", content_mesh, 0.01)

            def step():
                out["optimizer"].zero_grad()
                mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
                cur, masks = U.render_meshes(renderer, mesh, cameras)
                loss = L.compute_second_approach_loss(cur, content, style, vgg, 1e6, 1.0, out["verts"], verts, mesh, {},
                                                      "texture", batch_denom=B, style_scales=scales)
                loss.backward()
                out["optimizer"].step()
                return loss

            line["ms_per_step"][name].append(round(_timed(step, args.steps, args.warmup), 3))
            losses[name] = float(step().detach())
    line["ms_per_step_median"] = {k: statistics.median(v) for k, v in line["ms_per_step"].items()}
    base = line["ms_per_step_median"]["1"]
    line["extra_ms_over_single_scale"] = {k: round(v - base, 3) for k, v in line["ms_per_step_median"].items() if k != "1"}
    line["loss_after_the_timed_steps"] = losses
    line["plan_bytes"] = {str(S // f): vgg.plan(B, S // f).bytes() for f in (1, 2, 4)}

    # the pyramid step alone: (8,3,512,512) in, a quarter of it out
    x = torch.rand(B, 3, S, S, device=dev)
    g = torch.rand(B, 3, S // 2, S // 2, device=dev)
    m = (torch.rand(B, S, S, device=dev) < 0.3).to(torch.uint8)
    moved = 4 * (x.numel() + g.numel())                     # one side read, the other written
    k = {"pyr_down_fwd": _timed(lambda: ops.pyr_down_fwd(x), 200, 20), "pyr_down_bwd": _timed(lambda: ops.pyr_down_bwd(g), 200, 20),
         "pyr_down_need": _timed(lambda: ops.pyr_down_need(m), 200, 20)}
    line["kernel_ms"] = {n: round(t, 4) for n, t in k.items()}
    line["kernel_bytes"] = {"pyr_down_fwd": moved, "pyr_down_bwd": moved, "pyr_down_need": m.numel() + m.numel() // 4}
    line["kernel_gb_per_s"] = {n: round(line["kernel_bytes"][n] / (t * 1e-3) / 1e9, 1) for n, t in k.items()}
    line["note"] = "kernel_ms holds the wrapper call: the launch plus the allocation of its output, timed back to back"
    print(json.dumps(line))


if __name__ == "__main__":
    main()
