#!/usr/bin/env python3
"""Cost of --style_regions at the config-2 shape (cow, 512^2, 8 views, texture only, second_approach loop body): ms per
optimisation step through the public API with --style_mask object (the yardstick: the fused plan), with the cow split x:0
(R = 2) and with a 4-slab split along x, the three timed in turn, --rounds times over, so that a drift of the machine shows
up as spread and not as a difference.  The region runs keep the planes of the view batch, as a texture-only run does.  Then
st3d_region_planes on (8,512,512) at R = 2, 4, 8 by device events next to the bytes it must move: 4 B read and
R (4/3) 4 B written per pixel (the labels are a gather from a table of F bytes).  Prints one JSON line.

    python tools/regions_bench.py [--steps 30] [--warmup 5] [--rounds 3]
    python tools/regions_bench.py --planes_only      # the launches alone, for a kernel trace in a run of its own
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]

import numpy as np  # noqa: E402
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


def _slabs(RG, verts, faces, R):
    """R slabs along x: x:0 for R = 2, else the quantiles of the face centroids"""
    if R == 2:
        return RG.regions_from_axis(verts, faces, "x", [0.0])
    c = verts.double().cpu().numpy()[faces.cpu().numpy(), 0].mean(1)
    return RG.regions_from_axis(verts, faces, "x", list(np.quantile(c, np.arange(1, R) / R)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--planes_only", action="store_true")
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops, regions as RG, render as R
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    Rm, T = R.join_cameras(cameras)
    p2f = ops.raster_fwd(ops.project_verts(verts, Rm.to(dev), T.to(dev)), content_mesh.faces_i32(), S)[0]
    labels = {Rn: RG.check_face_regions(_slabs(RG, verts, faces, Rn), int(faces.shape[0]), device=dev)[0] for Rn in (2, 4, 8)}
    line = {"shape": {"mesh": "cow", "size": S, "views": B, "target": "texture"}}

    # the kernel pair alone
    reps = 20 if args.planes_only else 200
    k = {Rn: _timed(lambda Rn=Rn: RG.region_planes(p2f, labels[Rn], Rn), reps, 5) for Rn in (2, 4, 8)}
    per_pixel = {Rn: 4 + Rn * 4 * sum(0.25 ** l for l in range(5)) for Rn in (2, 4, 8)}
    line["region_planes_ms"] = {str(Rn): round(t, 4) for Rn, t in k.items()}
    line["region_planes_bytes"] = {str(Rn): int(per_pixel[Rn] * B * S * S) for Rn in (2, 4, 8)}
    line["region_planes_gb_per_s"] = {str(Rn): round(per_pixel[Rn] * B * S * S / (k[Rn] * 1e-3) / 1e9, 1) for Rn in (2, 4, 8)}
    line["region_planes_note"] = ("the wrapper call by device events: both launches plus the allocation of q, sums and partials; the "
                                  "second launch reads and rewrites q, which the byte count leaves out")
    if args.planes_only:
        print(json.dumps(line))
        return

    vgg = U.get_vgg(seed=0)
    style = style_image.expand(B, -1, -1, -1)
    styles = torch.stack([bench.load_assets(S, dev, "cow", kk)[5] for kk in (1, 3, 4, 5)]).contiguous()
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, content_mesh, cameras)
    settings = {"style_mask object": None, "style_regions x:0 (R=2)": 2, "style_regions 4 slabs (R=4)": 4}
    style_sets = {2: styles[:2].contiguous(), 4: styles}
    line.update({"steps": args.steps, "rounds": args.rounds, "ms_per_step": {k_: [] for k_ in settings}})
    losses = {}
    for rnd in range(args.rounds):
        for name, Rn in settings.items():
            out = U.setup_optimizations("texture", content_mesh, 0.01)
            kept = {}

            def step():
                out["optimizer"].zero_grad()
                mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
                cur, masks = U.render_meshes(renderer, mesh, cameras)
                if Rn is None:
                    loss = L.compute_second_approach_loss(cur, content, style, vgg, 1e6, 1.0, out["verts"], verts, mesh, {},
                                                          "texture", batch_denom=B, style_masks=masks)
                else:
                    if "planes" not in kept:        # the step's own fragments, once: the geometry does not move
                        kept["planes"] = RG.region_planes(RG.fragments_of(cur), labels[Rn], Rn)
                    loss = L.compute_region_style_loss(cur, content, style_sets[Rn], None, labels[Rn], vgg, 1e6, 1.0,
                                                       batch_denom=B, planes=kept["planes"])
                loss.backward()
                out["optimizer"].step()
                return loss

            line["ms_per_step"][name].append(round(_timed(step, args.steps, args.warmup), 3))
            losses[name] = float(step().detach())
    line["ms_per_step_median"] = {k_: statistics.median(v) for k_, v in line["ms_per_step"].items()}
    base = line["ms_per_step_median"]["style_mask object"]
    line["extra_ms_over_style_mask_object"] = {k_: round(v - base, 3) for k_, v in line["ms_per_step_median"].items()
                                               if k_ != "style_mask object"}
    line["loss_after_the_timed_steps"] = losses
    print(json.dumps(line))


if __name__ == "__main__":
    main()
