#!/usr/bin/env python3
"""Cost of --preserve_color at the config-2 shape (cow, 512^2, 8 views, texture only, second_approach loop body): ms per
optimisation step with the flag off, with match, with luminance, and with luminance while the need / flat / epoch tags are
switched off (ST3D_NEED_MASK=0 ST3D_FLAT=0 ST3D_EPOCHS=0) -- what carrying the tags through luma() saves -- and the five
wrapper calls alone on (8,3,512,512), next to the bytes they move.  The settings are timed in turn, --rounds times over, so
that a drift of the machine shows up as spread and not as a difference.  Prints one JSON line.

    python tools/color_bench.py [--steps 100] [--warmup 5] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/color_bench.py --kernels_only

wrapper_call_ms is what a Python caller pays per call -- the launch(es) and the allocation of the output, issued back to back
over a window of at least 0.3 s -- and its bytes/s are rates of that call, not of the kernel.  Kernel times proper come from
the second form: a run of its own under the profiler, 50 calls of each wrapper, whose kernel statistics name the kernels.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]

import torch  # noqa: E402

TAG_SWITCHES = ("ST3D_NEED_MASK", "ST3D_FLAT", "ST3D_EPOCHS")


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--kernels_only", action="store_true", help="50 calls of each wrapper and nothing else (for a profiler)")
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only(args)
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import color, ops, render as R
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    vgg = U.get_vgg(seed=0)
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))
    with torch.no_grad():
        content, cover = U.render_meshes(renderer, content_mesh, cameras)
        style_rgb = style_image.reshape(1, 3, S, S)
        styles = {"off": style_rgb, "match": color.match_style(style_rgb, content, cover > 0),
                  "luminance": color.match_style_luminance(style_rgb, content, cover > 0)}
    # name -> (the style image, the loss sees luminance, the tags are on)
    settings = {"off": ("off", False, True), "match": ("match", False, True), "luminance": ("luminance", True, True),
                "luminance_untagged": ("luminance", True, False)}
    line = {"shape": {"mesh": "cow", "size": S, "views": B, "target": "texture"}, "steps": args.steps, "rounds": args.rounds,
            "ms_per_step": {k: [] for k in settings}}
    losses = {}
    saved = {k: os.environ.get(k) for k in TAG_SWITCHES}
    for rnd in range(args.rounds):
        for name, (style_key, luminance, tags) in settings.items():
            for k in TAG_SWITCHES:
                if tags:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = "0"
            out = U.setup_optimizations("texture", content_mesh, 0.01)
            style = styles[style_key].expand(B, -1, -1, -1)

            def step():
                out["optimizer"].zero_grad()
                mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
                cur, masks = U.render_meshes(renderer, mesh, cameras)
                seen, seen_content = (color.luma(cur), color.luma_cached(content)) if luminance else (cur, content)
                loss = L.compute_second_approach_loss(seen, seen_content, style, vgg, 1e6, 1.0, out["verts"], verts, mesh, {},
                                                      "texture", batch_denom=B)
                loss.backward()
                out["optimizer"].step()
                return loss

            line["ms_per_step"][name].append(round(_timed(step, args.steps, args.warmup), 3))
            losses[name] = float(step().detach())
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    line["ms_per_step_median"] = {k: statistics.median(v) for k, v in line["ms_per_step"].items()}
    base = line["ms_per_step_median"]["off"]
    line["extra_ms_over_off"] = {k: round(v - base, 3) for k, v in line["ms_per_step_median"].items() if k != "off"}
    line["tags_save_ms"] = round(line["ms_per_step_median"]["luminance_untagged"] - line["ms_per_step_median"]["luminance"], 3)
    line["loss_after_the_timed_steps"] = losses

    # the wrapper calls alone on (8,3,512,512): a first window sizes the second to at least 0.3 s
    calls, x, m = _wrapper_calls(B, S, dev)
    k = {}
    for name, fn in calls.items():
        first = _timed(fn, 200, 20)
        k[name] = _timed(fn, max(200, int(300.0 / first)), 20)
    n = 4 * x.numel()
    line["wrapper_call_ms"] = {name: round(t, 4) for name, t in k.items()}
    line["wrapper_call_bytes"] = {"luma_fwd": 2 * n, "luma_bwd": 2 * n, "luma_recombine": 3 * n, "color_affine": 2 * n,
                                  "color_sums": n + m.numel()}
    line["wrapper_call_gb_per_s"] = {name: round(line["wrapper_call_bytes"][name] / (t * 1e-3) / 1e9, 1) for name, t in k.items()}
    line["note"] = ("wrapper_call_ms holds the Python call: the launch(es) plus the allocation of its output, issued back to "
                    "back over >= 0.3 s; color_sums is two launches; kernel times proper: --kernels_only under a profiler")
    print(json.dumps(line))


def _wrapper_calls(B, S, dev):
    from st3d import ops
    x, y = torch.rand(B, 3, S, S, device=dev), torch.rand(B, 3, S, S, device=dev)
    m = (torch.rand(B, S, S, device=dev) < 0.3).to(torch.uint8)
    A, b = torch.eye(3).numpy() * 0.9, [0.01, 0.02, 0.03]
    return {"luma_fwd": lambda: ops.luma_fwd(x), "luma_bwd": lambda: ops.luma_bwd(x),
            "luma_recombine": lambda: ops.luma_recombine(x, y), "color_affine": lambda: ops.color_affine(x, A, b),
            "color_sums": lambda: ops.color_sums(x, m)}, x, m


def kernels_only(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    calls, _, _ = _wrapper_calls(args.views, args.size, dev)
    for fn in calls.values():
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "calls_of_each": 50, "shape": [args.views, 3, args.size, args.size]}))


if __name__ == "__main__":
    main()
