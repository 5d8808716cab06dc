#!/usr/bin/env python3
"""Cost of the Laplacian content term (--lap_weight): the lap_loss wrapper with gradient on (8,3,512,512) at p = 4 and p = 16
next to its yardstick luma_fwd + luma_bwd -- the pair reads the planes once and writes them once, as the term does -- and ms
per optimisation step at the config-2 shape (cow, 512^2, 8 views, texture only, second_approach loop body) with the term off
and on.  The settings are timed in turn, --rounds times over, so that a drift of the machine shows up as spread and not as a
difference.  Prints one JSON line.

    python tools/lap_bench.py [--steps 100] [--warmup 5] [--rounds 3] [--no_steps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lap_bench.py --kernels_only

wrapper_call_ms is what a Python caller pays per call -- the launches and the allocation of the outputs and the workspace,
issued back to back over a window of at least 0.3 s.  Kernel times proper come from the second form: a run of its own under
the profiler, 50 calls of each wrapper, whose kernel statistics name the kernels.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]

import torch  # noqa: E402

POOLS = (4, 16)


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


def _wrapper_calls(B, S, dev):
    from st3d import lap, ops
    x, c = torch.rand(B, 3, S, S, device=dev), torch.rand(B, 3, S, S, device=dev)
    calls = {"luma_fwd": lambda: ops.luma_fwd(x), "luma_bwd": lambda: ops.luma_bwd(x)}
    for p in POOLS:
        T, scale = ops.lap_fwd(c, p), lap.term_scale(x.shape, p)
        calls[f"lap_loss_p{p}"] = lambda T=T, p=p, scale=scale: ops.lap_loss(x, T, p, scale)
        calls[f"lap_loss_p{p}_value_only"] = lambda T=T, p=p, scale=scale: ops.lap_loss(x, T, p, scale, want_grad=False)
        calls[f"lap_fwd_p{p}"] = lambda p=p: ops.lap_fwd(x, p)
    return calls, x


def kernels_only(args):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    calls, _ = _wrapper_calls(args.views, args.size, dev)
    for fn in calls.values():
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "calls_of_each": 50, "shape": [args.views, 3, args.size, args.size]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--lap_weight", type=float, default=1e4)
    ap.add_argument("--no_steps", action="store_true", help="the wrapper calls alone, not the optimisation steps")
    ap.add_argument("--kernels_only", action="store_true", help="50 calls of each wrapper and nothing else (for a profiler)")
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only(args)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    S, B = args.size, args.views
    line = {"shape": {"mesh": "cow", "size": S, "views": B, "target": "texture"}, "steps": args.steps, "rounds": args.rounds}

    # the wrapper calls alone, in turn, --rounds times over: a first window sizes the second to at least 0.3 s
    calls, x = _wrapper_calls(B, S, dev)
    rounds = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            first = _timed(fn, 200, 20)
            rounds[name].append(_timed(fn, max(200, int(300.0 / first)), 20))
    k = {name: statistics.median(v) for name, v in rounds.items()}
    n = 4 * x.numel()
    line["wrapper_call_ms"] = {name: round(t, 4) for name, t in k.items()}
    line["wrapper_call_ms_rounds"] = {name: [round(t, 4) for t in v] for name, v in rounds.items()}
    line["wrapper_call_bytes"] = {"luma_fwd": 2 * n, "luma_bwd": 2 * n}
    for p in POOLS:
        cells = n // (p * p)
        line["wrapper_call_bytes"][f"lap_loss_p{p}"] = 2 * n + 3 * cells        # x and grad; the target, r written and read
        line["wrapper_call_bytes"][f"lap_loss_p{p}_value_only"] = n + cells
        line["wrapper_call_bytes"][f"lap_fwd_p{p}"] = n + cells
    yard = k["luma_fwd"] + k["luma_bwd"]
    line["yardstick_luma_fwd_plus_bwd_ms"] = round(yard, 4)
    line["lap_loss_over_yardstick"] = {f"p{p}": round(k[f"lap_loss_p{p}"] / yard, 3) for p in POOLS}
    line["note"] = ("wrapper_call_ms holds the Python call: the launches plus the allocation of outputs and workspace, issued "
                    "back to back over >= 0.3 s, median of the rounds; lap_loss is three launches, two without the gradient; "
                    "kernel times proper: --kernels_only under a profiler")
    if args.no_steps:
        print(json.dumps(line))
        return

    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import render as R
    U.device = ST.device = L.device = dev
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    vgg = U.get_vgg(seed=0)
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, content_mesh, cameras)
    style = style_image.reshape(1, 3, S, S).expand(B, -1, -1, -1)
    settings = {"off": None, "pool_4": (4,), "pools_4_16": (4, 16)}
    line["ms_per_step"] = {name: [] for name in settings}
    losses = {}
    for _ in range(args.rounds):
        for name, pools in settings.items():
            out = U.setup_optimizations("texture", content_mesh, 0.01)

            def step():
                out["optimizer"].zero_grad()
                mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
                cur, masks = U.render_meshes(renderer, mesh, cameras)
                loss = L.compute_second_approach_loss(cur, content, style, vgg, 1e6, 1.0, out["verts"], verts, mesh, {},
                                                      "texture", batch_denom=B)
                if pools is not None:
                    loss = loss + args.lap_weight * L.compute_laplacian_loss(cur, content, pools, batch_denom=B)
                loss.backward()
                out["optimizer"].step()
                return loss

            line["ms_per_step"][name].append(round(_timed(step, args.steps, args.warmup), 3))
            losses[name] = float(step().detach())
    line["ms_per_step_median"] = {name: statistics.median(v) for name, v in line["ms_per_step"].items()}
    base = line["ms_per_step_median"]["off"]
    line["extra_ms_over_off"] = {name: round(v - base, 3) for name, v in line["ms_per_step_median"].items() if name != "off"}
    line["loss_after_the_timed_steps"] = losses
    print(json.dumps(line))


if __name__ == "__main__":
    main()
