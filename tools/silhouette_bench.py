#!/usr/bin/env python3
"""Cost of the silhouette term at the config-5 shape (bob, 512^2, 8 views, K = 8), in one process, alternating:

  * the fused st3d_silhouette_loss against the composition it replaces -- silhouette_fwd, squared difference (sqdiff_sum
    keeping the difference), its scaling by 2 * scale, silhouette_bwd -- by HIP events, with the bytes each moves per
    pixel at K = 8 (fused 32 + 32 + 4 read, 32 written = 100 B; composition 68 + 12 + 100 = 180 B, + 8 B for the scaling
    launch) turned into bytes/s;
  * one second_approach-style step on that scene (what ``bench.py --mesh bob --target both`` runs) with
    --silhouette_weight on against off.

Prints one JSON line.

    python tools/silhouette_bench.py [--reps 50] [--rounds 5] [--steps 10] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]

import torch  # noqa: E402


def _window(fn, reps):
    """ms per call over one window of `reps` calls (device events)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(fns, reps, rounds, warm):
    """{name: [ms per call of every round]}; the candidates take turns inside every round"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            out[n].append(_window(fn, reps))
    return out


def _summary(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="kernel calls per timing window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per candidate")
    ap.add_argument("--steps", type=int, default=10, help="optimisation steps per timing window (keep warmup + rounds * steps "
                    "small: a joint run at lr 0.01 changes the mesh, and with it the work, as it goes)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--mesh", default="bob")
    ap.add_argument("--weight", type=float, default=10.0)
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops, render as R
    if not torch.cuda.is_available():
        raise SystemExit("silhouette_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B, K, sigma = args.size, args.views, L.SILHOUETTE_FACES_PER_PIXEL, 1e-4
    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, args.mesh, 1)
    content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))
    with torch.no_grad():
        content, outline = U.render_meshes(renderer, content_mesh, cameras)
    line = {"shape": {"mesh": args.mesh, "size": S, "views": B, "K": K, "sigma": sigma}, "deterministic": ops.is_deterministic()}

    # ---- the kernels, on the fragments of the silhouette pass
    R_, T_ = R.join_cameras(cameras)
    ndc = ops.project_verts(verts.detach().float().contiguous(), R_.to(dev), T_.to(dev))
    p2f, _, _, dists, _ = ops.raster_soft_fwd(ndc, content_mesh.faces_i32(), S, K, L.silhouette_blur_radius(sigma), True, z_clip=0.5)
    scale = 1.0 / (S * S * B)
    n_pix = B * S * S

    def fused():
        return ops.silhouette_loss(p2f, dists, outline, sigma, scale)

    def composition():
        alpha = ops.silhouette_fwd(p2f, dists, sigma)
        loss, diff = ops.sqdiff_sum(alpha, outline, scale=scale, want_diff=True)
        return loss, ops.silhouette_bwd(diff.mul_(2.0 * scale), p2f, dists, sigma)

    (lf, gf), (lc, gc) = fused(), composition()
    line["fused_equals_composition"] = {"grad_dists_bitwise": bool(torch.equal(gf, gc)),
                                        "loss_rel_diff": abs(float(lf) - float(lc)) / max(abs(float(lc)), 1e-30)}
    t = _alternate({"fused": fused, "composition": composition}, args.reps, args.rounds, args.warmup)
    bytes_per_pixel = {"fused": 4 * (K + K + 1 + K), "composition": 4 * ((K + K + 1) + 3 + (1 + K + K + K)) + 8}
    line["kernels"] = {}
    for name, samples in t.items():
        s = _summary(samples)
        s["bytes_per_pixel"] = bytes_per_pixel[name]
        s["GB_per_s_at_median"] = round(bytes_per_pixel[name] * n_pix / (s["median_ms"] * 1e-3) / 1e9, 1)
        line["kernels"][name] = s
    line["kernels"]["fused_over_composition"] = round(line["kernels"]["fused"]["median_ms"] / line["kernels"]["composition"]["median_ms"], 3)
    for name, fn in (("silhouette_fwd", lambda: ops.silhouette_fwd(p2f, dists, sigma)),
                     ("silhouette_bwd", lambda: ops.silhouette_bwd(outline, p2f, dists, sigma))):
        line["kernels"][name] = _summary(_alternate({name: fn}, args.reps, args.rounds, args.warmup)[name])

    # ---- where the rest of the term's time goes: the silhouette pass is a K = 8 soft raster of its own
    v32, fi = verts.detach().float().contiguous(), content_mesh.faces_i32()
    Rd, Td = R_.to(dev), T_.to(dev)
    blur = L.silhouette_blur_radius(sigma)
    gd = gf
    vleaf = verts.detach().clone().requires_grad_(True)
    leaf_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, vleaf, faces)

    def whole_term():
        vleaf.grad = None
        L.compute_silhouette_loss(renderer, leaf_mesh, cameras, outline, sigma=sigma, batch_denom=B).backward()

    pieces = {"project_and_soft_raster_fwd_K8": lambda: ops.raster_soft_fwd(ops.project_verts(v32, Rd, Td), fi, S, K, blur, True, z_clip=0.5),
              "project_and_hard_raster_fwd_K1": lambda: ops.raster_fwd(ops.project_verts(v32, Rd, Td), fi, S),
              "soft_raster_bwd_dists_only": lambda: ops.raster_soft_bwd((None, None, gd), p2f, ndc, fi, True, True, _slots, 0.5),
              "compute_silhouette_loss_fwd_bwd": whole_term}
    _slots = ops.raster_soft_fwd(ndc, fi, S, K, blur, True, z_clip=0.5)[4]
    line["silhouette_pass"] = {n: _summary(_alternate({n: fn}, 20, 3, 3)[n]) for n, fn in pieces.items()}

    # ---- one optimisation step, term on against off (off = no silhouette op at all)
    vgg = U.get_vgg(seed=0)
    style = style_image.expand(B, -1, -1, -1)
    reg = {"main_loss_weight": 3.0, "mesh_verts_weight": 1.0, "mesh_edge_loss_weight": 1.0,
           "mesh_laplacian_smoothing_weight": 1.0, "mesh_normal_consistency_weight": 1.0}

    def make_step(weight):
        out = U.setup_optimizations("both", content_mesh, 0.01)

        def step():
            out["optimizer"].zero_grad()
            mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
            cur, _ = U.render_meshes(renderer, mesh, cameras)
            loss = L.compute_second_approach_loss(cur, content, style, vgg, 1e6, 1.0, out["verts"], verts, mesh, reg, "both",
                                                  batch_denom=B)
            if weight:
                loss = loss + weight * L.compute_silhouette_loss(renderer, mesh, cameras, outline, sigma=sigma, batch_denom=B)
            loss.backward()
            out["optimizer"].step()
        return step

    st = _alternate({"off": make_step(0.0), "on": make_step(args.weight)}, args.steps, args.rounds, args.warmup)
    line["step"] = {n: dict(_summary(s), windows_ms=[round(x, 3) for x in s]) for n, s in st.items()}
    line["step"]["on_minus_off_ms"] = round(line["step"]["on"]["median_ms"] - line["step"]["off"]["median_ms"], 4)
    line["step"]["steps_per_window"], line["step"]["rounds"] = args.steps, args.rounds
    print(json.dumps(line))


if __name__ == "__main__":
    main()
