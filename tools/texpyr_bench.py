#!/usr/bin/env python3
"""Cost and effect of the texture pyramid (csrc/texpyr.hip, --texture_pyramid_levels), in one process:

  (a) kernels   st3d_texpyr_synth and st3d_texpyr_adjoint at T = 512 and 1024 with levels = 0 (auto), by HIP events in
                alternating windows, against the floor of their algorithmic bytes: 12 T^2 (1 + 1/3) read and as much
                written per direction at --hbm_tbs TB/s;
  (b) step      one second_approach-style texture step at the config-2 shape (cow, 512^2, 8 views) with levels = 1 against
                levels = 0, alternating (what bench.py runs, which cannot carry the flag);
  (c) quality   --quality_steps steps of that loop on cow and on bob with levels = 1 and levels = 0: the share of in-chart
                texels (inside a UV triangle, dilated by one texel) still EQUAL to the original map, and the last loss.

Prints one JSON line.

    python tools/texpyr_bench.py [--reps 200] [--rounds 7] [--steps 10] [--quality_steps 200]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from silhouette_bench import _alternate, _summary  # noqa: E402


def chart_mask(verts_uvs, faces_uvs, T):
    """(T,T) bool: texels whose centre lies inside a UV triangle, dilated by one texel (texel (x, y) has its centre at
    u = (x + 0.5) / T, v = 1 - (y + 0.5) / T)."""
    uv = np.asarray(verts_uvs, np.float64).reshape(-1, 2)
    px = np.stack([uv[:, 0] * T - 0.5, (1.0 - uv[:, 1]) * T - 0.5], 1)
    inside = np.zeros((T, T), bool)
    for tri in px[np.asarray(faces_uvs).reshape(-1, 3)]:
        lo = np.maximum(np.floor(tri.min(0)).astype(int), 0)
        hi = np.minimum(np.ceil(tri.max(0)).astype(int), T - 1)
        if (hi < lo).any():
            continue
        xs, ys = np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1))
        (ax, ay), (bx, by), (cx, cy) = tri
        e0 = (bx - ax) * (ys - ay) - (by - ay) * (xs - ax)
        e1 = (cx - bx) * (ys - by) - (cy - by) * (xs - bx)
        e2 = (ax - cx) * (ys - cy) - (ay - cy) * (xs - cx)
        hit = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        inside[ys[hit], xs[hit]] = True
    out = inside.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out[max(dy, 0):T + min(dy, 0), max(dx, 0):T + min(dx, 0)] |= inside[max(-dy, 0):T + min(-dy, 0), max(-dx, 0):T + min(-dx, 0)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="kernel calls per timing window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per candidate")
    ap.add_argument("--steps", type=int, default=10, help="optimisation steps per timing window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--quality_steps", type=int, default=200, help="0 = skip (c)")
    ap.add_argument("--hbm_tbs", type=float, default=4.0, help="streaming rate the byte floor is stated at, TB/s")
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops, render as R
    if not torch.cuda.is_available():
        raise SystemExit("texpyr_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    line = {"deterministic": ops.is_deterministic()}

    # (a) the two kernels
    kernels = {}
    for T in (512, 1024):
        Lv = len(ops.texpyr_sides(T, 0))
        P = ops.texpyr_numel(T, Lv)
        params = torch.randn(P, device=dev)
        grad = torch.randn(1, T, T, 3, device=dev)
        tex, gp = torch.empty(1, T, T, 3, device=dev), torch.empty(P, device=dev)
        copy_to = torch.empty(1, T, T, 3, device=dev)
        fns = {"synth": lambda: ops.texpyr_synth(params, T, Lv, out=tex), "adjoint": lambda: ops.texpyr_adjoint(grad, T, Lv, out=gp),
               "copy_of_one_map": lambda: copy_to.copy_(grad)}          # a plain 12 T^2-byte device copy, for scale
        res = {n: _summary(s) for n, s in _alternate(fns, args.reps, args.rounds, args.warmup).items()}
        floor_bytes = 4 * (P + 3 * T * T)                               # the parameters once, the map once
        floor_ms = floor_bytes / (args.hbm_tbs * 1e12) * 1e3
        for n in ("synth", "adjoint"):
            res[n]["fraction_of_byte_floor"] = round(floor_ms / res[n]["median_ms"], 4)
        res.update(levels=Lv, params=P, floor_bytes=floor_bytes, floor_ms_at_hbm_rate=round(floor_ms, 5))
        kernels[f"T{T}"] = res
    line["kernels"] = kernels

    # (b) and (c): the second_approach step through the public API
    S, B = args.size, args.views
    vgg = U.get_vgg(seed=0)
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    renderer = R.MeshRenderer(R.MeshRasterizer(R.FoVPerspectiveCameras(device=dev), R.RasterizationSettings(image_size=S)),
                              R.SoftPhongShader(device=dev))

    def make_run(mesh_name, levels):
        verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, mesh_name, 1)
        content_mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
        style = style_image.expand(B, -1, -1, -1)
        with torch.no_grad():
            content, _ = U.render_meshes(renderer, content_mesh, cameras)
        out = U.setup_optimizations("texture", content_mesh, 0.01, texture_pyramid_levels=levels)
        pyr = out.get("texture_pyramid")
        state = {"loss": None}

        def texture():
            return pyr.texture() if pyr is not None else out["texture_map"]

        def step():
            out["optimizer"].zero_grad()
            mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], texture(), out["verts"], out["faces"])
            cur, _ = U.render_meshes(renderer, mesh, cameras)
            loss = L.compute_perceptual_loss(cur, content, style, vgg, batch_denom=B)
            loss.backward()
            out["optimizer"].step()
            state["loss"] = loss.detach()
        return step, texture, tex, state, (verts_uvs, faces_uvs)

    plain, _, _, _, _ = make_run("cow", 1)
    pyramid, _, _, _, _ = make_run("cow", 0)
    steps = {n: _summary(s) for n, s in _alternate({"levels_1": plain, "levels_0": pyramid}, args.steps, args.rounds, args.warmup).items()}
    extra = steps["levels_0"]["median_ms"] - steps["levels_1"]["median_ms"]
    steps.update(shape={"mesh": "cow", "size": S, "views": B}, pyramid_cost_ms=round(extra, 4),
                 pyramid_cost_percent=round(100.0 * extra / steps["levels_1"]["median_ms"], 3))
    line["step"] = steps

    if args.quality_steps > 0:
        quality = {}
        for mesh_name in ("cow", "bob"):
            entry = {}
            for levels in (1, 0):
                step, texture, tex0, state, (uvs, fuv) = make_run(mesh_name, levels)
                for _ in range(args.quality_steps):
                    step()
                with torch.no_grad():
                    same = (texture().detach() == tex0).all(dim=-1)[0].cpu().numpy()
                chart = chart_mask(uvs.cpu().numpy(), fuv.cpu().numpy(), S)
                entry[f"levels_{levels}"] = {"in_chart_texels_equal_to_original": round(float(same[chart].mean()), 5),
                                             "all_texels_equal_to_original": round(float(same.mean()), 5),
                                             "last_loss": float(state["loss"])}
            entry["chart_share"] = round(float(chart.mean()), 4)
            quality[mesh_name] = entry
        line["quality"] = dict(quality, steps=args.quality_steps)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
