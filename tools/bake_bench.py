#!/usr/bin/env python3
"""The figures of DESIGN.md 7 "Baking views into the texture", at the shape of BASELINE config 2: the cow, image and texture
side 512, 8 random views of seed 0.

  * texel_surface (once per mesh) and one bake_views launch per mode, each bracketed by its own pair of HIP events; medians,
    minima and maxima over --repeats calls after --warmup;
  * 100 steps of the existing phase-B loop (render, masked MSE, backward, Adam) on a host clock between device synchronises;
  * the share of texel-views whose visibility differs between half and twice the default of depth_tol and of min_cos (power
    changes no visibility; the largest change of a texel's colour between power 1 and 4 is reported instead);
  * the phase-B loss at steps 0, 10 and 100 from the loaded map and from the map baked ('mean', 'best') out of the targets
    that --phase_a_steps of 2-D style transfer (first_approach's phase A, started from the content renders) produce.

The figures are reported, nothing is bounded by them.  Prints one JSON line and writes it to --out.

    python tools/bake_bench.py [--repeats 20] [--phase_a_steps 3000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512, help="image side and texture side")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--phase_a_steps", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bake_bench needs a GPU (there is nothing to time without one)")
    import _scenes
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import bake, ops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    cow = _scenes.load_asset("cow")
    S = T = args.size
    B = args.views
    R, Tr = _scenes.random_cameras(B, 0)
    mesh, renderer, cams = _scenes.device_scene(U, dev, cow["verts"], cow["faces"], cow["verts_uvs"], cow["faces_uvs"],
                                                _scenes.texture_at(cow, T), R, Tr, S)
    tex = mesh.textures
    verts, faces = mesh.verts_packed().contiguous(), mesh.faces_i32()
    uvs = tex.verts_uvs_padded().reshape(-1, 2).contiguous()
    fuv = tex.faces_uvs_i32()
    loaded = tex.maps_padded()[0].contiguous()

    def stats(ms):
        return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return out, a.elapsed_time(b)

    def timed(fn):
        ms = [events(fn)[1] for _ in range(args.warmup + args.repeats)]
        return stats(ms[args.warmup:])

    line = {"mesh": "cow", "image_size": S, "texture_size": T, "views": B, "repeats": args.repeats, "warmup": args.warmup}
    t2f, tbary = bake.texel_surface(uvs, fuv, T)
    line["texel_surface_ms"] = timed(lambda: bake.texel_surface(uvs, fuv, T))
    line["texels_owned"] = int((t2f >= 0).sum())
    line["texels_inside_chart"] = int((bake.texel_surface(uvs, fuv, T, 0.0)[0] >= 0).sum())
    dR, dT = cams.R.contiguous(), cams.T.contiguous()
    p2f, zbuf, _, _ = ops.raster_fwd(ops.project_verts(verts, dR, dT), faces, S)
    with torch.no_grad():
        content, outline = U.render_meshes(renderer, mesh, cams)
    content = content.detach().contiguous()
    for mode in ("mean", "best"):
        line[f"bake_views_{mode}_ms"] = timed(lambda: bake.bake_views(verts, faces, t2f, tbary, dR, dT, content, p2f, zbuf, mode=mode))

    # ---- how much the untuned defaults matter: per-view visibility (acc.w > 0 of a one-view bake)
    def visible(**kw):
        return torch.stack([bake.bake_views(verts, faces, t2f, tbary, dR[b:b + 1].contiguous(), dT[b:b + 1].contiguous(),
                                            content[b:b + 1].contiguous(), p2f[b:b + 1].contiguous(), zbuf[b:b + 1].contiguous(),
                                            **kw)[..., 3] > 0 for b in range(B)])
    base = visible()
    texel_views = int((t2f >= 0).sum()) * B
    line["texel_views"] = texel_views
    line["texel_views_visible_at_defaults"] = int(base.sum())
    for name, default in (("depth_tol", 0.01), ("min_cos", 0.1)):
        lo, hi = visible(**{name: default / 2}), visible(**{name: default * 2})
        line[f"visibility_changed_{name}_half_vs_twice"] = round(int((lo != hi).sum()) / texel_views, 6)
    fallback = torch.zeros_like(loaded)
    t1 = bake.baked_texture(bake.bake_views(verts, faces, t2f, tbary, dR, dT, content, p2f, zbuf, power=1.0), fallback)
    t4 = bake.baked_texture(bake.bake_views(verts, faces, t2f, tbary, dR, dT, content, p2f, zbuf, power=4.0), fallback)
    line["colour_change_power_1_vs_4"] = {"max": round(float((t1 - t4).abs().max()), 6), "mean": round(float((t1 - t4).abs().mean()), 6)}

    # ---- phase B from the loaded map and from the baked maps, on the targets of a real phase A
    style = _scenes.style_at(1, S).to(dev).expand(B, -1, -1, -1)
    vgg = U.get_vgg(weights=os.environ.get("ST3D_VGG19_WEIGHTS"))
    line["vgg_weights"] = "file" if os.environ.get("ST3D_VGG19_WEIGHTS") else "seeded"
    background = U.apply_background(content, outline, background_type='white', background=style)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    targets = U.finalize_tensor(ST.style_transfer(background, background, style, vgg, steps=args.phase_a_steps, style_weight=1e6,
                                                  content_weight=1.0, lr=0.01)).detach().contiguous()
    torch.cuda.synchronize()
    line["phase_a_steps"], line["phase_a_s"] = args.phase_a_steps, round(time.perf_counter() - t0, 3)

    def phase_b(start, steps=101):
        m0 = U.build_mesh(tex.verts_uvs_padded(), tex.faces_uvs_padded(), start[None].clone(), mesh.verts_packed(), mesh.faces_packed())
        opt = U.setup_optimizations("texture", m0, 0.01)
        losses = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt["optimizer"].zero_grad()
            m = U.build_mesh(opt["verts_uvs"], opt["faces_uvs"], opt["texture_map"], opt["verts"], opt["faces"])
            img, cov = U.render_meshes(renderer, m, cams)
            loss = L.compute_first_approach_loss(rendered=img, masks=cov, target_rendered=targets, verts=opt["verts"],
                                                 target_verts=mesh.verts_packed(), mesh=m, weights={}, opt_type='texture')
            loss.backward()
            opt["optimizer"].step()
            losses.append(loss.detach())
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        losses = [float(x) for x in losses]
        return {f"step_{k}": losses[k] for k in (0, 10, 100) if k < steps}, ms * 100.0 / steps

    phase_b(loaded, steps=11)                    # warm-up
    line["phase_b_loss"] = {}
    line["phase_b_loss"]["loaded_map"], line["phase_b_100_steps_ms"] = phase_b(loaded)
    line["phase_b_100_steps_ms"] = round(line["phase_b_100_steps_ms"], 3)
    for mode in ("mean", "best"):
        baked, acc = U.bake_texture(mesh, targets, cams, S, mode=mode, surface=(t2f, tbary))
        line["phase_b_loss"][f"baked_{mode}"], _ = phase_b(baked)
        line[f"texels_written_{mode}"] = int((acc[..., 3] > 0).sum())
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
