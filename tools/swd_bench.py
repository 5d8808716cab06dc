#!/usr/bin/env python3
"""Cost of the sliced Wasserstein style term (csrc/swd.hip), in one process, medians of alternating windows
timed with events after a warm-up:

  * per tap at the bench's proportions (eight 512^2 views of the cow from bench.py's cameras, K = C directions): the
    projection, the sort (render side, with perm and count), loss + bwd, and the back-projection with V^T, each alone;
    and the style side (projection + sort of the one style image);
  * one public forward + backward of the term (losses.compute_swd_loss over the default layers, gradient to the pixels),
    which includes its own partial VGG forward and backward, with and without the coverage masks.

The figures are reported, nothing is bounded by them.  Prints one JSON line and writes it to --out.

    python tools/swd_bench.py [--reps 3] [--rounds 5] [--layers conv1_1,conv2_1,conv3_1,conv4_1,conv5_1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from silhouette_bench import _alternate, _summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="calls per timing window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per candidate")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--layers", default="conv1_1,conv2_1,conv3_1,conv4_1,conv5_1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swd_bench.json"))
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops
    from st3d.render import (AmbientLights, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings,
                             SoftPhongShader)
    if not torch.cuda.is_available():
        raise SystemExit("swd_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views
    layers = ST.check_swd_layers(args.layers)

    verts, faces, verts_uvs, faces_uvs, tex, style_image = bench.load_assets(S, dev, "cow", 1)
    mesh = U.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
    cams0 = FoVPerspectiveCameras(device=dev)
    renderer = MeshRenderer(MeshRasterizer(cams0, RasterizationSettings(image_size=S, blur_radius=0.0, faces_per_pixel=1)),
                            SoftPhongShader(device=dev, cameras=cams0, lights=AmbientLights(device=dev)))
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        renders, cov = U.render_meshes(renderer, mesh, cameras)
    vgg = U.get_vgg(seed=0)
    style_image = style_image.reshape((1,) + tuple(style_image.shape[-3:]))
    style = style_image.expand(B, -1, -1, -1)
    taps = {v: k for k, v in ST._DEFAULT_LAYERS.items()}
    tap_map = {taps[name]: name for name in layers}
    with torch.no_grad():
        fr, fs = ST.get_features(renders, vgg, tap_map), ST.get_features(style_image, vgg, tap_map)
    directions = ST.swd_draw(layers, 0, torch.Generator().manual_seed(0), dev)

    cases, shapes = {}, {}
    for name in layers:
        f, s, v = fr[name], fs[name], directions[name]
        vt = v.t().contiguous()
        w = ST.nnfm_pool_mask(cov, B, f.shape[2], f.shape[3])
        proj = ops.swd_project(f, v)
        rows, perm, count = ops.swd_sort(proj, w)
        tsorted = ops.swd_sort(ops.swd_project(s, v), None, want_perm=False)[0]
        gproj = ops.swd_bwd(rows, perm, count, tsorted)
        N = f.shape[2] * f.shape[3]
        shapes[name] = {"B": B, "C": int(f.shape[1]), "K": int(v.shape[0]), "N": N, "M": int(s.shape[2] * s.shape[3]),
                        "sort_block_and_global_passes": ops.swd_geometry(N), "active": round(float((w > 0).float().mean()), 4)}
        cases[name + "/project"] = lambda f=f, v=v: ops.swd_project(f, v)
        cases[name + "/sort"] = lambda proj=proj, w=w: ops.swd_sort(proj, w)
        cases[name + "/style_project_sort"] = lambda s=s, v=v: ops.swd_sort(ops.swd_project(s, v), None, want_perm=False)
        cases[name + "/loss_bwd"] = lambda r=rows, p=perm, c=count, t=tsorted: (ops.swd_loss(r, c, t), ops.swd_bwd(r, p, c, t))
        cases[name + "/back_project"] = lambda g=gproj, vt=vt: ops.swd_project(g, vt)

    default = tuple(n for n in ST.SWD_DEFAULT_LAYERS if n in layers) or layers
    pixels = renders.clone().requires_grad_(True)
    generator = torch.Generator().manual_seed(0)

    def term(masks):
        def run():
            pixels.grad = None
            L.compute_swd_loss(pixels, style, vgg, default, generator=generator, masks=masks).backward()
        return run
    cases["term_fwd_bwd_full"] = term(None)
    cases["term_fwd_bwd_coverage"] = term(cov)

    samples = _alternate(cases, args.reps, args.rounds, args.warmup)
    ms = {k: _summary(s) for k, s in samples.items()}
    per_tap = {name: round(sum(ms[name + "/" + part]["median_ms"] for part in
                               ("project", "sort", "style_project_sort", "loss_bwd", "back_project")), 4) for name in layers}
    line = {"reps": args.reps, "rounds": args.rounds, "size": S, "views": B, "shapes": shapes, "ms_per_call": ms,
            "kernels_per_tap_ms": per_tap, "term_layers": list(default)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
