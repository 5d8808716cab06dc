#!/usr/bin/env python3
"""Cost of the NNFM style term (csrc/nnfm.hip), in one process, medians of alternating windows:

  * the search alone at relu3_1 of eight 512^2 views (B = 8, N = M = 16 384, C = 256): the full frame, and under the coverage
    masks of the cow seen from bench.py's cameras (pooled to the tap as the term pools them);
  * the search alone at N = M = 4 096, C = 512 (relu4_1 of a 512^2 view);
  * one public forward + backward of the term (losses.compute_nnfm_loss on conv3_1, gradient to the pixels) at config 2's
    shape, with and without the coverage masks.

The search's rate is 2 N M C flop over its time, stated next to the 122 TF/s the guide measured for an untuned fp32-MFMA GEMM
-- a reference point, not a pass mark.  The figures are reported, nothing is bounded by them.

Prints one JSON line and writes it to --out.

    python tools/nnfm_bench.py [--reps 5] [--rounds 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from silhouette_bench import _alternate, _summary  # noqa: E402

GUIDE_TFLOPS = 122.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per timing window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per candidate")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnfm_bench.json"))
    args = ap.parse_args()
    import bench
    import losses as L
    import style_transfer as ST
    import utils as U
    from st3d import ops
    from st3d.render import (AmbientLights, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings,
                             SoftPhongShader)
    if not torch.cuda.is_available():
        raise SystemExit("nnfm_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = ST.device = L.device = dev
    S, B = args.size, args.views

    # config 2's scene: the cow from bench.py's cameras, its coverage, its style image
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

    def tap(images, name):
        with torch.no_grad():
            return ST.get_features(images, vgg, {taps[name]: name})[name]

    def search_case(feat, style_tap, weights):
        hat = ops.nnfm_normalise(style_tap)[0]
        normalised = ops.nnfm_normalise(feat)
        return lambda: ops.nnfm_search(feat, hat, weights, normalised=normalised)

    f3, s3 = tap(renders, "conv3_1"), tap(style_image, "conv3_1")
    w3 = ST.nnfm_pool_mask(cov, B, f3.shape[2], f3.shape[3])
    f4, s4 = tap(renders[:1], "conv4_1"), tap(style_image, "conv4_1")
    tq = ops.nnfm_geometry(f3.shape[2] * f3.shape[3], s3.shape[2] * s3.shape[3], f3.shape[1])[0]
    tiles = (w3.reshape(B, -1, tq) != 0).any(dim=2)

    pixels = renders.clone().requires_grad_(True)

    def term(masks):
        def run():
            pixels.grad = None
            L.compute_nnfm_loss(pixels, style, vgg, masks=masks).backward()
        return run

    samples = _alternate({"search_relu3_1_full": search_case(f3, s3, None), "search_relu3_1_coverage": search_case(f3, s3, w3),
                          "search_relu4_1_one_view": search_case(f4, s4, None), "term_fwd_bwd_full": term(None),
                          "term_fwd_bwd_coverage": term(cov)}, args.reps, args.rounds, args.warmup)

    def shape(f, s):
        return {"B": int(f.shape[0]), "N": int(f.shape[2] * f.shape[3]), "M": int(s.shape[2] * s.shape[3]), "C": int(f.shape[1])}

    def tflops(f, s, key, share=1.0):
        g = shape(f, s)
        flop = 2.0 * g["B"] * g["N"] * g["M"] * g["C"] * share
        return round(flop / (_summary(samples[key])["median_ms"] * 1e-3) / 1e12, 2)

    active = float(tiles.float().mean())
    line = {"reps": args.reps, "rounds": args.rounds, "size": S, "views": B, "guide_untuned_fp32_mfma_gemm_tflops": GUIDE_TFLOPS,
            "coverage": {"pixels": round(float((cov != 0).float().mean()), 4), "tap_positions": round(float((w3 != 0).float().mean()), 4),
                         "query_tiles_searched": round(active, 4)},
            "shapes": {"relu3_1": shape(f3, s3), "relu4_1_one_view": shape(f4, s4)},
            "geometry": {"relu3_1": ops.nnfm_geometry(shape(f3, s3)["N"], shape(f3, s3)["M"], shape(f3, s3)["C"]),
                         "relu4_1": ops.nnfm_geometry(shape(f4, s4)["N"], shape(f4, s4)["M"], shape(f4, s4)["C"])},
            "ms_per_call": {k: _summary(s) for k, s in samples.items()},
            "tflops": {"search_relu3_1_full": tflops(f3, s3, "search_relu3_1_full"),
                       "search_relu3_1_coverage_of_tiles_searched": tflops(f3, s3, "search_relu3_1_coverage", active),
                       "search_relu4_1_one_view": tflops(f4, s4, "search_relu4_1_one_view")}}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
