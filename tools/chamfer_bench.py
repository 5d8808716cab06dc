#!/usr/bin/env python3
"""Cost of the Chamfer term: one forward + backward (sample N points from the moving cow, chamfer_distance against N target
points, gradient to the vertices) at N = 5 000 and N = 20 000, and beside it the two nearest-neighbour searches alone (the
st3d_knn1 share), in one process, medians of alternating windows.  The figures are reported, nothing is
bounded by them.

Prints one JSON line and writes it to --out.

    python tools/chamfer_bench.py [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from silhouette_bench import _alternate, _summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timing window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per candidate")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[5000, 20000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_bench.json"))
    args = ap.parse_args()
    import _scenes as SC
    from st3d import mesh_losses as ML, ops, render as R
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cow = SC.load_asset("cow")
    target_verts = torch.from_numpy(np.ascontiguousarray(cow["verts"])).float().to(dev)
    faces = torch.from_numpy(cow["faces"].astype(np.int64)).to(dev)
    verts = (target_verts * 1.02).requires_grad_(True)
    gen = torch.Generator(device=dev).manual_seed(0)
    area = ML.surface_area(R.Meshes(target_verts, faces))
    line = {"reps": args.reps, "rounds": args.rounds, "mesh": "cow", "verts": int(verts.shape[0]), "faces": int(faces.shape[0]),
            "surface_area": round(area, 6), "samples": {}}
    for n in args.samples:
        with torch.no_grad():
            target = ML.sample_points_from_meshes(R.Meshes(target_verts, faces), n, generator=gen)
            current = ML.sample_points_from_meshes(R.Meshes(verts.detach(), faces), n, generator=gen)[0].contiguous()
        value = []

        def term():
            verts.grad = None
            loss, _ = ML.chamfer_distance(ML.sample_points_from_meshes(R.Meshes(verts, faces), n, generator=gen), target)
            loss.backward()
            value[:] = [loss.detach()]

        def knn_only():
            ops.knn1(current, target[0])
            ops.knn1(target[0], current)
        samples = _alternate({"term_fwd_bwd": term, "knn1_both_directions": knn_only}, args.reps, args.rounds, args.warmup)
        tile, segments = ops.knn1_geometry(n, n)
        line["samples"][str(n)] = {"chamfer": float(value[0]), "floor_2A_over_piN": ML.chamfer_floor(area, n),
                                   "knn1_tile": tile, "knn1_segments": segments,
                                   "ms_per_call": {k: _summary(s) for k, s in samples.items()}}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
