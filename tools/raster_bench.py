#!/usr/bin/env python3
"""Time st3d.ops.raster_fwd with faces in parallel per tile (the default) against the per-pixel walk (ST3D_RASTER_WALK=1,
read on every call) in one process, in alternating windows, and check that the two return the same bits.

    python tools/raster_bench.py [--reps 50] [--rounds 7] [--out profiles/rastertiles_ab.json] [--lib path/to/libst3d.so]

--lib names another build of the library to time instead of the tree's own (a timing probe).

Scenes: the bench's views (cow, 8 views at 512^2, seed-0 cameras), the densest of them alone (fewest covered pixels: the
same faces on the fewest tiles), the mesh pushed off screen (no tile lists a face: the sweep and the -1 rows alone) and
`large_faces` (tools/vcolor_bench.py: two triangles fill every image, sixteen items per face and tile)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]
import numpy as np
import torch

from st3d import _lib

if "--lib" in sys.argv:
    _lib.SO_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from st3d import ops
import utils as U


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="calls per timing window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per variant")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libst3d.so (set before the library loads)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    U.device = dev
    S, B = args.size, args.views
    cow = np.load(os.path.join(ROOT, "tests/golden/assets_cow_mesh.npz"))
    verts = torch.from_numpy(cow["verts"]).to(dev)
    faces = torch.from_numpy(cow["faces"].astype(np.int32)).to(dev)
    cams = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    ndc = ops.project_verts(verts, cams.R.to(dev), cams.T.to(dev))
    os.environ.pop("ST3D_RASTER_WALK", None)
    covered = (ops.raster_fwd(ndc, faces, S)[0] >= 0).float().mean((1, 2))
    dense = int(covered.argmin())
    off = ndc.clone()
    off[:, :, 0] += 5.0
    qv = torch.tensor([[-4.0, -4, 0], [5, -4, 0], [5, 4, 0], [-4, 4, 0]], device=dev)
    qf = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)
    qR = torch.eye(3, device=dev).expand(B, 3, 3).contiguous()
    qT = torch.tensor([[0.0, 0, 3]], device=dev).expand(B, 3).contiguous()
    scenes = {
        "bench_views": (ndc, faces),
        "densest_view_%d" % dense: (ndc[dense:dense + 1].contiguous(), faces),
        "off_screen": (off, faces),
        "large_faces": (ops.project_verts(qv, qR, qT), qf),
    }

    def variant(walk, n, f):
        def run():
            if walk:
                os.environ["ST3D_RASTER_WALK"] = "1"
            else:
                os.environ.pop("ST3D_RASTER_WALK", None)
            return ops.raster_fwd(n, f, S)
        return run

    line = {"shape": {"mesh": "cow", "size": S, "views": B, "faces": int(faces.shape[0])}, "reps": args.reps, "rounds": args.rounds,
            "covered_share_per_view": [round(float(c), 4) for c in covered]}
    for name, (n, f) in scenes.items():
        fns = {"faces_us": variant(False, n, f), "walk_us": variant(True, n, f)}
        outs = {k: fn() for k, fn in fns.items()}
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["faces_us"], outs["walk_us"]))
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                samples[k].append(window(fn, args.reps))
        line[name] = {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                      for k, v in samples.items()}
        line[name]["same_bits"] = same
        line[name]["walk_over_faces"] = round(statistics.median(samples["walk_us"]) / statistics.median(samples["faces_us"]), 3)
        print(name, json.dumps(line[name]), flush=True)
    os.environ.pop("ST3D_RASTER_WALK", None)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
