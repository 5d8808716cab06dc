#!/usr/bin/env python3
"""Time of one coverage-driven view selection at the shape of BASELINE config 2: the cow, image and texture side
512, 256 candidate directions of seed 0, 8 views picked.  The whole st3d.cover.select_cameras call -- rasterising and marking
the candidates, the greedy rounds, the counts and its one host read -- between a device synchronise before and after, on a
host clock; then its three device stages (texel_masks, greedy_views, coverage_counts), each bracketed by its own pair of HIP
events.  Medians, minima and maxima over --repeats calls after --warmup.  The figures are reported, nothing is bounded by them.

Prints one JSON line and writes it to --out.

    python tools/cover_bench.py [--repeats 20]
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
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cover_bench needs a GPU (there is nothing to time without one)")
    import _scenes
    import utils as U
    from st3d import cover
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    U.device = dev
    cow = _scenes.load_asset("cow")
    S = T = args.size
    mesh = U.build_mesh(torch.from_numpy(cow["verts_uvs"].astype(np.float32))[None].to(dev),
                        torch.from_numpy(cow["faces_uvs"].astype(np.int64))[None].to(dev),
                        torch.from_numpy(_scenes.texture_at(cow, T))[None].to(dev),
                        torch.from_numpy(cow["verts"]).to(dev), torch.from_numpy(cow["faces"].astype(np.int64)).to(dev))
    cams = U.build_random_cameras(args.candidates, generator=torch.Generator().manual_seed(0))

    def stats(ms):
        return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return out, a.elapsed_time(b)

    whole, stages = [], {"texel_masks": [], "greedy_views": [], "coverage_counts": []}
    report = None
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, report = cover.select_cameras(mesh, cams, args.views, S)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        masks, m_ms = events(lambda: cover.texel_masks(mesh, cams.R, cams.T, S))
        (picks, _, _), g_ms = events(lambda: cover.greedy_views(masks, args.views))
        _, c_ms = events(lambda: cover.coverage_counts(masks[picks.long()].contiguous(), T))
        if i >= args.warmup:
            whole.append(ms)
            for k, v in (("texel_masks", m_ms), ("greedy_views", g_ms), ("coverage_counts", c_ms)):
                stages[k].append(v)
    line = {"mesh": "cow", "image_size": S, "texture_size": T, "candidates": args.candidates, "views": args.views,
            "repeats": args.repeats, "warmup": args.warmup, "select_cameras_ms": stats(whole),
            "stage_ms": {k: stats(v) for k, v in stages.items()},
            "report": {k: v for k, v in report.items() if k != "counts"}}
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
