#!/usr/bin/env python3
"""Time of one st3d_diffuse_solve: the cow, bob (the mesh of BASELINE config 5), bob subdivided once (21 k vertices: more LDS than a kernel gets without asking), an open
213 x 192 sheet (40 896 vertices: all 160 KiB), the cow subdivided once (11.7 k vertices, the search direction
still fits LDS) and twice (47 k, it does not), lambda = 19, tol = 1e-6, right-hand side u = M verts (what verts() solves
every step) and seeded noise (what the backward sees), in each of the three homes of the vectors that applies: x, r, A p in
registers (V <= 4096), the search direction in LDS with the rest in global memory (V <= 40896), everything in global memory.  Every solve is bracketed by its own pair of HIP events; the figure is the median of --solves of them.  The figures
are reported, nothing is bounded by them.

Prints one JSON line and writes it to --out.

    python tools/diffuse_bench.py [--solves 200]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

LDS_LIMIT_VERTS = (160 * 1024 - 256) // 4
REG_LIMIT_VERTS = 4 * 1024


def subdivide(verts, faces):
    """every triangle into four through its edge midpoints"""
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    edges, inv = np.unique(e, axis=0, return_inverse=True)
    mid = len(verts) + inv.reshape(-1).reshape(3, -1).T                      # midpoint vertex of edges 01, 12, 20 of every face
    v = np.concatenate([verts, 0.5 * (verts[edges[:, 0]] + verts[edges[:, 1]])]).astype(np.float32)
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    f = np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return v, f.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lam", type=float, default=19.0)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffuse_bench needs a GPU (there is nothing to time without one)")
    from st3d import largesteps as LS
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    def fixture(name):
        d = np.load(os.path.join(ROOT, "tests", "golden", f"assets_{name}_mesh.npz"))
        return np.ascontiguousarray(d["verts"], np.float32), d["faces"].astype(np.int64)
    def sheet(nx, ny):
        y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        v = np.stack([x / (nx - 1), y / (ny - 1), 0.1 * np.sin(3.0 * x / nx) * np.cos(2.0 * y / ny)], -1).reshape(-1, 3)
        i = (y[:-1, :-1] * nx + x[:-1, :-1]).reshape(-1)
        f = np.concatenate([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)])
        return v.astype(np.float32), f.astype(np.int64)
    cow = fixture("cow")
    once = subdivide(*cow)
    line = {"solves": args.solves, "lambda": args.lam, "tol": args.tol, "meshes": {}}
    # bob subdivided once needs 86 KB of LDS (above the 64 KiB a kernel gets without asking), the 213 x 192 sheet all 160 KiB
    for name, (v, f) in (("cow", cow), ("bob", fixture("bob")), ("cow_subdivided_once", once),
                         ("bob_subdivided_once", subdivide(*fixture("bob"))), ("sheet_213x192", sheet(213, 192)),
                         ("cow_subdivided_twice", subdivide(*once))):
        assert name != "sheet_213x192" or len(v) == LDS_LIMIT_VERTS
        dv = LS.DiffusedVertices(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), args.lam, tol=args.tol)
        noise = torch.randn(v.shape, generator=torch.Generator().manual_seed(0)).to(dev)
        entry = {"verts": len(v), "max_degree": dv.max_degree, "max_iter": dv.max_iter, "ms_per_solve": {}}
        for what, b in (("M_verts", dv.params.detach()), ("noise", noise)):
            first = None
            for home in ("registers", "lds", "global"):        # where x, r, A p / the search direction live (csrc/diffuse.hip)
                if (home == "registers" and len(v) > REG_LIMIT_VERTS) or (home == "lds" and len(v) > LDS_LIMIT_VERTS):
                    continue
                os.environ["ST3D_DIFFUSE_LDS"] = "0" if home == "global" else "1"
                os.environ["ST3D_DIFFUSE_REGS"] = "1" if home == "registers" else "0"
                ms = []
                for k in range(args.warmup + args.solves):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    x, info = LS.diffuse_solve(dv.nbr_off, dv.nbr_idx, b, args.lam, args.tol, dv.max_iter)
                    t1.record()
                    t1.synchronize()
                    if k >= args.warmup:
                        ms.append(t0.elapsed_time(t1))
                got = LS.read_info(info)
                if first is None:
                    first = (x, info)
                elif not (torch.equal(first[0].view(torch.int32), x.view(torch.int32)) and torch.equal(first[1], info)):
                    raise SystemExit(f"{name} {what}: the {home} variant differs from the first one in its bits")
                entry["ms_per_solve"][f"{what}/{home}"] = {
                    "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                    "iterations": got["iterations"], "converged": got["converged"]}
        line["meshes"][name] = entry
    os.environ.pop("ST3D_DIFFUSE_LDS", None)
    os.environ.pop("ST3D_DIFFUSE_REGS", None)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
