#!/usr/bin/env python3
"""Cost of the mesh regularisers per Laplacian method: one call of all four weighted terms with their gradient
(st3d_mesh_reg for 'uniform', st3d_mesh_reg_ex for 'cot' / 'cotcurv', each also with an edge target length) on the cow and on
the cow subdivided twice, in one process, medians of alternating windows.  The figures are reported, nothing
is bounded by them.

Prints one JSON line and writes it to --out.

    python tools/mesh_reg_bench.py [--reps 50] [--rounds 7]
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
    ap.add_argument("--reps", type=int, default=50, help="calls per timing window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per candidate")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_reg_bench.json"))
    args = ap.parse_args()
    import _scenes as SC
    from st3d import cli, mesh_losses as ML, ops
    if not torch.cuda.is_available():
        raise SystemExit("mesh_reg_bench needs a GPU (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cow = SC.load_asset("cow")
    v, f, uv, fuv = cow["verts"], cow["faces"], cow["verts_uvs"], cow["faces_uvs"]
    line = {"reps": args.reps, "rounds": args.rounds, "weights": [1.0, 1.0, 1.0, 1.0], "meshes": {}}
    for name, levels in (("cow", 0), ("cow_subdivided_twice", 2)):
        for _ in range(levels):
            v, f, uv, fuv = SC.subdivide(v, f, uv, fuv)
        target = torch.from_numpy(np.ascontiguousarray(v)).float().to(dev)
        faces = torch.from_numpy(f.astype(np.int64)).to(dev)
        verts = target + 0.01 * torch.randn(target.shape, generator=torch.Generator().manual_seed(0)).to(dev)
        topo, cot = ML.build_topology(faces, verts.shape[0]), ML.build_cot_topology(faces, verts.shape[0])
        t = cli.mean_edge_length(target, faces)
        w = [1.0, 1.0, 1.0, 1.0]
        fns = {"uniform": lambda: ops.mesh_reg(verts, target, topo, w)}
        for method in ("uniform", "cot", "cotcurv"):
            if method != "uniform":
                fns[method] = lambda m=method: ops.mesh_reg_ex(verts, target, topo, cot, w, m, 0.0)
            fns[method + "+edge_target"] = lambda m=method: ops.mesh_reg_ex(verts, target, topo, cot, w, m, t)
        samples = _alternate(fns, args.reps, args.rounds, args.warmup)
        line["meshes"][name] = {"verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "edges": int(topo["edges"].shape[0]),
                                "mean_edge_length": round(t, 6), "ms_per_call": {k: _summary(s) for k, s in samples.items()}}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
