#!/usr/bin/env python3
"""Time st3d.ops.shade_bwd (fixed point and float atomics, with and without d/d bary) at the shape of config 2 (8 views,
512^2, cow; textures 512^2 and 1024^2) and print the share of 16x16 tiles that hold a face.

    python tools/scatter_tiles_bench.py [path/to/libst3d.so]

The optional argument names another build of the library to time instead of the tree's own (the parent commit's, or a
timing probe; profiles/README.md says how the ones of profiles/uncovered_scatter_split.json were made)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]
import numpy as np
import torch

from st3d import _lib

if len(sys.argv) > 1:
    _lib.SO_PATH = os.path.abspath(sys.argv[1])
from st3d import ops
from st3d.render import look_at_view_transform

B, S = 8, 512


def timed(fn, name, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"  {name:44s} {e0.elapsed_time(e1) / reps * 1e3:8.1f} us", flush=True)


def main():
    cow = np.load(os.path.join(ROOT, "tests/golden/assets_cow_mesh.npz"))
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    elev = torch.acos(torch.rand(B, generator=g) * 2 - 1) * 180 / torch.pi - 90
    azim = torch.rand(B, generator=g) * 360 - 180
    Rt, Tt = look_at_view_transform(dist=2.10, elev=elev, azim=azim, at=((0, 0.10, 0.25),))
    verts = torch.from_numpy(cow["verts"]).to(dev)
    faces = torch.from_numpy(cow["faces"]).to(dev)
    uvs = torch.from_numpy(cow["verts_uvs"]).to(dev)
    fuv = torch.from_numpy(cow["faces_uvs"]).to(dev)
    ndc = ops.project_verts(verts, Rt.to(dev), Tt.to(dev))
    frag = ops.raster_fwd(ndc, faces, S)
    grad = torch.randn(B, 3, S, S, device=dev)
    cov = frag[0] >= 0
    tiles = cov.view(B, S // 16, 16, S // 16, 16).any(4).any(2).float().mean()
    print("lib %s coverage %.3f non-empty tiles %.3f" % (os.path.basename(_lib.SO_PATH), float(cov.float().mean()), float(tiles)))
    for T in (512, 1024):
        tex = torch.rand(T, T, 3, device=dev)
        gt = torch.zeros(T, T, 3, device=dev)
        for det in (True, False):
            ops.set_deterministic(det)
            timed(lambda: ops.shade_bwd(grad, frag, uvs, fuv, tex, grad_texture=gt), f"T={T} det={det} texture only (all launches)")
            timed(lambda: ops.shade_bwd(grad, frag, uvs, fuv, tex, grad_texture=gt, want_bary=True), f"T={T} det={det} texture + bary")


if __name__ == "__main__":
    main()
