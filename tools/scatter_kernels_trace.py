#!/usr/bin/env python3
"""Calls the K = 1 gradient scatters that sum through csrc/tilebins.h -- plain, supersampled (a = 2), mip-mapped, per-vertex
colours, lit (ambient) -- at the bench's shape (cow, 512^2, 8 views), in fixed point and with float atomics, REPS times
each.  It times nothing itself: run it under a kernel trace and read the rows of the shade_*_bwd kernels,

    rocprofv3 --kernel-trace --stats -d OUT -o k --output-format csv -- python tools/scatter_kernels_trace.py

from the root of the tree whose library is to be timed (a copy of this file there serves an older commit: it uses only
st3d.ops calls).  REPS=300 ONLY_PLAIN=1: the benchmark's kernel (st3d_shade_bwd_det) alone."""
import os
import sys

import numpy as np

ROOT = os.getcwd()
sys.path[:0] = [ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]
import torch  # noqa: E402

REPS, WARM = int(os.environ.get("REPS", "30")), 3
ONLY_PLAIN = os.environ.get("ONLY_PLAIN", "0") == "1"


class Lit:
    def __init__(self, dev, B, faces_i32):
        block = np.zeros((1, 24), np.float32)
        block[0, 0:3] = 0.5
        block[0, 12:15] = 1.0
        self.block, self.kind, self.weight_bound = torch.from_numpy(block).to(dev), 0, 0.5
        self.verts = self.normals = None
        self.faces_i32 = faces_i32
        self.R = torch.eye(3, device=dev).repeat(B, 1, 1).contiguous()
        self.T = torch.zeros((B, 3), device=dev)


def main():
    import bench
    import utils as U
    from st3d import cli, ops, render as R
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    S, B = 512, 8
    verts, faces, verts_uvs, faces_uvs, tex, _ = bench.load_assets(S, dev, "cow", 1)
    colours = cli.vertex_colors_from_map(verts.shape[0], faces, verts_uvs[0], faces_uvs[0], tex[0]).contiguous()
    cameras = U.build_random_cameras(B, generator=torch.Generator().manual_seed(0))
    Rm, Tm = R.join_cameras(cameras)
    f32, fuv32 = faces.to(torch.int32).contiguous(), faces_uvs[0].to(torch.int32).contiguous()
    uvs, tmap = verts_uvs[0].contiguous(), tex[0].contiguous()
    T = tmap.shape[0]
    frag = ops.raster_fwd(ops.project_verts(verts, Rm.to(dev), Tm.to(dev)), f32, S)
    gen = torch.Generator().manual_seed(1)
    g = torch.randn((B, 3, S, S), generator=gen).to(dev)
    g2 = torch.randn((B, 3, S // 2, S // 2), generator=gen).to(dev)
    L = 4
    pyr = ops.mip_build(tmap, L)
    lod = (torch.rand((B, S, S), generator=gen) * (L - 1)).to(dev)
    lit = Lit(dev, B, f32)
    gtex, gcol = torch.zeros_like(tmap), torch.zeros_like(colours)

    def calls():
        ops.shade_bwd(g, frag, uvs, fuv32, tmap, grad_texture=gtex)
        if ONLY_PLAIN:
            return
        ops.shade_ss_bwd(g2, frag, uvs, fuv32, tmap, 2, grad_texture=gtex)
        ops.shade_mip_bwd(g, frag, uvs, fuv32, pyr, lod, T, L, grad_texture=gtex)
        ops.shade_vc_bwd(g, frag, f32, colours, grad_colours=gcol)
        ops.shade_lit_bwd(g, frag, uvs, fuv32, tmap, lit, want_texture=True, want_geometry=False)

    was = ops.is_deterministic()
    for det in ((True,) if ONLY_PLAIN else (True, False)):
        ops.set_deterministic(det)
        for _ in range(WARM + REPS):
            calls()
        torch.cuda.synchronize()
    ops.set_deterministic(was)
    print("touched kernels: T=%d covered %.3f" % (T, float((frag[0] >= 0).float().mean())))


if __name__ == "__main__":
    main()
