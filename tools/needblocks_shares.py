#!/usr/bin/env python3
"""Need mask per block, the size of the problem (the shares table of DESIGN.md section 6): on the bench's views (cow, 512^2,
the 8 seed-0 cameras, rendered by the CPU oracle) the listed share of tiles of every input-gradient launch conv1_2 ..
conv3_3 under the tile-granular rule (tests/_needref.py, two lists) and the per-block rule (tests/_needblocks_ref.py) in
either geometry and per strip (tests/_needstrips_ref.py: 4 x 16 pixels, four to a step, every image padded to whole steps),
the share of needed blocks, the rounds a persistent workgroup walks (listed tiles / slots, slots = CUs /
cout tiles), and the share of 64-pixel runs of the relu2_1 Gram backward.

    python tools/needblocks_shares.py [--cus 256]            # no GPU; about a minute"""
import argparse
import math
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]
import numpy as np
import _needblocks_ref as NB
import _needref as NR
import _needstrips_ref as NS
import _scenes as SC
from oracle import render_ref as RR

ap = argparse.ArgumentParser()
ap.add_argument("--cus", type=int, default=256)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--views", type=int, default=8)
args = ap.parse_args()
S, B = args.size, args.views
a = SC.load_asset("cow")
R, T = SC.random_cameras(B, seed=0)
_, masks, _ = RR.render_views(a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], SC.texture_at(a, S), R, T, S, 4)
mask = (np.asarray(masks).reshape(B, S, S) > 0).astype(np.uint8)
print(f"coverage {mask.mean():.3f}")
_, old = NR.need_model(mask, 3)
m64 = NB.need_blocks_model(mask, tile_cols=[64] * 6)
m32 = NB.need_blocks_model(mask, tile_cols=[32] * 6)
CIN = (64, 64, 128, 128, 256, 256)          # channels the input gradient of list k produces: cout tiles of 64
print("launch   map   tiles  slots | tile-granular | per block 4x64 (rounds) | per block 8x32 (rounds) | strips 4x16, 4 per step: steps (rounds) | needed blocks")
for k, name in enumerate(NB.LIST_NAMES):
    Rk = S >> NB.LIST_SHIFT[k]
    tiles = B * Rk * Rk // 256
    slots = args.cus // (CIN[k] // 64)
    full = math.ceil(tiles / slots)
    o = f"{len(old[k]) / tiles:.3f}" if k < len(old) else "  -  "
    r = lambda n: f"{n / tiles:.3f} ({math.ceil(n / slots)} of {full})"
    blocks = NR.tiles_any(m64["need"][k], 4, 4).mean()
    steps = NS.strip_list(m64["need"][k])[1]         # a step is 16 blocks, like a tile
    print(f"{name}  {Rk:4d}  {tiles:5d}  {slots:4d}  |     {o}     |   {r(len(m64['lists'][k]))}    |   {r(len(m32['lists'][k]))}    |"
          f"   {steps:5d} steps {r(steps)}    | {blocks:.3f}")
runs = B * (S // 2) * (S // 2) // 64
print(f"relu2_1 Gram backward: {len(m64['gram'])} of {runs} 64-pixel runs = {len(m64['gram']) / runs:.3f}")
