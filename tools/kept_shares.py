#!/usr/bin/env python3
"""Kept lists, the size of the problem (the shares table of DESIGN.md section 6, "Fixed views: forward convs over the tiles the
mesh can change"): on the bench's views (cow, 512^2, the 8 seed-0 cameras, rendered by the CPU oracle) the share of 4x4
output blocks of every forward launch conv1_2 .. conv3_3 that the coverage can change (tests/_keptref.py), the share of 4 x 64
and 8 x 32 tiles and of 4 x 16 strips (four to a step, every image padded to whole steps) that hold one, and the rounds a
persistent workgroup walks (listed tiles or steps / slots, slots = CUs / cout tiles).

    python tools/kept_shares.py [--cus 256]            # no GPU; about a minute"""
import argparse
import math
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]
import numpy as np
import _keptref as KR
import _needref as NR
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
cover = (np.asarray(masks).reshape(B, S, S) > 0).astype(np.uint8)
print(f"coverage {cover.mean():.3f}")
COUT = (64, 128, 128, 256, 256, 256)        # channels the forward of list k produces: cout tiles of 64
m64 = KR.kept_model(cover, tile_cols=[64] * 6)
m32 = KR.kept_model(cover, tile_cols=[32] * 6)
m16 = KR.kept_model(cover, tile_cols=[16] * 6)
print("forward launch   map   tiles  slots | may-change blocks | 4x64 tiles (rounds of) | 8x32 tiles (rounds) | strips 4x16, 4 per step: steps (rounds)")
for k, name in enumerate(KR.LIST_NAMES):
    Rk = S >> KR.LIST_SHIFT[k]
    tiles = B * (Rk // 4) * (Rk // 64)
    slots = args.cus // (COUT[k] // 64)
    rounds = lambda n: math.ceil(n / slots)
    blocks = NR.tiles_any(m64["K"][k], 4, 4).mean()
    c64, c32, c16 = m64["counts"][k], m32["counts"][k], m16["counts"][k]
    print(f"{name + (' (+pool)' if KR.LIST_POOLS[k] else ''):16s} {Rk:4d} {tiles:6d} {slots:5d} | {blocks:17.3f} | "
          f"{c64 / tiles:.3f} ({rounds(c64)} of {rounds(tiles)}) | {c32 / tiles:.3f} ({rounds(c32)}) | {c16 / tiles:.3f} ({rounds(c16)})")
