#!/usr/bin/env python3
"""What supersampling buys, on the CPU oracle (the table of DESIGN.md section 7): cow, 8 seeded random views, render side S,
texture side T = S and T = 2S.  A texel counts as touched at factor a when the oracle's shade_bwd of an all-ones gradient
over the fragments at side a * S leaves it non-zero in some view.  The figure is the share of the texels an a = 8 render
touches that an a = 1..4 render leaves untouched.  Reads tests/golden only.

    python tools/supersample_shares.py [--sizes 128 256] [--write]      # no GPU; --write replaces the table in DESIGN.md"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import _scenes as SC  # noqa: E402
from oracle import render_ref as RR  # noqa: E402

BEGIN, END = "<!-- supersample_shares:begin -->", "<!-- supersample_shares:end -->"


def touched(mesh, R, T, side, tex_side, threads):
    tex = np.full((tex_side, tex_side, 3), 0.5, np.float32)
    acc = np.zeros((tex_side, tex_side, 3), np.float64)
    ones = np.ones((3, side, side), np.float32)
    covered = 0
    for b in range(R.shape[0]):
        frag = RR.rasterize(RR.project_verts(mesh["verts"], R[b], T[b]), mesh["faces"], side, 0.0, threads)
        covered += int((frag[0] >= 0).sum())
        RR.shade_bwd(ones, frag, mesh["verts_uvs"], mesh["faces_uvs"], tex, acc)
    return (acc != 0).any(-1), covered / (R.shape[0] * side * side)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--write", action="store_true", help="replace the marked table in DESIGN.md")
    args = ap.parse_args()
    mesh = SC.load_asset("cow")
    R, T = SC.random_cameras(args.views, args.seed)
    cols = [(S, k) for k in (1, 2) for S in args.sizes]
    table = {a: [] for a in (1, 2, 3, 4)}
    cover = []
    for S, k in cols:
        ref, _ = touched(mesh, R, T, 8 * S, k * S, args.threads)
        for a in table:
            hit, cov = touched(mesh, R, T, a * S, k * S, args.threads)
            if a == 1:
                cover.append(cov)
            table[a].append(float((ref & ~hit).sum()) / float(ref.sum()))
            print(f"S={S} T={k * S} a={a}: {100 * table[a][-1]:.1f} % of the {int(ref.sum())} texels an a = 8 render touches stay "
                  f"untouched (coverage {100 * cov:.0f} % of the pixels)", flush=True)
    lines = ["| a | " + " | ".join(f"S = {S}, T = {k * S}" for S, k in cols) + " |", "|---|" + "---|" * len(cols)]
    lines += [f"| {a} | " + " | ".join(f"{100 * v:.1f} %" for v in table[a]) + " |" for a in table]
    lines.append("")
    lines.append(f"(cow, {args.views} views of `random_cameras({args.views}, {args.seed})`, coverage " +
                 ", ".join(f"{100 * c:.0f} %" for c in cover[:len(args.sizes)]) + " of the pixels; `tools/supersample_shares.py`)")
    block = "\n".join(lines)
    print(block)
    if args.write:
        path = os.path.join(ROOT, "DESIGN.md")
        text = open(path).read()
        if BEGIN not in text or END not in text:
            raise SystemExit(f"DESIGN.md holds no {BEGIN} ... {END} block")
        text = re.sub(re.escape(BEGIN) + r".*?" + re.escape(END), lambda m: BEGIN + "\n" + block + "\n" + END, text, flags=re.S)
        open(path, "w").write(text)


if __name__ == "__main__":
    main()
