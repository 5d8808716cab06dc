"""Record the bits of the K = 1 shading variants on the scatter scene: tests/golden/scatter_variants_parent.npz.

A change that moves the shading arithmetic or the per-tile scatter table around (csrc/shadek1.h, csrc/tilebins.h) must
leave every result bit alone.  tests/_scatter_scene.py::variants is the one definition of the cases -- the forward
kernels, the supersampled, lit, mip-mapped, per-vertex-colour and soft (K = 1) backward in fixed point, all on the S = 40
scene -- and this tool runs it on the commit whose behaviour is to be kept: copy that commit's tree somewhere, add this
file and the tests/_scatter_scene.py of the new tree to the copy (nothing else), build, and run the copy's tool there.
It uses only st3d.ops calls, so it runs on any commit that has the variants.  tests/test_gpu_scatter_tiles.py replays
the cases against the file.

Every case runs twice and the two runs must agree bit for bit (fixed-point sums are order-free); the tool exits non-zero
where they do not and writes nothing.

Per output the file holds `<name>.nnz` (the number of non-zero 32-bit patterns) and `<name>.sha256` (of the array's bytes).
Stored the way the plain case's fixture stores its values (scatter_tiles_parent.npz: indices and bit patterns of what
differs from the fill, compressed) the 25 outputs are 119 686 values and 587 KB, two and a half times that fixture: the
mantissas do not compress.  A digest pins every bit of an output in 32 bytes; a mismatch names the output, and the
values to compare come from running this tool on both commits.

    python tools/record_scatter_parent.py [--out tests/golden/scatter_variants_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "2d-to-3d-style-transfer_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scatter_variants_parent.npz"))
    a = ap.parse_args()
    import torch
    import _scatter_scene as sc
    from st3d import ops
    dev = torch.device("cuda:0")
    first, second = sc.variants(ops, dev), sc.variants(ops, dev)
    bad = sorted(k for k in first if not np.array_equal(first[k].view(np.uint32), second[k].view(np.uint32)))
    if bad:
        print("NOT REPRODUCED: " + ", ".join(bad))
        return 1
    doc, total = {}, 0
    for name, arr in first.items():
        nnz, sha = sc.digest(arr)
        assert nnz > 0 and np.isfinite(arr).all(), name
        doc[name + ".nnz"], doc[name + ".sha256"] = nnz, sha
        total += int(nnz)
        print("%-28s %-18s %6d non-zero  %s" % (name, arr.shape, nnz, sha.tobytes().hex()[:16]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **doc)
    print("wrote %s (%d outputs, %d non-zero values, %d bytes)" % (a.out, len(first), total, os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
