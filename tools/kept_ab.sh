#!/bin/bash
# on the GPU box: this tree against a checkout of the parent commit (PARENT=dir, library built), same box, one call.
# STAGES (default "ab dump loops full levels shallow") chooses among:
#   ab      bench.py with default arguments, alternating parent / tree, three runs each: $OUT/ab_<k>_<side>.json in run order
#   dump    --dump-outputs of both at --steps 1 --warmup 0 and at --steps 3 --warmup 0 (the second and third step take the kept
#           path), compared byte for byte
#   loops   the other loops once per side, parent then tree: --background noise, --approach first_a, --target both,
#           --approach first_b --steps 500
#   full    --full --layers --no-cpu-baseline of both (per-launch HIP-event times)
#   levels  this tree under ST3D_KEEP_DEPTH = 0 .. 3 and, at full depth, ST3D_KEEP_TILE = 32 and 64 against the default strips:
#           two runs per setting, the settings interleaved
#   shallow this tree under ST3D_KEEP_SHALLOW = 0,0,0 / 32,0,0 / 0,16,0 / 0,0,32 / 32,16,0 / 64,16,0 and the default 32,16,32
#           (conv1_2, conv2_1, conv2_2 on their kept lists in clean calls), likewise
# Every GPU step has its own time limit and the script stops at the first one that fails.
cd "$(dirname "$0")/.." || exit 1
TREE=$(pwd)
PARENT=${PARENT:?PARENT=<checkout of the parent commit>}
PARENT=$(cd "$PARENT" && pwd) || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
STAGES=${STAGES:-ab dump loops full levels shallow}
run() {     # run <side> <name> <limit> <bench args...>: one bench.py run of that side, its JSON line kept
  local side=$1 name=$2 limit=$3; shift 3
  local dir=$TREE; [ "$side" = parent ] && dir=$PARENT
  (cd "$dir" && timeout -k 10 "$limit" python bench.py "$@") > "$OUT/${name}_$side.json" 2> "$OUT/${name}_$side.err" \
    || { echo "FAILED: $side $name (exit $?)"; tail -5 "$OUT/${name}_$side.err"; exit 1; }
}
has() { case " $STAGES " in *" $1 "*) return 0;; esac; return 1; }
if has ab; then
  for k in 1 2 3; do
    for side in parent tree; do run $side ab_$k 240; done
  done
fi
if has dump; then
  for steps in 1 3; do
    for side in parent tree; do
      rm -rf "$OUT/dump_${steps}_$side"
      run $side dump_$steps 240 --steps $steps --warmup 0 --dump-outputs "$OUT/dump_${steps}_$side"
    done
    for f in "$OUT/dump_${steps}_parent"/*.npy; do
      cmp "$f" "$OUT/dump_${steps}_tree/$(basename "$f")" || { echo "DIFFERENT: $f"; exit 1; }
    done
    echo "dump --steps $steps --warmup 0: $(ls "$OUT/dump_${steps}_parent" | tr '\n' ' ')byte-identical"
    rm -rf "$OUT/dump_${steps}_parent" "$OUT/dump_${steps}_tree"
  done
fi
if has loops; then
  for side in parent tree; do run $side noise 300 --background noise; done
  for side in parent tree; do run $side first_a 300 --approach first_a; done
  for side in parent tree; do run $side both 300 --target both; done
  for side in parent tree; do run $side first_b 300 --approach first_b --steps 500; done
fi
if has full; then
  for side in parent tree; do run $side full 600 --full --layers --no-cpu-baseline; done
fi
if has levels; then
  for k in 1 2; do
    for d in 0 1 2 3; do
      export ST3D_KEEP_DEPTH=$d; run tree depth_${d}_$k 240; unset ST3D_KEEP_DEPTH
    done
    for t in 32 64; do
      export ST3D_KEEP_TILE=$t; run tree tile_${t}_$k 240; unset ST3D_KEEP_TILE
    done
  done
fi
SHALLOW="0,0,0 32,0,0 0,16,0 0,0,32 32,16,32 32,16,0 64,16,0"
if has shallow; then
  for k in 1 2; do
    for sh in $SHALLOW; do
      export ST3D_KEEP_SHALLOW=$sh; run tree shallow_${sh}_$k 240; unset ST3D_KEEP_SHALLOW
    done
  done
fi
python - "$OUT" "$STAGES" "$SHALLOW" <<'P'
import json, sys, os
out, stages = sys.argv[1], sys.argv[2].split()
def line(name):
    with open(os.path.join(out, name)) as f:
        return json.loads(f.read().strip().splitlines()[-1])
ok = True
if "ab" in stages:
    ab = {s: [line("ab_%d_%s.json" % (k, s)) for k in (1, 2, 3)] for s in ("parent", "tree")}
    for s in ab:
        print(s, "ms/step", [d["ms_per_step"] for d in ab[s]], "median", [d["median_ms_per_step"] for d in ab[s]],
              "first/final loss", {(d["first_step_loss"], d["final_loss"]) for d in ab[s]})
    p, t = [d["median_ms_per_step"] for d in ab["parent"]], [d["median_ms_per_step"] for d in ab["tree"]]
    spread = max(p) - min(p)
    print("median ms/step: parent fastest %.3f, spread %.3f; tree slowest %.3f; gap %.3f = %.1f spreads" %
          (min(p), spread, max(t), min(p) - max(t), (min(p) - max(t)) / max(spread, 1e-9)))
    losses = {(d["first_step_loss"], d["final_loss"]) for s in ab for d in ab[s]}
    print("losses identical in all six lines:", len(losses) == 1)
    ok = len(losses) == 1
if "loops" in stages:
    for name in ("noise", "first_a", "both", "first_b"):
        print(name, {s: (line("%s_%s.json" % (name, s))["ms_per_step"], line("%s_%s.json" % (name, s))["final_loss"]) for s in ("parent", "tree")})
if "levels" in stages:
    for d in (0, 1, 2, 3):
        print("ST3D_KEEP_DEPTH=%d" % d, [line("depth_%d_%d_tree.json" % (d, k))["median_ms_per_step"] for k in (1, 2)])
    for t in (32, 64):
        print("ST3D_KEEP_TILE=%d" % t, [line("tile_%d_%d_tree.json" % (t, k))["median_ms_per_step"] for k in (1, 2)])
if "shallow" in stages:
    for sh in sys.argv[3].split():
        print("ST3D_KEEP_SHALLOW=%s" % sh, [line("shallow_%s_%d_tree.json" % (sh, k))["median_ms_per_step"] for k in (1, 2)])
sys.exit(0 if ok else 1)
P
