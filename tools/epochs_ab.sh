#!/bin/bash
# on the GPU box: this tree against a checkout of the parent commit (PARENT=dir, library built), same box, one call.
#   1. bench.py with default arguments, alternating parent / tree, three runs each: $OUT/ab_<k>_<side>.json in run order
#   2. --dump-outputs of both at --steps 1 --warmup 0 and at --steps 3 --warmup 2 (the first step of a run never takes the
#      skip path), compared byte for byte
#   3. the other loops once per tree: --target both, --background noise, --approach first_a, --approach first_b --steps 500
#   4. --full --layers --no-cpu-baseline of both (per-family times)
#   5. this tree with each stage switched off, two runs with and two without, alternating: ST3D_FLAT_CONV1=0 (conv1_1 in
#      full), ST3D_EPOCHS=0 (no keyed calls: every step builds and fills), ST3D_FRAG_CACHE=0 (every step rasterises)
# Every GPU step has its own time limit and the script stops at the first one that fails.
cd "$(dirname "$0")/.." || exit 1
TREE=$(pwd)
PARENT=${PARENT:?PARENT=<checkout of the parent commit>}
PARENT=$(cd "$PARENT" && pwd) || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
run() {     # run <side> <name> <limit> <bench args...>: one bench.py run of that side, its JSON line kept
  local side=$1 name=$2 limit=$3; shift 3
  local dir=$TREE; [ "$side" = parent ] && dir=$PARENT
  (cd "$dir" && timeout -k 10 "$limit" python bench.py "$@") > "$OUT/${name}_$side.json" 2> "$OUT/${name}_$side.err" \
    || { echo "FAILED: $side $name (exit $?)"; tail -5 "$OUT/${name}_$side.err"; exit 1; }
}
for k in 1 2 3; do
  for side in parent tree; do run $side ab_$k 240; done
done
for spec in "1 0" "3 2"; do
  set -- $spec
  for side in parent tree; do
    rm -rf "$OUT/dump_$1_$side"
    run $side dump_$1 240 --steps $1 --warmup $2 --dump-outputs "$OUT/dump_$1_$side"
  done
  for f in "$OUT/dump_$1_parent"/*.npy; do
    cmp "$f" "$OUT/dump_$1_tree/$(basename "$f")" || { echo "DIFFERENT: $f"; exit 1; }
  done
  echo "dump --steps $1 --warmup $2: $(ls "$OUT/dump_$1_parent" | wc -l) arrays byte-identical"
  rm -rf "$OUT/dump_$1_parent" "$OUT/dump_$1_tree"
done
for side in parent tree; do
  run $side both 300 --target both
  run $side noise 300 --background noise
  run $side first_a 300 --approach first_a
  run $side first_b 300 --approach first_b --steps 500
done
if [ -z "$NO_FULL" ]; then
  for side in parent tree; do run $side full 600 --full --layers --no-cpu-baseline; done
fi
for sw in ST3D_FLAT_CONV1 ST3D_EPOCHS ST3D_FRAG_CACHE; do
  for k in 1 2; do
    export $sw=0; run tree sw_${sw}_off_$k 240; unset $sw
    run tree sw_${sw}_on_$k 240
  done
done
python - "$OUT" <<'P'
import json, sys, os
out = sys.argv[1]
def line(name):
    with open(os.path.join(out, name)) as f:
        return json.loads(f.read().strip().splitlines()[-1])
ab = {s: [line("ab_%d_%s.json" % (k, s)) for k in (1, 2, 3)] for s in ("parent", "tree")}
for s in ab:
    print(s, "ms/step", [d["ms_per_step"] for d in ab[s]], "first/final loss", {(d["first_step_loss"], d["final_loss"]) for d in ab[s]})
p, t = [d["ms_per_step"] for d in ab["parent"]], [d["ms_per_step"] for d in ab["tree"]]
spread = max(p) - min(p)
print("parent fastest %.3f, spread %.3f; tree slowest %.3f; gap %.3f = %.1f spreads" % (min(p), spread, max(t), min(p) - max(t), (min(p) - max(t)) / max(spread, 1e-9)))
losses = {(d["first_step_loss"], d["final_loss"]) for s in ab for d in ab[s]}
print("losses identical in all six lines:", len(losses) == 1)
for name in ("both", "noise", "first_a", "first_b"):
    print(name, {s: line("%s_%s.json" % (name, s))["ms_per_step"] for s in ("parent", "tree")})
for sw in ("ST3D_FLAT_CONV1", "ST3D_EPOCHS", "ST3D_FRAG_CACHE"):
    print(sw, {w: [line("sw_%s_%s_%d_tree.json" % (sw, w, k))["ms_per_step"] for k in (1, 2)] for w in ("off", "on")})
sys.exit(0 if len(losses) == 1 else 1)
P
