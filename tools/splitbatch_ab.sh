#!/bin/bash
# on the GPU box: this tree against a checkout of the parent commit (PARENT=dir, library built), same box, one call.
# STAGES (default "ab modes dump loops trace") chooses among:
#   ab      bench.py with default arguments, alternating parent / tree, three runs each: $OUT/ab_<k>_<side>.json in run order.
#           SPLIT=<value> exports ST3D_SPLIT_BATCH for the tree's runs (default: the tree's own default)
#   modes   this tree under ST3D_SPLIT_BATCH = 0, 1, fwd, bwd: two runs per setting, the settings interleaved
#   dump    --dump-outputs of both at --steps 1 --warmup 0 and at --steps 3 --warmup 0 (the second and third step are clean
#           calls), compared byte for byte; the tree under SPLIT as above
#   loops   the other loops once per side, parent then tree: --background noise, --approach first_a, --target both,
#           --approach first_b --steps 500
#   trace   one rocprofv3 --kernel-trace --stats run of bench.py --steps 20 --warmup 5 per side and, for the tree, per setting
#           0 and 1: the per-kernel totals ($OUT/trace_<name>_stats.csv) and the launch gaps (tools/launch_gaps.py)
# Every GPU step has its own time limit and the script stops at the first one that fails.
cd "$(dirname "$0")/.." || exit 1
TREE=$(pwd)
PARENT=${PARENT:?PARENT=<checkout of the parent commit>}
PARENT=$(cd "$PARENT" && pwd) || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
STAGES=${STAGES:-ab modes dump loops trace}
run() {     # run <side> <name> <limit> <bench args...>: one bench.py run of that side, its JSON line kept
  local side=$1 name=$2 limit=$3; shift 3
  local dir=$TREE; [ "$side" = parent ] && dir=$PARENT
  (cd "$dir" && timeout -k 10 "$limit" python bench.py "$@") > "$OUT/${name}_$side.json" 2> "$OUT/${name}_$side.err" \
    || { echo "FAILED: $side $name (exit $?)"; tail -5 "$OUT/${name}_$side.err"; exit 1; }
}
tree_run() {    # the same for the tree under SPLIT
  if [ -n "$SPLIT" ]; then export ST3D_SPLIT_BATCH=$SPLIT; fi
  run tree "$@"
  unset ST3D_SPLIT_BATCH
}
has() { case " $STAGES " in *" $1 "*) return 0;; esac; return 1; }
if has ab; then
  for k in 1 2 3; do
    run parent ab_$k 240
    tree_run ab_$k 240
  done
fi
MODES="0 1 fwd bwd"
if has modes; then
  for k in 1 2; do
    for m in $MODES; do
      export ST3D_SPLIT_BATCH=$m; run tree mode_${m}_$k 240; unset ST3D_SPLIT_BATCH
    done
  done
fi
if has dump; then
  for steps in 1 3; do
    rm -rf "$OUT/dump_${steps}_parent" "$OUT/dump_${steps}_tree"
    run parent dump_$steps 240 --steps $steps --warmup 0 --dump-outputs "$OUT/dump_${steps}_parent"
    tree_run dump_$steps 240 --steps $steps --warmup 0 --dump-outputs "$OUT/dump_${steps}_tree"
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
trace() {   # trace <name> <dir>: kernel trace + stats of one bench run in <dir>
  local name=$1 dir=$2
  rm -rf "$OUT/trace_$name"
  (cd "$dir" && timeout -k 10 420 rocprofv3 --kernel-trace --stats -f csv -d "$OUT/trace_$name" -- python bench.py --steps 20 --warmup 5) \
    > "$OUT/trace_$name.json" 2> "$OUT/trace_$name.err" || { echo "FAILED: trace $name (exit $?)"; tail -5 "$OUT/trace_$name.err"; exit 1; }
  local t s
  t=$(find "$OUT/trace_$name" -name '*kernel_trace.csv' | head -1)
  s=$(find "$OUT/trace_$name" -name '*kernel_stats.csv' | head -1)
  cp "$s" "$OUT/trace_${name}_stats.csv"
  echo "== $name: $(tail -1 "$OUT/trace_$name.json" | python -c 'import json,sys; print(json.loads(sys.stdin.read())["median_ms_per_step"])') ms/step under the tracer"
  python tools/launch_gaps.py "$t" --rows "$OUT/trace_${name}_rows.csv" | tee "$OUT/trace_${name}_gaps.txt"
  gzip -c "$t" > "$OUT/trace_${name}_kernel_trace.csv.gz"
  rm -rf "$OUT/trace_$name"
}
if has trace; then
  trace parent "$PARENT"
  export ST3D_SPLIT_BATCH=0; trace tree_0 "$TREE"
  export ST3D_SPLIT_BATCH=1; trace tree_1 "$TREE"
  unset ST3D_SPLIT_BATCH
fi
python - "$OUT" "$STAGES" "$MODES" <<'P'
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
if "modes" in stages:
    for m in sys.argv[3].split():
        ds = [line("mode_%s_%d_tree.json" % (m, k)) for k in (1, 2)]
        print("ST3D_SPLIT_BATCH=%s" % m, [d["median_ms_per_step"] for d in ds], {(d["first_step_loss"], d["final_loss"]) for d in ds})
if "loops" in stages:
    for name in ("noise", "first_a", "both", "first_b"):
        print(name, {s: (line("%s_%s.json" % (name, s))["ms_per_step"], line("%s_%s.json" % (name, s))["final_loss"]) for s in ("parent", "tree")})
sys.exit(0 if ok else 1)
P
