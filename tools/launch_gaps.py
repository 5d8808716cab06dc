#!/usr/bin/env python3
"""End-to-start gaps between the kernels of a bench.py step, from one `rocprofv3 --kernel-trace -f csv` run.

    rocprofv3 --kernel-trace -f csv -d DIR -- python bench.py --steps 20 --warmup 5
    python tools/launch_gaps.py DIR/**/*_kernel_trace.csv --rows profiles/NAME.csv [--steps 10]

Adam runs once per step on the caller's queue, so the trace is cut behind every `adam_kernel` and the last --steps cuts that
have the commonest launch count are kept.  A queue runs its launches in order, so positions are counted per queue (the split
batch of csrc/plan.hip runs two more).  Per queue and position: kernel, mean duration, and the mean gap from its end to the
start of the next launch of the same queue.  Per step: its span from the first start to the last end, the time some kernel was
running (the union of the intervals), their difference (the idle time), and the sum of the durations (above the union where
launches of two queues overlap).  --rows writes the per-position rows as CSV.  (.csv.gz is read too.)
"""
import argparse
import collections
import csv
import re
import sys


def short(name):
    name = re.sub(r"^void ", "", name)
    m = re.match(r"(?:\(anonymous namespace\)::|st3d::)?([A-Za-z_0-9:]+)(<[^(]*>)?", name)
    if not m:
        return name[:60]
    base = m.group(1).split("::")[-1]
    targs = (m.group(2) or "")
    targs = targs.replace("(anonymous namespace)::", "").replace(" ", "")
    return (base + targs)[:70]


def load(path):
    import gzip
    rows = []
    with (gzip.open(path, "rt", newline="") if path.endswith(".gz") else open(path, newline="")) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], str(r["Queue_Id"])))
    rows.sort()
    return rows


def cut_steps(rows, marker):
    steps, cur = [], []
    for r in rows:
        cur.append(r)
        if marker in r[2]:
            steps.append(cur)
            cur = []
    return steps


def union_busy(step):
    busy, hi = 0, None
    for a, b, _, _ in step:             # sorted by start
        if hi is None or a >= hi:
            busy += b - a
            hi = b
        elif b > hi:
            busy += b - hi
            hi = b
    return busy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--marker", default="adam_kernel")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rows")
    a = ap.parse_args()
    steps = cut_steps(load(a.trace), a.marker)
    if len(steps) < 2:
        sys.exit("no launch matching %r in the trace" % a.marker)
    common = collections.Counter(len(s) for s in steps[1:]).most_common(1)[0][0]
    steps = [s for s in steps[1:] if len(s) == common][-a.steps:]

    def by_queue(step):             # {queue: its launches in order}, queues numbered by their first launch in the step
        qs = collections.OrderedDict()
        for r in step:
            qs.setdefault(r[3], []).append(r)
        return list(qs.values())
    sig_of = lambda step: tuple(tuple(short(r[2]) for r in q) for q in by_queue(step))
    sig = collections.Counter(sig_of(s) for s in steps).most_common(1)[0][0]
    steps = [s for s in steps if sig_of(s) == sig]
    n = len(steps)
    print("%d steps of %d launches each on %d queue(s)" % (n, common, len(sig)))
    out = []
    for qi, names in enumerate(sig):
        per = [by_queue(s)[qi] for s in steps]
        for i, name in enumerate(names):
            dur = sum(q[i][1] - q[i][0] for q in per) / n / 1e3
            gap = sum(q[i + 1][0] - q[i][1] for q in per) / n / 1e3 if i + 1 < len(names) else float("nan")
            out.append((qi, i, name, dur, gap))
    fam = collections.OrderedDict()
    for qi, i, name, dur, gap in out:
        f = fam.setdefault((qi, name.split("<")[0]), [0, 0.0, 0.0])
        f[0] += 1
        f[1] += dur
        f[2] += 0.0 if gap != gap else gap
    print("%-5s %-34s %8s %10s %12s" % ("queue", "kernel", "launches", "us/step", "gap-after us"))
    for (qi, k), (c, d, g) in fam.items():
        print("%-5d %-34s %8d %10.1f %12.1f" % (qi, k, c, d, g))
    last_end = [max(r[1] for r in s) for s in steps]
    span = sum(e - s[0][0] for e, s in zip(last_end, steps)) / n / 1e3
    busy = sum(union_busy(s) for s in steps) / n / 1e3
    total = sum(r[1] - r[0] for s in steps for r in s) / n / 1e3
    print("step span %.1f us, some kernel running %.1f us, idle inside the step %.1f us, sum of durations %.1f us" % (span, busy, span - busy, total))
    if a.rows:
        with open(a.rows, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["queue", "position", "kernel", "mean_duration_us", "mean_gap_to_next_start_on_queue_us", "steps"])
            for qi, i, name, dur, gap in out:
                w.writerow([qi, i, name, "%.2f" % dur, "" if gap != gap else "%.2f" % gap, n])


if __name__ == "__main__":
    main()
