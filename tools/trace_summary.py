"""What bounds a bench tick: per env group (= HIP stream) the launch durations and the gaps between consecutive
launches, and how many of the groups' launches are in flight at a time -- from a rocprofv3 kernel trace.

  rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python bench.py --full --solver Newton --no-cpu-baseline
  python tools/trace_summary.py TRACE_DIR k_step_newton [warmup_launches_per_group=20]
  python tools/trace_summary.py TRACE_DIR k_step_queue_newton 1        (queue launches: bench.py's default cut)

A launch "starts" when its first workgroup gets a slot: with every slot of the GPU taken, the gap between two launches
of one group is the wait for a slot, not host latency (the host enqueues a group's next launch before the running one
has ended: csrc/mre_sched.cpp, launch_group)."""
import collections
import csv
import glob
import os
import sys

import numpy as np

d, kern = sys.argv[1], sys.argv[2]
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 20
f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
rows = list(csv.DictReader(open(f)))
if kern.startswith("k_step_queue"):
    # queue launches (round 5): one launch of all envs per <= 200 ticks, the large kernel's two launches beside / behind it
    q = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", "?")))
               for r in rows if r["Kernel_Name"].startswith("mre::k_step_queue"))
    t00 = q[0][0]
    print("queue launches in the trace (warm-up window first): kernel, start, duration, grid (threads)")
    for s0, e0, name, grid in q:
        print(f"  {name:40s} start {(s0 - t00) / 1e6:10.3f} ms  duration {(e0 - s0) / 1e6:9.3f} ms  grid {grid}")
    comp = [(s0, e0) for s0, e0, name, _ in q if name == "mre::" + kern][warm:]
    if comp:
        print(f"{kern}: {len(comp)} timed launch(es); span {(comp[-1][1] - comp[0][0]) / 1e6:.3f} ms; "
              f"launch ms {[round((e0 - s0) / 1e6, 3) for s0, e0 in comp]}; end -> next start us {[round((comp[i + 1][0] - comp[i][1]) / 1e3, 1) for i in range(len(comp) - 1)]}")
    others = collections.Counter(r["Kernel_Name"].split("(")[0] for r in rows if not r["Kernel_Name"].startswith("mre::k_step_queue"))
    print("  other kernels in the trace:", dict(others.most_common(8)))
    sys.exit(0)
by = collections.defaultdict(list)
for r in rows:
    if r["Kernel_Name"].startswith("mre::" + kern + "("):
        by[r["Stream_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
for k in by:
    by[k] = sorted(by[k])[warm:]
t0 = min(s for v in by.values() for s, e in v)
t1 = max(e for v in by.values() for s, e in v)
n = min(len(v) for v in by.values())
print(f"{kern}: {len(by)} streams x {n} timed launches; span {(t1 - t0) / 1e6:.1f} ms = {(t1 - t0) / 1e6 / n:.3f} ms per tick")
for st, v in sorted(by.items()):
    dur = np.array([e - s for s, e in v]) / 1e3
    gap = np.array([v[i + 1][0] - v[i][1] for i in range(len(v) - 1)]) / 1e3
    print(f"  stream {st}: launch us mean {dur.mean():.0f} p10 {np.percentile(dur, 10):.0f} p90 {np.percentile(dur, 90):.0f} | "
          f"end -> next start us mean {gap.mean():.0f} median {np.median(gap):.0f} p90 {np.percentile(gap, 90):.0f}")
ev = []
for v in by.values():
    for s, e in v:
        ev += [(s, 1), (e, -1)]
ev.sort()
cur, last, acc = 0, ev[0][0], collections.Counter()
for t, dl in ev:
    acc[cur] += t - last
    last = t
    cur += dl
tot = sum(acc.values())
print("  launches in flight (share of the span):", {k: round(v / tot, 3) for k, v in sorted(acc.items())})
others = collections.Counter(r["Kernel_Name"].split("(")[0] for r in rows if not r["Kernel_Name"].startswith("mre::" + kern + "("))
print("  other kernels in the trace:", dict(others.most_common(6)))
