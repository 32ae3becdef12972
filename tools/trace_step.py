#!/usr/bin/env python3
"""Timeline of ONE steady-state benchmark step from a rocprofv3 --kernel-trace CSV of bench.py: per kernel start / end /
duration in us relative to the step's first kernel and its queue; kernel count, span, start of the next step, sum of the
kernel durations, busy union and idle time inside the step.
    python tools/trace_step.py <kernel_trace.csv> [step_index_from_end]
CAUTION: tracing changes how the two chunk streams overlap (traced: chunk 1's entry kernel starts ~0.6 ms after chunk
0's; three plan orderings derived from that picture were all slower than the unordered plan when timed WITHOUT the
tracer, round 3) -- use it for per-kernel durations at the chunk batch size, not for the overlap structure."""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
back = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?")) for r in rows]
ev.sort()
# a step = from one entry kernel (stem block / stem) on a queue to the next one on the SAME queue (both queues' kernels)
ent = [i for i, e in enumerate(ev) if "stem" in e[2]]
q0 = ev[ent[0]][3]
starts = [i for i in ent if ev[i][3] == q0]
i0, i1 = starts[-back - 1], starts[-back]
seg = ev[i0:i1]
t0 = seg[0][0]
tend = max(e[1] for e in seg)
print(f"step: {len(seg)} kernels, span {(tend - t0) / 1e3:.1f} us, next step starts at {(ev[i1][0] - t0) / 1e3:.1f} us")
busy = 0; cur_end = t0; sum_dur = 0
for s, e, n, q in seg:
    sum_dur += e - s
    if e > cur_end:
        busy += e - max(s, cur_end); cur_end = e
print(f"sum of kernel durations {sum_dur / 1e3:.1f} us, union busy {busy / 1e3:.1f} us, idle inside step {(tend - t0 - busy) / 1e3:.1f} us")
for s, e, n, q in seg:
    short = n.replace("void ", "").replace("(YlConvMulti)", "").replace("(YlConvP)", "")[:44]
    print(f"{(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} {(e - s) / 1e3:7.1f}  q{q}  {short}")
