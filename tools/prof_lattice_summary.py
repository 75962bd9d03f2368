"""Join a rocprofv3 kernel trace of tools/gpu_lattice_order.py with its plan.

    python tools/prof_lattice_summary.py <plan file> <trace dir>

The dispatches in start order are cut at every select kernel that begins a select call (select_mark*, select_lattice_build): one
segment per entry of the plan tools/gpu_lattice_order.py wrote (<out>/lattice_order_<tag>_plan.json).  Per label: min / median / max over its segments of the device
time of the trace kernels (trace_paths*, primary*) and of everything else the launch ran (accumulate).  Also the select kernels'
own times: select_lattice_build against mark + scan + scatter."""
import csv
import glob
import json
import os
import statistics
import sys

plan_file, d = sys.argv[1], sys.argv[2]
scene = os.path.basename(plan_file)[len("lattice_order_"):-len("_plan.json")]
plan = json.load(open(plan_file))
rows = []
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
segments, select = [], {}
for start, end, name in rows:
    us = (end - start) / 1e3
    if "select_" in name:
        key = name.split("(")[0].replace("rt::", "").split("<")[0].replace("void ", "")
        select.setdefault(key, []).append(us)
        if "select_mark" in name or "select_lattice_build" in name:
            segments.append({"trace": 0.0, "other": 0.0})
    elif segments:
        segments[-1]["trace" if ("trace_paths" in name or "primary" in name) else "other"] += us
# the warm-up of tools/gpu_lattice_order.py (refresh + sample(1) per context) runs before the first select: no segment
assert len(segments) == len(plan), (len(segments), len(plan))
by = {}
for label, seg in zip(plan, segments):
    if label != "warm-up":
        by.setdefault(label, []).append(seg)


def stats(v):
    return {"min_us": round(min(v), 1), "median_us": round(statistics.median(v), 1), "max_us": round(max(v), 1), "n": len(v)}


out = {"scene": scene, "source": "rocprofv3 --kernel-trace, device time per launch",
       "trace_kernels": {k: stats([s["trace"] for s in v]) for k, v in by.items()},
       "accumulate_kernels": {k: stats([s["other"] for s in v]) for k, v in by.items()},
       "select_kernels": {k: stats(v) for k, v in select.items()}}
print(json.dumps(out, indent=1))
