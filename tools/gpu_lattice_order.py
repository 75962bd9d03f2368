"""Selected launches at 1080p through three lists of the same lattice: built by select_mask (ascending, mark / scan /
scatter), built on the device in ascending order, built on the device in the tiled order.

    [RTPBR_HIP_LIB=other build] [rocprofv3 --kernel-trace --output-format csv -d DIR -o trace --] \
        python tools/gpu_lattice_order.py cornell|bunny [--device-order tiled] [--tag NAME] [--out out] [--rounds 1] [--reps 5]

A build of the library has one device order (RT_LATTICE_ORDER, rt_select.hip): the other order is a second build, named by
$RTPBR_HIP_LIB, in a process of its own (--device-order says which one this is), and the caller alternates the two processes.
Every timed launch follows a select call of its own: in a kernel trace the select kernels (select_mark, select_lattice_build) cut
the dispatches into one segment per launch, in the order of <out>/lattice_order_<tag>_plan.json
(tools/prof_lattice_summary.py joins the two).  The event times of rtpbr_last_sample_ms are printed as well: min and median of
the trace kernels per (list, period, n), and sample(1)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracingpbr_amd import SHAPE, Config, Renderer, _capi, bunny, cornell_box      # noqa: E402
from raytracingpbr_amd.ibl import load_bunny_weights, synthetic_env      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("scene", choices=("cornell", "bunny"))
ap.add_argument("--device-order", default="tiled")
ap.add_argument("--tag", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "out"))
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
a = ap.parse_args()
W, H = a.size


def make():
    if a.scene == "cornell":
        return Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3))
    r = Renderer(bunny(aspect=W / H), Config.bunny_glass(W, H, 0, 16, frame=17))
    r.set_env(synthetic_env(3072, 1536, seed=0), 1.8, 2.2)
    r.set_shape_data(SHAPE.BUNNY, load_bunny_weights())
    return r


shipped = make()
lists = {"select_mask": (shipped, False), "device_" + a.device_order: (shipped, True)}
shipped.refresh()
shipped.sample(1)
shipped.sync()

plan, times = [], {}


def timed(label, r, select, launch):
    select()
    launch()
    trace_ms, total_ms, launches = r.last_sample_ms()      # (synchronises)
    plan.append(label)
    times.setdefault(label, []).append(trace_ms)


for rnd in range(a.rounds + 1):      # round 0 warms every shape up and is dropped
    for period in ((2, 2), (4, 4)):
        for name, (r, device) in lists.items():
            for n in (1, 4):
                for _ in range(a.reps):
                    timed(f"{name} {period[0]}x{period[1]} n={n}" if rnd else "warm-up", r,
                          lambda: r.select_lattice(period, (0, 0), device=device), lambda: r.sample_selected(n))
    for _ in range(a.reps):
        timed("sample(1)" if rnd else "warm-up", shipped, lambda: shipped.select_lattice((2, 2), (0, 0), device=True), lambda: shipped.sample(1))

os.makedirs(a.out, exist_ok=True)
json.dump(plan, open(os.path.join(a.out, f"lattice_order_{a.tag or a.scene}_plan.json"), "w"))
summary = {k: {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4), "calls": len(v)}
           for k, v in times.items() if k != "warm-up"}
print(json.dumps({"scene": a.scene, "library": _capi.HIP_LIB_PATH, "size": [W, H], "source": "rtpbr_last_sample_ms (events around the trace kernels)", "trace_ms": summary}, indent=1))
