#!/usr/bin/env python3
"""Measurements of the line map (plv_camera_used_lines, line_segments_kernel) -> profiles/line_map.json.

    python tools/line_map_profile.py calls --cache DIR --out calls.json
        the bench's boulevard scene (bench.py workload C: side-looking camera, points + lines) at 752 x 480 and at 1280 x 720 through
        SystemManager(line_map=True): after a warmed-up drive, on the first frame whose line update left a batch, the wall time of 200
        plv_camera_used_lines calls on prepared arguments (p50 / p99) with the lines and observations behind them
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/line_map_profile.py kernels --cache DIR --plan DIR/plan.json
    python tools/line_map_profile.py parse --plan DIR/plan.json --trace DIR --out kernels.json
        the same drive and calls under the profiler, in a run of its own: the dispatches of line_segments_kernel in the plan's order
    python tools/line_map_profile.py resources --out resources.json
        registers and scratch of line_segments_kernel from the compiler's own metadata (cross-compiles for gfx950, no GPU needed)
    python tools/line_map_profile.py bench --parent DIR --runs 5 [--cache DIR] --out bench.json
        `python bench.py --gpus 1 --steps K --warmup W` of this tree and of a built checkout of the parent commit in DIR, alternating
    python tools/line_map_profile.py merge --parts calls.json kernels.json resources.json bench.json --out profiles/line_map.json
"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

WARM_FRAMES = 75          # bench.py's prologue (60) and a warm-up: the clone window is full, the tracks have their history
EXTRA_FRAMES = 25         # ... and up to this many more until a line update leaves a batch behind
HIPCC = "/opt/rocm/bin/hipcc"


def _workloads():
    import bench
    c = dict(bench.WORKLOADS["C"])
    big = dict(c, w=1280, h=720, points=500, num_features=780)      # the same scene and mount at workload D's size and point count
    return (("752x480", c), ("1280x720", big))


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def _driven_system(wl, workers, cache=None):
    """bench.py's stream and driver with the map on: stops behind the first camera frame past WARM_FRAMES whose line update left a
    batch.  Returns (SystemManager, frames played, lines of the batch, launches of line_segments_kernel so far)."""
    import bench
    stream = bench.build_stream(wl, WARM_FRAMES + EXTRA_FRAMES, workers, cache=cache)
    system = importlib.import_module("plviwo_amd.system")
    sm = system.SystemManager(bench.load_options(wl), max_obs=24, line_map=True)
    pl = bench.Player(stream, sm, staged=False)
    launched, inner = [0], sm.ctx.camera_used_lines

    def counted(*args, **kw):      # (a call that finds a batch launches line_segments_kernel once: the profiled run's plan counts them)
        r = inner(*args, **kw)
        launched[0] += len(r["ids"]) > 0
        return r
    sm.ctx.camera_used_lines = counted
    frames = 0
    while True:
        nxt = pl.next_frame()
        if nxt is None:
            break
        pl.camera(*nxt)
        frames += 1
        if frames >= WARM_FRAMES:
            n = len(sm.ctx.camera_used_lines(sm.state.view())["ids"])
            if n > 0:
                return sm, frames, n, launched[0]
    raise SystemExit(f"no line update left a batch in frames {WARM_FRAMES} .. {frames}")


def _prepared_call(pkg, sm, n):
    """plv_camera_used_lines on arguments marshalled beforehand, as a C++ caller makes it"""
    ctx, sv = sm.ctx, sm.state.view()
    ids, acc, ok = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    lg, ep, cnt = np.zeros((n, 6)), np.zeros((n, 6)), C.c_int()
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    args = (ctx.h, C.byref(sv.c), n, C.byref(cnt), ids.ctypes.data_as(C.POINTER(C.c_uint64)), acc.ctypes.data_as(u8p), lg.ctypes.data_as(dp),
            ep.ctypes.data_as(dp), ok.ctypes.data_as(u8p))
    fn = ctx.lib.plv_camera_used_lines

    def call():
        rc = fn(*args)
        if rc != pkg.PLV_OK or cnt.value != n:
            raise SystemExit(f"plv_camera_used_lines: {rc} ({cnt.value} lines) {ctx.lib.plv_last_error()}")
    call.keep = (sv, ids, acc, ok, lg, ep)
    return call


def calls(a):
    pkg = ge.load_pkg()
    runs = []
    for name, wl in _workloads():
        sm, frames, n, _ = _driven_system(wl, a.workers, a.cache and os.path.join(a.cache, f"frames_{name}.npz"))
        call = _prepared_call(pkg, sm, n)
        for _ in range(20):
            call()
        us = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            us.append((time.perf_counter() - t0) * 1e6)
        ok = call.keep[3]
        runs.append(dict(size=name, scene=wl["scene"], frames_played=frames, lines=n, lines_with_end_points=int(ok.sum()),
                         lines_accepted=int(call.keep[2].sum()), clones=len(sm.state.clones), calls=a.calls,
                         wall_us=dict(p50=round(statistics.median(us), 1), p99=round(_pct(us, 0.99), 1), min=round(min(us), 1), max=round(max(us), 1))))
        print(runs[-1], flush=True)
        sm.close()
    out = dict(what="wall time of plv_camera_used_lines (microseconds, prepared arguments, time.perf_counter around the ctypes call) behind the "
                    f"first camera frame past {WARM_FRAMES} of bench.py's workload C stream (boulevard scene, points + lines) whose line update "
                    "left a batch, through SystemManager(line_map=True); 20 untimed calls first", runs=runs)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def kernels(a):
    """the drive and REPEAT calls per size, in the order the plan records; cached frames only (a profiled run must not fork)"""
    pkg = ge.load_pkg()
    plan = []
    for name, wl in _workloads():
        sm, frames, n, before = _driven_system(wl, 1, a.cache and os.path.join(a.cache, f"frames_{name}.npz"))
        call = _prepared_call(pkg, sm, n)
        for _ in range(a.repeat):
            call()
        plan.append(dict(size=name, lines=n, launches=a.repeat, launches_before=int(before)))      # (before: the driver's own, during the drive)
        sm.close()
    with open(a.plan, "w") as f:
        json.dump(plan, f, indent=1)


def parse(a):
    plan = json.load(open(a.plan))
    files = sorted(glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.trace}")
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "line_segments_kernel" in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    want = sum(g["launches"] + g["launches_before"] for g in plan)
    if len(rows) != want:
        raise SystemExit(f"{len(rows)} dispatches of line_segments_kernel in the trace, the plan has {want}")
    out, k = [], 0
    for g in plan:
        k += g["launches_before"]
        us = [(e - s) * 1e-3 for s, e in rows[k:k + g["launches"]]][3:]    # (the first launches of a group: cold caches)
        k += g["launches"]
        out.append(dict(g, kernel_us=dict(p50=round(statistics.median(us), 2), p99=round(_pct(us, 0.99), 2), min=round(min(us), 2), max=round(max(us), 2))))
        print(out[-1])
    with open(a.out, "w") as f:
        json.dump(dict(what="line_segments_kernel, rocprofv3 --kernel-trace --stats in a run of its own: End - Start per dispatch, microseconds, "
                            "launches 4.. of each group", groups=out), f, indent=1)


def resources(a):
    src = os.path.join(ROOT, "pl-viwo_amd", "csrc", "line_map_kernels.hip")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "line_map_kernels.s")
        # (the flags of pl-viwo_amd/Makefile)
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-result",
                        "--cuda-device-only", "-S", "-o", asm, src], check=True)
        text = open(asm).read()
    m = re.search(r"\.name:\s+(\S*line_segments_kernel\S*)\n", text)
    if not m:
        raise SystemExit("line_segments_kernel not found in the assembly's metadata")
    # the kernel's entry of amdhsa.kernels: from the list item that holds the name to the next one
    start, end = text.rfind("\n  - .", 0, m.start()), text.find("\n  - .", m.end())
    meta = dict(re.findall(r"\.(\w+):\s+(\d+)\n", text[start:end if end > 0 else len(text)]))
    out = dict(what="line_segments_kernel, the compiler's resource metadata (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off)", kernel=m.group(1),
               vgpr_count=int(meta["vgpr_count"]), sgpr_count=int(meta["sgpr_count"]), scratch_bytes=int(meta["private_segment_fixed_size"]),
               lds_bytes=int(meta["group_segment_fixed_size"]), vgpr_spills=int(meta.get("vgpr_spill_count", 0)), sgpr_spills=int(meta.get("sgpr_spill_count", 0)))
    print(out)
    if out["scratch_bytes"] != 0:
        raise SystemExit("FAILED: line_segments_kernel uses scratch memory")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def bench(a):
    """bench.py of this tree and of the parent's, alternating, the map mode off (the default): frames/s of every run"""
    trees = (("parent", os.path.abspath(a.parent)), ("this_change", ROOT))
    runs = {name: [] for name, _ in trees}
    for k in range(a.runs):
        for name, root in trees:
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
            if a.cache:      # (both trees play the same rendered stream: the first run writes it, the others load it)
                os.makedirs(a.cache, exist_ok=True)
                cmd += ["--stream-cache", os.path.join(os.path.abspath(a.cache), "bench_stream.npz")]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench.py in {root}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            runs[name].append(round(float(line["value"]), 1))
            print(k, name, line["value"], line.get("unit"), flush=True)
    out = dict(what=f"python bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}, the parent commit's tree and this one alternating in one process "
                    f"chain ({a.runs} runs each, parent first), frames/s; plv_line_map_mode off (the default)", runs=runs,
               mean={k: round(statistics.mean(v), 1) for k, v in runs.items()}, median={k: round(statistics.median(v), 1) for k, v in runs.items()},
               spread={k: [min(v), max(v)] for k, v in runs.items()})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def merge(a):
    out = dict(device="AMD Instinct MI355X (gfx950)", how="tools/line_map_profile.py: calls, kernels (under rocprofv3 --kernel-trace --stats, a run "
               "of its own) + parse, resources, bench; merged")
    for path in a.parts:
        name = os.path.splitext(os.path.basename(path))[0]
        out[name] = json.load(open(path))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("calls", "kernels", "parse", "resources", "bench", "merge"))
    ap.add_argument("--plan")
    ap.add_argument("--trace")
    ap.add_argument("--out")
    ap.add_argument("--parts", nargs="*")
    ap.add_argument("--cache", help="directory for the rendered frames: `calls` saves them, `kernels` reads them; `bench`: both trees share one stream")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--parent", help="bench: a built checkout of the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    {"calls": calls, "kernels": kernels, "parse": parse, "resources": resources, "bench": bench, "merge": merge}[a.mode](a)


if __name__ == "__main__":
    main()
