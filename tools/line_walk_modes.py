#!/usr/bin/env python3
"""Times plv_detect_lines in the three modes of plv_line_walk_mode, in one process, alternating frame by frame, on frames of the
bench's scenes at workloads C (752 x 480, "boulevard") and D (1280 x 720, "avenue"), and writes profiles/line_walk_modes.json:
p50 / p99 per mode (the call from its start to its return: post to done), the components walked and the largest of them, and — from a
second run of the same frames as a child process under `rocprofv3 --kernel-trace --stats` — the line kernels' average durations.
Hardware counters are not collected here: they take a run of their own (tools/profile_round.sh).

    python tools/line_walk_modes.py                 # both workloads, timing + kernel statistics
    python tools/line_walk_modes.py --no-rocprof    # timing only
"""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (bench.py's WORKLOADS: size, camera rate, scene and mount)
WORKLOADS = {"C": dict(w=752, h=480, hz=15, scene="boulevard", mount=(16.0, 90.0)),
             "D": dict(w=1280, h=720, hz=20, scene="avenue", mount=(12.0, 0.0))}
MODES = (0, 1, 2)
KERNELS = ("canny_kernel", "ccl_boundary_kernel", "ccl_roots_kernel", "fld_components_kernel", "ccl_bbox_kernel", "fld_walk_components_kernel",
           "fld_chain_order_kernel", "fld_fit_wave_kernel", "fld_walk_kernel", "fld_fit_kernel")


def render(wl, n_frames):
    """frames of the drive (forks nothing with one worker; still called before the GPU is touched)"""
    import synth_dataset as sd
    sd.set_camera(wl["w"], wl["h"])
    sd.set_mount(*wl["mount"])
    try:
        sim = sd.simulate(seconds=(n_frames + 4) / wl["hz"] + 0.2, cam_hz=wl["hz"], style=wl["scene"])
        return sd.render_frames(sim["cam_times"][3:3 + n_frames], wl["scene"], 1)
    finally:
        sd.set_mount()


def run_workload(pkg, name, imgs, reps, mode1_reps):
    wl = WORKLOADS[name]
    ctx = pkg.Context(pkg.default_config(wl["w"], wl["h"]))
    times = {m: [] for m in MODES}
    info, n_lines = {}, {}
    try:
        for m in MODES:  # warm-up: buffers, threads, code objects
            ctx.line_walk_mode(m)
            ctx.feed_image(imgs[0])
            ctx.detect_lines(0)
        for rep in range(reps):
            for img in imgs:
                ctx.feed_image(img)
                ctx.synchronize()
                for m in MODES:
                    if m == 1 and rep >= mode1_reps:   # (tens of milliseconds per call: fewer samples are enough)
                        continue
                    ctx.line_walk_mode(m)
                    t0 = time.perf_counter()
                    if m == 0:   # the detection a frame uses: launched ahead, labelled and split by components over the library's threads
                        ctx.line_detect_launch(0)
                    lines = ctx.detect_lines(0)
                    times[m].append((time.perf_counter() - t0) * 1e6)
                    n_lines.setdefault(m, []).append(len(lines))
                    if m == 2:
                        i = ctx.line_walk_info()
                        for k, v in i.items():
                            info.setdefault(k, []).append(v)
    finally:
        ctx.line_walk_mode(0)
        ctx.close()
    out = dict(width=wl["w"], height=wl["h"], scene=wl["scene"], frames=len(imgs))
    for m in MODES:
        t = np.array(times[m])
        out[f"mode{m}"] = dict(calls=int(t.size), p50_us=float(np.percentile(t, 50)), p99_us=float(np.percentile(t, 99)), mean_us=float(t.mean()),
                               lines_mean=float(np.mean(n_lines[m])))
    out["same_line_counts"] = bool(n_lines[2] == n_lines[0] and n_lines[1] == n_lines[0][:len(n_lines[1])])
    out["n_components"] = dict(mean=float(np.mean(info["n_components"])), max=int(np.max(info["n_components"])))
    out["longest_component"] = dict(mean=float(np.mean(info["longest_component"])), max=int(np.max(info["longest_component"])))
    out["n_chains_mean"] = float(np.mean(info["n_chains"]))
    out["fell_back_calls"] = int(np.sum(info["fell_back"]))
    out["mode2_over_mode1_p50"] = out["mode2"]["p50_us"] / out["mode1"]["p50_us"]
    out["mode2_over_mode0_p50"] = out["mode2"]["p50_us"] / out["mode0"]["p50_us"]
    return out


def kernel_stats(args):
    """the same run as a child under rocprofv3 (a fresh process: the profiler's library initialises the GPU before Python starts)"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"error": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="plv_lwm_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--child", "--frames", str(args.frames), "--reps", "2", "--mode1-reps", "1", "--workloads", args.workloads]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=d, start_new_session=True)
        try:
            _, err = p.communicate(timeout=args.rocprof_timeout)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)   # the profiler and the run under it
            p.communicate()
            return {"error": f"rocprofv3 run exceeded {args.rocprof_timeout} s"}
        if p.returncode != 0:
            return {"error": f"rocprofv3 run failed ({p.returncode})", "stderr_tail": err[-600:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv written"}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k + "(" in row["Name"] or k + "<" in row["Name"]:
                        e = out.setdefault(k, dict(calls=0, total_ns=0))
                        e["calls"] += int(row["Calls"])
                        e["total_ns"] += int(row["TotalDurationNs"])
        for e in out.values():
            e["average_us"] = e.pop("total_ns") / max(e["calls"], 1) / 1e3
        out["note"] = "all workloads and modes of the run together; averages over every launch of the kernel"
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C,D")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--mode1-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_walk_modes.json"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--rocprof-timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true", help="(internal) the profiled run: times nothing, writes nothing")
    args = ap.parse_args()
    names = [n for n in args.workloads.split(",") if n]
    frames = {n: render(WORKLOADS[n], args.frames) for n in names}   # before the GPU is touched
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    res = {n: run_workload(pkg, n, frames[n], args.reps, args.mode1_reps) for n in names}
    if args.child:
        return
    doc = dict(tool="tools/line_walk_modes.py", what="plv_detect_lines, start of the call to its return (mode 0: plv_line_detect_launch + plv_detect_lines, the labelled detection of a frame), "
                    "modes alternating frame by frame in one process",
               workloads=res)
    if not args.no_rocprof:
        doc["kernel_stats"] = kernel_stats(args)
    for n in names:
        r = res[n]
        print(f"{n}: mode 0 p50 {r['mode0']['p50_us']:.1f} us, mode 1 p50 {r['mode1']['p50_us']:.1f} us, mode 2 p50 {r['mode2']['p50_us']:.1f} us "
              f"(p99 {r['mode2']['p99_us']:.1f}); components {r['n_components']['mean']:.0f}, largest {r['longest_component']['max']}")
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
