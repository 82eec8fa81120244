#!/usr/bin/env python3
"""Measurements of the track image (plv_track_image, draw_tile_kernel) -> profiles/track_image.json.

    python tools/track_image_profile.py calls --cache DIR --out calls.json
        the bench's boulevard scene (bench.py workload C: side-looking camera, points + lines) at 752 x 480 and at 1280 x 720: after a
        warmed-up drive through the filter, the wall time of 200 plv_track_image calls on prepared arguments (p50 / p99), for the
        history layer and for all layers, with the primitive count of each and the bytes the call has to move
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/track_image_profile.py kernels --cache DIR --plan DIR/plan.json
    python tools/track_image_profile.py parse --plan DIR/plan.json --trace DIR --out kernels.json
        the same drive and calls under the profiler, in a run of its own: the dispatches of draw_tile_kernel in the order of the plan
    python tools/track_image_profile.py replay --out replay.json
        a 24 s synthetic drive (tests/synth_dataset.py, what tools/replay.py --synthetic 24 renders) replayed in one process without,
        with, with and without the picture after every frame (what tools/replay.py --track-images does): ms per camera frame
    python tools/track_image_profile.py merge --parts calls.json kernels.json replay.json --out profiles/track_image.json
"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

WARM_FRAMES = 75          # bench.py's prologue (60) and a warm-up: the clone window is full, the tracks have their history
LAYER_SETS = (("history", 1), ("all", 1 | 2 | 4 | 8))


def _workloads():
    import bench
    c = dict(bench.WORKLOADS["C"])
    big = dict(c, w=1280, h=720, points=500, num_features=780)      # the same scene and mount at workload D's size and point count
    return (("752x480", c), ("1280x720", big))


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def _driven_system(wl, workers, cache=None):
    """bench.py's stream and driver, WARM_FRAMES camera frames in: returns the SystemManager.  cache: where the rendered frames are kept
    (the profiled run must not fork render workers and takes them from there)"""
    import bench
    stream = bench.build_stream(wl, WARM_FRAMES, workers, cache=cache)
    system = importlib.import_module("plviwo_amd.system")
    sm = system.SystemManager(bench.load_options(wl), max_obs=24)
    pl = bench.Player(stream, sm, staged=False)
    while True:
        nxt = pl.next_frame()
        if nxt is None:
            break
        pl.camera(*nxt)
    return sm


def _prepared_call(pkg, sm, layers):
    """plv_track_image on arguments marshalled beforehand, as a C++ caller makes it: returns (call, n_primitives)"""
    ctx = sm.ctx
    opt, keep = ctx._track_image_options(layers, None, None, list(sm.state.slam), None)
    out = np.zeros((ctx.cfg.height, ctx.cfg.width, 3), dtype=np.uint8)
    ptr, stride, fn, h = out.ctypes.data_as(C.POINTER(C.c_uint8)), 3 * ctx.cfg.width, ctx.lib.plv_track_image, ctx.h

    def call():
        rc = fn(h, C.byref(opt), ptr, stride)
        if rc != pkg.PLV_OK:
            raise SystemExit(f"plv_track_image: {rc} {ctx.lib.plv_last_error()}")
    call.keep = (keep, out)
    return call, len(ctx.track_image_primitives(layers, highlighted=list(sm.state.slam)))


def calls(a):
    pkg = ge.load_pkg()
    runs = []
    for name, wl in _workloads():
        sm = _driven_system(wl, a.workers, a.cache and os.path.join(a.cache, f"frames_{name}.npz"))
        w, h = wl["w"], wl["h"]
        for lname, layers in LAYER_SETS:
            call, n_prims = _prepared_call(pkg, sm, layers)
            for _ in range(20):
                call()
            us = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                call()
                us.append((time.perf_counter() - t0) * 1e6)
            runs.append(dict(size=name, scene=wl["scene"], layers=lname, primitives=n_prims, tracked_points=len(sm.ctx.tracker_last()[1]),
                             lines=len(sm.ctx.line_tracker_last()[1]), calls=a.calls, wall_us=dict(p50=round(statistics.median(us), 1), p99=round(_pct(us, 0.99), 1),
                                                                                                 min=round(min(us), 1), max=round(max(us), 1)),
                             bytes=dict(read_grey=w * h, written_rgb=3 * w * h, copied_back=3 * w * h, primitives_up=32 * n_prims)))
            print(runs[-1], flush=True)
        sm.close()
    out = dict(what="wall time of plv_track_image (microseconds, prepared arguments, time.perf_counter around the ctypes call) after "
                    f"{WARM_FRAMES} camera frames of bench.py's workload C stream (boulevard scene, points + lines) through SystemManager; "
                    "20 untimed calls first", runs=runs)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def kernels(a):
    """the drive and REPEAT calls per (size, layer set), in the order the plan records; cached frames only (a profiled run must not fork)"""
    pkg = ge.load_pkg()
    plan = []
    for name, wl in _workloads():
        sm = _driven_system(wl, 1, a.cache and os.path.join(a.cache, f"frames_{name}.npz"))
        for lname, layers in LAYER_SETS:
            call, n_prims = _prepared_call(pkg, sm, layers)
            for _ in range(a.repeat):
                call()
            plan.append(dict(size=name, layers=lname, primitives=n_prims, launches=a.repeat))
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
                if "draw_tile_kernel" in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    want = sum(g["launches"] for g in plan)
    if len(rows) != want:
        raise SystemExit(f"{len(rows)} dispatches of draw_tile_kernel in the trace, the plan has {want}")
    out, k = [], 0
    for g in plan:
        us = [(e - s) * 1e-3 for s, e in rows[k:k + g["launches"]]][3:]    # (the first launches of a group: cold caches)
        k += g["launches"]
        out.append(dict(g, kernel_us=dict(p50=round(statistics.median(us), 2), p99=round(_pct(us, 0.99), 2), min=round(min(us), 2), max=round(max(us), 2))))
        print(out[-1])
    with open(a.out, "w") as f:
        json.dump(dict(what="draw_tile_kernel, rocprofv3 --kernel-trace --stats in a run of its own: End - Start per dispatch, microseconds, "
                            "launches 4.. of each group", groups=out), f, indent=1)


def replay(a):
    import synth_dataset as sd
    pkg = ge.load_pkg()
    tmp = tempfile.mkdtemp(prefix="plv_track_image_")
    sd.make_dataset(tmp, a.seconds, workers=a.workers)
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    pics = os.path.join(tmp, "pics")
    os.makedirs(pics)
    layers = pkg.viz_layers("history")

    def after_camera(system, frame, t):
        rgb, _ = system.get_track_img(layers)
        rp.write_ppm(os.path.join(pics, f"{frame:06d}.ppm"), rgb)

    runs, poses = [], []
    for k, with_images in enumerate((False, True, True, False)):
        op = options.load_options(sd.write_config(os.path.join(tmp, "config"), tmp, os.path.join(tmp, f"traj_{k}.txt")))
        stats, times, p = rp.replay(op, after_camera=after_camera if with_images else None)
        n = max(stats["camera_messages"], 1)
        extra = stats.get("time_after_camera_s", 0.0)
        runs.append(dict(order=k, track_images=with_images, camera_messages=stats["camera_messages"],
                         frame_ms=round(1e3 * stats["time_camera_s"] / n, 3), picture_and_file_ms=round(1e3 * extra / n, 3),
                         total_ms_per_camera_frame=round(1e3 * (stats["time_camera_s"] + extra) / n, 3)))
        poses.append(p)
        print(runs[-1], flush=True)
    same = all(np.array_equal(poses[0], p) for p in poses[1:])
    with open(a.out, "w") as f:
        json.dump(dict(what=f"{a.seconds:g} s synthetic drive (tests/synth_dataset.py 'room', 752 x 480, points + lines + wheel: the dataset of "
                            f"tools/replay.py --synthetic {a.seconds:g}) replayed four times in one process: without, with, with, without the track image "
                            "(history layer) fetched and written as a PPM after every camera frame; wall time per camera message past the file read",
                       runs=runs, same_trajectory_in_all_runs=bool(same)), f, indent=1)
    if not same:
        raise SystemExit("FAILED: the picture changed the trajectory")


def merge(a):
    out = dict(device="AMD Instinct MI355X (gfx950)", how="tools/track_image_profile.py: calls, kernels (under rocprofv3 --kernel-trace --stats, "
               "a run of its own) + parse, replay; merged")
    for path in a.parts:
        name = os.path.splitext(os.path.basename(path))[0]
        out[name] = json.load(open(path))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("calls", "kernels", "parse", "replay", "merge"))
    ap.add_argument("--plan")
    ap.add_argument("--trace")
    ap.add_argument("--out")
    ap.add_argument("--parts", nargs="*")
    ap.add_argument("--cache", help="directory for the rendered frames: `calls` saves them, `kernels` reads them")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=24.0)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    {"calls": calls, "kernels": kernels, "parse": parse, "replay": replay, "merge": merge}[a.mode](a)


if __name__ == "__main__":
    main()
