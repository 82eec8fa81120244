#!/usr/bin/env python3
"""What a camera frame costs under est.use_imu_res (observation poses from the CPI records), per frame of a replayed drive: host
time around the driver's camera call (feed + try_update, however the driver splits it; every form ends in a synchronisation), and
the library's launches, synchronisations and copied bytes inside it (plv_counters).  Written for the comparison of two builds of
the library on one dataset — the tree this file lies in against a copy of another commit — run alternately, several rounds each, so
that the spread between rounds of one build stands next to the difference between the builds.

    python tools/imu_res_route.py run --dataset DIR [--render 24] [--tree OTHER_ROOT] --out ROUND.json
        one replay of DIR (rendered first, tests/synth_dataset.py, when DIR holds none) through the package of this tree or of
        OTHER_ROOT, use_imu_res on, lines on; the figures of the frames after the first --warmup updating ones
    python tools/imu_res_route.py merge --parent P1.json P2.json P3.json --change C1.json C2.json C3.json
                                        [--bench-parent B.jsonl ...] [--bench-change B.jsonl ...] [--bench-order WORDS] [--kernel-stats STATS.csv]
                                        --out profiles/imu_res_route.json
        the rounds side by side: per build the rounds' p50 / p99 and their spread (largest minus smallest p50), the difference of
        the builds' median p50; the same for bench.py result lines (polynomial poses); the pose launch's row of a
        `rocprofv3 --kernel-trace --stats` run
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(a):
    root = os.path.abspath(a.tree) if a.tree else HERE
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    import synth_dataset as sd
    pkg = ge.load_pkg()
    options = importlib.import_module("plviwo_amd.options")
    rp = importlib.import_module("plviwo_amd.replay")
    system = importlib.import_module("plviwo_amd.system")
    if not os.path.exists(os.path.join(a.dataset, "gt.txt")):
        t0 = time.time()
        sd.make_dataset(a.dataset, a.render, workers=min(16, os.cpu_count() or 1))
        print(f"rendered {a.render} s into {a.dataset} ({time.time() - t0:.1f} s)", flush=True)
    out_dir = os.path.join(a.dataset, "out_" + str(os.getpid()))
    op = options.load_options(sd.write_config(os.path.join(out_dir, "config"), a.dataset, os.path.join(out_dir, "traj.txt")))
    op.est.use_imu_res, op.est.cam.use_lines = True, True
    rows = []
    inner = system.SystemManager.feed_measurement_camera
    keys = ("launches", "syncs", "copy_bytes", "frame_ns")

    def timed(self, t, img, mask=None, staged_slot=None):
        updating = bool(self.state.initialized)
        c0, t0 = pkg.counters(), time.perf_counter()
        r = inner(self, t, img, mask, staged_slot=staged_slot)
        ms = (time.perf_counter() - t0) * 1e3
        c1 = pkg.counters()
        if updating:
            rows.append([ms] + [c1[k] - c0[k] for k in keys])
        return r

    system.SystemManager.feed_measurement_camera = timed
    try:
        stats, times, poses = rp.replay(op)
    finally:
        system.SystemManager.feed_measurement_camera = inner
    m = np.array(rows[a.warmup:], dtype=np.float64)
    if len(m) < 1:
        raise SystemExit(f"{len(rows)} updating frames: none left after {a.warmup} warm-up frames")
    res = dict(frames=int(len(m)), warmup=a.warmup, ms_p50=float(np.percentile(m[:, 0], 50)), ms_p99=float(np.percentile(m[:, 0], 99)),
               ms_mean=float(m[:, 0].mean()), launches_per_frame=float(m[:, 1].mean()), syncs_per_frame=float(m[:, 2].mean()),
               copy_bytes_per_frame=float(m[:, 3].mean()), ms_inside_plv_camera_frame_per_frame=float(m[:, 4].mean() / 1e6),
               cam_updates=stats["cam_updates"], line_updates=stats["line_updates"], cam_accepted=stats["cam_accepted"], not_psd=stats["not_psd"])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


def _side(rounds, key):
    vals = [r[key] for r in rounds]
    s = sorted(vals)
    return dict(rounds=vals, median=s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]), spread=max(vals) - min(vals))


def _compare(parent, change, key):
    if not parent or not change:
        return "not measured"
    p, c = _side(parent, key), _side(change, key)
    d = c["median"] - p["median"]
    return dict(parent=p, change=c, change_minus_parent=d, within_the_parents_spread=bool(d <= p["spread"]))


def _bench_lines(paths):
    out = []
    for path in paths or []:
        for line in open(path):
            line = line.strip()
            if line.startswith("{") and '"ms_per_step"' in line:
                r = json.loads(line)
                out.append(dict(ms_per_step=r["ms_per_step"], p50_ms=r.get("latency_p50_ms"), p99_ms=r.get("latency_p99_ms"), frames_per_s=r.get("value"),
                                steps=r.get("steps")))
    return out


def merge(a):
    load = lambda paths: [{k: v for k, v in json.load(open(p)).items() if k != "tree"} for p in paths or []]
    parent, change = load(a.parent), load(a.change)
    res = dict(drive="tools/replay.py --synthetic 24 with est.use_imu_res: true, lines on; host clock around the driver's camera call of every "
                     "updating frame after the warm-up frames, plv_counters around the same call",
               order="the builds alternate, parent first, one replay per round, same dataset and seed",
               rounds=dict(parent=parent, change=change),
               ms_per_camera_frame=dict(p50=_compare(parent, change, "ms_p50"), p99=_compare(parent, change, "ms_p99")),
               per_frame={k: _compare(parent, change, k) for k in ("launches_per_frame", "syncs_per_frame", "copy_bytes_per_frame",
                                                                   "ms_inside_plv_camera_frame_per_frame")})
    bp, bc = _bench_lines(a.bench_parent), _bench_lines(a.bench_change)
    res["bench_polynomial_poses"] = dict(order=a.bench_order, rounds=dict(parent=bp, change=bc), ms_per_step=_compare(bp, bc, "ms_per_step"),
                                         p50_ms=_compare(bp, bc, "p50_ms"))
    res["pose_launch"] = "not measured"
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        for row in csv.DictReader(open(a.kernel_stats)):
            if "cpi_pose_kernel" in (row.get("Name") or ""):
                res["pose_launch"] = {k: row[k] for k in row if k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage")}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--dataset", required=True)
    r.add_argument("--render", type=float, default=24.0, help="seconds of the synthetic drive to render when the directory holds none")
    r.add_argument("--tree", help="root of the checkout whose package is measured (default: this one)")
    r.add_argument("--warmup", type=int, default=20)
    r.add_argument("--out", required=True)
    m = sub.add_parser("merge")
    m.add_argument("--parent", nargs="*")
    m.add_argument("--change", nargs="*")
    m.add_argument("--bench-parent", nargs="*")
    m.add_argument("--bench-change", nargs="*")
    m.add_argument("--bench-order", default="the builds alternate, parent first", help="how the bench runs were ordered, in words")
    m.add_argument("--kernel-stats")
    m.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
