#!/usr/bin/env python3
"""The landmark stage of a camera frame, per-landmark loop against the two passes -> profiles/slam_pass.json.

    python tools/slam_pass_profile.py --out profiles/slam_pass.json [--ratios LOG]

One replay per landmark budget (cam.max_slam 12 and 25) of a rendered 752 x 480 dataset with a 15-clone window (clone_freq 15,
window_size 1 s), GLOBAL_3D so that both forms can run; SystemManager.slam_pass is flipped every BLOCK frames of the same replay, so
both forms meet the same filter in the same process.  The host clock runs around SystemManager._slam_update_and_init and ends behind
plv_ctx_synchronize; plv_counters are read around the same span.  --warmup frames are left out, at least --frames are timed.  Exits
non-zero when the passes' median frame is above the loop's.  --ratios: the output of tests/test_gpu_slam_pass.py -s, whose
"[largest ratio]" lines are recorded."""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

BLOCK = 5
KEYS = ("launches", "syncs", "copies", "copy_bytes")


def _spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return dict(n=len(xs), median=statistics.median(xs), p10=q(0.10), p90=q(0.90), p99=q(0.99), min=xs[0], max=xs[-1])


def run(pkg, dataset, tmp, max_slam, warmup):
    import synth_dataset as sd
    options, rp, system = (importlib.import_module("plviwo_amd." + m) for m in ("options", "replay", "system"))
    op = options.load_options(sd.write_config(os.path.join(tmp, f"config_{max_slam}"), dataset, os.path.join(tmp, "traj.txt"), clone_freq=15))
    op.est.cam.max_slam, op.est.cam.use_lines, op.est.cam.feat_rep = max_slam, False, 0
    rec = []
    inner = system.SystemManager._slam_update_and_init

    def timed(self, out, cpi=None):
        frame = len(rec)
        self.slam_pass = (frame // BLOCK) % 2 == 1
        self.ctx.synchronize()
        c0 = pkg.counters()
        t0 = time.perf_counter()
        inner(self, out, cpi)
        self.ctx.synchronize()
        us = (time.perf_counter() - t0) * 1e6
        c1 = pkg.counters()
        rec.append(dict(form="pass" if self.slam_pass else "loop", landmarks=int(out["n_slam"]) + int(out["n_init"]), n_slam=int(out["n_slam"]),
                        n_init=int(out["n_init"]), us=us, clones=len(self.state.clones), **{k: c1[k] - c0[k] for k in KEYS}))

    system.SystemManager._slam_update_and_init = timed
    try:
        stats, times, poses = rp.replay(op)
    finally:
        system.SystemManager._slam_update_and_init = inner
        system.SystemManager.slam_pass = True
    used = [r for r in rec[warmup:] if r["landmarks"] > 0]
    res = dict(max_slam=max_slam, frames_with_a_stage=len(rec), frames_timed=len(used), median_clones=statistics.median(r["clones"] for r in used),
               median_landmarks_per_frame=statistics.median(r["landmarks"] for r in used),
               stats={k: stats[k] for k in ("slam_initialized", "slam_updates", "slam_marginalized", "not_psd", "n_state")})
    for form in ("loop", "pass"):
        f = [r for r in used if r["form"] == form]
        lm = max(1, sum(r["landmarks"] for r in f))
        res[form] = dict(frame_us=_spread([r["us"] for r in f]), landmarks=lm, us_per_landmark=round(sum(r["us"] for r in f) / lm, 2),
                         per_landmark={k: round(sum(r[k] for r in f) / lm, 2) for k in KEYS})
    res["median_ratio_pass_over_loop"] = round(res["pass"]["frame_us"]["median"] / res["loop"]["frame_us"]["median"], 4)
    print(json.dumps(res, indent=1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--ratios")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--budgets", default="12,25")
    a = ap.parse_args()
    import synth_dataset as sd
    pkg = ge.load_pkg()
    tmp = tempfile.mkdtemp(prefix="plv_slam_")
    dataset = os.path.join(tmp, "data")
    seconds = (a.frames + a.warmup) / 10.0 + 2.5      # (the filter takes its first update a second or so in)
    sd.make_dataset(dataset, seconds=seconds, cam_hz=10.0, workers=min(16, os.cpu_count() or 1))
    runs = [run(pkg, dataset, tmp, int(b), a.warmup) for b in a.budgets.split(",")]
    ratios = {}
    if a.ratios and os.path.exists(a.ratios):
        for m in re.finditer(r"\[largest ratio\] (.+?): ([0-9.eE+-]+)", open(a.ratios).read()):
            ratios[m.group(1)] = max(ratios.get(m.group(1), 0.0), float(m.group(2)))
    out = dict(what="wall time of the landmark stage of a camera frame (SystemManager._slam_update_and_init + plv_ctx_synchronize), microseconds, "
                    "per-landmark loop against plv_camera_update_slam / plv_camera_init_slam: one replay, the form alternating every "
                    f"{BLOCK} frames; plv_counters per landmark over the same spans (the closing synchronise included)",
               image="752 x 480", clone_freq=15, window_size_s=1.0, warmup_frames=a.warmup, runs=runs,
               parity_tolerance_ratios=ratios)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    bad = [r["max_slam"] for r in runs if r["pass"]["frame_us"]["median"] > r["loop"]["frame_us"]["median"]]
    if bad:
        raise SystemExit(f"FAILED: the passes' median frame is above the loop's at max_slam {bad}")


if __name__ == "__main__":
    main()
