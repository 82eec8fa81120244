#!/usr/bin/env python3
"""What a stereo frame costs through plv_tracker_feed_stereo, beside what could be done without it: two plv_tracker_feed calls on
two contexts with the same two image streams -> profiles/stereo_front.json.

    python tools/stereo_front_profile.py --out profiles/stereo_front.json

Per size (752 x 480 and 1280 x 560, the KAIST size; num_features of bench.py's default workload) and round: one stereo context and
two monocular ones in one process, every frame fed in both forms (which goes first alternates frame by frame), each form's clock
around its calls and the synchronise that ends them; p50 / p99 over the frames after the warm-up, and the launches and
synchronisations per frame of each form from plv_counters.  The stereo form does more work: the left-to-right LK of new corners
and the right camera's pruning and top-up."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

SIZES = [(752, 480), (1280, 560)]
NUM_FEATURES = 440  # bench.py, workload C
DISPARITY = 9.0


def _pairs(w, h, n=16):
    import synth
    canvas = synth.texture_canvas(w, h, seed=42)
    left = [synth.render_frame(canvas, w, h, tx=1.5 * k, ty=-0.75 * k) for k in range(n)]
    right = [synth.render_frame(canvas, w, h, tx=1.5 * k + DISPARITY, ty=-0.75 * k) for k in range(n)]
    return left, right


def _spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return dict(n=len(xs), p50=round(statistics.median(xs), 1), p99=round(q(0.99), 1), min=round(xs[0], 1), mean=round(sum(xs) / len(xs), 1))


def _round(pkg, w, h, left, right, frames, warmup):
    def cfg():
        c = pkg.default_config(w, h)
        c.num_features = NUM_FEATURES
        return c
    K = np.array(list(cfg().intrinsics))
    st, ma, mb = pkg.Context(cfg()), pkg.Context(cfg()), pkg.Context(cfg())
    st.stereo_configure(K, 0)
    order = list(range(len(left))) + list(range(len(left) - 2, 0, -1))  # back and forth: small motion between neighbours
    t_st, t_mo = [], []
    count = dict(stereo=dict(launches=0, syncs=0), mono=dict(launches=0, syncs=0))

    def stereo(t, i):
        st.tracker_feed_stereo(t, left[i], right[i])
        st.synchronize()

    def mono(t, i):
        ma.tracker_feed(t, left[i])
        mb.tracker_feed(t, right[i])
        ma.synchronize()
        mb.synchronize()

    for k in range(warmup + frames):
        i, t = order[k % len(order)], 0.05 * k
        us = {}
        for name, fn in ((("stereo", stereo), ("mono", mono)) if k % 2 == 0 else (("mono", mono), ("stereo", stereo))):
            c0 = pkg.counters()
            t0 = time.perf_counter()
            fn(t, i)
            us[name] = (time.perf_counter() - t0) * 1e6
            c1 = pkg.counters()
            if k >= warmup:
                count[name]["launches"] += c1["launches"] - c0["launches"]
                count[name]["syncs"] += c1["syncs"] - c0["syncs"]
        if k >= warmup:
            t_st.append(us["stereo"]), t_mo.append(us["mono"])
    tracked = dict(stereo_left=len(st.stereo_last(0)[1]), stereo_right=len(st.stereo_last(1)[1]), mono_left=len(ma.tracker_last()[1]),
                   mono_right=len(mb.tracker_last()[1]))
    for c in (st, ma, mb):
        c.close()
    per_frame = {k: {q: round(v / frames, 2) for q, v in d.items()} for k, d in count.items()}
    return dict(stereo_us=_spread(t_st), two_mono_us=_spread(t_mo), difference_us=_spread([a - b for a, b in zip(t_st, t_mo)]),
                per_frame=per_frame, tracked_at_the_end=tracked)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    pkg = ge.load_pkg()
    runs = []
    for w, h in SIZES:
        left, right = _pairs(w, h)
        for rnd in range(a.rounds):
            r = dict(width=w, height=h, round=rnd, **_round(pkg, w, h, left, right, a.frames, a.warmup))
            runs.append(r)
            print(f"{w}x{h} round {rnd}: stereo p50 {r['stereo_us']['p50']} p99 {r['stereo_us']['p99']} us, two monocular feeds p50 "
                  f"{r['two_mono_us']['p50']} p99 {r['two_mono_us']['p99']} us; per frame {r['per_frame']}", flush=True)
    out = dict(what="wall time per frame, microseconds: plv_tracker_feed_stereo + plv_ctx_synchronize on one context against "
                    "plv_tracker_feed on two contexts (left, right) + their two synchronises; both forms every frame, alternating which "
                    "goes first; launches and synchronisations per frame from plv_counters",
               num_features=NUM_FEATURES, disparity_px=DISPARITY, frames=a.frames, warmup=a.warmup, runs=runs)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
