#!/usr/bin/env python3
"""Measurements of the image-encoding feature (grey_from_encoded_kernel and the entry points around it) -> profiles/image_encodings.json.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/image_encodings_profile.py kernels --plan DIR/plan.json
    python tools/image_encodings_profile.py parse --plan DIR/plan.json --trace DIR --out kernels.json
        the conversion kernel per encoding, size and source kind (page-locked host block / HBM): the workload issues the launches in
        a known order (the plan), the parser reads the dispatches of the kernel trace in that order
    python tools/image_encodings_profile.py handover --out handover.json
        per-frame wall time of raw block + plv_image_stage_encoded + plv_tracker_feed_staged against plv_image_stage of a ready grey
        image + plv_tracker_feed_staged: two contexts of one process, alternating frame by frame, every frame ending in a synchronise
    python tools/image_encodings_profile.py replay --out replay.json
        a KAIST-layout directory (tests/kaist_synth.py) replayed with the device route and with host_images=True, alternating; the
        camera-side wall time per frame of both; exits non-zero unless the device route is the faster one
"""
import argparse
import csv
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

SIZES = [(1280, 560), (752, 480)]
BPP = {"mono8": 1, "bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1, "bayer_grbg8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}
REPEAT = 50


def _spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return dict(n=len(xs), median=statistics.median(xs), p10=q(0.10), p90=q(0.90), min=xs[0], max=xs[-1], mean=sum(xs) / len(xs))


def kernels(a):
    """REPEAT launches per (size, encoding, source kind), in the order the plan records"""
    pkg = ge.load_pkg()
    rng = np.random.default_rng(0)
    plan = []
    for (w, h) in SIZES:
        ctx = pkg.Context(pkg.default_config(w, h))
        ctx.prof_enable(True)
        for name, bpp in BPP.items():
            img = rng.integers(0, 256, (h, w) if bpp == 1 else (h, w, bpp), dtype=np.uint8)
            blk = ctx.raw_image_buffer(0, name)
            blk[...] = img
            for source in ("pinned", "hbm"):
                ctx.synchronize()
                ctx.prof_reset()
                for _ in range(REPEAT):
                    if source == "pinned":
                        ctx.image_stage_encoded(0, blk, name)      # the kernel reads the page-locked block
                    else:
                        ctx.image_convert(img, name)               # upload, then the kernel reads HBM
                ctx.synchronize()
                ev = ctx.prof_table().get("grey_from_encoded_kernel")
                plan.append(dict(width=w, height=h, encoding=name, source=source, launches=REPEAT,
                                 hip_event_us=round(1e3 * ev[1] / max(ev[0], 1), 3) if ev else None))
        ctx.close()
    with open(a.plan, "w") as f:
        json.dump(plan, f, indent=1)
    print(f"{len(plan)} groups of {REPEAT} launches")


def parse(a):
    plan = json.load(open(a.plan))
    files = sorted(glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.trace}")
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "grey_from_encoded_kernel" in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    want = sum(g["launches"] for g in plan)
    if len(rows) != want:
        raise SystemExit(f"{len(rows)} dispatches of grey_from_encoded_kernel in the trace, the plan has {want}")
    out, k = [], 0
    for g in plan:
        part = rows[k:k + g["launches"]]
        k += g["launches"]
        us = [(e - s) * 1e-3 for s, e, _ in part][5:]              # (the first launches of a group: cold instruction cache, first touch)
        w, h, bpp = g["width"], g["height"], BPP[g["encoding"]]
        read, written = w * h * bpp, w * h
        sp = _spread(us)
        out.append(dict(g, kernel=part[0][2], kernel_us=sp, bytes_read=read, bytes_written=written,
                        gb_per_s=round((read + written) / (sp["median"] * 1e-6) / 1e9, 2),
                        read_gb_per_s=round(read / (sp["median"] * 1e-6) / 1e9, 2),
                        limit="the PCIe link, which carries the bytes read (read_gb_per_s)" if g["source"] == "pinned" else
                              "HBM for the bytes, but an image this small is launch- and latency-bound"))
    res = dict(what="grey_from_encoded_kernel, rocprofv3 --kernel-trace: per dispatch End - Start, microseconds, launches 6.. of each group",
               groups=out)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for g in out:
        print(f"{g['width']:5d}x{g['height']:<4d} {g['encoding']:12s} {g['source']:6s} {g['kernel_us']['median']:8.2f} us  {g['gb_per_s']:8.2f} GB/s  read {g['read_gb_per_s']:7.2f} GB/s")


def _frames(w, h, n=16):
    import synth
    canvas = synth.texture_canvas(w, h, seed=42)
    return [synth.render_frame(canvas, w, h, tx=1.5 * k, ty=-0.75 * k) for k in range(n)]


def _colour(grey, name):
    g = grey.astype(np.int32)
    rgb = np.stack([g, (g * 3) // 4 + 20, 255 - g // 2], axis=2).astype(np.uint8)
    if name.startswith("bayer"):
        yy, xx = np.mgrid[0:grey.shape[0], 0:grey.shape[1]]
        ch = np.array([[0, 1], [1, 2]])[yy % 2, xx % 2]            # RGGB
        return np.take_along_axis(rgb, ch[:, :, None], axis=2)[:, :, 0].copy()
    return np.ascontiguousarray(rgb[:, :, ::-1])                   # bgr8


def handover(a):
    pkg = ge.load_pkg()
    res = []
    for (w, h) in SIZES:
        grey = _frames(w, h)
        order = list(range(16)) + list(range(14, 0, -1))           # back and forth: small motion between neighbours
        for name in ("bayer_rggb8", "bgr8"):
            enc = [_colour(g, name) for g in grey]
            ca, cb = pkg.Context(pkg.default_config(w, h)), pkg.Context(pkg.default_config(w, h))
            ready = [ca.image_convert(e, name) for e in enc]
            ta, tb = [], []
            for k in range(a.warmup + a.frames):
                i = order[k % len(order)]
                t = 0.05 * k
                blk = ca.raw_image_buffer(k % 4, name)
                blk[...] = enc[i]                                  # (the driver's write into the block: outside the timed region, as the
                ca.synchronize(), cb.synchronize()                 #  grey image of the other side is ready before its clock starts)
                t0 = time.perf_counter()
                ca.image_stage_encoded(k % 8, blk, name)
                ca.tracker_feed_staged(t, k % 8)
                ca.synchronize()
                t1 = time.perf_counter()
                cb.image_stage(k % 8, ready[i])
                cb.tracker_feed_staged(t, k % 8)
                cb.synchronize()
                t2 = time.perf_counter()
                if k >= a.warmup:
                    ta.append((t1 - t0) * 1e6), tb.append((t2 - t1) * 1e6)
            pa, ia = ca.tracker_last()
            pb, ib = cb.tracker_last()
            same = bool(np.array_equal(ia, ib) and np.array_equal(pa, pb))
            ca.close(), cb.close()
            d = [x - y for x, y in zip(ta, tb)]
            r = dict(width=w, height=h, encoding=name, frames=len(ta), same_tracks=same, encoded_us=_spread(ta), grey_us=_spread(tb),
                     difference_us=_spread(d))
            res.append(r)
            print(f"{w}x{h} {name}: encoded {r['encoded_us']['median']:.1f} us, grey {r['grey_us']['median']:.1f} us, difference "
                  f"{r['difference_us']['median']:+.1f} us (p10 {r['difference_us']['p10']:+.1f}, p90 {r['difference_us']['p90']:+.1f}); same tracks: {same}")
    out = dict(what="wall time per frame, microseconds: raw_image_buffer block + image_stage_encoded + tracker_feed_staged + synchronize against "
                    "image_stage of the ready grey image + tracker_feed_staged + synchronize; two contexts, alternating frame by frame",
               warmup=a.warmup, runs=res)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def replay(a):
    import kaist_synth
    import synth_dataset as sd
    ge.load_pkg()
    tmp = tempfile.mkdtemp(prefix="plv_enc_")
    src, kdir = os.path.join(tmp, "src"), os.path.join(tmp, "urban_synth")
    sd.make_dataset(src, seconds=a.seconds, cam_hz=10.0, style="street", workers=min(16, os.cpu_count() or 1))
    kaist_synth.convert(src, kdir, sd.RL, sd.RR, sd.BASE, t0_ns=1000 * 10**9)
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    runs, poses = [], {}
    for rnd in range(a.rounds):
        for route in ("device", "host"):
            op = options.load_options(sd.write_config(os.path.join(tmp, "config"), kdir, os.path.join(tmp, f"traj_{route}.txt"), use_wheel=True))
            stats, times, p = rp.replay(op, host_images=route == "host")
            assert stats["image_route"] == route
            poses[route] = p
            runs.append(dict(round=rnd, route=route, camera_messages=stats["camera_messages"], camera_wall_s=stats["time_camera_s"],
                             camera_ms_per_frame=round(1e3 * stats["time_camera_s"] / max(stats["camera_messages"], 1), 3),
                             cam_accepted=stats["cam_accepted"], poses=len(times)))
            print(runs[-1])
    best = {r: min(x["camera_ms_per_frame"] for x in runs if x["route"] == r) for r in ("device", "host")}
    worst = {r: max(x["camera_ms_per_frame"] for x in runs if x["route"] == r) for r in ("device", "host")}
    same = bool(np.array_equal(poses["device"], poses["host"]))
    faster = worst["device"] < best["host"]
    out = dict(what="KAIST-layout directory (752 x 480 Bayer RGGB frames, points + lines + wheel): camera-side wall time per frame past the "
                    "file read (conversion + feed + update), device route against host_images=True in one process, alternating",
               seconds=a.seconds, runs=runs, same_trajectory=same, device_faster_in_every_pairing=faster)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"device route {best['device']:.3f} .. {worst['device']:.3f} ms per frame, host route {best['host']:.3f} .. {worst['host']:.3f}; "
          f"same trajectory: {same}; device faster: {faster}")
    if not (faster and same):
        raise SystemExit("FAILED: the device route must be faster than the host route and give the same trajectory")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "parse", "handover", "replay"))
    ap.add_argument("--plan")
    ap.add_argument("--trace")
    ap.add_argument("--out")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    {"kernels": kernels, "parse": parse, "handover": handover, "replay": replay}[a.mode](a)


if __name__ == "__main__":
    main()
