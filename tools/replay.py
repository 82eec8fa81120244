#!/usr/bin/env python3
"""Replays a dataset directory through the filter on the GPU and scores the trajectory (run_bag + ov_eval in one command).

    python tools/replay.py CONFIG.yaml [--dataset DIR] [--gt FILE] [--align posyaw] [--rpe 8,16,24] [--nees] [--out result.json]
    python tools/replay.py --synthetic 12 [--out result.json]        # renders tests/synth_dataset.py first (CPU), then replays it
    python tools/replay.py CONFIG.yaml --dataset KAIST_DIR [--host-images]   # Bayer frames: converted on the device unless --host-images
    python tools/replay.py --synthetic 12 --max-slam 12 --feat-rep GLOBAL_FULL_INVERSE_DEPTH   # in-state landmarks, either representation
    python tools/replay.py --synthetic 12 --track-images DIR [--track-image-every 5] [--track-image-layers history,lines,mask]
                                                                     # the track picture of the chosen frames as DIR/<frame>.ppm
    python tools/replay.py --synthetic 12 --map map.ply              # the map of the whole replay: MSCKF points, landmarks, 3-D line segments
    python tools/replay.py --synthetic 12 --stereo [--workers 8]     # renders a stereo pair (tests/synth_stereo_dataset.py) and replays it
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?")
    ap.add_argument("--dataset")
    ap.add_argument("--gt")
    ap.add_argument("--align", default="posyaw")
    ap.add_argument("--out")
    ap.add_argument("--rpe", help="comma-separated segment lengths in metres: relative pose error per length (ov_eval's calculate_rpe)")
    ap.add_argument("--nees", action="store_true", help="NEES of the logged pose covariance against the ground truth (calculate_nees)")
    ap.add_argument("--synthetic", type=float, default=0.0, help="seconds of the synthetic dataset to render and replay")
    ap.add_argument("--stereo", action="store_true", help="with --synthetic: a second camera 0.5 m to the right of the first, replayed as a stereo pair")
    ap.add_argument("--workers", type=int, default=1, help="with --synthetic: processes that render the images")
    ap.add_argument("--imu-res", action="store_true", help="override est.use_imu_res: observation poses from the preintegrated IMU records")
    ap.add_argument("--no-wheel", action="store_true")
    ap.add_argument("--no-lines", action="store_true")
    ap.add_argument("--keep", help="directory to keep the synthetic dataset in")
    ap.add_argument("--max-slam", type=int, help="override cam.max_slam: long tracks become in-state landmarks")
    ap.add_argument("--feat-rep", choices=("GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH"), help="override cam.feat_rep")
    ap.add_argument("--host-images", action="store_true", help="frames that are not grey (a KAIST directory's Bayer mosaics) are converted on the "
                    "host by the dataset reader instead of on the device by the library (the comparison run)")
    ap.add_argument("--track-images", metavar="DIR", help="write the track image (SystemManager.get_track_img) behind the chosen camera frames "
                    "as binary PPM files DIR/<frame>.ppm")
    ap.add_argument("--track-image-every", type=int, default=1, metavar="N", help="every N-th camera frame (default: every frame)")
    ap.add_argument("--track-image-layers", default="history", help="comma-separated: history, active, lines, mask")
    ap.add_argument("--map", metavar="FILE.ply", help="write the map of the whole replay as an ASCII PLY: the accepted MSCKF points, the in-state "
                    "landmarks and the end points of the used lines as vertices (property kind: 0 / 1 / 2), one edge per line segment")
    ap.add_argument("--map-all-lines", action="store_true", help="every triangulated line of the updates' batches (the reference's list), not "
                    "only those the gate accepted")
    a = ap.parse_args()
    if a.track_image_every < 1:
        ap.error("--track-image-every: a positive number")
    pkg = ge.load_pkg()
    options = importlib.import_module("plviwo_amd.options")
    rp = importlib.import_module("plviwo_amd.replay")
    tmp = None
    if a.synthetic > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import synth_dataset as sd
        tmp = a.keep or tempfile.mkdtemp(prefix="plv_synth_")
        t0 = time.time()
        if a.stereo:
            import synth_stereo_dataset as sd      # (the same generator for the left camera, the right one beside it)
        sd.make_dataset(tmp, a.synthetic, workers=max(1, a.workers), log=lambda s: print("  [render]", s, flush=True))
        a.config = sd.write_config(os.path.join(tmp, "config"), tmp, os.path.join(tmp, "out", "traj.txt"), use_wheel=not a.no_wheel)
        a.gt = os.path.join(tmp, "gt.txt")
        print(f"synthetic dataset in {tmp} ({time.time() - t0:.1f} s)", flush=True)
    op = options.load_options(a.config)
    if a.dataset:
        op.sys.path_bag = a.dataset
    if a.no_lines:
        op.est.cam.use_lines = False
    if a.imu_res:
        op.est.use_imu_res = True
    if a.max_slam is not None:
        op.est.cam.max_slam = a.max_slam
    if a.feat_rep:
        op.est.cam.feat_rep = options.FEAT_REP[a.feat_rep]
    if not op.sys.save_trajectory:
        op.sys.save_trajectory, op.sys.path_trajectory = True, os.path.join(tempfile.mkdtemp(prefix="plv_out_"), "traj.txt")
    written, after_camera = [], None
    if a.track_images:
        layers = pkg.viz_layers(a.track_image_layers)
        os.makedirs(a.track_images, exist_ok=True)

        def after_camera(system, frame, t):
            if frame % a.track_image_every == 0:
                rgb, _overlay = system.get_track_img(layers)
                path = os.path.join(a.track_images, f"{frame:06d}.ppm")
                rp.write_ppm(path, rgb)
                written.append(path)
    the_map, system_kw = None, {}
    if a.map:
        the_map, system_kw, picture = rp.MapAccumulator(accepted_only=not a.map_all_lines), dict(line_map=True), after_camera

        def after_camera(system, frame, t):
            the_map.after_camera(system, frame, t)
            if picture is not None:
                picture(system, frame, t)
    t0, c0 = time.time(), pkg.counters()
    stats, times, poses = rp.replay(op, host_images=a.host_images, after_camera=after_camera, **system_kw, progress=lambda s, t: print(f"  t={t:8.3f}  clones {s.stats['clones']}  cam accepted "
                                                                    f"{s.stats['cam_accepted']}/{s.stats['cam_features']}  wheel {s.stats['wheel_accepted']}  zupt {s.stats['zupt_updates']}", flush=True))
    res = dict(config=a.config, wall_s=round(time.time() - t0, 2), stats=stats, poses_logged=len(times), trajectory=op.sys.path_trajectory)
    c1, frames = pkg.counters(), max(1, stats["camera_messages"])
    # what the whole replay submitted (plv_counters), per camera message: propagation and wheel updates between the frames included
    res["per_camera_message"] = dict(time_camera_s=stats["time_camera_s"] / frames, launches=(c1["launches"] - c0["launches"]) / frames,
                                     synchronisations=(c1["syncs"] - c0["syncs"]) / frames, bytes_copied=(c1["copy_bytes"] - c0["copy_bytes"]) / frames)
    if a.track_images:
        res["track_images_written"] = len(written)
    if the_map is not None:
        the_map.write_ply(a.map)
        stats.update(the_map.stats())
        res["map"] = a.map
    if a.gt and len(times) > 2:
        ctx = pkg.Context(pkg.default_config(752, 480))
        et, ep, co, cp = pkg.traj_load(op.sys.path_trajectory)
        gt_t, gt_p = pkg.traj_load(a.gt)[:2]
        ei, gi = pkg.traj_associate(et, gt_t)
        r = ctx.traj_ate(ep[ei], gt_p[gi], a.align)
        res["ate"] = dict(method=a.align, n=len(ei), pos=r["pos"], ori=r["ori"], length_m=pkg.traj_length(ep))
        if a.rpe:
            lengths = [float(x) for x in a.rpe.split(",") if x.strip()]
            res["rpe"] = [dict(length_m=s["length"], n=s["n"], pos=s["pos"], ori=s["ori"])
                          for s in ctx.traj_rpe(ep[ei], gt_p[gi], lengths, a.align)]
        if a.nees:
            if len(co) != len(et):
                raise SystemExit(f"--nees: {len(co)} of {len(et)} logged poses carry a covariance")
            r = ctx.traj_nees(ep[ei], gt_p[gi], co[ei], cp[ei], a.align)
            res["nees"] = dict(method=a.align, n=r["n"], n_poses=len(ei), pos=r["pos"], ori=r["ori"])
        ctx.close()
    print(json.dumps(res, indent=1, default=float))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, default=float)


if __name__ == "__main__":
    main()
