"""A stereo pair end to end through the driver: a 4 s "street" pair at 10 Hz, 752 x 480, use_imu_res, lines, online intrinsics of both
cameras and the wheel, over the HIP library and over the CPU stand-in (tests/stereo_mirror_context.py) — the rules of
tests/test_gpu_replay.py::test_replay_with_lines_against_the_cpu_oracle; and the same pair as RGGB bytes through the KAIST layout."""
import importlib
import os

import numpy as np
import pytest

import kaist_synth
import synth_dataset as sd
import synth_stereo_dataset as ssd
from oracle_context import OracleIwInitializer
from stereo_mirror_context import StereoMirrorContext

pytestmark = pytest.mark.gpu

# what the CPU mirror gives on this drive (it needs no device): cam_accepted 716, line_updates 6; the floors are about 80 % of that
FLOOR_CAM_ACCEPTED, FLOOR_LINE_UPDATES = 570, 5


@pytest.fixture(scope="module")
def pair_dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("street_pair"))
    ssd.make_dataset(d, seconds=4.0, cam_hz=10.0, style="street", workers=min(16, os.cpu_count() or 1))
    return d


def _ate(pkg, traj, gt):
    ctx = pkg.Context(pkg.default_config(752, 480))
    try:
        et, ep = pkg.traj_load(traj)[:2]
        gt_t, gt_p = pkg.traj_load(gt)[:2]
        ei, gi = pkg.traj_associate(et, gt_t)
        return ctx.traj_ate(ep[ei], gt_p[gi], "posyaw")["pos"]["rmse"]
    finally:
        ctx.close()


def test_stereo_replay_against_the_cpu_mirror(pkg, pair_dataset, tmp_path):
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    runs = {}
    for name, kw in (("hip", {}), ("cpu", dict(context_factory=StereoMirrorContext, iw_initializer_factory=OracleIwInitializer))):
        traj = str(tmp_path / f"traj_{name}.txt")
        op = options.load_options(ssd.write_config(str(tmp_path / "config"), pair_dataset, traj, calib_int=True))
        op.est.use_imu_res = True
        assert op.est.cam.use_lines and op.est.cam.do_calib_int and op.est.wheel.enabled and op.est.cam.use_stereo
        stats, times, poses = rp.replay(op, **kw)
        print(name, {k: v for k, v in stats.items() if k != "time_s"})
        assert stats["stereo"] and stats["pairs_skipped"] == 0
        assert stats["initialized"] and stats["not_psd"] == 0, (name, stats)
        runs[name] = (stats, times, poses, traj)
    sh, sc = runs["hip"][0], runs["cpu"][0]
    for key in ("clones", "frames", "lines_tracked", "wheel_accepted"):   # what the (bit-identical) front ends alone decide
        assert sh[key] == sc[key], (key, sh[key], sc[key])
    assert np.array_equal(runs["hip"][1], runs["cpu"][1])
    for key in ("cam_features", "cam_accepted", "cam_updates", "line_pool", "lines_triangulated", "lines_accepted", "line_updates"):
        assert abs(sh[key] - sc[key]) <= max(2, 0.03 * sc[key]), (key, sh[key], sc[key])   # threshold ties of the fp64 update side
    assert sh["cam_accepted"] >= FLOOR_CAM_ACCEPTED and sh["line_updates"] >= FLOOR_LINE_UPDATES, sh
    ph, pc = runs["hip"][2][:, :3], runs["cpu"][2][:, :3]
    d = np.abs(ph - pc).max()
    print("largest distance between the two trajectories %.3g m" % d)
    # rounding only: the first run measured 1.49e-11 m (profiles/stereo_replay.json); the bound is 100 x that — far inside 1e-6 m,
    # the level at which a triangulation refinement stopping one iteration apart shows (tests/test_gpu_replay.py)
    assert d < TRAJECTORY_BOUND, d
    ctx = pkg.Context(pkg.default_config(752, 480))
    try:
        assert ctx.traj_ate(runs["hip"][2], runs["cpu"][2], "none")["pos"]["rmse"] < 0.01
    finally:
        ctx.close()
    gt = os.path.join(pair_dataset, "gt.txt")
    ate = {name: _ate(pkg, runs[name][3], gt) for name in runs}
    print("ATE", ate)
    assert abs(ate["hip"] - ate["cpu"]) < 0.005, ate


TRAJECTORY_BOUND = 1.5e-9


def test_bayer_pair_through_the_kaist_layout(pkg, pair_dataset, tmp_path):
    """the first second of the pair as RGGB bytes in the KAIST raw layout: the library converts the pair on the device
    (plv_tracker_feed_stereo takes the encoding); the same counts as the replay of the same frames converted to grey on the host"""
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    k = kaist_synth.convert(pair_dataset, str(tmp_path / "kaist"), sd.RL, sd.RR, sd.BASE, t0_ns=1000 * 10**9)
    src = rp.Dataset(pair_dataset)
    os.makedirs(os.path.join(k, "image", "stereo_right"))
    for i, (t, _) in enumerate(src.frames):
        kaist_synth.write_png(os.path.join(k, "image", "stereo_right", f"{1000 * 10**9 + int(round(t * 1e9))}.png"), src.image(i, 1))
    runs = {}
    for name, host in (("device", False), ("host", True)):
        op = options.load_options(ssd.write_config(str(tmp_path / "config"), k, str(tmp_path / f"traj_{name}.txt"), calib_int=True))
        op.est.use_imu_res = True
        op.sys.bag_durr = 1.0
        stats, times, poses = rp.replay(op, host_images=host)
        print(name, {key: v for key, v in stats.items() if key != "time_s"})
        assert stats["stereo"] and stats["image_route"] == name and stats["initialized"] and stats["not_psd"] == 0
        runs[name] = (stats, times, poses)
    a, b = runs["device"][0], runs["host"][0]
    for key in a:
        if not key.startswith("time") and key != "image_route":
            assert a[key] == b[key], (key, a[key], b[key])
    assert a["frames"] >= 9 and a["cam_accepted"] > 0
    assert np.array_equal(runs["device"][1], runs["host"][1]) and np.array_equal(runs["device"][2], runs["host"][2])


# ---- a pair of equidistant (fisheye) cameras: both `distortion_model: equidistant` in the YAML
@pytest.fixture(scope="module")
def fisheye_pair_dataset(tmp_path_factory):
    import synth_fisheye as sf
    return sf.make_stereo_dataset(str(tmp_path_factory.mktemp("fisheye_pair")), seconds=4.0, cam_hz=10.0)


def test_fisheye_pair_replays_to_an_ate(pkg, fisheye_pair_dataset, tmp_path):
    """tests/synth_fisheye.py's drive (4 s at 10 Hz) seen by two equidistant cameras 0.5 m apart, through the driver from its
    Kalibr-style files: the rules of tests/test_gpu_equidistant.py::test_fisheye_drive_replays_to_an_ate — it initialises, updates,
    tracks lines on camera 0 and stays under that test's ATE bound; the same data with both cameras read as radtan (same fx fy cx cy,
    zero coefficients) is clearly worse.  Camera 0 alone on the same 4 s is replayed for the comparison DESIGN.md reports."""
    import synth_fisheye as sf
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    gt = os.path.join(fisheye_pair_dataset, "gt.txt")

    def run(name, write, model):
        traj = str(tmp_path / f"traj_{name}.txt")
        op = options.load_options(write(str(tmp_path / name), fisheye_pair_dataset, traj, model=model))
        stats, times, poses = rp.replay(op)
        frac = stats["cam_accepted"] / max(stats["cam_features"], 1)
        ate = _ate(pkg, traj, gt) if stats["initialized"] and len(times) > 2 else float("inf")
        print(f"{name}: ATE {ate:.4f} m over {len(times)} poses, accepted {stats['cam_accepted']} / {stats['cam_features']} ({frac:.3f}), "
              f"{stats['cam_updates']} updates in {stats['frames']} frames, lines tracked {stats['lines_tracked']}, not_psd {stats['not_psd']}")
        return stats, ate, frac, op

    stats, ate, frac, op = run("pair equidistant", sf.write_stereo_config, "equidistant")
    assert op.est.cam.use_stereo and dict(op.est.cam.distortion_model) == {0: "equidistant", 1: "equidistant"}
    assert stats["stereo"] and stats["pairs_skipped"] == 0 and stats["frames"] == 40
    assert stats["initialized"] and stats["not_psd"] == 0
    assert stats["cam_updates"] > 0 and stats["cam_accepted"] > 0
    assert stats["lines_tracked"] > 0
    assert ate < 0.10
    fstats, fate, ffrac, _ = run("pair read as radtan", sf.write_stereo_config, "radtan")
    assert ffrac < frac - 0.05 or fate > 1.5 * ate
    run("camera 0 alone, equidistant", sf.write_config, "equidistant")
