"""est.use_imu_res (the shipped configuration's choice) end to end through the one-call forms: the street drive of
test_gpu_replay.py::test_one_call_try_update_equals_the_two_calls with the observation poses from the CPI records and lines on, as
plv_camera_frame per frame, as plv_camera_try_update after separate feeds, and as the two update calls with the dx applied by the
driver.  Under a CPI table nothing is speculative and no line launch is chained, so the three are the same filter bit for bit."""
import importlib
import os

import numpy as np
import pytest

import synth_dataset as sd

pytestmark = pytest.mark.gpu

MODES = {"frame": (True, True), "try_update": (True, False), "two_calls": (False, False)}      # (one_call_update, one_call_frame)


@pytest.fixture(scope="module")
def street_dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("street"))
    sd.make_dataset(d, seconds=6.0, cam_hz=10.0, style="street", workers=min(16, os.cpu_count() or 1))
    return d


@pytest.fixture(scope="module")
def runs(pkg, street_dataset, tmp_path_factory):
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    system = importlib.import_module("plviwo_amd.system")
    tmp = tmp_path_factory.mktemp("imu_res")
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for mode, (update, frame) in MODES.items():
            mp.setattr(system.SystemManager, "one_call_update", update)
            mp.setattr(system.SystemManager, "one_call_frame", frame)
            traj = str(tmp / f"traj_{mode}.txt")
            op = options.load_options(sd.write_config(str(tmp / "config"), street_dataset, traj))
            op.est.use_imu_res, op.est.cam.use_lines = True, True
            spec0, chain0, ns0 = pkg.route_counts()[7], pkg.chain_count(), pkg.counters()["frame_ns"]
            stats, times, poses = rp.replay(op)
            out[mode] = dict(stats=stats, times=times, poses=poses, traj=traj, speculated=pkg.route_counts()[7] - spec0,
                             chained=pkg.chain_count() - chain0, frame_ns=pkg.counters()["frame_ns"] - ns0)
    return out


def test_imu_res_drive_updates_with_points_and_lines(runs):
    s = runs["two_calls"]["stats"]
    assert s["initialized"] and s["not_psd"] == 0 and s["cam_updates"] >= 40 and s["line_updates"] >= 10, s


@pytest.mark.parametrize("mode", ["frame", "try_update"])
def test_one_call_forms_equal_the_two_calls_under_imu_res(runs, mode):
    s0, s1 = runs["two_calls"]["stats"], runs[mode]["stats"]
    for key in s0:
        if not key.startswith("time"):
            assert s1[key] == s0[key], (mode, key, s1[key], s0[key])
    assert np.array_equal(runs[mode]["times"], runs["two_calls"]["times"])
    assert np.array_equal(runs[mode]["poses"], runs["two_calls"]["poses"])


def test_nothing_speculative_and_nothing_chained_under_imu_res(runs):
    for mode in MODES:
        assert runs[mode]["speculated"] == 0 and runs[mode]["chained"] == 0, (mode, runs[mode]["speculated"], runs[mode]["chained"])


def test_imu_res_drive_goes_through_plv_camera_frame(runs):
    """time spent inside plv_camera_frame: the driver makes that call under use_imu_res, and only in the frame mode"""
    assert runs["frame"]["frame_ns"] > 0
    assert runs["try_update"]["frame_ns"] == 0 and runs["two_calls"]["frame_ns"] == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_imu_res_drive_stays_on_the_ground_truth(pkg, street_dataset, runs, mode):
    """the bound of test_gpu_replay.py::test_replay_with_imu_residual_poses for this option"""
    ctx = pkg.Context(pkg.default_config(752, 480))
    try:
        et, ep = pkg.traj_load(runs[mode]["traj"])[:2]
        gt_t, gt_p = pkg.traj_load(os.path.join(street_dataset, "gt.txt"))[:2]
        ei, gi = pkg.traj_associate(et, gt_t)
        r = ctx.traj_ate(ep[ei], gt_p[gi], "posyaw")
    finally:
        ctx.close()
    print(mode, "position RMSE", r["pos"]["rmse"], "over", len(ei), "poses")
    assert len(ei) >= 40 and r["pos"]["rmse"] < 0.10, r
