"""The YAML option loader against a configuration directory in the reference's layout
(tests/golden/config_sample: the reference's keys, this repository's own values)."""
import os
import shutil

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "golden", "config_sample", "config.yaml")


@pytest.fixture(scope="module")
def options(pkg):
    import importlib
    return importlib.import_module("plviwo_amd.options")


def test_sample_configuration(options):
    op = options.load_options(SAMPLE)
    s, e = op.sys, op.est
    assert (s.verbosity, s.exp_id, s.save_trajectory, s.path_trajectory, s.bag_start, s.bag_durr) == (3, 4, True, "out/traj.txt", 0.5, -1.0)
    assert s.path_gt == ""                                        # optional entry absent: the default stays
    assert list(e.gravity) == [0.0, 0.0, 9.81] and e.clone_freq == 10 and e.window_size == 1.0 and e.intr_order == 3
    assert (e.use_imu_res, e.use_imu_cov, e.use_pol_cov, e.dynamic_cloning) == (False, False, True, False)
    ie = e.intr_err
    assert ie.mlt == 2.0 and ie.threshold_ori == pytest.approx(0.004) and ie.threshold_pos == pytest.approx(0.002)
    # a rate needs both tables (Hz_25 has no orientation row) and five non-negative entries
    assert ie.available_clone_hz() == [5, 10, 20]
    assert ie.ori_slope[10][3] == 0.0012 and ie.pos_slope[20][9] == 0.00003
    assert ie.ori_std(10, 3, 0.5) == pytest.approx(2 * 0.5 * 0.0012) and ie.pos_cov(5, 1, 2.0) == pytest.approx((2 * 2.0 * 0.035) ** 2)
    assert (e.imu.sigma_w, e.imu.sigma_wb, e.imu.sigma_a, e.imu.sigma_ab) == (1.7e-4, 1.9e-5, 2.0e-3, 3.0e-3)
    i = e.init
    assert (i.window_time, i.imu_thresh, i.imu_wheel_thresh, i.imu_only_init, i.imu_gravity_aligned, i.use_gt, i.cov_size) == \
        (1.0, 0.3, 0.2, False, False, False, 1e-3)
    c = e.cam
    assert c.enabled and c.max_n == 1 and not c.use_stereo and c.stereo_pairs == {}
    assert (c.n_pts, c.fast, c.grid_x, c.grid_y, c.min_px_dist, c.max_slam, c.max_msckf) == (200, 25, 6, 4, 12, 0, 40)
    assert c.histogram == options.HISTOGRAM["CLAHE"] and c.feat_rep == options.FEAT_REP["GLOBAL_3D"] and c.sigma_pix == 1.5
    assert c.do_calib_int and not c.do_calib_ext and not c.do_calib_dt and c.downsample
    # downsample halves the four projection parameters and the resolution, not the distortion (OptionsCamera.cpp:123-138)
    assert np.allclose(c.intrinsics[0], [458.65, 457.3, 367.2, 248.4, -0.28, 0.07, 0.0002, 0.00002]) and c.wh[0] == [752, 480]
    assert c.dt[0] == 0.002 and c.distortion_model[0] == "radtan" and c.topic == ["cam0"]
    fi = c.featinit
    assert (fi.min_dist, fi.max_dist, fi.max_cond_number, fi.max_baseline, fi.refine_features) == (0.25, 80.0, 20000.0, 40.0, True)
    # extrinsics: q_ItoC, p_IinC from T_imu_cam = [R_CtoI p_CinI]
    R_CtoI = np.array([[0, 0, 1.0], [-1, 0, 0], [0, -1, 0]])
    q, p_IinC = c.extrinsics[0][:4], c.extrinsics[0][4:]
    x, y, z, w = q
    R_ItoC = (2 * w * w - 1) * np.eye(3) - 2 * w * np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]]) + 2 * np.outer(q[:3], q[:3])
    assert np.allclose(R_ItoC, R_CtoI.T, atol=1e-12) and np.allclose(p_IinC, -R_CtoI.T @ [0.10, 0.02, -0.03])
    wl = e.wheel
    assert wl.enabled and wl.type == "Wheel3DLin" and (wl.noise_w, wl.noise_v, wl.noise_p, wl.chi2_mult, wl.dt) == (0.02, 0.05, 0.01, 2.0, 0.01)
    assert not wl.do_calib_int                                     # only the ...Ang types have intrinsics to calibrate (OptionsWheel.cpp:71-73)
    assert np.allclose(wl.intrinsics, [0.31, 0.305, 1.52]) and np.allclose(wl.extrinsics, [0, 0, 0, 1, -0.07, 0, 1.7])


def _copy(tmp_path, edit):
    d = tmp_path / "cfg"
    shutil.copytree(os.path.dirname(SAMPLE), d)
    for name, (old, new) in edit.items():
        f = d / name
        text = f.read_text()
        assert old in text
        f.write_text(text.replace(old, new))
    return str(d / "config.yaml")


def test_rejections_follow_the_reference(options, tmp_path):
    bad = {
        "even order": ({"config_estimator.yaml": ("intr_order: 3", "intr_order: 4")}, "odd"),
        "window too short": ({"config_estimator.yaml": ("window_size: 1.0", "window_size: 0.2")}, "Max clone size"),
        "two covariance models": ({"config_estimator.yaml": ("use_imu_cov: false", "use_imu_cov: true")}, "More than 1"),
        "wheel type": ({"config_wheel.yaml": ('"Wheel3DLin"', '"Wheel4D"')}, "not a supported type"),
        "histogram": ({"config_camera.yaml": ('"CLAHE"', '"GAMMA"')}, "invalid feature histogram"),
        "representation": ({"config_camera.yaml": ('"GLOBAL_3D"', '"ANCHORED_3D"')}, "unsupported feature representation"),
        "missing required": ({"config_imu.yaml": ("  gyro_bias: 1.9e-05\n", "")}, "required entry imu.gyro_bias"),
    }
    for i, (name, (edit, msg)) in enumerate(bad.items()):
        with pytest.raises(options.OptionsError, match=msg):
            options.load_options(_copy(tmp_path / str(i), edit))
    # not strict: the default is used, as the reference does before it checks YamlParser::successful()
    cfg = _copy(tmp_path / "lenient", {"config_imu.yaml": ("  gyro_bias: 1.9e-05\n", "")})
    assert options.load_options(cfg, strict=False).est.imu.sigma_wb == 1.9393e-05


def test_sections_without_a_file_are_disabled(options, tmp_path):
    cfg = _copy(tmp_path, {})
    os.remove(os.path.join(os.path.dirname(cfg), "config_wheel.yaml"))
    os.remove(os.path.join(os.path.dirname(cfg), "config_camera.yaml"))
    op = options.load_options(cfg)
    assert not op.est.wheel.enabled and not op.est.cam.enabled


def test_stereo_pairs_share_a_time_offset(options, tmp_path):
    cam1 = '''cam1:
  timeoffset: 0.009
  T_imu_cam:
    - [0.0, 0.0, 1.0, 0.10]
    - [-1.0, 0.0, 0.0, -0.09]
    - [0.0, -1.0, 0.0, -0.03]
    - [0.0, 0.0, 0.0, 1.0]
  distortion_coeffs: [-0.28, 0.07, 0.0002, 0.00002]
  distortion_model: radtan
  intrinsics: [917.3, 914.6, 734.4, 496.8]
  resolution: [1504, 960]
  topic: "cam1"
'''
    cfg = _copy(tmp_path, {"config_camera.yaml": ("  max_n: 1\n  use_stereo: false\n", "  max_n: 2\n  use_stereo: true\n  stereo_pair: [0, 1]\n")})
    with open(os.path.join(os.path.dirname(cfg), "config_camera.yaml"), "a") as f:
        f.write(cam1)
    c = options.load_options(cfg).est.cam
    assert c.use_stereo and c.stereo_pairs == {0: 1, 1: 0} and c.dt == {0: 0.002, 1: 0.002} and c.topic == ["cam0", "cam1"]


def test_reads_the_shipped_kaist_configuration(options):
    """The reference's own configuration directory loads as is (values checked by hand against its files; a verbatim copy of
    PL-VIWO/config/kaist/kaist_C is kept under tests/golden/kaist_C)."""
    op = options.load_options(os.path.join(HERE, "golden", "kaist_C", "config.yaml"))
    e = op.est
    assert e.clone_freq == 20 and e.window_size == 1.0 and e.use_imu_res and e.use_pol_cov and e.dynamic_cloning
    assert e.intr_err.available_clone_hz() == [4, 5, 6, 7, 9, 10, 15, 20, 25, 30] and e.intr_err.threshold_ori == pytest.approx(0.0035)
    assert e.cam.n_pts == 1500 and e.cam.max_msckf == 70 and e.cam.max_slam == 0 and e.cam.feat_rep == 1 and e.cam.wh[0] == [1280, 560]
    assert e.cam.stereo_pairs == {0: 1, 1: 0} and e.cam.dt[1] == e.cam.dt[0] == 0.0
    assert e.wheel.type == "Wheel3DAng" and list(e.wheel.intrinsics) == [0.3, 0.3, 1.5] and not e.wheel.do_calib_int
    assert e.init.imu_gravity_aligned and not e.init.imu_only_init and e.init.cov_size == 1e-2 and e.imu.sigma_a == 5.886e-02
