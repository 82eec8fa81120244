"""The driver on a stereo configuration, without a device: the shipped configuration (tests/golden/kaist_C) constructs a
SystemManager over the CPU stand-in (tests/stereo_mirror_context.py), the state has the reference's variable order for a pair
(State.cpp:58-112), what the driver does not build for a pair raises OptionsError with its word, and a short synthetic pair replays
over the mirror to an initialised filter with camera and line updates, the CameraSide current after every one."""
import copy
import importlib
import os

import numpy as np
import pytest

import synth_stereo_dataset as ssd
from oracle_context import OracleIwInitializer
from stereo_mirror_context import StereoMirrorContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAIST_C = os.path.join(ROOT, "tests", "golden", "kaist_C", "config.yaml")


@pytest.fixture(scope="module")
def mods(pkg):
    name = pkg.__name__
    return importlib.import_module(name + ".options"), importlib.import_module(name + ".system"), importlib.import_module(name + ".replay")


def _manager(system, op, **kw):
    return system.SystemManager(op, context_factory=StereoMirrorContext, iw_initializer_factory=OracleIwInitializer, **kw)


def test_shipped_stereo_configuration_constructs_a_driver(mods):
    options, system, _ = mods
    op = options.load_options(KAIST_C)
    c = op.est.cam
    assert c.max_n == 2 and c.use_stereo and c.stereo_pairs == {0: 1, 1: 0} and op.est.use_imu_res and not op.est.use_imu_cov
    assert c.do_calib_int and not c.do_calib_ext and not c.do_calib_dt and c.use_lines
    sm = _manager(system, op)
    st = sm.state
    # State.cpp:58-112 with do_calib_int only: [IMU 15][intrinsics 0: 8][intrinsics 1: 8] (+ what the wheel calibrates)
    assert sm.stereo and st.cam_intr.id == 15 and st.cam_intr1.id == 23 and st.cam_ext.id == st.cam_ext1.id == -1 and st.cam_dt.id == -1
    wheel_dim = (1 if st.wheel_dt is not None and st.wheel_dt.id >= 0 else 0) + (6 if st.wheel_ext is not None and st.wheel_ext.id >= 0 else 0) + \
                (3 if st.wheel_intr is not None and st.wheel_intr.id >= 0 else 0)
    assert st.n == 31 + wheel_dim
    assert np.array_equal(st.cam_intr1.v, c.intrinsics[1]) and not np.array_equal(st.cam_intr1.v, st.cam_intr.v)
    assert np.array_equal(sm.ctx.sref.K8[1], c.intrinsics[1])                       # stereo_configure: camera 1's intrinsics
    P = sm.ctx.cov_download(st.n)
    r2 = (np.sqrt(c.init_cov_in_r) / 10.0) ** 2 if c.init_cov_in_r > 1e-5 else c.init_cov_in_r
    prior = [c.init_cov_in_k] * 2 + [c.init_cov_in_c] * 2 + [c.init_cov_in_r] * 2 + [r2] * 2
    assert np.array_equal(np.diag(P)[15:23], prior) and np.array_equal(np.diag(P)[23:31], prior)


def test_full_calibration_order_and_the_shared_time_offset(mods):
    options, system, _ = mods
    op = options.load_options(KAIST_C)
    op.est.cam.do_calib_ext = op.est.cam.do_calib_dt = True
    st = _manager(system, op).state
    # per camera: extrinsics, intrinsics, then camera 0's time offset — camera 1 shares it (State.cpp:102-103)
    assert (st.cam_ext.id, st.cam_intr.id, st.cam_dt.id, st.cam_ext1.id, st.cam_intr1.id) == (15, 21, 29, 30, 36)
    side = st.side()
    assert side.c.extrinsic_state_id == 30 and side.c.intrinsic_state_id == 36 and st.view().c.dt_state_id == 29


@pytest.mark.parametrize("word, change, kw", [
    ("one stereo pair", lambda op: setattr(op.est.cam, "use_stereo", False), {}),
    ("one stereo pair", lambda op: setattr(op.est.cam, "stereo_pairs", {}), {}),
    ("max_slam", lambda op: setattr(op.est.cam, "max_slam", 5), {}),
    ("downsample", lambda op: setattr(op.est.cam, "downsample", True), {}),
    ("use_imu_cov", lambda op: setattr(op.est, "use_imu_cov", True), {}),
    ("zero-velocity", lambda op: setattr(op.est.zupt, "enabled", True), {}),
    ("decision trace", lambda op: None, dict(decisions=[])),
    ("line map", lambda op: None, dict(line_map=True)),
])
def test_what_a_stereo_driver_refuses(mods, word, change, kw):
    options, system, _ = mods
    op = options.load_options(KAIST_C)
    change(op)
    with pytest.raises(options.OptionsError) as e:
        _manager(system, op, **kw)
    assert word in str(e.value), str(e.value)


def test_stereo_needs_a_context_with_stereo_try_update_and_has_no_track_image(mods):
    options, system, _ = mods
    from oracle_context import PyMirrorContext
    op = options.load_options(KAIST_C)
    with pytest.raises(options.OptionsError) as e:
        system.SystemManager(op, context_factory=PyMirrorContext, iw_initializer_factory=OracleIwInitializer)
    assert "stereo_try_update" in str(e.value)
    with pytest.raises(options.OptionsError) as e:
        _manager(system, op).get_track_img()
    assert "track image" in str(e.value)


def _side_values(side):
    return np.array(side.c.R_ItoC), np.array(side.c.p_IinC), np.array(side.c.intrinsics)


def test_short_pair_replays_over_the_mirror(mods, tmp_path):
    options, system, rp = mods
    d = str(tmp_path / "pair")
    ssd.make_dataset(d, seconds=1.5, cam_hz=10.0, style="street", workers=min(8, os.cpu_count() or 1))
    op = options.load_options(ssd.write_config(str(tmp_path / "config"), d, str(tmp_path / "traj.txt"), calib_int=True))
    assert op.est.cam.max_n == 2 and op.est.cam.use_stereo and op.est.cam.use_lines and op.est.cam.do_calib_int
    checked = []

    def after_camera(sm, frame, t):
        st = sm.state
        if not st.initialized:
            return
        R, p, K = _side_values(st.side())
        # the CameraSide is bit-equal to the state's camera-1 variables after every update
        assert np.array_equal(R, st.cam_ext1.Rot().ravel()) and np.array_equal(p, st.cam_ext1.p) and np.array_equal(K, st.cam_intr1.v)
        assert np.array_equal(np.array(st.view().c.intrinsics), st.cam_intr.v)
        assert np.array_equal(sm.ctx.sref.K8[0], st.cam_intr.v) and np.array_equal(sm.ctx.sref.K8[1], st.cam_intr1.v)    # the tracker was told
        checked.append(K.copy())

    stats, times, poses = rp.replay(op, after_camera=after_camera, context_factory=StereoMirrorContext, iw_initializer_factory=OracleIwInitializer)
    print(stats)
    assert stats["stereo"] and stats["pairs_skipped"] == 0 and stats["frames"] == 15
    assert stats["initialized"] and stats["not_psd"] == 0
    assert stats["cam_updates"] >= 1 and stats["cam_accepted"] >= 1 and stats["line_updates"] >= 1, stats
    assert len(checked) >= 3 and np.abs(checked[-1] - np.asarray(op.est.cam.intrinsics[1])).max() > 0      # camera 1's intrinsics moved
