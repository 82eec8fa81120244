"""The equidistant camera model without a GPU: the numpy restatement's own properties, the option loader on a Kalibr-style
equidistant camera, and the replay driver's choice of model (a context factory that declares CAMERA_MODELS gets the model set; one
that does not, like the CPU oracle, is refused before it is built)."""
import importlib
import os
import re
import shutil

import numpy as np
import pytest

import cam_equi
import oracle_context as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K8 = np.array([350.0, 351.5, 376.25, 239.5, 3.2e-3, -1.1e-3, 2.4e-3, -6.0e-4])


def test_restatement_round_trip_centre_and_clamp():
    rng = np.random.default_rng(0)
    uv = np.stack([rng.uniform(0, 752, 400), rng.uniform(0, 480, 400)], 1).astype(np.float32)
    xn = cam_equi.undistort(K8, uv)
    back = cam_equi.distort(K8, xn).astype(np.float64)
    assert np.abs(back - uv).max() < 1e-3
    assert np.abs(cam_equi.undistort_double(K8, uv) - xn).max() < 1e-6
    # the exact principal point: theta_d = 0, scale 1
    assert np.array_equal(cam_equi.undistort(K8, np.float32([K8[2:4]]))[0], np.zeros(2, np.float32))
    # theta_d past pi/2 is clamped: theta is solved for pi/2 whatever the pixel and the scale is tan(theta) / (pi/2), so the
    # result grows linearly with the distance from the centre along a ray
    far = K8[2:4] + np.array([[800.0, 0.0], [1200.0, 0.0]])
    a, b = cam_equi.undistort(K8, far)
    assert abs(a[0] / b[0] - 800.0 / 1200.0) < 1e-6 and a[1] == b[1] == 0


def test_restatement_jacobian_against_differences():
    rng = np.random.default_rng(1)
    xy = rng.uniform(-0.9, 0.9, (20, 2))
    dzn, dzeta = cam_equi.distort_jacobian(K8, xy)

    def _distort_d(K, p):
        r = np.hypot(*p)
        th = np.arctan(r)
        thd = th * (1 + K[4] * th ** 2 + K[5] * th ** 4 + K[6] * th ** 6 + K[7] * th ** 8)
        return np.array([K[0] * p[0] * thd / r + K[2], K[1] * p[1] * thd / r + K[3]])

    h = 1e-6
    for i, p in enumerate(xy):
        num = np.stack([(_distort_d(K8, p + h * e) - _distort_d(K8, p - h * e)) / (2 * h) for e in np.eye(2)], 1)
        assert np.abs(num - dzn[i]).max() < 1e-5 * np.abs(dzn[i]).max()
        numz = np.stack([(_distort_d(K8 + h * e, p) - _distort_d(K8 - h * e, p)) / (2 * h) for e in np.eye(8)], 1)
        assert np.abs(numz - dzeta[i]).max() < 1e-5 * max(1.0, np.abs(dzeta[i]).max())


def _equidistant_config(tmp_path):
    d = str(tmp_path / "config")
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "config_sample"), d)
    p = os.path.join(d, "config_camera.yaml")
    text = open(p).read()
    text = re.sub(r"distortion_model: *\S+", "distortion_model: equidistant", text)
    text = re.sub(r"distortion_coeffs: *\[[^\]]*\]", "distortion_coeffs: [0.0032, -0.0011, 0.0024, -0.0006]", text)
    open(p, "w").write(text)
    return os.path.join(d, "config.yaml")


def test_options_load_equidistant_camera(pkg, tmp_path):
    options = importlib.import_module("plviwo_amd.options")
    op = options.load_options(_equidistant_config(tmp_path))
    c = op.est.cam
    assert c.distortion_model[0] == "equidistant"
    assert list(c.intrinsics[0][4:]) == [0.0032, -0.0011, 0.0024, -0.0006]


class _FisheyeOracle(oc.OracleContext):
    CAMERA_MODELS = ("radtan", "equidistant")
    models = []

    def set_camera_model(self, model):
        type(self).models.append(model)


def test_driver_sets_the_model_on_a_context_that_has_it(pkg, tmp_path):
    options, system = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.system")
    cfg = _equidistant_config(tmp_path)
    _FisheyeOracle.models = []
    system.SystemManager(options.load_options(cfg), context_factory=_FisheyeOracle)
    assert _FisheyeOracle.models == ["equidistant"]
    # radtan: no call
    op = options.load_options(cfg)
    op.est.cam.distortion_model[0] = "radtan"
    _FisheyeOracle.models = []
    system.SystemManager(op, context_factory=_FisheyeOracle)
    assert _FisheyeOracle.models == []
    # the CPU oracle has no fisheye model: refused before the context is built, "radtan" in the message
    with pytest.raises(options.OptionsError, match="radtan"):
        system.SystemManager(options.load_options(cfg), context_factory=oc.OracleContext)
    # a model nobody builds
    op = options.load_options(cfg)
    op.est.cam.distortion_model[0] = "double_sphere"
    with pytest.raises(options.OptionsError, match="double_sphere"):
        system.SystemManager(op, context_factory=_FisheyeOracle)


def test_library_context_declares_the_models(pkg):
    assert pkg.Context.CAMERA_MODELS == ("radtan", "equidistant")
    assert pkg.PLV_CAM_RADTAN == 0 and pkg.PLV_CAM_EQUIDISTANT == 1
