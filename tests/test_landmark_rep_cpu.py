"""In-state landmark representations without a GPU: plv_landmark_from_xyz / plv_landmark_xyz (host arithmetic of the library) against
the formulas of Landmark::set_from_xyz / get_xyz (open_vins/ov_core/src/types/Landmark.cpp:26-44, 65-101) written in numpy, and the
driver's rule for which context may be handed cam.max_slam > 0 in which representation."""
import importlib
import itertools

import numpy as np
import pytest

import oracle_context as oc
import synth_dataset as sd

EPS = np.finfo(np.float64).eps


def _points():
    rng = np.random.default_rng(5)
    pts = [np.array(s) * rng.uniform(0.3, 40.0, 3) for s in itertools.product((-1.0, 1.0), repeat=3)]   # every octant
    pts += [np.array([0.0, 0.0, 7.0]), np.array([0.0, 0.0, -7.0]), np.array([3.0, 0.0, 0.0]), np.array([0.0, -2.0, 0.0]),
            np.array([1e-3, 2e-3, 55.0]), np.array([-12.0, 1e-9, 0.4])]                                    # axes, near the pole
    return pts


def _from_xyz_numpy(p):      # Landmark.cpp:86-93
    rho = 1 / np.linalg.norm(p)
    return np.array([np.arctan2(p[1], p[0]), np.arccos(rho * p[2]), rho])


def _xyz_numpy(v):           # Landmark.cpp:39-43
    return np.array([(1 / v[2]) * np.cos(v[0]) * np.sin(v[1]), (1 / v[2]) * np.sin(v[0]) * np.sin(v[1]), (1 / v[2]) * np.cos(v[1])])


def test_representations_against_landmark_cpp(pkg):
    assert pkg.Context.LANDMARK_REPS == ("GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH")
    worst = 0.0
    for p in _points():
        # GLOBAL_3D: the value is the position
        assert np.array_equal(pkg.landmark_from_xyz("GLOBAL_3D", p), p) and np.array_equal(pkg.landmark_xyz(0, p), p)
        v = pkg.landmark_from_xyz("GLOBAL_FULL_INVERSE_DEPTH", p)
        v_np = _from_xyz_numpy(p)
        # the same handful of libm calls on both sides, each good to an ulp
        assert np.abs(v - v_np).max() <= 4 * EPS * max(1.0, np.abs(v_np).max()), (p, v, v_np)
        x = pkg.landmark_xyz(1, v)
        assert np.abs(x - _xyz_numpy(v)).max() <= 4 * EPS * np.linalg.norm(p), (p, x)
        # round trip: atan2 / acos / sqrt there, sin / cos / a division back, each good to an ulp: 8 eps |p| — away from the pole.
        # phi = acos(c) turns the half ulp of its argument c = z / |p| into eps / (2 sin phi) of angle (d acos / dc = -1 / sin phi), which
        # moves the point by |p| times that: the reference's own formula, so close to the z axis the bound carries the 1 / sin phi.
        sin_phi = np.hypot(p[0], p[1]) / np.linalg.norm(p)
        err = np.abs(x - p).max() / np.linalg.norm(p)
        bound = 8 * EPS * (1.0 if sin_phi == 0.0 or sin_phi > 0.1 else 1.0 / sin_phi)
        worst = max(worst, err / bound)
        assert err <= bound, (p, x, err / EPS)
    print(f"largest round-trip error: {worst:.3f} of its bound")


def test_unknown_representation_is_refused(pkg):
    lib = pkg.load_library()
    p, out = np.array([1.0, 2.0, 3.0]), np.full(3, -1.0)
    dp = lambda a: a.ctypes.data_as(pkg.C.POINTER(pkg.C.c_double))
    for rep in (-1, 2, 3, 4, 5, 99):          # the anchored representations of LandmarkRepresentation.h among them
        assert lib.plv_landmark_from_xyz(rep, dp(p), dp(out)) == pkg.PLV_E_BADARG
        assert lib.plv_landmark_xyz(rep, dp(p), dp(out)) == pkg.PLV_E_BADARG
        assert np.array_equal(out, [-1.0, -1.0, -1.0])
    assert lib.plv_landmark_from_xyz(1, None, dp(out)) == pkg.PLV_E_BADARG and lib.plv_landmark_xyz(1, dp(p), None) == pkg.PLV_E_BADARG
    for rep in ("ANCHORED_3D", "ANCHORED_MSCKF_INVERSE_DEPTH", 7):
        with pytest.raises(pkg.PlvError):
            pkg.landmark_from_xyz(rep, p)
        with pytest.raises(pkg.PlvError):
            pkg.landmark_xyz(rep, p)


def test_driver_landmark_holds_value_and_representation(pkg):
    system = importlib.import_module("plviwo_amd.system")
    p = np.array([-3.0, 4.0, 12.0])
    for rep in (0, 1):
        lm = system.Landmark(17, p, 40, rep)
        assert (lm.featid, lm.id, lm.rep) == (17, 40, rep)
        assert np.array_equal(lm.value, pkg.landmark_from_xyz(rep, p)) and np.array_equal(lm.fej, lm.value)
        assert np.abs(lm.p - p).max() <= 8 * EPS * np.linalg.norm(p) and np.abs(lm.p_fej - p).max() <= 8 * EPS * np.linalg.norm(p)
        lm.value = lm.value + np.array([1e-3, -2e-3, 5e-4])       # what State.apply does with dx
        assert np.array_equal(lm.p, pkg.landmark_xyz(rep, lm.value)) and np.array_equal(lm.p_fej, pkg.landmark_xyz(rep, lm.fej))


def test_driver_refuses_a_representation_only_without_the_passes(pkg, tmp_path):
    """cam.max_slam > 0 in GLOBAL_FULL_INVERSE_DEPTH: refused for a context class without LANDMARK_REPS (the per-landmark loop is
    GLOBAL_3D only), taken for one that has it — and refused again when the passes are switched off."""
    options, system = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.system")
    d = str(tmp_path / "data")
    sd.make_dataset(d, seconds=0.3, cam_hz=10.0)
    cfg = sd.write_config(str(tmp_path / "config"), d, str(tmp_path / "traj.txt"))

    class WithReps(oc.OracleContext):
        LANDMARK_REPS = pkg.Context.LANDMARK_REPS

    def options_with(rep):
        op = options.load_options(cfg)
        op.est.cam.max_slam, op.est.cam.feat_rep, op.est.cam.use_lines = 5, rep, False
        return op

    assert not hasattr(oc.OracleContext, "LANDMARK_REPS")
    with pytest.raises(options.OptionsError, match="GLOBAL_3D representation only"):
        system.SystemManager(options_with(1), context_factory=oc.OracleContext)
    system.SystemManager(options_with(0), context_factory=oc.OracleContext)
    system.SystemManager(options_with(1), context_factory=WithReps)
    system.SystemManager(options_with(0), context_factory=WithReps)

    class LoopOnly(system.SystemManager):
        slam_pass = False

    with pytest.raises(options.OptionsError, match="GLOBAL_3D representation only"):
        LoopOnly(options_with(1), context_factory=WithReps)
