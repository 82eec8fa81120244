"""The equidistant (fisheye) camera model on the device: plv_set_camera_model(ctx, PLV_CAM_EQUIDISTANT) reaches the undistortion
(plv_undistort, the LK tail of the tracker), the point Jacobians (unfused and fused launches) and the triangulation's reprojection
error.  The CPU oracle has no fisheye model, so the model is anchored to the numpy restatement of CamEqui (tests/cam_equi.py) and to
the radtan path with zero distortion, whose dz/dzn is exactly diag(fx, fy)."""
import importlib
import os

import numpy as np
import pytest

import cam_equi
import synth
import synth_fisheye as sf

pytestmark = pytest.mark.gpu

W, H = 752, 480
MILD = np.array([350.0, 351.5, 376.25, 239.5, 3.2e-3, -1.1e-3, 2.4e-3, -6.0e-4])       # TUM-VI-like
STRONG = np.array([350.0, 348.0, 370.0, 245.0, -0.35, 0.12, -0.03, 0.004])


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _newton_steps(K8, uv):
    """Newton steps cv::fisheye::undistortPoints runs for one pixel (to show the strong set reaches the cap of 10)."""
    fx, fy, cx, cy, k1, k2, k3, k4 = K8
    pw = np.array([(uv[0] - cx) / fx, (uv[1] - cy) / fy])
    theta_d = min(np.hypot(*pw), np.pi / 2)
    theta = theta_d
    for j in range(10):
        t2 = theta * theta
        fix = (theta * (1 + k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4) - theta_d) / \
              (1 + 3 * k1 * t2 + 5 * k2 * t2 ** 2 + 7 * k3 * t2 ** 3 + 9 * k4 * t2 ** 4)
        theta -= fix
        if abs(fix) < 1e-8:
            return j + 1
    return 10


def _model_ctx(pkg, K8, model="equidistant"):
    ctx = pkg.Context(pkg.default_config(W, H))
    ctx.set_camera_intrinsics(K8)
    ctx.set_camera_model(model)
    return ctx


@pytest.mark.parametrize("name,K8", [("mild", MILD), ("strong", STRONG)])
def test_undistort_matches_restatement(pkg, name, K8):
    gx, gy = np.meshgrid(np.linspace(0, W - 1, 95), np.linspace(0, H - 1, 61))
    pts = [np.stack([gx.ravel(), gy.ravel()], 1), K8[None, 2:4],                            # dense grid, the exact principal point
           np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]),                      # corners
           K8[None, 2:4] + np.array([[700.0, 0.0], [-650.0, 400.0], [0.0, -900.0]])]         # past pi/2: the clamp
    uv = np.concatenate(pts).astype(np.float32)
    ctx = _model_ctx(pkg, K8)
    got = ctx.undistort(uv)
    want = cam_equi.undistort(K8, uv)
    d = _ulps(got, want)
    print(f"{name}: {int((d > 0).any(axis=1).sum())} of {len(uv)} points not identical, max {int(d.max())} ulp")
    assert d.max() <= 1
    assert np.array_equal(got[len(pts[0])], np.zeros(2, np.float32))                         # theta_d <= 1e-8: scale 1
    steps = np.array([_newton_steps(K8, p) for p in uv[:len(pts[0])]])
    if name == "strong":
        assert steps.max() == 10
    # round trip inside the valid field of view: theta_d below the largest value theta_d(theta) reaches for theta < pi/2 (the strong
    # set peaks at 0.89; beyond, a pixel has no preimage and the 10 Newton steps wander)
    t = np.linspace(0.0, np.pi / 2, 4001)
    td_max = (t * (1 + K8[4] * t ** 2 + K8[5] * t ** 4 + K8[6] * t ** 6 + K8[7] * t ** 8)).max()
    inside = np.hypot(*((uv[:len(pts[0])] - K8[2:4]) / K8[:2]).T) < min(0.98 * td_max, 1.3)
    assert inside.sum() > 0.5 * len(inside)
    back = cam_equi.distort(K8, got[:len(pts[0])][inside])
    assert np.abs(back.astype(np.float64) - uv[:len(pts[0])][inside]).max() < 1e-3
    # radtan stays what it was on the same context
    ctx.set_camera_model("radtan")
    ref = pkg.Context(pkg.default_config(W, H))
    ref.set_camera_intrinsics(K8)
    assert np.array_equal(ctx.undistort(uv), ref.undistort(uv))
    ctx.close()
    ref.close()


def test_tracker_obs_uvn_follow_the_model(pkg):
    """plv_tracker_feed on frames rendered through the fisheye camera of tests/synth_fisheye.py: every observation's obs_uvn is the
    model applied to its obs_uv (LK tail and detection path); with the model left at radtan they differ."""
    times = 0.1 + 0.1 * np.arange(5)
    frames = sf.render_frames(times)
    runs = {}
    for model in ("equidistant", "radtan"):
        ctx = _model_ctx(pkg, sf.K8, model)
        for t, img in zip(times, frames):
            ctx.tracker_feed(float(t), img)
        pts, ids = ctx.tracker_last()
        assert len(ids) > 100
        ptr, _, uv, uvn = ctx.db_export(ids)
        runs[model] = (uv, uvn)
        ctx.close()
    uv, uvn = runs["equidistant"]
    assert len(uv) > 300
    assert _ulps(uvn, cam_equi.undistort(sf.K8, uv)).max() <= 1
    # with the model left at radtan (k1..k4 then read as k1 k2 p1 p2), the same frames give normalised points that are not the
    # fisheye ones (the RANSAC inliers, hence the tracks, differ too)
    uv_r, uvn_r = runs["radtan"]
    assert np.abs(uvn_r - cam_equi.undistort(sf.K8, uv_r)).max() > 1e-3


def _equi_scene(pkg, K8, calib=True, noise_px=0.4):
    """synth.vio_scene's geometry with fisheye observations, residual poses at the observation times, extrinsics / intrinsics / dt
    calibrated (state layout IMU | intrinsics | clones | extrinsics | dt)."""
    sc = synth.vio_scene(F=40, M=12, noise_px=0.0, seed=21)
    rng = np.random.default_rng(8)
    res_R, res_p, uvn = [], [], []
    for o, tm in enumerate(sc["obs_time"]):
        R, p = sc["pose_fn"](tm)
        res_R.append(R)
        res_p.append(p)
    sc["res_R"], sc["res_p"] = np.array(res_R), np.array(res_p)
    uv = []
    for f in range(len(sc["obs_ptr"]) - 1):
        for o in range(sc["obs_ptr"][f], sc["obs_ptr"][f + 1]):
            pc = sc["R_ItoC"] @ (sc["res_R"][o] @ (sc["pts"][f] - sc["res_p"][o])) + sc["p_IinC"]
            uvn.append(pc[:2] / pc[2])
    uvn = np.array(uvn)
    sc["uvn"] = uvn
    sc["obs_uv"] = (cam_equi.distort(K8, uvn) + rng.normal(0, noise_px, uvn.shape)).astype(np.float32)
    n = sc["n_state"]
    kw = dict(extrinsic_state_id=n, dt_state_id=n + 6) if calib else {}
    return sc, kw


def _views(pkg, sc, K8, kw):
    st = pkg.StateView(sc["t"], sc["R"], sc["p"], sc["ids"], sc["R_ItoC"], sc["p_IinC"], K8, clone_R_fej=sc["Rf"], clone_p_fej=sc["pf"],
                       intrinsic_state_id=sc["intr_id"], sigma_pix=1.5, use_pol_cov=0, **kw)
    tr = pkg.Tracks(sc["obs_ptr"], sc["obs_time"], sc["obs_uv"], sc["pts"], res_R=sc["res_R"], res_p=sc["res_p"])
    return st, tr


def test_jacobians_identity_against_radtan(pkg):
    K8 = MILD
    K0 = np.concatenate([K8[:4], np.zeros(4)])
    sc, kw = _equi_scene(pkg, K8)
    st_e, tr = _views(pkg, sc, K8, kw)
    st_r, _ = _views(pkg, sc, K0, kw)
    ctx = pkg.Context(pkg.default_config(W, H))
    cols = ctx.jacobian_columns(st_e, tr)
    assert np.array_equal(cols, ctx.jacobian_columns(st_r, tr))
    ld = 2 * 12
    rows_r, Hf_r, Hx_r, res_r = ctx.build_jacobians(st_r, tr, cols, ld)
    ctx.set_camera_model("equidistant")
    rows_e, Hf_e, Hx_e, res_e = ctx.build_jacobians(st_e, tr, cols, ld)
    ctx.close()
    assert np.array_equal(rows_r, rows_e) and rows_e.sum() > 0
    intr = [j for j, c in enumerate(cols) if 15 <= c < 23]
    other = [j for j in range(len(cols)) if j not in intr]
    assert len(intr) == 8 and len(other) > 6
    dzn, dzeta = cam_equi.distort_jacobian(K8, sc["uvn"])
    d_uv = cam_equi.distort(K8, sc["uvn"]).astype(np.float64)
    sigma = 1.5
    S = np.diag([1 / K8[0], 1 / K8[1]])
    ptr = sc["obs_ptr"]
    for f in range(len(ptr) - 1):
        m = ptr[f + 1] - ptr[f]
        assert rows_e[f] == 2 * m
        for c in range(m):
            o = ptr[f] + c
            A = dzn[o] @ S
            r = slice(2 * c, 2 * c + 2)
            hf_want = A @ Hf_r[f][:, r].T
            assert np.abs(Hf_e[f][:, r].T - hf_want).max() <= 1e-10 * np.abs(Hf_e[f]).max()
            hx_e, hx_r = Hx_e[f][:, r].T, Hx_r[f][:, r].T
            assert np.abs(hx_e[:, other] - A @ hx_r[:, other]).max() <= 1e-10 * np.abs(hx_e[:, other]).max()
            assert np.abs(hx_e[:, intr] - dzeta[o] / sigma).max() <= 1e-10 * np.abs(dzeta[o]).max() / sigma
            want = (sc["obs_uv"][o].astype(np.float64) - d_uv[o]) / sigma
            ulp = np.spacing(np.abs(d_uv[o]).astype(np.float32)).astype(np.float64) / sigma
            assert (np.abs(res_e[f][r] - want) <= ulp + 1e-12).all(), (f, c, res_e[f][r], want)


def test_triangulation_reprojection_error(pkg):
    K8 = MILD
    sc, kw = _equi_scene(pkg, K8, calib=False, noise_px=0.6)
    st, _ = _views(pkg, sc, K8, kw)
    ctx = pkg.Context(pkg.default_config(W, H))
    ctx.set_camera_model("equidistant")
    uvn = cam_equi.undistort(K8, sc["obs_uv"])
    tr = pkg.Tracks(sc["obs_ptr"], sc["obs_time"], sc["obs_uv"], np.zeros_like(sc["pts"]), res_R=sc["res_R"], res_p=sc["res_p"],
                    obs_uvn=uvn)
    p, ok, err = ctx.triangulate(st, tr, max_dist=500.0, max_cond=1e9, max_baseline=1e4)   # (the gates are not under test)
    ctx.close()
    assert ok.sum() >= 0.9 * len(ok)
    ptr = sc["obs_ptr"]
    for f in np.nonzero(ok)[0]:
        e = []
        for o in range(ptr[f], ptr[f + 1]):
            pc = sc["R_ItoC"] @ (sc["res_R"][o] @ (p[f] - sc["res_p"][o])) + sc["p_IinC"]
            d = cam_equi.distort(K8, pc[:2] / pc[2])[0].astype(np.float64)
            e.append(np.hypot(*(sc["obs_uv"][o].astype(np.float64) - d)))
        assert abs(err[f] - np.mean(e)) <= 1e-6, (f, err[f], np.mean(e))
    assert 0.1 < np.median(err[ok > 0]) < 3.0


def test_fused_path_matches_composition(pkg):
    """The fused build + null-space projection launch (jacobian_nullspace_kernel) under the equidistant model against the host
    systems of the unfused build and the general update (the pattern of test_gpu_jacobian::test_fused_build_project_paths_agree)."""
    K8 = MILD
    sc, kw = _equi_scene(pkg, K8, calib=True, noise_px=0.4)
    sc["res_R"] = sc["res_p"] = None
    st, _ = _views(pkg, sc, K8, kw)
    tr = pkg.Tracks(sc["obs_ptr"], sc["obs_time"], sc["obs_uv"], sc["pts"])
    n = sc["n_state"] + 7
    P = synth.spd_cov(n, seed=4) * 1e-4
    ctx = pkg.Context(pkg.default_config(W, H))
    ctx.set_camera_model("equidistant")
    cols = ctx.jacobian_columns(st, tr)
    s2 = 1.5 ** 2
    rows, Hf, Hx, res = ctx.build_jacobians(st, tr, cols, 30)
    rc_a, P_a, dx_a, acc_a, nr_a = ctx.msckf_update(P, rows, Hf, Hx, res, cols, s2)
    assert rc_a == 0 and acc_a.sum() > 20
    ctx.cov_upload(P)
    ctx.build_jacobians_resident(st, tr, cols, 30)
    rc_b, dx_b, acc_b, nr_b = ctx.msckf_update_resident(n, s2)
    P_b = ctx.cov_download(n)
    ctx.close()
    assert rc_b == 0 and np.array_equal(acc_b, acc_a) and nr_b == nr_a
    assert np.abs(dx_b - dx_a).max() <= 1e-9 * max(1.0, np.abs(dx_a).max())
    assert np.abs(P_b - P_a).max() <= 1e-9 * np.abs(P_a).max()


def test_vanishing_points_keep_the_radtan_formula(pkg):
    """LineHelper::Distort applies radtan whatever the model (its fisheye branch is commented out).  plv_vanishing_points takes no
    context, hence no model: it is the radtan formula on the 8 intrinsics it is given, which under the equidistant model are
    k1..k4 read as k1 k2 p1 p2.  The tracker's line classification gets its vanishing points from this function on the state's
    intrinsics (tracker_api.hip, plv_camera_frame), so this pins the value it uses; the end-to-end replay below runs that path."""
    ctx = _model_ctx(pkg, STRONG)
    R = synth._exp_so3(np.array([0.1, -0.3, 0.05]))
    got = ctx.vanishing_points(R, STRONG)
    ctx.close()
    K = STRONG
    want = np.zeros((3, 2))
    for a in range(3):
        x, y = R[0, a], R[1, a]                           # column a, no division by z (LineHelper.cpp:1037-1046)
        r = np.sqrt(x * x + y * y)
        r2 = r * r
        x1 = x * (1 + K[4] * r2 + K[5] * r2 * r2) + 2 * K[6] * x * y + K[7] * (r2 + 2 * x * x)
        y1 = y * (1 + K[4] * r2 + K[5] * r2 * r2) + K[6] * (r2 + 2 * y * y) + 2 * K[7] * x * y
        want[a] = np.float32(K[0] * x1 + K[2]), np.float32(K[1] * y1 + K[3])
    want[2, 1] *= 1000
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def fisheye_dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("synthetic_fisheye"))
    return sf.make_dataset(d, seconds=8.0)


def _replay(pkg, dataset, cfg_dir, model):
    options, rp = importlib.import_module("plviwo_amd.options"), importlib.import_module("plviwo_amd.replay")
    traj = os.path.join(cfg_dir, "out", "traj.txt")
    op = options.load_options(sf.write_config(cfg_dir, dataset, traj, model=model))
    stats, times, poses = rp.replay(op)
    ctx = pkg.Context(pkg.default_config(W, H))
    et, ep = pkg.traj_load(traj)[:2]
    gt_t, gt_p = pkg.traj_load(os.path.join(dataset, "gt.txt"))[:2]
    ei, gi = pkg.traj_associate(et, gt_t)
    r = ctx.traj_ate(ep[ei], gt_p[gi], "posyaw")
    ctx.close()
    return stats, r["pos"]["rmse"], len(ei)


def test_fisheye_drive_replays_to_an_ate(pkg, fisheye_dataset, tmp_path):
    """The synthetic drive (camera, IMU, wheel, lines) rendered through an equidistant camera, replayed through the driver from its
    Kalibr-style config files: it initialises, updates and tracks to the radtan replay tests' bound.  The same data with the YAML
    saying radtan (same fx fy cx cy, zero coefficients) is clearly worse: the data really are fisheye."""
    stats, ate, n = _replay(pkg, fisheye_dataset, str(tmp_path / "equidistant"), "equidistant")
    frac = stats["cam_accepted"] / max(stats["cam_features"], 1)
    print(f"equidistant: ATE {ate:.4f} m over {n} poses, accepted {stats['cam_accepted']} / {stats['cam_features']} ({frac:.3f}), "
          f"{stats['cam_updates']} updates, lines tracked {stats['lines_tracked']}")
    assert stats["initialized"] and stats["frames"] == 80 and stats["not_psd"] == 0
    assert stats["cam_updates"] >= 60 and stats["wheel_accepted"] >= 60 and stats["lines_tracked"] > 0
    assert n >= 70
    assert ate < 0.10
    fstats, fate, _ = _replay(pkg, fisheye_dataset, str(tmp_path / "false_radtan"), "radtan")
    ffrac = fstats["cam_accepted"] / max(fstats["cam_features"], 1)
    print(f"false radtan: ATE {fate:.4f} m, accepted {fstats['cam_accepted']} / {fstats['cam_features']} ({ffrac:.3f})")
    assert ffrac < frac - 0.05 or fate > 1.5 * ate
