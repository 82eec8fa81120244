"""The zero-velocity updater on the GPU against its numpy restatement (zupt_cases.py): the 9 x 12 system of plv_zupt_system against
the closed form, plv_zupt_update (gate + EKF update on the resident covariance) against the FULL stack compressed by SVD and applied
to a dense P, the exits that must leave P as it was, plv_db_disparity against numpy, and the detector of plv_zupt_try_update over
the eight combinations of its three inputs.

Bounds: the system to 1e-12 relative (H against its largest entry; a residual against the largest term that enters it: it is a
difference c (a_bar - ba - R g) of terms c |g| ~ 5e3 whose fp64 spacing alone is 1e-12), chi2 to 1e-9 relative, P to 1e-9 of its
largest entry, dx to 1e-8: the bounds test_gpu_wheel.py / test_gpu_between_frames.py hold the wheel and landmark updates to."""
import numpy as np
import pytest

import zupt_cases as zc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zx(pkg):
    c = pkg.Context(pkg.default_config(752, 480))
    yield c
    c.close()


def _args(pkg, c, **opt):
    o = dict(chi2_mult=c["chi2_mult"], noise_mult=c["noise_mult"], sigma_v=c["sigma_v"])
    o.update(opt)
    imu = pkg.PlvImuState.make(c["q"], [0.3, -0.2, 0.1], c["v"], c["bg"], c["ba"], q_fej=c["q_fej"])
    return pkg.zupt_options(**o), imu, pkg.imu_noise(sigma_w=zc.SIGMA_W, sigma_a=zc.SIGMA_A, gravity=tuple(zc.GRAVITY))


def _update(pkg, zx, c, force=False, **opt):
    o, imu, noise = _args(pkg, c, **opt)
    return zx.zupt_update(o, imu, noise, c["t"], c["wm"], c["am"], c["size"], imu_id=c["imu_id"], force=force)


def test_system_is_the_closed_form(pkg, zx):
    worst_H = worst_r = 0.0
    for c in zc.cases():
        o, imu, noise = _args(pkg, c)
        H, res, cols = zx.zupt_system(o, imu, noise, c["t"], c["wm"], c["am"], imu_id=c["imu_id"])
        Hk, rk, scale = zc.closed_form(c)
        assert np.array_equal(cols, zc.columns(c["imu_id"])), c["name"]
        assert np.array_equal(H == 0.0, Hk == 0.0), c["name"]          # the pattern itself: exact zeros where the stack has none
        eH, er = np.abs(H - Hk).max() / max(1.0, np.abs(Hk).max()), (np.abs(res - rk) / scale).max()
        worst_H, worst_r = max(worst_H, eH), max(worst_r, er)
        assert eH < 1e-12 and er < 1e-12, (c["name"], eH, er)
    print(f"plv_zupt_system against the closed form: H {worst_H:.3g}, res {worst_r:.3g} (relative)")


def test_update_is_the_update_of_the_full_stack(pkg, zx):
    """every case of the matrix: the same chi-square, the same verdict, the same posterior and correction as the stack compressed by
    SVD on a dense P; a rejection leaves P bit for bit and dx zero"""
    w_chi = w_P = w_dx = w_dx_rel = 0.0
    for c in zc.cases():
        P = c["P"]
        zx.cov_upload(P)
        rc, chi2, acc, dx = _update(pkg, zx, c)
        Pd = zx.cov_download(c["size"])
        e_chi = abs(chi2 - c["chi2"]) / c["chi2"]
        w_chi = max(w_chi, e_chi)
        assert rc == 0 and e_chi < 1e-9, (c["name"], chi2, c["chi2"])
        assert bool(acc) == c["accepted"], (c["name"], chi2)
        if c["accepted"]:
            e_P = np.abs(Pd - c["P_new"]).max() / np.abs(P).max()
            e_dx = np.abs(dx - c["dx"]).max()
            w_P, w_dx, w_dx_rel = max(w_P, e_P), max(w_dx, e_dx), max(w_dx_rel, e_dx / np.abs(c["dx"]).max())
            assert e_P < 1e-9, (c["name"], e_P)
            assert e_dx < 1e-8 * max(1.0, np.abs(c["dx"]).max()), (c["name"], e_dx)
            assert e_dx < 1e-6 * np.abs(c["dx"]).max(), (c["name"], e_dx)      # (a dx of 1e-4 held to a fraction of itself as well)
        else:
            assert not dx.any() and np.array_equal(Pd, P), c["name"]
    print(f"plv_zupt_update against the full stack: chi2 {w_chi:.3g} relative, P {w_P:.3g} of max |P|, dx {w_dx:.3g} absolute "
          f"({w_dx_rel:.3g} of max |dx|)")


def _pick(motion, accepted, **kw):
    return next(c for c in zc.cases() if c["motion"] == motion and c["accepted"] == accepted and all(c[k] == v for k, v in kw.items()))


def test_force_applies_what_the_gate_rejects(pkg, zx):
    for motion in ("turning", "moving"):
        c = _pick(motion, False)
        zx.cov_upload(c["P"])
        rc, chi2, acc, dx = _update(pkg, zx, c)
        assert rc == 0 and acc == 0 and np.array_equal(zx.cov_download(c["size"]), c["P"])
        rc, chi2_f, acc, dx = _update(pkg, zx, c, force=True)
        assert rc == 0 and acc == 1 and chi2_f == chi2
        chi_ref, _, dx_ref, P_ref = zc.reference_update(c, force=True)
        assert abs(chi2_f - chi_ref) < 1e-9 * chi_ref
        assert np.abs(dx - dx_ref).max() < 1e-8 * max(1.0, np.abs(dx_ref).max())
        assert np.abs(zx.cov_download(c["size"]) - P_ref).max() < 1e-9 * np.abs(c["P"]).max()


def test_refused_calls_leave_the_covariance(pkg, zx):
    """PLV_E_BADARG (n < 2, times that do not increase, a sigma or noise_mult that is not positive, an IMU block outside the state) and
    PLV_E_NUMERIC (a sample that is not finite): P bit for bit as it was"""
    c = _pick("standing", True, n=65)
    P, n = c["P"], c["size"]
    zx.cov_upload(P)
    o, imu, noise = _args(pkg, c)
    t, wm, am = c["t"], c["wm"], c["am"]

    def refused(code, opt=o, noise=noise, t=t, wm=wm, am=am, imu_id=c["imu_id"]):
        with pytest.raises(pkg.PlvError) as e:
            zx.zupt_update(opt, imu, noise, t, wm, am, n, imu_id=imu_id)
        assert e.value.code == code
        with pytest.raises(pkg.PlvError) as e:
            zx.zupt_try_update(opt, imu, noise, t, wm, am, n, 1.0, 1.1, imu_id=imu_id)
        assert e.value.code == code
        if imu_id == c["imu_id"]:
            with pytest.raises(pkg.PlvError) as e:
                zx.zupt_system(opt, imu, noise, t, wm, am, imu_id=imu_id)
            assert e.value.code == code
        assert np.array_equal(zx.cov_download(n), P)

    refused(pkg.PLV_E_BADARG, t=t[:1], wm=wm[:1], am=am[:1])
    t_bad = t.copy()
    t_bad[7] = t_bad[6]
    refused(pkg.PLV_E_BADARG, t=t_bad)
    refused(pkg.PLV_E_BADARG, t=t[::-1].copy())
    refused(pkg.PLV_E_BADARG, opt=_args(pkg, c, noise_mult=0.0)[0])
    refused(pkg.PLV_E_BADARG, opt=_args(pkg, c, sigma_v=-0.05)[0])
    refused(pkg.PLV_E_BADARG, noise=pkg.imu_noise(sigma_w=0.0))
    refused(pkg.PLV_E_BADARG, noise=pkg.imu_noise(sigma_a=-1.0))
    refused(pkg.PLV_E_BADARG, imu_id=n - 14)
    for arr, val in ((wm, np.nan), (am, np.inf)):
        bad = arr.copy()
        bad[11, 1] = val
        refused(pkg.PLV_E_NUMERIC, **({"wm": bad} if arr is wm else {"am": bad}))
    rc, chi2, acc, dx = zx.zupt_update(o, imu, noise, t, wm, am, n, imu_id=c["imu_id"])      # and the context is still usable
    assert rc == 0 and acc == 1 and abs(chi2 - c["chi2"]) < 1e-9 * c["chi2"]


def test_not_psd_leaves_the_covariance(pkg, zx):
    """A prior that is indefinite in the plane of v_x and p_x (made the way test_gpu_between_frames.py makes one: the measured
    block P[cols, cols] is healthy, so the gate passes; the update takes (h P_36)^2 / S off P_33 through the cross-covariance and
    the negative diagonal rejects it)."""
    c = dict(_pick("standing", True, n=65))
    n = 21
    P = np.eye(n) * 1e-6
    P[3, 6] = P[6, 3] = 2e-4
    P = np.asfortranarray(P)
    c.update(size=n, imu_id=0, P=P)
    chi_ref, acc_ref, _, P_ref = zc.reference_update(c)
    assert acc_ref and P_ref[3, 3] < 0                       # the reference would apply it and go indefinite
    zx.cov_upload(P)
    rc, chi2, acc, dx = _update(pkg, zx, c)
    assert rc == pkg.PLV_E_NOT_PSD and acc == 0 and not dx.any()
    assert abs(chi2 - chi_ref) < 1e-9 * chi_ref
    assert np.array_equal(zx.cov_download(n), P)
    o, imu, noise = _args(pkg, c)
    rc, res, dx = zx.zupt_try_update(o, imu, noise, c["t"], c["wm"], c["am"], n, 1.0, 1.1)
    assert rc == pkg.PLV_E_NOT_PSD and res["stationary"] == 1 and res["updated"] == 0 and not dx.any()
    assert np.array_equal(zx.cov_download(n), P)


def test_two_calls_give_the_same_bits(pkg, zx):
    for c in (_pick("standing", True, n=257), _pick("standing", True, n=66), _pick("bias_error", True)):
        o, imu, noise = _args(pkg, c)
        outs = []
        for _ in range(2):
            zx.cov_upload(c["P"])
            H, res, _ = zx.zupt_system(o, imu, noise, c["t"], c["wm"], c["am"], imu_id=c["imu_id"])
            rc, chi2, acc, dx = _update(pkg, zx, c)
            outs.append((H, res, np.array([chi2]), dx, zx.cov_download(c["size"])))
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), c["name"]


# ------------------------------------------------------------------------------------------------ disparity + detector
T_A, T_B, T_C, T_OTHER = 30.0517, 30.1517, 30.2517, 29.9517


def _fill_database(ctx, n_both=30, seed=5):
    """Tracks seen at T_A and T_B (0.2 px apart) and at T_C (6 px further); tracks seen at one of the stamps only; tracks seen at
    neither.  Returns the raw pixel coordinates of the common tracks by stamp, in ascending id."""
    rng = np.random.default_rng(seed)
    uv = {}
    ids = rng.permutation(np.arange(100, 100 + n_both + 9))      # appended in no particular order
    common = sorted(int(i) for i in ids[:n_both])
    for fid in ids[:n_both]:
        a = rng.uniform(20, 700, 2)
        b = a + rng.normal(0, 0.2, 2)
        c = b + rng.normal(0, 1.0, 2) + np.array([6.0, 0.0])
        tr = np.array([rng.uniform(20, 700, 2), a, b, c], dtype=np.float32)
        ctx.db_append_measurements(int(fid), [T_OTHER, T_A, T_B, T_C], tr, tr / 500.0)
        uv[int(fid)] = tr
    for j, fid in enumerate(ids[n_both:]):
        stamps = ([T_A], [T_B], [T_OTHER, T_A], [T_B, T_C + 0.05], [T_C], [T_OTHER], [T_OTHER, T_OTHER + 0.05], [T_A + 1e-9, T_B], [T_A, T_B - 1e-9])[j]
        tr = rng.uniform(20, 700, (len(stamps), 2)).astype(np.float32)
        ctx.db_append_measurements(int(fid), stamps, tr, tr / 500.0)
    return {T_A: np.array([uv[i][1] for i in common]), T_B: np.array([uv[i][2] for i in common]), T_C: np.array([uv[i][3] for i in common])}


def _disparity(uv0, uv1):
    d = (uv1 - uv0).astype(np.float32)
    d = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64)      # the norm in float, the statistics in double
    mean = 0.0
    for x in d:
        mean += x
    mean /= len(d)
    var = 0.0
    for x in d:
        var += (x - mean) * (x - mean)
    return mean, np.sqrt(var / (len(d) - 1)), len(d)


@pytest.fixture(scope="module")
def dbx(pkg):
    c = pkg.Context(pkg.default_config(752, 480))
    uv = _fill_database(c)
    yield c, uv
    c.close()


def test_db_disparity_is_compute_disparity(dbx):
    ctx, uv = dbx
    for t0, t1 in ((T_A, T_B), (T_A, T_C), (T_B, T_C), (T_B, T_A)):
        mean, std, n = ctx.db_disparity(t0, t1)
        m_ref, s_ref, n_ref = _disparity(uv[t0], uv[t1])
        assert n == n_ref == 30                                   # tracks at one stamp only, or at neither, do not count
        assert mean == pytest.approx(m_ref, rel=1e-13) and std == pytest.approx(s_ref, rel=1e-12)
    assert ctx.db_disparity(T_A, T_B)[0] < 0.5 < 4.0 < ctx.db_disparity(T_A, T_C)[0]
    mean, std, n = ctx.db_disparity(T_A, T_A)
    assert (mean, std) == (0.0, 0.0) and n == 33                  # (every track that has T_A)
    # fewer than two pairs: no track at the stamp, and exactly one track (id of the [T_OTHER, T_OTHER + 0.05] entry)
    assert ctx.db_disparity(T_A, 99.0) == (-1.0, -1.0, 0)
    assert ctx.db_disparity(T_OTHER, T_OTHER + 0.05) == (-1.0, -1.0, 0)
    assert ctx.db_size() == 39


@pytest.mark.parametrize("veto", (False, True))
@pytest.mark.parametrize("disparity", (False, True))
@pytest.mark.parametrize("imu", (False, True))
def test_try_update_follows_the_rule(pkg, dbx, veto, disparity, imu):
    """wheel veto x disparity x IMU: stationary = !veto && (disparity || imu); applied when stationary, forced when the disparity
    alone passed; otherwise nothing changes"""
    ctx, _ = dbx
    c = _pick("standing", True, n=65) if imu else _pick("turning", False, n=65)
    o, im, noise = _args(pkg, c)
    P, n = c["P"], c["size"]
    ctx.cov_upload(P)
    rc, res, dx = ctx.zupt_try_update(o, im, noise, c["t"], c["wm"], c["am"], n, T_A, T_B if disparity else T_C,
                                      wheel_speed_max=0.2 if veto else 0.03, imu_id=c["imu_id"])
    assert rc == 0
    assert (res["wheel_vetoed"], res["disparity_passed"], res["imu_passed"]) == (int(veto), int(disparity), int(imu)), res
    stationary = (not veto) and (disparity or imu)
    assert res["stationary"] == int(stationary) and res["updated"] == int(stationary)
    assert abs(res["chi2"] - c["chi2"]) < 1e-9 * c["chi2"] and res["chi2_threshold"] == pytest.approx(zc.Q95_9, rel=1e-9)
    assert res["speed"] == pytest.approx(np.linalg.norm(c["v"]), rel=1e-14) and res["disparity_n"] == 30
    Pd = ctx.cov_download(n)
    if stationary:
        _, _, dx_ref, P_ref = zc.reference_update(c, force=True)
        assert np.abs(dx - dx_ref).max() < 1e-8 * max(1.0, np.abs(dx_ref).max())
        assert np.abs(Pd - P_ref).max() < 1e-9 * np.abs(P).max()
    else:
        assert not dx.any() and np.array_equal(Pd, P)


def test_forced_update_on_a_decelerating_window(pkg, dbx):
    """Known limitation of the rule, pinned: the tracked points hardly move (the disparity passes), the wheels do not veto, and the
    window still holds 0.5 m/s^2 of acceleration, which the IMU test rejects by a wide margin.  The update is applied all the same,
    as upstream applies it, and it explains the acceleration with the state: the correction is the forced update of the full stack,
    and it moves the accelerometer bias and the tilt by many times their prior deviation."""
    ctx, _ = dbx
    c = _pick("accelerating", False, n=65)
    o, im, noise = _args(pkg, c)
    P, n, cols = c["P"], c["size"], zc.columns(c["imu_id"])
    ctx.cov_upload(P)
    rc, res, dx = ctx.zupt_try_update(o, im, noise, c["t"], c["wm"], c["am"], n, T_A, T_B, wheel_speed_max=0.04, imu_id=c["imu_id"])
    assert rc == 0 and (res["wheel_vetoed"], res["disparity_passed"], res["imu_passed"], res["stationary"], res["updated"]) == (0, 1, 0, 1, 1)
    assert res["chi2"] > 10 * res["chi2_threshold"]
    _, _, dx_ref, P_ref = zc.reference_update(c, force=True)
    assert np.abs(dx - dx_ref).max() < 1e-8 * max(1.0, np.abs(dx_ref).max())
    assert np.abs(ctx.cov_download(n) - P_ref).max() < 1e-9 * np.abs(P).max()
    moved = np.abs(dx[cols]) / np.sqrt(np.diag(P)[cols])          # in prior standard deviations: theta, v, bg, ba
    print("forced update on a window with 0.5 m/s^2 left in it: largest correction %.1f prior sigmas (theta %.1f, ba %.1f)"
          % (moved.max(), moved[:3].max(), moved[9:].max()))
    assert max(moved[:3].max(), moved[9:].max()) > 5.0


def test_try_update_detector_edges(pkg, dbx):
    ctx, _ = dbx
    c = _pick("standing", True, n=65)
    P, n = c["P"], c["size"]

    def run(wheel=-1.0, t1=T_C, **opt):
        o, im, noise = _args(pkg, c, **opt)
        ctx.cov_upload(P)
        rc, res, dx = ctx.zupt_try_update(o, im, noise, c["t"], c["wm"], c["am"], n, T_A, t1, wheel_speed_max=wheel, imu_id=c["imu_id"])
        assert rc == 0
        return res

    assert run(wheel=-1.0)["wheel_vetoed"] == 0 and run(wheel=-1.0, max_wheel_speed=-2.0)["wheel_vetoed"] == 0    # no wheel data: no veto
    assert run(wheel=0.05)["wheel_vetoed"] == 0 and run(wheel=0.0500001)["wheel_vetoed"] == 1                  # strictly above
    # the chi-square passes but the state's speed does not
    r = run(max_velocity=0.5 * float(np.linalg.norm(c["v"])))
    assert r["chi2"] < r["chi2_threshold"] and r["imu_passed"] == 0 and r["stationary"] == 0 and r["updated"] == 0
    # the disparity is small but on too few tracks / just at the bound
    assert run(t1=T_B, min_disparity_feats=31)["disparity_passed"] == 0 and run(t1=T_B, min_disparity_feats=30)["disparity_passed"] == 1
    m = ctx.db_disparity(T_A, T_B)[0]
    assert run(t1=T_B, max_disparity=m)["disparity_passed"] == 0                                                  # mean < max, strictly
    # no common track at all: the disparity is reported as -1 on 0 tracks and does not pass
    r = run(t1=99.0)
    assert (r["disparity_mean"], r["disparity_std"], r["disparity_n"], r["disparity_passed"]) == (-1.0, -1.0, 0, 0) and r["stationary"] == 1
