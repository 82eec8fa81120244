"""What the case matrix of the between-frame path (tests/between_frame_cases.py) must contain, asserted on the CPU oracle alone: no case
of tests/test_gpu_between_frames.py can pass vacuously.  Every case is finite on the oracle; every IMU stream sits, step by step, on
the side of the CPI small-rotation threshold it claims; the duplicated stamp really reaches the selected window; the clone /
marginalise shapes include the first one that strides; the landmark systems initialise, the rejections reject for the reason they
name (the revert case passes initialize_invertible and fails in the update); the wheel covariance is positive definite for the 3D
types and exactly singular for the 2D types at standstill; the wheel updates decide both ways."""
import numpy as np
import pytest

import between_frame_cases as bf
import oracle_lib
import synth


@pytest.fixture(scope="module")
def po(pkg):
    return oracle_lib.load_prop(pkg)


def _finite(*xs):
    return all(np.isfinite(np.asarray(x)).all() for x in xs)


def test_every_axis_value_occurs():
    cases = bf.PROP_CASES
    assert len({c.name for c in cases}) == len(cases)
    shapes = {(c.n, c.imu_id) for c in cases}
    assert {(15, 0), (16, 0), (16, 1), (17, 0), (18, 0), (45, 30), (63, 12), (119, 0), (149, 0), (205, 15)} <= shapes
    for m in bf.MOTIONS:
        assert sum(c.motion == m for c in cases) >= 2, m
        assert any(c.motion == m and c.n >= 119 for c in cases) and any(c.motion == m and c.n <= 63 for c in cases), m
    for s in (2, 41, 400):
        assert sum(c.samples == s for c in cases) >= 2
    assert all(c.jitter for c in cases if c.samples == 400)
    assert sum(c.lin_bias for c in cases) >= 4 and {c.motion for c in cases if c.lin_bias} >= {"turning", "straight", "mixed", "above", "tiny"}
    assert all(c.samples - 1 >= 20 for c in bf.CARRIED_CASES) and any(c.lin_bias for c in bf.CARRIED_CASES)
    assert {(15, 0, 6), (45, 15, 6), (40, 39, 1), (60, 20, 8), (123, 0, 6), (199, 15, 6)} <= set(bf.CLONE_CASES)
    m = bf.MARG_CASES
    assert {s for _, _, s in m} == {1, 3, 6, 8} and {128, 129, 200} <= {n - s for n, _, s in m}
    for rows_out in (128, 129, 200):       # each stride shape with the block first, inside and last
        sub = [(n, i, s) for n, i, s in m if n - s == rows_out]
        assert any(i == 0 for _, i, _ in sub) and any(i + s == n for n, i, s in sub) and any(0 < i and i + s < n for n, i, s in sub)
    assert max(n + s for n, _, s in bf.CLONE_CASES) <= bf.CAPACITY
    si = bf.SLAM_INIT_CASES
    assert {c.rows for c in si} >= {4, 5, 19, 20, 35, 36, 46, 66} and bf.SLAM_OVER.rows == 67
    assert {c.k for c in si} >= {15, 16, 17, 98, 128, 129, 192} and {c.n for c in si} == {40, 143, 199}
    wu = bf.WHEEL_UPDATE_CASES
    assert {c.kind for c in wu} == set(range(6)) and {c.n for c in wu} == {39, 119, 149}
    for flag in range(3):
        assert sum(c.calib[flag] for c in wu) >= 2 and sum(not c.calib[flag] for c in wu) >= 2
    assert any(abs(c.pose_ids[0] - c.pose_ids[1]) == 6 for c in wu) and any(abs(c.pose_ids[0] - c.pose_ids[1]) > 60 for c in wu)
    for kind in (3, 4, 5):
        assert any(c.kind == kind and c.motion == "standstill" for c in wu) and any(c.kind == kind and c.motion == "creeping" for c in wu)


@pytest.mark.parametrize("case", bf.PROP_CASES + bf.CARRIED_CASES, ids=lambda c: c.name)
def test_imu_case_is_finite_and_on_its_side(pkg, po, case):
    t, wm, am, imu, bw, ba = bf.imu_case(pkg, case)
    assert len(t) == case.samples and (np.diff(t) > 5e-4).all()        # no repeated stamp: EKFPropagation divides by dt
    w = bf.w_hat_norms(wm, bw)
    for i, side in enumerate(bf.claimed_side(case, len(w))):
        if side is not None:
            assert (w[i] < bf.CPI_SMALL_W) == side, (i, w[i])
    if case.motion in ("below", "above", "mixed"):                     # ... and next to the threshold, not far from it
        assert np.abs(w - bf.CPI_SMALL_W).max() < 3e-5
    if case.motion == "turning":
        assert (w > 0.4).all()
    if case.motion == "tiny":                                          # below both limits of the SO(3) helpers
        assert (np.diff(t) * w < 1e-7).all() and (w > 0).all()
    if case.motion == "standing":                                      # the Jacobian's Jl(dt (wm - bg)) sees an exact zero
        assert not (wm - np.array(bf.BG)).any()
    if case.lin_bias:
        assert np.abs(bw - np.array(imu.bg)).max() > 1e-4 and np.abs(ba - np.array(imu.ba)).max() > 1e-3
    acc = bf.make_acc(po.reset_cpi, imu, case)
    P = synth.spd_cov(case.n, seed=2) * 1e-3
    Phi, Qd, rec, P1 = po.propagate(imu, pkg.imu_noise(), t, wm, am, P=P, acc=acc, imu_id=case.imu_id)
    assert _finite(Phi, Qd, P1, imu.vec(), acc.P_meas, acc.alpha_tau, acc.R_k2tau) and len(rec) == case.samples - 1
    assert all(_finite(r.Q, r.alpha, r.v, r.R_I0toIk) for r in rec)
    assert np.abs(Qd).max() > 0 and np.abs(np.array(acc.P_meas)).max() > 0


@pytest.mark.parametrize("c", bf.CPI_CASES, ids=lambda c: c.name)
def test_cpi_case_windows_and_the_duplicate(pkg, po, c):
    nz = pkg.imu_noise()
    t, wm, am, Rc, vc, tq = bf.cpi_case(pkg, c)
    ok, r = po.cpi_integrate(nz, tq, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t, wm, am)
    assert ok and _finite(r.Q, r.alpha, r.v, r.R_I0toIk) and r.dt == tq - bf.CLONE_T
    lo, hi = min(tq, bf.CLONE_T), max(tq, bf.CLONE_T)
    sel = po.select_imu_readings(t, wm, am, lo, hi)[1]
    assert (len(sel) == 2) == (c.kind == "two-samples")
    if c.kind != "two-samples":
        at = bf.duplicate_index(t, lo, hi)
        t2, w2, a2 = bf.with_duplicate(t, wm, am, at)
        sel2 = po.select_imu_readings(t2, w2, a2, lo, hi)[1]
        assert len(sel2) == len(sel) + 1 and (np.diff(sel2) == 0).sum() == 1          # the delta_t == 0 branch is reached
        ok2, r2 = po.cpi_integrate(nz, tq, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t2, w2, a2)
        assert ok2 and bf.records_equal(r, r2)
    assert not po.cpi_integrate(nz, bf.CLONE_T, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t, wm, am)[0]


def test_clone_and_marginalise_references(pkg, po, oracle):
    for n, src, size in bf.CLONE_CASES:
        P = bf.tagged(n)
        P2 = po.cov_clone(P, src, size)
        assert np.array_equal(P2, bf.clone_ref(P, src, size))
        assert np.array_equal(oracle.cov_marginalize(P2, n, size), P)
    for n, idx, size in bf.MARG_CASES:
        P = bf.tagged(n)
        assert np.array_equal(oracle.cov_marginalize(P, idx, size), bf.marg_ref(P, idx, size))
    P = bf.tagged(7)
    assert not np.array_equal(P, P.T) and len(np.unique(P)) == 49


def test_landmark_cases_initialise_and_the_rejections_reject_for_their_reason(oracle):
    q95 = synth.q95_table()
    for c in bf.SLAM_INIT_CASES + [bf.SLAM_OVER]:
        P, cols, Hf, Hx, res = bf.landmark_system(c)
        ok, P2, dxi, dx = oracle.slam_initialize(P, Hf, Hx, res, cols, q95, chi2_mult=5.0)
        assert ok == 1 and _finite(P2, dxi, dx) and dx.any(), c
    c = bf.SLAM_INIT_CASES[2]
    P, cols, Hf, Hx, res = bf.landmark_system(c)
    assert oracle.slam_initialize(P, bf.rank_deficient(Hf), Hx, res, cols, q95, chi2_mult=5.0)[0] == 0
    assert np.linalg.matrix_rank(bf.rank_deficient(Hf)) == 2
    # Hf scaled down: the Givens angles, the updating rows and their gate stay as they are; H_L^-1 grows 1e3, P_LL 1e6 > 1000
    assert oracle.slam_initialize(P, Hf * 1e-3, Hx, res, cols, q95, chi2_mult=5.0)[0] == 0
    # the revert: dx_init is written after initialize_invertible accepted and before the update that fails
    P, cols, Hf, Hx, res = bf.revert_system()
    ok, _, dxi, dx = oracle.slam_initialize(P, Hf, Hx, res, cols, q95, chi2_mult=5.0)
    assert ok == 0 and dxi.any() and not dx.any()
    assert np.linalg.eigvalsh(P).min() < 0 and np.linalg.eigvalsh(P[np.ix_(cols, cols)]).min() > 0
    Ph = P.copy()
    Ph[0, 1] = Ph[1, 0] = 0.0                # the same system on a healthy prior goes through
    ok, _, dxi_h, _ = oracle.slam_initialize(Ph, Hf, Hx, res, cols, q95, chi2_mult=5.0)
    assert ok == 1 and np.array_equal(dxi_h, dxi)
    for rows in (2, 63):
        P, cols, H, res = bf.slam_update_system(143, 98, rows, 40 + rows)
        rc, P1, acc, dx = oracle.slam_update(P, H, res, cols, q95, chi2_mult=5.0)
        assert rc == 0 and acc == 1 and _finite(P1, dx)
    P, cols, H, res = bf.slam_update_system(143, 98, 1, 41)       # a single row is skipped, however well it fits (UpdaterCamera.cpp:313-316)
    rc, P1, acc, dx = oracle.slam_update(P, H, res, cols, q95, chi2_mult=5.0)
    assert rc == 0 and acc == 0 and not dx.any() and np.array_equal(P1, P)
    assert float(res[0] ** 2 / (H[0] @ P[np.ix_(cols, cols)] @ H[0] + 1.0)) < q95[1]


@pytest.mark.parametrize("motion", bf.WHEEL_MOTIONS)
def test_wheel_matrix_is_finite_and_singular_where_it_should_be(pkg, po, motion):
    for kind in range(6):
        for calib in bf.CALIB_SETS:
            opt, st, t, m1, m2 = bf.wheel_case(pkg, po, motion, kind, calib)
            H, res, Cov, cols, R3, p3 = po.wheel_linear_system(opt, st, t, m1, m2)
            assert _finite(H, res, Cov, R3, p3) and np.abs(Cov - Cov.T).max() == 0, (kind, calib)
            ev = np.linalg.eigvalsh(Cov)
            if kind < 3:
                assert ev.min() > 1e-3
            elif motion == "standstill":
                assert Cov[2, 2] == 0.0 and not Cov[2].any() and ev.max() > 1e-3
            elif motion == "creeping":
                assert 0 < Cov[2, 2] < 1e-9 and ev.max() / max(ev.min(), 1e-300) > 1e9
            else:
                assert ev.min() > 1e-6
    if motion == "standstill":
        for kind in range(6):          # not moving at all and clones that agree: R_3D = I exactly, the residual's log near the identity
            opt, st, t, m1, m2 = bf.wheel_case(pkg, po, motion, kind, (True, True, True), d_scale=0.0)
            H, res, Cov, cols, R3, p3 = po.wheel_linear_system(opt, st, t, m1, m2)
            assert not m1.any() and not m2.any() and _finite(H, res) and np.abs(res).max() < 1e-12
            assert kind >= 3 or np.array_equal(R3, np.eye(3))
    for stream, (count, uneven) in bf.WHEEL_STREAMS.items():
        opt, st, t, m1, m2 = bf.wheel_case(pkg, po, motion, 0, (True, True, True), stream=stream, noise=0.05)
        assert (len(t) == count or uneven) and (np.diff(t) > 1e-4).all()
        assert count <= 3 or (np.ptp(np.diff(t)[1:-1]) > 1e-3) == uneven
        assert _finite(*po.wheel_linear_system(opt, st, t, m1, m2)[:3])


def test_wheel_updates_decide_both_ways_and_the_creeping_tolerance(pkg, po):
    q95 = synth.q95_table()
    verdicts = {}
    for c in bf.WHEEL_UPDATE_CASES:
        opt, st, t, m1, m2 = bf.wheel_update_case(pkg, po, c)
        H, res, Cov, cols, _, _ = po.wheel_linear_system(opt, st, t, m1, m2)
        assert len(set(cols)) == len(cols) and 0 <= min(cols) and max(cols) < c.n
        P = bf.wheel_prior(c.n)
        chi2, acc, dx, P1 = bf.wheel_restatement(P, H, res, Cov, cols, c.n, opt.chi2_mult, q95)
        chi2_l, acc_l, dx_l, P1_l = bf.wheel_restatement(P, H, res, Cov, cols, c.n, opt.chi2_mult, q95, dtype=np.longdouble)
        thr = opt.chi2_mult * q95[len(res)]
        assert acc == acc_l and not 0.5 * thr < chi2 < 2.0 * thr, (c.name, chi2)       # no verdict hangs on rounding
        assert acc == c.name.endswith("-in"), (c.name, chi2, thr)
        d = max(np.abs(dx - dx_l).max() / max(1.0, np.abs(dx_l).max()), np.abs(P1 - P1_l).max() / np.abs(P).max())
        print(f"{c.name}: chi2 {chi2:.3e} (gate {thr:.2f}), cond(Cov) {np.linalg.cond(Cov):.1e}, numpy restatement vs long double {d:.2e}")
        verdicts[c.name] = acc
        assert d < 1e-10, c.name       # the fp64 restatement is itself within a tenth of the 1e-9 the library is held to
    assert sum(verdicts.values()) >= 8 and sum(not v for v in verdicts.values()) >= 4
