"""The between-frame filter path on the GPU, held to the oracle on the case matrix of tests/between_frame_cases.py: propagate_kernel,
ekf_prop_strip_kernel / ekf_prop_write_kernel, cov_clone_kernel, cov_marginalize_kernel, cov_init_invertible_kernel, wheel_kernel,
wheel2d_kernel and wheel_gate_kernel, through plv_propagate, plv_cpi_integrate, plv_cov_clone, plv_cov_marginalize,
plv_slam_initialize, plv_slam_update, plv_wheel_linear_system and plv_wheel_update.

Tolerances are the ones test_gpu_propagate.py, test_gpu_slam.py and test_gpu_wheel.py use (1e-12 relative for the propagation and the
wheel system, 1e-10 for the CPI covariance, 1e-9 / 1e-8 for the landmark and wheel updates); the copying kernels are held to
array_equal, and every refusal to a covariance that is bit for bit the one before the call.

The wheel update is held to UpdaterWheel::update restated in numpy, S = H P H^T + Cov with the FULL preintegrated covariance.  For the 2D
types at standstill that covariance is exactly singular (no noise enters the lateral coordinate) and at 1e-4 m/s its condition number
is 5e9 .. 3e10; the numpy restatement is 5e-17 .. 1.6e-16 from the same update in long double there (test_between_frame_cases_cpu
prints it), so the bound stays the larger of 1e-9 and ten times that distance: 1e-9.  The library whitens with the Cholesky factor
while every pivot keeps more than 1e-6 of its diagonal entry (all cases but standstill: the smallest fraction is 0.24) and goes through
the eigenbasis of the covariance otherwise (the standstill cases); with the whitening alone the four standstill cases end in
PLV_E_NUMERIC.

Over-limit sizes never reach a kernel: 64 updating rows are refused by launch_chi2 on the host (update_kernels.hip, `max_mp >
CHI2_MAXM`, before chi2_t_kernel / chi2_gate_kernel are launched) both for plv_slam_initialize and plv_slam_update, and a clone beyond
cfg.max_state_dim by plv_cov_clone's own check (propagate_api.hip, before d_P2 is reserved).

Sixteen one-line mutations of the three files and of so3_dev.hpp (since folded into so3.hpp: exp3 = exp_so3, Jl = Jl_so3; values only: no index or loop bound leaves its allocation),
each built into a library of its own on a scratch copy and run on the MI355X against this module and against the three files the suite
had before (test_gpu_propagate.py, test_gpu_wheel.py, test_gpu_slam.py):

  mutation                                                              caught here by (first of N failing tests)          before
  propagate_api.hip  small_w f_1 = -dt^3/3 -> /6                        test_propagate_case[straight-n16-id1-s41] (13)     no
  propagate_api.hip  small_w f_2 = dt^4/8 -> /6                         test_propagate_case[below-n119-id0-s400-jit] (1)   no
  propagate_api.hip  small_w R_mid: .5 dt w_x -> dt w_x                 test_propagate_case[straight-n16-id1-s41] (12)     no
  propagate_api.hip  small_w R_t2t1: dt^2/2 w_x^2 -> dt^2 w_x^2         test_propagate_case[straight-n16-id1-s41] (12)     no
  propagate_api.hip  ekf_prop_write_kernel Phi[rr][k] -> Phi[k][rr]     test_propagate_case[turning-n15-id0-s41] (24)      yes
  propagate_api.hip  cov_clone_kernel src + (r - n) -> src              test_cov_clone_case[15-0-6] (6)                    yes
  propagate_api.hip  cov_clone_kernel stride gridDim * 256 -> * 512     test_cov_clone_case[123-0-6] (3)                   no
  slam_api.hip       cov_marginalize_kernel i + size -> i + size - 1    test_cov_marginalize_case[20-0-1] (9)              yes
  slam_api.hip       cov_marginalize_kernel stride doubled              test_cov_marginalize_case[135-0-6] (8)             yes (one case)
  slam_api.hip       cov_init_invertible_kernel M[7] = M[5] -> M[2]     test_slam_initialize_case[n40-k15-rows4] (11)      yes
  slam_api.hip       the revert without its buffer swap                 test_slam_initialize_reverts_when_the_update_fails no
  wheel_api.hip      wheel2d_kernel intrinsic column -g_px -> +g_px     test_wheel_linear_system_matrix[turning-Wheel2DAng] (23)  yes
  wheel_api.hip      arc_sensitivities straight branch y_r: /2 -> /3    test_wheel_linear_system_matrix[straight-Wheel2DAng] (14) no
  wheel_api.hip      wheel2d_kernel noise eigenvalues -> 0              test_wheel_update_case[2dang-still-in] (3)         no
  so3_dev.hpp        exp3(0) = I -> 2 I                                 test_wheel_linear_system_matrix[straight-Wheel3DAng] (1)  no
  so3_dev.hpp        Jl below 1e-6 = I -> I / 2                         test_propagate_case[standing-n16-id0-s2] (20)      no

(the f_2 term is dt^4 |w|^2 / 8 of the position integral: only the 400-step stream with stamps up to 9 ms apart carries it above 1e-12.)

Measured on the MI355X: the propagation (Phi, Qd, records, accumulator, IMU state, P) is bit-identical to the oracle on every case of
the matrix; the landmark initialisation is within 2.5e-15 (P) and 5.6e-16 (dx_init) of it; the wheel system within 7.3e-14
(Wheel2DLin, turning), bit-identical for the 3D types; the wheel update within 1.9e-16 (P) and 4.3e-19 (dx) of the numpy restatement.
"""
import numpy as np
import pytest

import between_frame_cases as bf
import oracle_lib
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big(pkg):
    """a context whose state capacity holds the larger cases (the default cfg.max_state_dim is 160)"""
    cfg = pkg.default_config(752, 480)
    cfg.max_state_dim = bf.CAPACITY
    c = pkg.Context(cfg)
    yield c
    c.close()


@pytest.fixture(scope="module")
def po(pkg):
    return oracle_lib.load_prop(pkg)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _rec_eq(a, b, tol=1e-12):
    for f in ("t", "dt", "clone_t"):
        assert abs(getattr(a, f) - getattr(b, f)) <= 1e-15 * max(1.0, abs(getattr(b, f)))
    for f, scale in (("R_I0toIk", 1.0), ("alpha", 1.0), ("v", 10.0), ("w", 1.0)):
        assert np.abs(np.array(getattr(a, f)) - np.array(getattr(b, f))).max() < tol * scale, f
    qa, qb = np.array(a.Q), np.array(b.Q)
    assert np.abs(qa - qb).max() <= 1e-10 * np.abs(qb).max() + 1e-30


def _refused(pkg, code, fn, *a, **kw):
    with pytest.raises(pkg.PlvError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


# ------------------------------------------------------------------------------------------------ propagation
def _both(pkg, po, case):
    t, wm, am, imu_o, _, _ = bf.imu_case(pkg, case)
    imu_d = imu_o.copy()
    return t, wm, am, imu_o, imu_d, bf.make_acc(po.reset_cpi, imu_o, case), bf.make_acc(pkg.reset_cpi, imu_d, case)


def _prop_eq(case, imu_d, imu_o, Phi_d, Phi_o, Qd_d, Qd_o, acc_d, acc_o, Pd, P_o):
    pm_d, pm_o = np.array(acc_d.P_meas), np.array(acc_o.P_meas)
    print(f"{case.name}: imu {np.abs(imu_d.vec() - imu_o.vec()).max():.1e} Phi {_rel(Phi_d, Phi_o):.1e} Qd {_rel(Qd_d, Qd_o):.1e} "
          f"P_meas {_rel(pm_d, pm_o):.1e} alpha {np.abs(np.array(acc_d.alpha_tau) - np.array(acc_o.alpha_tau)).max():.1e} P {_rel(Pd, P_o):.1e}")
    assert np.abs(imu_d.vec() - imu_o.vec()).max() < 1e-12 and list(imu_d.q) == list(imu_d.q_fej)
    assert np.abs(Phi_d - Phi_o).max() < 1e-12 * np.abs(Phi_o).max()
    assert np.abs(Qd_d - Qd_o).max() < 1e-12 * np.abs(Qd_o).max() and np.abs(Qd_d - Qd_d.T).max() == 0
    assert abs(acc_d.DT - acc_o.DT) < 1e-15 and np.abs(pm_d - pm_o).max() <= 1e-10 * np.abs(pm_o).max()
    for f in ("R_k2tau", "alpha_tau", "beta_tau"):
        assert np.abs(np.array(getattr(acc_d, f)) - np.array(getattr(acc_o, f))).max() < 1e-12, f
    for f in ("b_w_lin", "b_a_lin", "v_clone"):
        assert list(getattr(acc_d, f)) == list(getattr(acc_o, f))
    assert np.abs(Pd - P_o).max() < 1e-12 * np.abs(P_o).max() and np.abs(Pd - Pd.T).max() < 1e-15 * np.abs(Pd).max()


@pytest.mark.parametrize("case", bf.PROP_CASES, ids=lambda c: c.name)
def test_propagate_case(pkg, big, po, case):
    nz = pkg.imu_noise()
    t, wm, am, imu_o, imu_d, acc_o, acc_d = _both(pkg, po, case)
    n = case.n
    P = synth.spd_cov(n, seed=2) * 1e-3
    Phi_o, Qd_o, rec_o, P_o = po.propagate(imu_o, nz, t, wm, am, P=P, acc=acc_o, imu_id=case.imu_id)
    big.cov_upload(P)
    Phi_d, Qd_d, rec_d = big.propagate(imu_d, nz, t, wm, am, n, acc=acc_d, imu_id=case.imu_id)
    assert len(rec_d) == len(rec_o) == case.samples - 1
    for a, b in zip(rec_d, rec_o):
        _rec_eq(a, b)
    _prop_eq(case, imu_d, imu_o, Phi_d, Phi_o, Qd_d, Qd_o, acc_d, acc_o, big.cov_download(n), P_o)
    # mean and Phi alone: no accumulator, no covariance
    _, _, _, imu_mo, imu_m, _, _ = _both(pkg, po, case)
    Phi_m, _, rec_m = big.propagate(imu_m, nz, t, wm, am, 0)
    Phi_mo = po.propagate(imu_mo, nz, t, wm, am)[0]
    assert rec_m == [] and np.abs(Phi_m - Phi_mo).max() < 1e-12 * np.abs(Phi_mo).max() and np.abs(imu_m.vec() - imu_mo.vec()).max() < 1e-12


@pytest.mark.parametrize("case", bf.CARRIED_CASES, ids=lambda c: c.name)
def test_propagate_message_by_message_with_the_accumulator_carried(pkg, big, po, case):
    nz = pkg.imu_noise()
    t, wm, am, imu_o, imu_d, acc_o, acc_d = _both(pkg, po, case)
    n = case.n
    P_o = synth.spd_cov(n, seed=2) * 1e-3
    big.cov_upload(P_o)
    assert len(t) - 1 >= 20
    for i in range(len(t) - 1):
        Phi_d, Qd_d, r_d = big.propagate(imu_d, nz, t[i:i + 2], wm[i:i + 2], am[i:i + 2], n, acc=acc_d, imu_id=case.imu_id)
        Phi_o, Qd_o, r_o, P_o = po.propagate(imu_o, nz, t[i:i + 2], wm[i:i + 2], am[i:i + 2], P=P_o, acc=acc_o, imu_id=case.imu_id)
        _rec_eq(r_d[0], r_o[0])
    _prop_eq(case, imu_d, imu_o, Phi_d, Phi_o, Qd_d, Qd_o, acc_d, acc_o, big.cov_download(n), P_o)


def test_propagate_refusals_leave_the_covariance(pkg, big, po):
    case = bf.PROP_CASES[5]
    nz = pkg.imu_noise()
    t, wm, am, _, imu, _, acc = _both(pkg, po, case)
    n = case.n
    P = np.asfortranarray(synth.spd_cov(n, seed=2) * 1e-3)
    big.cov_upload(P)
    before = imu.vec().copy()
    _refused(pkg, pkg.PLV_E_BADARG, big.propagate, imu, nz, t, wm, am, n + 1, acc=acc, imu_id=case.imu_id)      # n != cov_n
    _refused(pkg, pkg.PLV_E_BADARG, big.propagate, imu, nz, t, wm, am, n, acc=acc, imu_id=n - 14)               # imu_id + 15 > n
    _refused(pkg, pkg.PLV_E_BADARG, big.propagate, imu, nz, t, wm, am, n, acc=acc, imu_id=-1)
    tb = t.copy()
    tb[7], tb[8] = t[8], t[7]
    _refused(pkg, pkg.PLV_E_BADARG, big.propagate, imu, nz, tb, wm, am, n, acc=acc, imu_id=case.imu_id)         # decreasing stamps
    assert np.array_equal(big.cov_download(n), P) and np.array_equal(imu.vec(), before) and acc.DT == 0.0


@pytest.mark.parametrize("c", bf.CPI_CASES, ids=lambda c: c.name)
def test_cpi_integrate_case(pkg, big, po, c):
    nz = pkg.imu_noise()
    t, wm, am, Rc, vc, tq = bf.cpi_case(pkg, c)
    ok_o, r_o = po.cpi_integrate(nz, tq, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t, wm, am)
    ok_d, r_d = big.cpi_integrate(nz, tq, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t, wm, am)
    assert ok_o and ok_d
    _rec_eq(r_d, r_o)
    if c.kind != "two-samples":      # one IMU sample delivered twice inside the window: the step of dt = 0 changes nothing CpiV1 integrates
        lo, hi = min(tq, bf.CLONE_T), max(tq, bf.CLONE_T)
        t2, w2, a2 = bf.with_duplicate(t, wm, am, bf.duplicate_index(t, lo, hi))
        ok_o2, r_o2 = po.cpi_integrate(nz, tq, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t2, w2, a2)
        ok_d2, r_d2 = big.cpi_integrate(nz, tq, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t2, w2, a2)
        assert ok_o2 and ok_d2 and bf.records_equal(r_d2, r_d) and bf.records_equal(r_o2, r_o)
        _rec_eq(r_d2, r_o2)
    ok_d, r_d = big.cpi_integrate(nz, bf.CLONE_T, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t, wm, am)      # t_given == clone_t
    assert not ok_d and not po.cpi_integrate(nz, bf.CLONE_T, bf.CLONE_T, Rc, vc, bf.BG, bf.BA, t, wm, am)[0]


# ------------------------------------------------------------------------------------------------ clone / marginalise
@pytest.mark.parametrize("n,src,size", bf.CLONE_CASES)
def test_cov_clone_case(big, n, src, size):
    P = bf.tagged(n)
    big.cov_upload(P)
    big.cov_clone(n, src, size)
    got = big.cov_download(n + size)
    assert np.array_equal(got, bf.clone_ref(P, src, size))
    big.cov_marginalize(n, size)            # ... and marginalising the new block gives the original back
    assert np.array_equal(big.cov_download(n), P)


@pytest.mark.parametrize("n,idx,size", bf.MARG_CASES)
def test_cov_marginalize_case(big, n, idx, size):
    P = bf.tagged(n)
    big.cov_upload(P)
    big.cov_marginalize(idx, size)
    assert np.array_equal(big.cov_download(n - size), bf.marg_ref(P, idx, size))


def test_cov_clone_beyond_the_capacity_is_refused(pkg, big):
    n = bf.CAPACITY - 5
    P = bf.tagged(n)
    big.cov_upload(P)
    _refused(pkg, pkg.PLV_E_CAPACITY, big.cov_clone, n, 0, 6)       # host-side: plv_cov_clone, before any allocation or launch
    assert np.array_equal(big.cov_download(n), P)                  # cov_n and P as found (a download of another n is refused)
    big.cov_clone(n, 0, 5)
    assert np.array_equal(big.cov_download(bf.CAPACITY), bf.clone_ref(P, 0, 5))
    _refused(pkg, pkg.PLV_E_BADARG, big.cov_marginalize, bf.CAPACITY - 2, 3)
    _refused(pkg, pkg.PLV_E_BADARG, big.cov_clone, bf.CAPACITY - 1, 0, 1)      # stale n
    assert np.array_equal(big.cov_download(bf.CAPACITY), bf.clone_ref(P, 0, 5))


# ------------------------------------------------------------------------------------------------ landmarks
@pytest.mark.parametrize("c", bf.SLAM_INIT_CASES, ids=lambda c: f"n{c.n}-k{c.k}-rows{c.rows}")
def test_slam_initialize_case(big, oracle, c):
    q95 = synth.q95_table()
    n = c.n
    P, cols, Hf, Hx, res = bf.landmark_system(c)
    ok_o, P2_o, dxi_o, dx_o = oracle.slam_initialize(P, Hf, Hx, res, cols, q95, chi2_mult=5.0)
    big.cov_upload(P)
    ok, dxi, dx = big.slam_initialize(n, Hf, Hx, res, cols, chi2_mult=5.0)
    assert ok == ok_o == 1
    P2 = big.cov_download(n + 3)
    print(f"{c}: P {_rel(P2, P2_o):.1e} dx_init {np.abs(dxi - dxi_o).max():.1e} dx {np.abs(dx - dx_o).max():.1e}")
    assert np.abs(P2 - P2_o).max() <= 1e-9 * np.abs(P2_o).max()
    assert np.abs(dxi - dxi_o).max() <= 1e-9 * max(1.0, np.abs(dxi_o).max())
    assert np.abs(dx - dx_o).max() <= 1e-8 * max(1e-3, np.abs(dx_o).max())
    # an update whose columns include the landmark just appended
    rng = np.random.default_rng(c.seed)
    cols2 = np.concatenate([cols[:12], [n, n + 1, n + 2]]).astype(np.int32)
    H = rng.normal(size=(8, len(cols2)))
    r = rng.normal(0, 0.4, 8)
    rc_o, P3_o, acc_o, dxu_o = oracle.slam_update(P2_o, H, r, cols2, q95, chi2_mult=5.0)
    rc, acc, dxu = big.slam_update(n + 3, H, r, cols2, chi2_mult=5.0)
    assert rc == rc_o == 0 and acc == acc_o == 1
    assert np.abs(big.cov_download(n + 3) - P3_o).max() <= 1e-9 * np.abs(P3_o).max()
    assert np.abs(dxu - dxu_o).max() <= 1e-8 * max(1e-3, np.abs(dxu_o).max())


def test_slam_over_the_row_limit_is_refused_on_the_host(pkg, big):
    """64 updating rows: launch_chi2 returns PLV_E_CAPACITY before chi2_t_kernel / chi2_gate_kernel are launched"""
    c = bf.SLAM_OVER
    P, cols, Hf, Hx, res = bf.landmark_system(c)
    P = np.asfortranarray(P)
    big.cov_upload(P)
    _refused(pkg, pkg.PLV_E_CAPACITY, big.slam_initialize, c.n, Hf, Hx, res, cols, chi2_mult=5.0)
    assert np.array_equal(big.cov_download(c.n), P)
    P, cols, H, res = bf.slam_update_system(143, 98, 64, 104)
    big.cov_upload(P)
    _refused(pkg, pkg.PLV_E_CAPACITY, big.slam_update, 143, H, res, cols, chi2_mult=5.0)
    assert np.array_equal(big.cov_download(143), P)


def test_slam_rejections_leave_the_state(big, oracle):
    q95 = synth.q95_table()
    c = bf.SLAM_INIT_CASES[2]
    n = c.n
    P, cols, Hf, Hx, res = bf.landmark_system(c)
    P = np.asfortranarray(P)
    big.cov_upload(P)
    bad = res.copy()
    bad[5:] += 80.0
    for name, a in (("rank", (bf.rank_deficient(Hf), Hx, res)), ("dn > 1000", (Hf * 1e-3, Hx, res)), ("gate", (Hf, Hx, bad)),
                    ("chi < 1e-7", (Hf, Hx, np.zeros_like(res)))):
        assert oracle.slam_initialize(P, *a, cols, q95, chi2_mult=5.0)[0] == 0, name
        ok, dxi, dx = big.slam_initialize(n, *a, cols, chi2_mult=5.0)
        assert ok == 0 and not dx.any() and not dxi.any(), name
        assert np.array_equal(big.cov_download(n), P), name
    rc, acc, dx = big.slam_update(n, Hx, res + 60.0, cols, chi2_mult=5.0)
    assert rc == 0 and acc == 0 and not dx.any() and np.array_equal(big.cov_download(n), P)


def test_slam_initialize_reverts_when_the_update_fails(big, oracle):
    """initialize_invertible accepts, the EKF update of the remaining rows returns PLV_E_NOT_PSD: cov_n and the buffers go back"""
    q95 = synth.q95_table()
    P, cols, Hf, Hx, res = bf.revert_system()
    n = P.shape[0]
    ok_o, _, dxi_o, _ = oracle.slam_initialize(P, Hf, Hx, res, cols, q95, chi2_mult=5.0)
    assert ok_o == 0 and dxi_o.any()
    big.cov_upload(P)
    ok, dxi, dx = big.slam_initialize(n, Hf, Hx, res, cols, chi2_mult=5.0)
    assert ok == 0 and not dx.any() and not dxi.any()
    assert np.array_equal(big.cov_download(n), P)          # the old n (a download of n + 3 would be refused) and the old P, bit for bit
    # the state is usable: the same system on the healthy prior initialises, on the same context
    Ph = P.copy()
    Ph[0, 1] = Ph[1, 0] = 0.0
    ok_o, P2_o, dxi_o, dx_o = oracle.slam_initialize(Ph, Hf, Hx, res, cols, q95, chi2_mult=5.0)
    big.cov_upload(Ph)
    ok, dxi, dx = big.slam_initialize(n, Hf, Hx, res, cols, chi2_mult=5.0)
    assert ok == ok_o == 1 and np.abs(big.cov_download(n + 3) - P2_o).max() <= 1e-9 * np.abs(P2_o).max()
    assert np.abs(dxi - dxi_o).max() <= 1e-9 and np.abs(dx - dx_o).max() <= 1e-8 * max(1e-3, np.abs(dx_o).max())


@pytest.mark.parametrize("rows", (1, 2, 63))
def test_slam_update_rows(big, oracle, rows):
    q95 = synth.q95_table()
    P, cols, H, res = bf.slam_update_system(143, 98, rows, 40 + rows)
    rc_o, P1_o, acc_o, dx_o = oracle.slam_update(P, H, res, cols, q95, chi2_mult=5.0)
    big.cov_upload(P)
    rc, acc, dx = big.slam_update(143, H, res, cols, chi2_mult=5.0)
    assert rc == rc_o == 0 and acc == acc_o == (0 if rows == 1 else 1)
    P1 = big.cov_download(143)
    if rows == 1:
        assert not dx.any() and np.array_equal(P1, P)
    else:
        assert np.abs(P1 - P1_o).max() <= 1e-9 * np.abs(P1_o).max() and np.abs(dx - dx_o).max() <= 1e-8 * max(1e-3, np.abs(dx_o).max())


# ------------------------------------------------------------------------------------------------ wheel
def _wheel_eq(pkg, big, po, kind, opt, st, t, m1, m2, tag):
    H, res, Cov, cols, R3, p3 = big.wheel_linear_system(opt, st, t, m1, m2)
    Ho, reso, Covo, colso, R3o, p3o = po.wheel_linear_system(opt, st, t, m1, m2)
    assert H.shape == Ho.shape and np.array_equal(cols, colso), tag
    assert np.abs(H - Ho).max() < 1e-12 * max(1.0, np.abs(Ho).max()) and np.abs(res - reso).max() < 1e-12, tag
    assert np.abs(Cov - Covo).max() < 1e-12 * np.abs(Covo).max() and np.abs(Cov - Cov.T).max() == 0, tag
    assert H.shape[0] == (3 if kind >= 3 else 6) and Cov.shape == (H.shape[0], H.shape[0])
    assert np.abs(R3 - R3o).max() < 1e-13 and np.abs(p3 - p3o).max() < 1e-12, tag
    return max(_rel(H, Ho), _rel(Cov, Covo), float(np.abs(res - reso).max()))


@pytest.mark.parametrize("kind", range(6), ids=bf.KIND_NAMES)
@pytest.mark.parametrize("motion", bf.WHEEL_MOTIONS)
def test_wheel_linear_system_matrix(pkg, big, po, motion, kind):
    worst = 0.0
    for calib in bf.CALIB_SETS:
        for noise, d_scale in ((0.0, 0.01), (0.05, 0.01)) + (((0.0, 0.0),) if motion == "standstill" else ()):
            opt, st, t, m1, m2 = bf.wheel_case(pkg, po, motion, kind, calib, noise=noise, d_scale=d_scale, seed=kind)
            worst = max(worst, _wheel_eq(pkg, big, po, kind, opt, st, t, m1, m2, (calib, noise, d_scale)))
    print(f"{motion} {bf.KIND_NAMES[kind]}: worst {worst:.1e}")


@pytest.mark.parametrize("stream", list(bf.WHEEL_STREAMS))
def test_wheel_linear_system_streams(pkg, big, po, stream):
    for motion in ("turning", "standstill", "creeping"):
        for kind in range(6):
            opt, st, t, m1, m2 = bf.wheel_case(pkg, po, motion, kind, (True, True, kind % 3 == 0), stream=stream, noise=0.05 * (motion == "turning"))
            _wheel_eq(pkg, big, po, kind, opt, st, t, m1, m2, (motion, kind))


@pytest.mark.parametrize("c", bf.WHEEL_UPDATE_CASES, ids=lambda c: c.name)
def test_wheel_update_case(pkg, big, po, c):
    """UpdaterWheel::update: S = H P H^T + Cov with the full preintegrated covariance, gate, update — singular Cov included"""
    q95 = synth.q95_table()
    opt, st, t, m1, m2 = bf.wheel_update_case(pkg, po, c)
    n = c.n
    P = bf.wheel_prior(n)
    H, res, Cov, cols, _, _ = po.wheel_linear_system(opt, st, t, m1, m2)
    chi2, expect, dx_r, P_r = bf.wheel_restatement(P, H, res, Cov, cols, n, opt.chi2_mult, q95)
    _, _, dx_l, P_l = bf.wheel_restatement(P, H, res, Cov, cols, n, opt.chi2_mult, q95, dtype=np.longdouble)
    d_num = max(np.abs(dx_r - dx_l).max() / max(1.0, np.abs(dx_l).max()), np.abs(P_r - P_l).max() / np.abs(P).max())
    tol = max(1e-9, 10 * d_num)
    big.cov_upload(P)
    rc, acc, dx = big.wheel_update(opt, st, t, m1, m2, n)
    Pd = big.cov_download(n)
    assert rc == 0 and bool(acc) == bool(expect) == c.name.endswith("-in"), (c.name, rc, acc, chi2)
    if expect:
        e_dx, e_P = np.abs(dx - dx_r).max() / max(1.0, np.abs(dx_r).max()), np.abs(Pd - P_r).max() / np.abs(P).max()
        print(f"{c.name}: chi2 {chi2:.3e}, numpy vs long double {d_num:.1e}, library vs numpy dx {e_dx:.1e} P {e_P:.1e}, "
              f"library vs long double {max(np.abs(dx - dx_l).max(), np.abs(Pd - P_l).max() / np.abs(P).max()):.1e}")
        assert e_dx < tol and e_P < tol
    else:
        assert not dx.any() and np.array_equal(Pd, P)


def test_wheel_update_keeps_numeric_for_what_is_not_finite(pkg, big, po):
    c = bf.WHEEL_UPDATE_CASES[6]
    opt, st, t, m1, m2 = bf.wheel_update_case(pkg, po, c)
    P = bf.wheel_prior(c.n)
    big.cov_upload(P)
    bad = m1.copy()
    bad[len(bad) // 2] = np.nan
    _refused(pkg, pkg.PLV_E_NUMERIC, big.wheel_update, opt, st, t, bad, m2, c.n)
    assert np.array_equal(big.cov_download(c.n), P)
    st.pose1_id = c.n          # a state the columns do not fit
    _refused(pkg, pkg.PLV_E_BADARG, big.wheel_update, opt, st, t, m1, m2, c.n)
    assert np.array_equal(big.cov_download(c.n), P)
