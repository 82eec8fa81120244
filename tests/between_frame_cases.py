"""The case matrix of the between-frame filter path (test infrastructure; tests/test_between_frame_cases_cpu.py states on the oracle
alone what the cases must contain, tests/test_gpu_between_frames.py runs them on the device).

Between two camera frames the filter propagates (propagate_kernel, ekf_prop_strip_kernel / ekf_prop_write_kernel), clones and
marginalises (cov_clone_kernel, cov_marginalize_kernel), initialises and updates landmarks (cov_init_invertible_kernel) and takes the
wheel measurement (wheel_kernel, wheel2d_kernel, wheel_gate_kernel).  The trajectory and the vehicle of test_oracle_propagate /
test_oracle_wheel always turn and always drive; a city drive is long straight stretches and stops.  The cases below walk the inputs
on which those kernels take another branch or another launch shape:

  IMU motion     turning (test_oracle_propagate.traj), standing (wm == bg exactly), straight (gyro noise 1e-3 rad/s around the bias),
                 below / above (|w_hat| = 0.0087 / 0.00875 rad/s, either side of CpiV1's small-rotation threshold 0.008726646),
                 mixed (consecutive steps alternate sides), tiny (1e-9 rad/s: dt |w| below the 1e-6 / 1e-7 limits of the SO(3) helpers)
  covariance     (n, imu_id) from 15 .. 205 rows: one and two workgroups of the strip kernels, the IMU block first, inside, last
  stream         2, 41 and 400 samples (the last with jittered stamps), an accumulator carried over single-message calls, and an
                 accumulator whose linearisation biases are not the state's biases (as after an update)
  clone / marg   results of 128, 129 and 200 rows (cov_clone_kernel / cov_marginalize_kernel stride from 129 rows on)
  landmarks      1 .. 64 updating rows (chi2_gate_kernel<2> / <4> switch at 32, the limit at 63), k and n up to 192 / 199
  wheel          6 types x 8 calibration sets under turning, standstill, straight, creeping (1e-4 m/s), reversing, spin

Everything here runs on numpy and the CPU oracle; no case needs a device to be built."""
import functools
from collections import namedtuple

import numpy as np
from scipy.spatial.transform import Rotation

import synth
import test_oracle_wheel as tw
from test_oracle_propagate import imu_at, traj

G = np.array([0.0, 0.0, 9.81])
CPI_SMALL_W = 0.008726646          # CpiV1::feed_IMU: below this |w_hat| the small-rotation series is taken
BG, BA = (0.01, -0.02, 0.005), (0.05, 0.02, -0.03)
T0 = 50.0

# ------------------------------------------------------------------------------------------------ propagation
MOTIONS = ("turning", "standing", "straight", "below", "above", "mixed", "tiny")
RATE_OF = {"below": 0.0087, "above": 0.00875, "tiny": 1e-9}

PropCase = namedtuple("PropCase", "name motion n imu_id samples jitter lin_bias seed")


def _p(motion, n, imu_id, samples, jitter=False, lin_bias=False, seed=1):
    name = f"{motion}-n{n}-id{imu_id}-s{samples}" + ("-jit" if jitter else "") + ("-lin" if lin_bias else "")
    return PropCase(name, motion, n, imu_id, samples, jitter, lin_bias, seed)


PROP_CASES = [
    _p("turning", 15, 0, 41), _p("standing", 16, 0, 2), _p("straight", 16, 1, 41), _p("below", 17, 0, 41),
    _p("above", 18, 0, 41), _p("mixed", 45, 30, 41), _p("tiny", 63, 12, 41), _p("standing", 119, 0, 400, jitter=True),
    _p("straight", 149, 0, 400, jitter=True, lin_bias=True), _p("turning", 205, 15, 41, lin_bias=True),
    _p("tiny", 45, 15, 2, seed=2), _p("below", 119, 0, 400, jitter=True, seed=2), _p("above", 45, 15, 21, lin_bias=True, seed=2),
    _p("mixed", 149, 0, 41, lin_bias=True, seed=2), _p("standing", 45, 15, 21, lin_bias=True, seed=3),
    _p("straight", 18, 0, 2, seed=3), _p("tiny", 205, 15, 400, jitter=True, lin_bias=True, seed=3),
    _p("turning", 17, 0, 400, jitter=True, seed=3), _p("above", 119, 0, 41, seed=5),
]
# the accumulator carried across single-message calls (SystemManager::feed_measurement_imu), at least 20 of them
CARRIED_CASES = [_p("standing", 45, 15, 26), _p("straight", 63, 12, 26, lin_bias=True), _p("mixed", 45, 30, 31, lin_bias=True, seed=4),
                 _p("turning", 119, 0, 26, seed=4), _p("tiny", 18, 0, 26, seed=4)]

_R_REST = Rotation.from_rotvec([0.03, -0.05, 0.4]).as_matrix()      # R_GtoI of the motions that do not turn
_AXIS = np.array([0.36, -0.48, 0.8])                                # unit vector


def lin_biases(case):
    """the CPI accumulator's linearisation biases: the state's, or (lin_bias) what they were before an update moved the state"""
    if not case.lin_bias:
        return np.array(BG), np.array(BA)
    return np.array(BG) + np.array([2e-4, -1e-4, 3e-4]), np.array(BA) + np.array([-2e-3, 1e-3, 4e-3])


def stamps(case):
    t = T0 + np.arange(case.samples) / 200.0
    if case.jitter:
        rng = np.random.default_rng(100 + case.seed)
        t[1:-1] += rng.uniform(-0.002, 0.002, case.samples - 2)     # spacing 1 .. 9 ms, strictly increasing
    return t


def imu_case(pkg, case):
    """-> t, wm, am, imu (PlvImuState with first estimates that differ), b_w_lin, b_a_lin"""
    rng = np.random.default_rng(case.seed)
    t = stamps(case)
    ns = len(t)
    bw_lin, ba_lin = lin_biases(case)
    bg, ba = np.array(BG), np.array(BA)
    if case.motion == "turning":
        wm, am = np.zeros((ns, 3)), np.zeros((ns, 3))
        for i, ti in enumerate(t):          # (synth.imu_stream samples a regular grid: one sample per stamp here)
            _, w1, a1 = synth.imu_stream(traj, ti, ti, rate=200.0, bg=BG, ba=BA)
            wm[i], am[i] = w1[0], a1[0]
        wm, am = wm + rng.normal(0, 1e-3, wm.shape), am + rng.normal(0, 1e-2, am.shape)
        imu = imu_at(pkg, T0, BG, BA)
    else:
        import eval_oracle as eo
        v = {"standing": np.zeros(3)}.get(case.motion, np.array([8.0, 0.5, -0.1]))
        imu = pkg.PlvImuState.make(eo.rot_2_quat(_R_REST), np.array([3.0, -1.0, 0.5]), v, BG, BA)
        am = np.tile(_R_REST @ G + ba, (ns, 1))
        if case.motion == "standing":
            wm = np.tile(bg, (ns, 1))
        elif case.motion == "straight":
            wm = bg + rng.normal(0, 1e-3, (ns, 3))
            am = am + rng.normal(0, 1e-2, am.shape)
        elif case.motion == "mixed":
            # the mean of samples i, i + 1 alternates 0.0087 / 0.00875: r[i + 1] = 2 m[i] - r[i] (the rates drift by 1e-4 per two steps)
            r = np.zeros(ns)
            r[0] = RATE_OF["below"]
            for i in range(ns - 1):
                r[i + 1] = 2 * (RATE_OF["below"] if i % 2 == 0 else RATE_OF["above"]) - r[i]
            wm = bw_lin + r[:, None] * _AXIS
        else:
            wm = np.tile(bw_lin + RATE_OF[case.motion] * _AXIS, (ns, 1))    # around the bias the CPI means subtract
    imu.p_fej[0] += 0.01
    imu.v_fej[1] -= 0.02
    return t, wm, am, imu, bw_lin, ba_lin


def make_acc(reset_cpi, imu, case):
    """reset_cpi of either side, then the linearisation biases of the case"""
    acc = reset_cpi(imu, T0)
    bw, ba = lin_biases(case)
    for c in range(3):
        acc.b_w_lin[c], acc.b_a_lin[c] = bw[c], ba[c]
    return acc


def w_hat_norms(wm, b_w_lin):
    """|w_hat| of every step as CpiV1::feed_IMU forms it: 0.5 ((wm[i] - b) + (wm[i + 1] - b))"""
    w = 0.5 * ((wm[:-1] - b_w_lin) + (wm[1:] - b_w_lin))
    return np.sqrt((w * w).sum(axis=1))


def claimed_side(case, steps):
    """per step: True = the small-rotation branch, False = the general one, None = not claimed (turning / straight decide by their data)"""
    if case.motion in ("standing", "below", "tiny"):
        return [True] * steps
    if case.motion == "above":
        return [False] * steps
    if case.motion == "mixed":
        return [i % 2 == 0 for i in range(steps)]
    return [None] * steps


# plv_cpi_integrate: (name, motion, t_given - clone_t or None for "on a sample", kind)
CpiCase = namedtuple("CpiCase", "name motion kind")
CPI_CASES = [CpiCase(f"{m}-{k}", m, k) for m in ("standing", "straight", "turning") for k in ("forward", "backward", "two-samples")]
CLONE_T = T0 + 0.1


def cpi_case(pkg, c):
    """-> t, wm, am, R_clone, v_clone, t_given.  A 400 Hz stream of 0.2 s around the clone at T0 + 0.1."""
    pc = PropCase(c.name, c.motion, 0, 0, 81, False, False, 7)
    rng = np.random.default_rng(7)
    t = T0 + np.arange(81) / 400.0
    if c.motion == "turning":
        t, wm, am = synth.imu_stream(traj, T0, T0 + 0.2, rate=400.0)
        wm, am = wm + rng.normal(0, 1e-3, wm.shape), am + rng.normal(0, 1e-2, am.shape)
        Rc = traj(CLONE_T)[0]
        vc = (traj(CLONE_T + 1e-5)[1] - traj(CLONE_T - 1e-5)[1]) / 2e-5
    else:
        _, wm, am, imu, _, _ = imu_case(pkg, pc)
        Rc, vc = _R_REST, np.array(imu.v)
    tq = {"forward": CLONE_T + 0.0437, "backward": CLONE_T - 0.0612, "two-samples": CLONE_T + 0.0011}[c.kind]
    return t, wm, am, Rc, vc, tq


def with_duplicate(t, wm, am, at):
    """the stream with sample `at` delivered twice (same stamp, same reading)"""
    idx = np.concatenate([np.arange(at + 1), np.arange(at, len(t))])
    return t[idx], wm[idx], am[idx]


# ------------------------------------------------------------------------------------------------ clone / marginalise
CLONE_CASES = [(15, 0, 6), (45, 15, 6), (40, 39, 1), (60, 20, 8), (123, 0, 6), (199, 15, 6)]            # (n, src, size)
MARG_CASES = [(20, 0, 1), (46, 15, 6), (48, 40, 8), (131, 0, 3), (134, 60, 6), (129, 128, 1), (135, 0, 6), (130, 129, 1), (132, 63, 3),
              (137, 129, 8), (206, 15, 6), (203, 200, 3), (208, 0, 8), (201, 100, 1)]                   # (n, id, size)
CAPACITY = 256     # cfg.max_state_dim of the contexts the tests open (the default, 160, is below the larger cases)


def clone_ref(P, src, size):
    n = P.shape[0]
    idx = list(range(n)) + list(range(src, src + size))
    return P[np.ix_(idx, idx)]


def marg_ref(P, idx, size):
    keep = [i for i in range(P.shape[0]) if not idx <= i < idx + size]
    return P[np.ix_(keep, keep)]


def tagged(n):
    """entry (i, j) = i + j / 1024, exact in fp64 and not symmetric: a transposed, shifted or stale index shows under array_equal
    (the two kernels only copy)"""
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    return np.asfortranarray(i + j / 1024.0)


# ------------------------------------------------------------------------------------------------ landmarks
SlamCase = namedtuple("SlamCase", "n k rows seed")
SLAM_INIT_CASES = [SlamCase(40, 15, 4, 11), SlamCase(40, 16, 5, 12), SlamCase(40, 17, 19, 13), SlamCase(143, 98, 20, 14),
                   SlamCase(143, 128, 35, 15), SlamCase(199, 129, 36, 16), SlamCase(199, 192, 46, 17), SlamCase(143, 98, 66, 18),
                   SlamCase(199, 17, 20, 19), SlamCase(40, 16, 66, 20)]
SLAM_OVER = SlamCase(143, 98, 67, 21)              # 64 updating rows: refused by launch_chi2 on the host
SLAM_UPDATE_ROWS = (1, 2, 63, 64)                  # 1: returns; 64: refused


def landmark_system(c, noise=0.3):
    from test_oracle_slam import landmark_system as ls
    return ls(c.n, c.k, c.rows, c.seed, noise=noise)


def rank_deficient(Hf):
    """third column in the span of the first two: H_L of the Givens split is singular (inverse3 reports it)"""
    out = Hf.copy()
    out[:, 2] = 2.0 * out[:, 0] - 0.5 * out[:, 1]
    return out


def revert_system():
    """An initialisation that passes followed by an EKF update that must fail.  The prior is test_ekf_update_not_psd_leaves_state's:
    indefinite in the plane of states 0 and 1.  The measurement's columns hold state 0 (with a gain of 10) but not state 1, so every
    matrix the gate and initialize_invertible form (P[cols, cols] = 1e-4 I) is healthy and S is positive definite; the update then takes
    h^2 P01^2 / S = 2.5e-3 off P11 = 1e-4 through the cross-covariance, and the negative diagonal rejects it."""
    n, k, rows = 20, 8, 10
    P = np.eye(n) * 1e-4
    P[0, 1] = P[1, 0] = 5e-3
    cols = np.array([0, 2, 3, 4, 5, 6, 7, 8], dtype=np.int32)
    rng = np.random.default_rng(31)
    Hf = rng.normal(size=(rows, 3))
    Hx = rng.normal(size=(rows, k)) * 0.5
    Hx[:, 0] = rng.normal(size=rows) * 10.0
    res = Hf @ (rng.normal(size=3) * 0.4) + rng.normal(0, 0.3, rows)
    return np.asfortranarray(P), cols, Hf, Hx, res


# ------------------------------------------------------------------------------------------------ wheel
WHEEL_MOTIONS = ("turning", "standstill", "straight", "creeping", "reversing", "spin")
CALIB_SETS = [(e, d, i) for e in (False, True) for d in (False, True) for i in (False, True)]
# (selected samples, uneven stamps): the window [20.3007, t1] over a 100 Hz stream, t1 chosen for the count
WHEEL_STREAMS = {"2": (2, False), "3": (3, False), "51": (51, False), "500": (500, False), "uneven": (37, True)}
KIND_NAMES = ("Wheel3DAng", "Wheel3DLin", "Wheel3DCen", "Wheel2DAng", "Wheel2DLin", "Wheel2DCen")


def vehicle_of(motion):
    """yaw rate and forward speed of the odometry frame as functions of time"""
    return {"turning": tw.vehicle,
            "standstill": lambda t: (0.0, 0.0),
            "straight": lambda t: (0.0, 4.0 + 1.5 * np.cos(0.5 * t)),
            "creeping": lambda t: (0.0, 1e-4),
            "reversing": lambda t: (0.25 + 0.1 * np.sin(0.8 * t), -1.5 - 0.5 * np.cos(0.5 * t)),
            "spin": lambda t: (0.4 + 0.1 * np.sin(0.8 * t), 0.0)}[motion]


class moving:
    """test_oracle_wheel's vehicle (and with it odom_pose / imu_pose / wheel_stream / make) driven by another motion; level=True makes
    the odometry frame level, which the 2D model assumes"""

    def __init__(self, motion, level=False):
        self.motion, self.level = motion, level

    _poses = {}      # one odom_pose cache per motion (the fine RK4 behind it is the slow part of a case)

    def __enter__(self):
        self.keep = (tw.vehicle, tw.R_ITOO, tw.odom_pose)
        tw.vehicle = vehicle_of(self.motion)
        if self.level:
            tw.R_ITOO = Rotation.from_rotvec([0.0, 0.0, 0.6]).as_matrix()
        if self.motion not in self._poses:
            self._poses[self.motion] = functools.lru_cache(maxsize=None)(self.keep[2].__wrapped__)
        tw.odom_pose = self._poses[self.motion]

    def __exit__(self, *a):
        tw.vehicle, tw.R_ITOO, tw.odom_pose = self.keep


def wheel_case(pkg, po, motion, kind, calib, stream="51", noise=0.0, d_scale=0.01, seed=0, pose_ids=(15, 27), n=None):
    """-> opt, st, t, m1, m2 (the selected samples).  noise: on the wheel readings (0 at standstill keeps them exactly zero);
    d_scale: the clone errors that make the residual."""
    count, uneven = WHEEL_STREAMS[stream]
    ext, dt, intr = calib
    rng = np.random.default_rng(seed)
    with moving(motion, level=kind >= 3):
        dur = 6.0 if count > 100 else 1.0
        t, m1, m2 = tw.wheel_stream(20.0, 20.0 + dur, kind=kind)
        if uneven:
            t = t.copy()
            t[1:-1] += rng.uniform(-0.004, 0.004, len(t) - 2)
        if noise:
            m1, m2 = m1 + rng.normal(0, noise, m1.shape), m2 + rng.normal(0, noise, m2.shape)
        t0 = 20.3007
        # `count` selected samples: the interpolated start, count - 2 stream samples, the interpolated end
        i0 = int(np.searchsorted(t, t0, side="right"))
        t1 = t0 + 0.001 if count == 2 else 0.5 * (t[i0 + count - 3] + t[i0 + count - 2])
        ok, st_, s1, s2 = po.select_wheel_data(t, m1, m2, t0, t1)
        assert ok and (uneven or len(st_) == count), (len(st_), count)
        d0, d1 = rng.normal(0, d_scale, 6), rng.normal(0, d_scale, 6)
        opt, st = tw.make(pkg, kind, ext, dt, intr, t0=t0, t1=t1, d0=d0, d1=d1)
    st.R0_fej[1] += 1e-3
    st.p1_fej[0] -= 2e-3
    st.pose0_id, st.pose1_id = pose_ids
    if n is not None:        # calibration states behind the clones, at the end of the state
        st.ext_id = n - 10 if ext else -1
        st.dt_id = n - 4 if dt else -1
        st.intr_id = n - 3 if intr else -1
    return opt, st, st_, s1, s2


WheelUpd = namedtuple("WheelUpd", "name motion kind calib n pose_ids d_scale")
WHEEL_UPDATE_CASES = [
    WheelUpd("3dang-turn-in", "turning", 0, (True, True, True), 39, (15, 21), 0.001),
    WheelUpd("3dang-turn-out", "turning", 0, (True, False, False), 119, (15, 99), 0.5),
    WheelUpd("3dlin-straight-in", "straight", 1, (False, True, False), 149, (21, 129), 0.001),
    WheelUpd("3dlin-still-in", "standstill", 1, (True, False, True), 39, (15, 21), 0.001),
    WheelUpd("3dcen-reverse-in", "reversing", 2, (False, False, True), 119, (93, 99), 0.001),
    WheelUpd("3dcen-creep-out", "creeping", 2, (True, True, False), 149, (15, 21), 0.5),
    WheelUpd("2dang-still-in", "standstill", 3, (True, True, True), 39, (15, 21), 0.001),
    WheelUpd("2dang-still-out", "standstill", 3, (False, False, False), 119, (15, 99), 0.5),
    WheelUpd("2dang-creep-in", "creeping", 3, (False, True, True), 149, (123, 129), 0.001),
    WheelUpd("2dlin-still-in", "standstill", 4, (True, False, False), 149, (15, 129), 0.001),
    WheelUpd("2dlin-creep-in", "creeping", 4, (True, True, False), 39, (15, 21), 0.001),
    WheelUpd("2dlin-turn-out", "turning", 4, (False, False, True), 119, (15, 21), 3.0),
    WheelUpd("2dcen-still-in", "standstill", 5, (False, True, True), 119, (93, 99), 0.001),
    WheelUpd("2dcen-creep-in", "creeping", 5, (True, False, True), 39, (21, 15), 0.001),
    WheelUpd("2dcen-spin-in", "spin", 5, (True, True, False), 149, (15, 21), 0.001),
    WheelUpd("2dcen-straight-out", "straight", 5, (False, False, False), 39, (15, 27), 3.0),
]


def wheel_restatement(P, H, res, Cov, cols, n, mult, q95, dtype=np.float64):
    """UpdaterWheel::update from the linear system on: S = H P H^T + Cov, the gate, K = P H^T S^-1.  -> chi2, accepted, dx, P'.
    dtype=np.longdouble gives the same in extended precision (Cholesky written out: numpy's linalg has none)."""
    Hf = np.zeros((len(res), n), dtype=dtype)
    Hf[:, cols] = H
    Pl, r = P.astype(dtype), res.astype(dtype)
    S = Hf @ Pl @ Hf.T + Cov.astype(dtype)
    m = len(r)
    L = np.zeros_like(S)
    for i in range(m):
        for j in range(i + 1):
            v = S[i, j] - L[i, :j] @ L[j, :j]
            L[i, j] = np.sqrt(v) if i == j else v / L[j, j]

    def solve(B):
        Y = np.zeros_like(B)
        for i in range(m):
            Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
        X = np.zeros_like(B)
        for i in range(m - 1, -1, -1):
            X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
        return X
    if dtype is np.float64:
        chi2 = float(res @ np.linalg.solve(S, res))
        K = P @ Hf.T @ np.linalg.inv(S)
        return chi2, chi2 < mult * q95[m], K @ res, P - K @ Hf @ P
    M = Pl @ Hf.T
    KT = solve(M.T)
    chi2 = float(r @ solve(r))
    return chi2, chi2 < mult * q95[m], (KT.T @ r).astype(np.float64), (Pl - M @ KT).astype(np.float64)


def slam_update_system(n, k, rows, seed, offset=0.0):
    """a whitened measurement of `rows` rows on k states of an n-state covariance -> P, cols, H, res"""
    rng = np.random.default_rng(seed)
    P = synth.spd_cov(n, seed=seed) * 1e-3
    cols = synth.col_map(n, k, seed=seed + 1, skip=10)
    return np.asfortranarray(P), cols, rng.normal(size=(rows, k)), rng.normal(0, 0.5, rows) + offset


def duplicate_index(t, lo, hi):
    """a stream sample well inside the window (lo, hi): select_imu_readings keeps it and its copy"""
    inside = [i for i in range(len(t) - 1) if lo < t[i] and t[i + 1] < hi]
    return inside[len(inside) // 2]


def records_equal(a, b):
    """Two CPI records bit for bit in what CpiV1 integrates: a sample delivered twice is a step of dt = 0, which feed_IMU leaves at
    once.  (The record's v is not among them: create_new_cpi_integrate advances its R_GtoIk by the accumulated R_k2tau before EVERY
    feed, the empty one included, so v = v_clone - g DT + R_GtoIk^T beta moves with the number of samples whenever the IMU turns.)"""
    return all(np.array_equal(np.array(getattr(a, f)), np.array(getattr(b, f))) for f in ("t", "dt", "clone_t", "R_I0toIk", "alpha", "w", "Q"))


def wheel_prior(n):
    return np.asfortranarray(synth.spd_cov(n, seed=8) * 1e-3)


def wheel_update_case(pkg, po, c):
    return wheel_case(pkg, po, c.motion, c.kind, c.calib, d_scale=c.d_scale, seed=sum(map(ord, c.name)), pose_ids=c.pose_ids, n=c.n)
