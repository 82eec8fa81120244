"""The zero-velocity measurement restated in numpy (helper of test_zupt_cpu.py / test_gpu_zupt.py, not collected).

The restatement is of the FULL stack, interval by interval, and knows nothing of the closed form the device emits:

    full_stack      H (6 (n - 1) + 3 rows x 12), r: one gyro block and one accelerometer block per IMU interval, three velocity rows
    compress        thin SVD of H truncated at rank 9: H_c = diag(s) V^T, r_c = U^T r  (what measurement_compress_inplace leaves, in the
                    basis the SVD happens to pick)
    dense_update    Chi2Check and StateHelper::EKFUpdate with R = I on a dense P

closed_form is the device's 9 x 12 system written out a second time, with correctly rounded sums (math.fsum), for the parity of
plv_zupt_system; its relation to the stack (same H^T H and H^T r, same chi-square) is what test_zupt_cpu.py establishes.

Columns (k = 12): theta, v, bg, ba of the IMU block, at imu_id + 0..2, 6..8, 9..11, 12..14 of the state.
"""
import itertools
import math

import numpy as np
from scipy.spatial.transform import Rotation
from scipy.stats import chi2 as _chi2

GRAVITY = np.array([0.0, 0.0, 9.81])
SIGMA_W, SIGMA_A = 1.6968e-4, 2.0e-3          # continuous-time densities (the library's imu_noise defaults)
SIGMA_V = 0.05
Q95_9 = float(_chi2.ppf(0.95, 9))
IMU_RATE = 200.0

NS = (2, 3, 64, 65, 66, 257)                  # one interval; the lane count (64 intervals = n 65) from both sides; several passes
STAMPS = ("regular", "jittered")
IMU_IDS = (0, 6)
STATE_SIZES = (15, 21, 105, 160)
FEJ = (False, True)                           # q_fej equal to q / rotated 2 degrees from it
NOISE_MULTS = (1.0, 25.0)
MOTIONS = ("standing", "bias_error", "turning", "accelerating", "moving")


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def jpl_rot(q):
    """R of a JPL quaternion (x y z w): (2 w^2 - 1) I - 2 w [v x] + 2 v v^T   (ov_core quat_2_Rot)"""
    q = np.asarray(q, dtype=np.float64)
    v, w = q[:3], q[3]
    return (2 * w * w - 1) * np.eye(3) - 2 * w * skew(v) + 2 * np.outer(v, v)


def jpl_quat(R):
    """the JPL quaternion of R (Hamilton components of R^T), w >= 0"""
    q = Rotation.from_matrix(R.T).as_quat()
    return -q if q[3] < 0 else q


def columns(imu_id):
    return np.array([imu_id + o for o in (0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14)], dtype=np.int32)


def stamps(n, kind, t0=20.3007):
    dt = np.full(n - 1, 1.0 / IMU_RATE)
    if kind == "jittered":
        rng = np.random.default_rng(100 + n)
        dt = dt * rng.uniform(0.7, 1.3, n - 1)
        dt[0] = 1e-4                               # one very short and one long interval
        if n > 2:
            dt[-1] = 9e-3
    return t0 + np.concatenate([[0.0], np.cumsum(dt)])


def prior(size, seed, tight=False):
    """a dense symmetric positive definite P with correlations across the whole state; variances of 1e-7 .. 1e-5, or (tight) of
    1e-10 .. 1e-8: a filter that has converged and no longer explains a bias error of 1e-3 by its own uncertainty"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(size, size))
    C = A @ A.T / size + np.eye(size)
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    s = np.sqrt(10.0 ** (rng.uniform(-7.0, -5.0, size) - (3.0 if tight else 0.0)))
    return np.asfortranarray(C * np.outer(s, s))


def make_case(n, stamp_kind, imu_id, size, fej, noise_mult, motion, seed):
    """One case: the samples, the IMU state, the prior and the options, as plain arrays."""
    rng = np.random.default_rng(seed)
    t = stamps(n, stamp_kind)
    dt = np.diff(t)
    R = Rotation.from_rotvec(rng.normal(0, 0.08, 3)).as_matrix() @ Rotation.from_rotvec([0, 0, rng.uniform(-3, 3)]).as_matrix()   # R_GtoI
    q = jpl_quat(R)
    q_fej = q
    if fej:
        axis = rng.normal(size=3)
        q_fej = jpl_quat(Rotation.from_rotvec(np.deg2rad(2.0) * axis / np.linalg.norm(axis)).as_matrix() @ R)
    bg_true, ba_true = rng.normal(0, 3e-3, 3), rng.normal(0, 3e-2, 3)
    # sensor noise at the configured densities: sigma / sqrt(dt) per sample (the last sample's closes no interval)
    sd = 1.0 / np.sqrt(np.concatenate([dt, dt[-1:]]))[:, None]
    wm = bg_true + SIGMA_W * sd * rng.normal(size=(n, 3))
    am = ba_true + R @ GRAVITY + SIGMA_A * sd * rng.normal(size=(n, 3))
    bg, ba, v = bg_true.copy(), ba_true.copy(), rng.normal(0, 5e-3, 3)
    if motion == "bias_error":
        bg = bg + np.array([1e-3, -1e-3, 1e-3])
        ba = ba + np.array([-1e-3, 1e-3, 1e-3])
    elif motion == "turning":
        wm = wm + np.array([0.0, 0.0, 0.2])
    elif motion == "accelerating":
        am = am + R @ np.array([0.5, 0.0, 0.0])
    elif motion == "moving":
        v = 0.3 * np.array([np.cos(0.4), np.sin(0.4), 0.0])
    elif motion != "standing":
        raise ValueError(motion)
    return dict(name=f"n{n}-{stamp_kind}-id{imu_id}-s{size}-fej{int(fej)}-a{noise_mult:g}-{motion}", n=n, t=t, wm=wm, am=am, q=q, q_fej=q_fej,
                v=v, bg=bg, ba=ba, imu_id=imu_id, size=size, noise_mult=noise_mult, sigma_v=SIGMA_V, chi2_mult=1.0, motion=motion,
                P=prior(size, seed + 7, tight=bool(rng.integers(2))))


def case_matrix():
    """Every n x stamps x noise_mult x motion; imu_id, state size and first-estimate choice cycle through their 14 admissible
    combinations (an IMU block at 6 does not fit a state of 15) with a stride coprime to it, so each meets every n and every motion."""
    combos = [(i, s, f) for i in IMU_IDS for s in STATE_SIZES for f in FEJ if i + 15 <= s]
    out = []
    for k, (n, sk, a, mo) in enumerate(itertools.product(NS, STAMPS, NOISE_MULTS, MOTIONS)):
        imu_id, size, fej = combos[(3 * k) % len(combos)]
        out.append(make_case(n, sk, imu_id, size, fej, a, mo, seed=1000 + k))
    return out


# ------------------------------------------------------------------------------------------------ the restatement
def full_stack(c):
    """H (6 (n - 1) + 3, 12) and r of the whole stack, interval by interval"""
    n, t = c["n"], c["t"]
    R, Rf = jpl_rot(c["q"]), jpl_rot(c["q_fej"])
    H, r = np.zeros((6 * (n - 1) + 3, 12)), np.zeros(6 * (n - 1) + 3)
    for i in range(n - 1):
        dt = t[i + 1] - t[i]
        w_g, w_a = np.sqrt(dt / c["noise_mult"]) / SIGMA_W, np.sqrt(dt / c["noise_mult"]) / SIGMA_A
        H[6 * i:6 * i + 3, 6:9] = -w_g * np.eye(3)
        r[6 * i:6 * i + 3] = -w_g * (c["wm"][i] - c["bg"])
        H[6 * i + 3:6 * i + 6, 0:3] = -w_a * skew(Rf @ GRAVITY)
        H[6 * i + 3:6 * i + 6, 9:12] = -w_a * np.eye(3)
        r[6 * i + 3:6 * i + 6] = -w_a * (c["am"][i] - c["ba"] - R @ GRAVITY)
    H[-3:, 3:6] = np.eye(3) / c["sigma_v"]
    r[-3:] = -c["v"] / c["sigma_v"]
    return H, r


def compress(H, r, rank=9):
    """thin SVD truncated at `rank`: (H_c, r_c, U1) with H = U1 H_c up to the singular values dropped"""
    U, s, Vt = np.linalg.svd(H, full_matrices=False)
    assert s[rank - 1] > 1e-9 * s[0] and (len(s) == rank or s[rank] < 1e-9 * s[0]), s
    U1 = U[:, :rank]
    return s[:rank, None] * Vt[:rank], U1.T @ r, U1


def chi2_of(P, H, r, cols):
    S = H @ P[np.ix_(cols, cols)] @ H.T + np.eye(len(r))
    return float(r @ np.linalg.solve(S, r))


def dense_update(P, H, r, cols, chi2_mult=1.0, force=False):
    """Chi2Check + EKFUpdate with R = I: (chi2, accepted, dx, P_new)"""
    n = P.shape[0]
    Hf = np.zeros((len(r), n))
    Hf[:, cols] = H
    S = Hf @ P @ Hf.T + np.eye(len(r))
    chi = float(r @ np.linalg.solve(S, r))
    if not force and not chi < chi2_mult * Q95_9:
        return chi, False, np.zeros(n), P.copy()
    K = np.linalg.solve(S, Hf @ P).T
    Pn = P - K @ Hf @ P
    return chi, True, K @ r, 0.5 * (Pn + Pn.T)


def reference_update(c, force=False):
    """the full stack compressed by SVD, gated and applied on the case's dense P"""
    Hc, rc, _ = compress(*full_stack(c))
    return dense_update(np.array(c["P"]), Hc, rc, columns(c["imu_id"]), c["chi2_mult"], force)


def closed_form(c):
    """The device's 9 x 12 system with correctly rounded sums: (H, r, scale); scale [9] is the magnitude of the largest term that
    enters each residual (c_w |w_bar|, c_a |a_bar|, ...): the residual is a difference of such terms, so that is what an error
    of the residual is relative to."""
    t, wm, am = c["t"], c["wm"], c["am"]
    dt = np.diff(t)
    T = math.fsum(dt)
    w_bar = np.array([math.fsum(dt * wm[:-1, k]) for k in range(3)]) / T
    a_bar = np.array([math.fsum(dt * am[:-1, k]) for k in range(3)]) / T
    cw, ca = np.sqrt(T / c["noise_mult"]) / SIGMA_W, np.sqrt(T / c["noise_mult"]) / SIGMA_A
    g, gf = jpl_rot(c["q"]) @ GRAVITY, jpl_rot(c["q_fej"]) @ GRAVITY
    H, r = np.zeros((9, 12)), np.zeros(9)
    H[0:3, 6:9] = -cw * np.eye(3)
    r[0:3] = -cw * (w_bar - c["bg"])
    H[3:6, 0:3] = -ca * skew(gf)
    H[3:6, 9:12] = -ca * np.eye(3)
    r[3:6] = -ca * (a_bar - c["ba"] - g)
    H[6:9, 3:6] = np.eye(3) / c["sigma_v"]
    r[6:9] = -c["v"] / c["sigma_v"]
    scale = np.concatenate([cw * np.maximum(np.abs(w_bar), np.abs(c["bg"])), ca * np.maximum.reduce([np.abs(a_bar), np.abs(c["ba"]), np.abs(g)]),
                            np.abs(c["v"]) / c["sigma_v"]])
    return H, r, np.maximum(scale, 1.0)


_CASES = None


def cases():
    """the case matrix with the reference's verdict and chi-square on each case ("chi2", "accepted"); built once.  Asserts that the
    matrix decides both ways for every value of every factor (n, stamp kind, IMU block, state size, first-estimate choice,
    noise_mult) and for the bias error, the turn and the acceleration (a loose prior or noise_mult 25 over one short interval lets
    them through, a converged filter does not), and that no case sits on the threshold.  Two kinds decide one way by what they
    are: 0.3 m/s against sigma_v = 0.05 is 36 in the chi-square of the velocity rows alone and is rejected everywhere; a standing
    vehicle with true biases and noise at the configured sigmas has a chi-square(9) residual at most and is accepted wherever the
    draw stays under the 95 % quantile: it must be accepted in most cases, and is never asked to be rejected."""
    global _CASES
    if _CASES is None:
        cs = case_matrix()
        for c in cs:
            c["chi2"], c["accepted"], c["dx"], c["P_new"] = reference_update(c)
            assert abs(c["chi2"] / (c["chi2_mult"] * Q95_9) - 1.0) > 1e-6, (c["name"], c["chi2"])
        by = {m: [c["accepted"] for c in cs if c["motion"] == m] for m in MOTIONS}
        assert sum(by["standing"]) >= 0.8 * len(by["standing"]), "standing cases fail the gate"
        for m in ("bias_error", "turning", "accelerating"):
            assert any(by[m]) and not all(by[m]), f"the {m} cases decide one way only"
        assert not any(by["moving"]), "0.3 m/s passed the gate"
        assert any(c["accepted"] for c in cs) and not all(c["accepted"] for c in cs)
        for c in cs:
            c["stamps"], c["fej"] = ("jittered" if "jittered" in c["name"] else "regular"), not np.array_equal(c["q"], c["q_fej"])
        for vals, key in ((NS, "n"), (STAMPS, "stamps"), (IMU_IDS, "imu_id"), (STATE_SIZES, "size"), (FEJ, "fej"), (NOISE_MULTS, "noise_mult")):
            for v in vals:
                sub = [c["accepted"] for c in cs if c[key] == v]
                assert any(sub) and not all(sub), (key, v)
        _CASES = cs
    return _CASES
