"""The numpy restatement of the reference's RPE / NEES / 2-D ATE (tests/eval_metrics_ref.py) against closed forms, so that the
GPU tests (tests/test_gpu_eval_metrics.py) compare the library with a yardstick that was itself checked.  No GPU."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import eval_oracle as eo  # noqa: E402
import eval_metrics_ref as em  # noqa: E402


def exp_so3(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3) + eo.skew(w)
    K = eo.skew(np.asarray(w) / th)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def wavy_trajectory(n, length=30.0):
    s = np.linspace(0, length, n)
    gt = np.zeros((n, 7))
    gt[:, 0], gt[:, 1], gt[:, 2] = s * np.cos(0.05 * s), 6 * np.sin(0.3 * s), 0.1 * s
    for i in range(n):
        gt[i, 3:] = eo.rot_2_quat(exp_so3([0.05 * math.sin(s[i]), 0.04 * math.cos(s[i]), 0.2 * s[i]]))
    return gt


def test_rigid_transform_gives_zero_rpe_and_ate2d():
    from make_ate_toy import transform
    gt = wavy_trajectory(120)
    Rz, t = eo.rot_z(0.8), np.array([4.0, -2.0, 1.0])
    est = transform(gt, Rz.T, -Rz.T @ t)
    for m in ("posyaw", "se3", "sim3"):
        for seg in em.calculate_rpe(est, gt, [1.0, 5.0], m):
            assert seg["n"] > 50
            assert seg["pos"]["max"] < 1e-9 and seg["ori"]["max"] < 1e-5
        r = em.calculate_ate_2d(est, gt, m)
        assert np.abs(r["pos_err"]).max() < 1e-9 and np.abs(r["ori_err"]).max() < 1e-5
    # the RPE compares start-to-end transforms, so it does not need the alignment either
    for seg in em.calculate_rpe(est, gt, [5.0], "none"):
        assert seg["pos"]["max"] < 1e-9 and seg["ori"]["max"] < 1e-5


def test_yaw_drift_gives_k_times_length():
    """Straight drive sampled every 0.25 m (exact in binary, so segments of exactly L exist); the estimate's heading drifts
    by k degrees per metre.  The relative rotation over a segment is a yaw of k * L degrees whatever the alignment."""
    n, step, k = 200, 0.25, 0.3
    gt = np.zeros((n, 7))
    gt[:, 0] = step * np.arange(n)
    gt[:, 6] = 1.0
    est = gt.copy()
    for i in range(n):
        est[i, 3:] = eo.rot_2_quat(eo.rot_z(math.radians(k * gt[i, 0])))
    for m in ("none", "posyaw", "se3"):
        for L, seg in zip((2.0, 8.0, 16.0), em.calculate_rpe(est, gt, [2.0, 8.0, 16.0], m)):
            # starts 0 .. n-1-h have an end exactly L away; the next start still finds the last pose, one step (0.25 m < 0.5 m)
            # short, and the one after it misses by exactly the limit
            h = int(L / step)
            assert seg["n"] == n - h + 1
            assert np.array_equal(seg["end_idx"][:n - h], np.arange(n - h) + h) and seg["end_idx"][n - h] == n - 1
            assert (seg["end_idx"][n - h + 1:] == -1).all()
            assert np.abs(seg["ori_err"][:n - h] - k * L).max() < 1e-9, (m, L)
            assert abs(seg["ori_err"][n - h] - k * (L - step)) < 1e-9
    # the 2-D ATE keeps the sign of the heading error: log_so3(R_est^T R_gt)_z
    r = em.calculate_ate_2d(est, gt, "none")
    assert np.abs(np.abs(r["ori_err"]) - k * gt[:, 0]).max() < 1e-9
    assert (np.sign(r["ori_err"][1:]) == np.sign(r["ori_err"][1])).all()
    assert np.abs(r["pos_err"]).max() == 0


def test_nees_of_consistent_errors_is_three():
    """Errors drawn from N(0, P_i) with the logged P_i: each NEES value is chi-square with 3 degrees of freedom, the sum of N
    independent ones chi-square with 3 N (mean 3 N, variance 6 N).  For N = 4000 that law is normal to well within the margin
    used here, so the sample mean lies within 5 sqrt(6 / N) = 0.194 of 3 except with probability 6e-7; the seed is fixed."""
    N = 4000
    rng = np.random.default_rng(20240607)
    gt = wavy_trajectory(N, 80.0)
    est = gt.copy()
    cov_ori, cov_pos = np.zeros((N, 3, 3)), np.zeros((N, 3, 3))
    for i in range(N):
        A, B = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
        cov_ori[i] = 1e-4 * (A @ A.T + 0.5 * np.eye(3))
        cov_pos[i] = 1e-2 * (B @ B.T + 0.5 * np.eye(3))
        e = np.linalg.cholesky(cov_ori[i]) @ rng.normal(size=3)
        d = np.linalg.cholesky(cov_pos[i]) @ rng.normal(size=3)
        # e = -log_so3(R_gt R_est^T)  =>  R_est = Exp(e) R_gt;  d = p_gt - p_est
        est[i, 3:] = eo.rot_2_quat(exp_so3(e) @ eo.quat_2_rot(gt[i, 3:]))
        est[i, :3] = gt[i, :3] - d
    r = em.calculate_nees(est, gt, cov_ori, cov_pos, "none")
    bound = 5 * math.sqrt(6.0 / N)
    assert r["n"] == N
    assert abs(r["ori"]["mean"] - 3) < bound and abs(r["pos"]["mean"] - 3) < bound, (r["ori"]["mean"], r["pos"]["mean"], bound)
    # a covariance four times too small (an overconfident filter) shows as a NEES four times as large
    r4 = em.calculate_nees(est, gt, cov_ori / 4, cov_pos / 4, "none")
    assert abs(r4["ori"]["mean"] / r["ori"]["mean"] - 4) < 1e-9
    # a NaN covariance is skipped and counted out
    cov_ori[7] = np.nan
    r = em.calculate_nees(est, gt, cov_ori, cov_pos, "none")
    assert r["n"] == N - 1 and np.isnan(r["nees_ori"][7]) and np.isnan(r["nees_pos"][7])


def test_inverse3_is_the_inverse():
    rng = np.random.default_rng(3)
    for _ in range(20):
        A = rng.normal(size=(3, 3))
        P = A @ A.T + 0.1 * np.eye(3)
        assert np.abs(em.inverse3(P) @ P - np.eye(3)).max() < 1e-10


def bisect_indices(acc, distance, max_dist_diff=em.MAX_DIST_DIFF):
    """The rule traj_rpe_kernel implements: |acc[i] - target| never rises before j = the first acc[j] >= target and never falls
    after it, so the scan's answer is the first index that reaches the error of j - 1, or j if j is strictly better."""
    n = len(acc)
    out = np.full(n, -1, dtype=np.int32)
    for start in range(n):
        target = acc[start] + distance
        lo, hi = start, n
        while lo < hi:
            mid = (lo + hi) // 2
            if acc[mid] >= target:
                hi = mid
            else:
                lo = mid + 1
        j, best, best_err = lo, -1, max_dist_diff
        if j > start:
            e_left = abs(acc[j - 1] - target)
            lo, hi = start, j - 1
            while lo < hi:
                mid = (lo + hi) // 2
                if abs(acc[mid] - target) <= e_left:
                    hi = mid
                else:
                    lo = mid + 1
            if e_left < best_err:
                best, best_err = lo, e_left
        if j < n and abs(acc[j] - target) < best_err:
            best = j
        out[start] = best
    return out


def tie_trajectories():
    """Accumulated distances that exercise the tie rule, the 0.5 m limit, standing stretches and gaps."""
    rng = np.random.default_rng(11)
    out = {}
    out["quarter_metre"] = 0.25 * np.arange(60)                               # exact ties between neighbours for L = k / 8
    out["one_metre"] = 1.0 * np.arange(30)                                    # L = 0.5 / 1.5: the error is exactly the limit
    steps = rng.choice([0.0, 0.0, 0.125, 0.25, 0.375], size=300)             # standing still: runs of equal acc
    out["standing"] = np.concatenate([[0.0], np.cumsum(steps)])
    steps = rng.uniform(0.01, 0.3, size=200)
    steps[[40, 120]] = [0.9, 2.5]                                             # gaps wider than the limit
    out["gaps"] = np.concatenate([[0.0], np.cumsum(steps)])
    out["tiny_steps"] = np.concatenate([[0.0], np.cumsum(np.full(50, 1e-20))])  # every error rounds to the same value
    out["random"] = np.concatenate([[0.0], np.cumsum(rng.uniform(0, 0.4, size=400))])
    return out


def test_search_rules_agree_with_the_double_loop():
    for name, acc in tie_trajectories().items():
        for L in (0.0, 0.125, 0.3, 0.375, 0.5, 1.0, 1.5, 2.0, 7.875, 1000.0, -0.25):
            ref = em.comparison_indices(acc, L)
            assert np.array_equal(em.comparison_indices_fast(acc, L), ref), (name, L)
            assert np.array_equal(bisect_indices(acc, L), ref), (name, L)
    acc = tie_trajectories()
    # spot checks of the reference's rule itself: an earlier index wins a tie, the first of a standing run wins, and the limit is strict
    assert em.comparison_indices(acc["quarter_metre"], 0.125)[0] == 0          # |0 - 0.125| == |0.25 - 0.125|: index 0 stays
    assert em.comparison_indices(acc["quarter_metre"], 0.375)[0] == 1
    assert (em.comparison_indices(acc["one_metre"], 0.5) == -1).all()          # best error 0.5 is not < 0.5
    assert em.comparison_indices(np.array([0.0, 1.0, 1.0, 1.0, 2.0]), 1.0)[0] == 1
    assert em.comparison_indices(acc["gaps"], 1.0)[120] == -1                  # 1 m short of the target, then 1.5 m beyond it


def test_fixture_segment_counts_and_empty_statistics():
    """tests/golden/ate_toy.json: 40 poses over 10.59 m.  The reference's rule finds 37 / 33 / 26 / 13 / 0 segments of 1, 2, 4, 8
    and 16 m; no segment leaves the statistics at zero, one value gives NaN std (division by n - 1)."""
    with open(os.path.join(ROOT, "tests", "golden", "ate_toy.json")) as f:
        d = json.load(f)
    gt, est = np.array(d["gt"]), np.array(d["est"])
    r = em.calculate_rpe(est, gt, [1, 2, 4, 8, 16], "posyaw")
    assert [s["n"] for s in r] == [37, 33, 26, 13, 0]
    assert all(v == 0 for v in r[4]["pos"].values()) and all(v == 0 for v in r[4]["ori"].values())
    one = eo.statistics([2.5])
    assert one["mean"] == 2.5 and math.isnan(one["std"]) and math.isnan(one["ninetynine"])
