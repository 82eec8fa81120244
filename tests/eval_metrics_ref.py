"""TEST INFRASTRUCTURE ONLY: numpy restatement of the reference's RPE, NEES and 2-D ATE, the yardstick of
tests/test_eval_metrics_cpu.py (closed forms) and tests/test_gpu_eval_metrics.py (plv_traj_rpe / _nees / _ate_2d).

  ResultTrajectory ctor (both alignments)        REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:52-83
  ResultTrajectory::calculate_ate_2d             REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:99-137
  ResultTrajectory::calculate_rpe                REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:139-239
  ResultTrajectory::calculate_nees               REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:241-286
  compute_comparison_indices_length              REF: open_vins/ov_eval/src/calc/ResultTrajectory.h:169-198
  ov_core::Inv_se3                               REF: open_vins/ov_core/src/utils/quat_ops.h:439-444

The end-of-segment search is the reference's double loop, literally: it is what the device's two binary searches
have to reproduce index for index.  Alignment, quaternion algebra and the statistics come from oracle/eval_oracle.py.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import eval_oracle as eo  # noqa: E402

MAX_DIST_DIFF = 0.5  # ResultTrajectory.cpp:154


def align_poses(src, dst, method):
    """The ctor's loop (:72-82) for one direction: src expressed in dst's frame."""
    R, t, s = eo.align_trajectory(src, dst, method)
    q_inv = eo.quat_inv(eo.rot_2_quat(R))
    out = np.zeros_like(src)
    for i in range(len(src)):
        out[i, :3] = s * R @ src[i, :3] + t
        out[i, 3:] = eo.quat_multiply(src[i, 3:], q_inv)
    return out


def accumulated_distances(gt):
    """:143-149: acc[i] = acc[i - 1] + |p_i - p_(i-1)|, summed in that order."""
    acc = np.zeros(len(gt))
    for i in range(1, len(gt)):
        d = gt[i, :3] - gt[i - 1, :3]
        acc[i] = acc[i - 1] + math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return acc


def comparison_indices(acc, distance, max_dist_diff=MAX_DIST_DIFF):
    """compute_comparison_indices_length, the double loop as written (strict <, so the first minimiser wins)."""
    out = np.full(len(acc), -1, dtype=np.int32)
    for idx in range(len(acc)):
        start = acc[idx]
        best_idx, best_error = -1, max_dist_diff
        for i in range(idx, len(acc)):
            e = abs(acc[i] - (start + distance))
            if e < best_error:
                best_idx, best_error = i, e
        out[idx] = best_idx
    return out


def comparison_indices_fast(acc, distance, max_dist_diff=MAX_DIST_DIFF):
    """The same rule with the inner loop as one numpy reduction per start (argmin returns the first minimiser): for
    inputs on which the literal double loop would take hours.  tests/test_eval_metrics_cpu.py pins it to the loop."""
    out = np.full(len(acc), -1, dtype=np.int32)
    for idx in range(len(acc)):
        e = np.abs(acc[idx:] - (acc[idx] + distance))
        k = int(np.argmin(e))
        if e[k] < max_dist_diff:
            out[idx] = idx + k
    return out


def _T(pose):
    T = np.eye(4)
    T[:3, :3] = eo.quat_2_rot(pose[3:]).T
    T[:3, 3] = pose[:3]
    return T


def _inv_se3(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -Ti[:3, :3] @ T[:3, 3]
    return Ti


def calculate_rpe(est, gt, segments, method="posyaw", search=comparison_indices):
    """-> one dict per segment length: end_idx [n], ori_err / pos_err [n] (NaN where end_idx < 0), n, ori, pos."""
    aligned = align_poses(est, gt, method)
    acc = accumulated_distances(gt)
    out = []
    for L in segments:
        end = search(acc, float(L))
        ori, pos = np.full(len(gt), np.nan), np.full(len(gt), np.nan)
        for a in range(len(gt)):
            b = end[a]
            if b < 0:
                continue
            T_c2 = _T(aligned[b])
            T_c1_c2 = _inv_se3(_T(aligned[a])) @ T_c2
            T_m1_m2 = _inv_se3(_T(gt[a])) @ _T(gt[b])
            T_err_c2 = _inv_se3(T_m1_m2) @ T_c1_c2
            rot, rot_inv = np.eye(4), np.eye(4)
            rot[:3, :3], rot_inv[:3, :3] = T_c2[:3, :3], T_c2[:3, :3].T
            T_err_w = rot @ T_err_c2 @ rot_inv
            pos[a] = np.linalg.norm(T_err_w[:3, 3])
            ori[a] = 180.0 / math.pi * np.linalg.norm(eo.log_so3(T_err_w[:3, :3]))
        ok = end >= 0
        out.append(dict(length=float(L), end_idx=end, ori_err=ori, pos_err=pos, n=int(ok.sum()), ori=eo.statistics(ori[ok]),
                        pos=eo.statistics(pos[ok])))
    return out


def inverse3(m):
    """Eigen's fixed-size 3x3 inverse(): cofactors over the determinant."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]

    c0 = np.array([cof(0, 0), cof(1, 0), cof(2, 0)])
    with np.errstate(divide="ignore", invalid="ignore"):
        invdet = np.float64(1.0) / np.float64(c0[0] * m[0, 0] + c0[1] * m[1, 0] + c0[2] * m[2, 0])
        inv = np.zeros((3, 3))
        inv[0] = c0 * invdet
        for j in (1, 2):
            for i in range(3):
                inv[j, i] = cof(i, j) * invdet
    return inv


def calculate_nees(est, gt, cov_ori, cov_pos, method="posyaw"):
    """-> nees_ori / nees_pos [n] (NaN where the reference skips the pose), n, ori, pos."""
    gt_in_est = align_poses(gt, est, method)
    n = len(est)
    no, npos = np.full(n, np.nan), np.full(n, np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            e_R = eo.quat_2_rot(gt_in_est[i, 3:]) @ eo.quat_2_rot(est[i, 3:]).T
            e = -eo.log_so3(e_R)
            o = float(e @ inverse3(cov_ori[i]) @ e)
            d = gt_in_est[i, :3] - est[i, :3]
            p = float(d @ inverse3(cov_pos[i]) @ d)
            if math.isnan(o) or math.isnan(p):
                continue
            no[i], npos[i] = o, p
    ok = ~np.isnan(no)
    return dict(nees_ori=no, nees_pos=npos, n=int(ok.sum()), ori=eo.statistics(no[ok]), pos=eo.statistics(npos[ok]))


def calculate_ate_2d(est, gt, method="posyaw"):
    aligned = align_poses(est, gt, method)
    ori, pos = np.zeros(len(est)), np.zeros(len(est))
    for i in range(len(est)):
        e_R = eo.quat_2_rot(aligned[i, 3:]).T @ eo.quat_2_rot(gt[i, 3:])
        ori[i] = 180.0 / math.pi * eo.log_so3(e_R)[2]
        pos[i] = np.linalg.norm(gt[i, :2] - aligned[i, :2])
    return dict(ori_err=ori, pos_err=pos, ori=eo.statistics(ori), pos=eo.statistics(pos))
