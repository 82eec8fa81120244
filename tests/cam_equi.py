"""numpy restatement of the equidistant (fisheye) camera model: CamEqui::undistort_f (cv::fisheye::undistortPoints of OpenCV 4.2),
CamEqui::distort_f behind CamBase::distort_d, and CamEqui::compute_distort_jacobian.  K8 = fx fy cx cy k1 k2 k3 k4.  Test helper:
the CPU oracle has no fisheye model, so the library's equidistant path is checked against this."""
import numpy as np


def undistort(K8, uv):
    """[n, 2] float pixels -> [n, 2] float32 normalised coordinates (float in, double arithmetic, float out)."""
    fx, fy, cx, cy, k1, k2, k3, k4 = (float(v) for v in K8)
    uv = np.asarray(uv, np.float32).reshape(-1, 2).astype(np.float64)
    out = np.zeros(uv.shape, np.float32)
    for i, (u, v) in enumerate(uv):
        pwx, pwy = (u - cx) / fx, (v - cy) / fy
        scale = 1.0
        theta_d = np.sqrt(pwx * pwx + pwy * pwy)
        theta_d = min(max(-np.pi / 2.0, theta_d), np.pi / 2.0)
        if theta_d > 1e-8:
            theta = theta_d
            for _ in range(10):
                t2 = theta * theta
                t4 = t2 * t2
                t6 = t4 * t2
                t8 = t6 * t2
                a, b, c, d = k1 * t2, k2 * t4, k3 * t6, k4 * t8
                fix = (theta * (1 + a + b + c + d) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
                theta = theta - fix
                if abs(fix) < 1e-8:
                    break
            scale = np.tan(theta) / theta_d
        out[i] = (np.float32(pwx * scale), np.float32(pwy * scale))
    return out


def distort_norm(K8, xy):
    """CamEqui::distort_f on float-rounded normalised points: r from float products and a float square root, the rest in double.
    Returns the distorted normalised points [n, 2] float64 (x1, y1) before the pixel mapping."""
    K = np.asarray(K8, np.float64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2).astype(np.float32)
    x, y = xy[:, 0], xy[:, 1]
    r = np.sqrt(x * x + y * y).astype(np.float64)      # float32 arithmetic throughout, as Eigen::Vector2f
    theta = np.arctan(r)
    t2 = theta * theta
    t3 = t2 * theta
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    theta_d = theta + K[4] * t3 + K[5] * t5 + K[6] * t7 + K[7] * t9
    inv_r = np.where(r > 1e-8, 1.0 / np.where(r > 1e-8, r, 1.0), 1.0)
    cdist = np.where(r > 1e-8, theta_d * inv_r, 1.0)
    return np.stack([x.astype(np.float64) * cdist, y.astype(np.float64) * cdist], axis=1)


def distort(K8, xy):
    """CamBase::distort_d under CamEqui: normalised [n, 2] -> pixels [n, 2] float32."""
    K = np.asarray(K8, np.float64)
    x1 = distort_norm(K8, xy)
    return np.stack([(K[0] * x1[:, 0] + K[2]).astype(np.float32), (K[1] * x1[:, 1] + K[3]).astype(np.float32)], axis=1)


def distort_jacobian(K8, xy):
    """CamEqui::compute_distort_jacobian at double normalised points: dz/dzn [n, 2, 2], dz/dzeta [n, 2, 8]."""
    K = np.asarray(K8, np.float64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    dzn, dzeta = np.zeros((n, 2, 2)), np.zeros((n, 2, 8))
    for i, (x, y) in enumerate(xy):
        r = np.sqrt(x * x + y * y)
        theta = np.arctan(r)
        t2 = theta * theta
        t3, t4 = t2 * theta, t2 * t2
        t5, t6 = t3 * t2, t4 * t2
        t7, t8 = t5 * t2, t4 * t4
        t9 = t7 * t2
        theta_d = theta + K[4] * t3 + K[5] * t5 + K[6] * t7 + K[7] * t9
        inv_r = 1.0 / r if r > 1e-8 else 1.0
        cdist = theta_d * inv_r if r > 1e-8 else 1.0
        dthd_dth = 1 + 3 * K[4] * t2 + 5 * K[5] * t4 + 7 * K[6] * t6 + 9 * K[7] * t8
        dth_dr = 1 / (r * r + 1)
        a = np.array([-x * theta_d * inv_r * inv_r + x * inv_r * dthd_dth * dth_dr,
                      -y * theta_d * inv_r * inv_r + y * inv_r * dthd_dth * dth_dr])
        b = np.array([x * inv_r, y * inv_r])
        M = np.eye(2) * (theta_d * inv_r) + np.outer(a, b)
        dzn[i] = np.diag([K[0], K[1]]) @ M
        dzeta[i, 0, 0], dzeta[i, 0, 2] = x * cdist, 1.0
        dzeta[i, 1, 1], dzeta[i, 1, 3] = y * cdist, 1.0
        for j, tp in enumerate((t3, t5, t7, t9)):
            dzeta[i, 0, 4 + j] = K[0] * x * inv_r * tp
            dzeta[i, 1, 4 + j] = K[1] * y * inv_r * tp
    return dzn, dzeta


def unproject(K8, uv):
    """Pixel -> unit ray in the camera frame, by the model's exact inverse in double (the renderer of tests/synth_fisheye.py)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    xn = undistort_double(K8, uv)
    ray = np.concatenate([xn, np.ones((len(xn), 1))], axis=1)
    return ray / np.linalg.norm(ray, axis=1, keepdims=True)


def undistort_double(K8, uv, iters=30):
    """Double-precision inverse of the model (Newton to convergence): pixels [n, 2] -> normalised [n, 2]."""
    K = np.asarray(K8, np.float64)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    pw = (uv - K[2:4]) / K[0:2]
    theta_d = np.linalg.norm(pw, axis=1)
    theta = theta_d.copy()
    for _ in range(iters):
        t2 = theta * theta
        f = theta * (1 + K[4] * t2 + K[5] * t2 ** 2 + K[6] * t2 ** 3 + K[7] * t2 ** 4) - theta_d
        fp = 1 + 3 * K[4] * t2 + 5 * K[5] * t2 ** 2 + 7 * K[6] * t2 ** 3 + 9 * K[7] * t2 ** 4
        theta = theta - f / fp
    scale = np.where(theta_d > 1e-12, np.tan(theta) / np.where(theta_d > 1e-12, theta_d, 1.0), 1.0)
    return pw * scale[:, None]
