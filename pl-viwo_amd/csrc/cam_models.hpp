// cam_models.hpp — the equidistant (fisheye) camera model next to radtan_core.hpp, and the dispatch on the model id
// (PLV_CAM_RADTAN / PLV_CAM_EQUIDISTANT of include/plviwo.h) that every (un)distortion call site goes through.  One source for the
// device kernels (lk_kernel tail, undistort kernels, the Jacobian kernels) and the host (the kept lines' end points): plain IEEE
// add / multiply / divide / sqrt plus atan / tan, so the host and the device agree to the ulp of the libm they call.
//   REF: open_vins/ov_core/src/cam/CamEqui.h:108-131 undistort_f (-> cv::fisheye::undistortPoints of OpenCV 4.2),
//        :136-161 distort_f, :166-229 compute_distort_jacobian; CamBase.h:150 distort_d (float in, float out).
// K8 = {fx, fy, cx, cy, k1, k2, k3, k4} under the equidistant model (k1..k4 of theta^3 .. theta^9).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/plviwo.h"
#include "radtan_core.hpp"

namespace plv {

// cv::fisheye::undistortPoints (OpenCV 4.2: no convergence flag, no sign-flip rejection) with K = [fx 0 cx; 0 fy cy], D = k1..k4,
// no R / P: float in, double arithmetic, float out.
__host__ __device__ __forceinline__ void undistort_equidistant(const double *K, float u, float v, float &xn, float &yn) {
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], k1 = K[4], k2 = K[5], k3 = K[6], k4 = K[7];
  const double pwx = ((double)u - cx) / fx, pwy = ((double)v - cy) / fy;
  double scale = 1.0;
  double theta_d = sqrt(pwx * pwx + pwy * pwy);
  const double half_pi = 3.14159265358979323846 / 2.;
  theta_d = fmin(fmax(-half_pi, theta_d), half_pi);
  if (theta_d > 1e-8) {
    double theta = theta_d;
    for (int j = 0; j < 10; ++j) {
      const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta6 * theta2;
      const double k0_theta2 = k1 * theta2, k1_theta4 = k2 * theta4, k2_theta6 = k3 * theta6, k3_theta8 = k4 * theta8;
      const double theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                               (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
      theta = theta - theta_fix;
      if (fabs(theta_fix) < 1e-8) break;
    }
    scale = tan(theta) / theta_d;
  }
  xn = (float)(pwx * scale);
  yn = (float)(pwy * scale);
}

__host__ __device__ __forceinline__ void undistort_model(int model, const double *K, float u, float v, float &xn, float &yn) {
  if (model == PLV_CAM_EQUIDISTANT)
    undistort_equidistant(K, u, v, xn, yn);
  else
    undistort_radtan(K, u, v, xn, yn);
}

// CamEqui::distort_f behind CamBase::distort_d: (x, y) are the float-rounded normalised coordinates; r is formed from float
// products and a float square root as the reference's Eigen::Vector2f arithmetic does, the rest in double; the caller rounds the
// pixel (fx x1 + cx, fy y1 + cy) through float.  Returns x1, y1 (the distorted normalised point).
__host__ __device__ __forceinline__ void distort_equidistant_f(const double *K, float x, float y, double &x1, double &y1) {
  const double r = (double)sqrtf(x * x + y * y);
  const double theta = atan(r), t2 = theta * theta, t3 = t2 * theta, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
  const double theta_d = theta + K[4] * t3 + K[5] * t5 + K[6] * t7 + K[7] * t9;
  const double inv_r = (r > 1e-8) ? 1.0 / r : 1.0;
  const double cdist = (r > 1e-8) ? theta_d * inv_r : 1.0;
  x1 = (double)x * cdist;
  y1 = (double)y * cdist;
}

// CamEqui::compute_distort_jacobian at the (double) normalised point (x, y): dzn = dz/dzn (2 x 2 row-major), dzeta = dz/dzeta
// (2 x 8 row-major, columns fx fy cx cy k1 k2 k3 k4).
__host__ __device__ __forceinline__ void distort_jacobian_equidistant(const double *K, double x, double y, double *dzn, double *dzeta) {
  const double r = sqrt(x * x + y * y);
  const double theta = atan(r), t2 = theta * theta, t3 = t2 * theta, t4 = t2 * t2, t5 = t3 * t2, t6 = t4 * t2, t7 = t5 * t2,
               t8 = t4 * t4, t9 = t7 * t2;
  const double theta_d = theta + K[4] * t3 + K[5] * t5 + K[6] * t7 + K[7] * t9;
  const double inv_r = (r > 1e-8) ? 1.0 / r : 1.0;
  const double cdist = (r > 1e-8) ? theta_d * inv_r : 1.0;
  // duv_dxy (dxy_dxyn + (dxy_dr + dxy_dthd dthd_dth dth_dr) dr_dxyn)
  const double dthd_dth = 1 + 3 * K[4] * t2 + 5 * K[5] * t4 + 7 * K[6] * t6 + 9 * K[7] * t8;
  const double dth_dr = 1 / (r * r + 1);
  const double a0 = -x * theta_d * inv_r * inv_r + x * inv_r * dthd_dth * dth_dr;
  const double a1 = -y * theta_d * inv_r * inv_r + y * inv_r * dthd_dth * dth_dr;
  const double b0 = x * inv_r, b1 = y * inv_r;
  const double d = theta_d * inv_r;
  dzn[0] = K[0] * (d + a0 * b0);
  dzn[1] = K[0] * (a0 * b1);
  dzn[2] = K[1] * (a1 * b0);
  dzn[3] = K[1] * (d + a1 * b1);
#pragma unroll
  for (int i = 0; i < 16; ++i) dzeta[i] = 0;
  dzeta[0] = x * cdist;
  dzeta[2] = 1;
  dzeta[4] = K[0] * x * inv_r * t3;
  dzeta[5] = K[0] * x * inv_r * t5;
  dzeta[6] = K[0] * x * inv_r * t7;
  dzeta[7] = K[0] * x * inv_r * t9;
  dzeta[9] = y * cdist;
  dzeta[11] = 1;
  dzeta[12] = K[1] * y * inv_r * t3;
  dzeta[13] = K[1] * y * inv_r * t5;
  dzeta[14] = K[1] * y * inv_r * t7;
  dzeta[15] = K[1] * y * inv_r * t9;
}

}  // namespace plv
