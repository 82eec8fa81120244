// obs_pose.hpp — the pose an observation was made at, as the updates form it: State::bounding_times (order 3), the polynomial
// through the four bounding clones (State::get_interpolated_pose_poly / get_interpolated_jacobian) or the residual pose the track
// carries (res_R / res_p), and the camera pose behind it (CamHelper::get_imu_poses / get_cam_poses).  Shared by the Jacobian and
// triangulation kernels (jacobian_kernels.hip) and the line map (line_map_kernels.hip): one copy of the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include "jacobian_kernels.hpp"
#include "so3.hpp"

namespace plv {

// State::bounding_times + bounding_poses_n (order 3)   REF: State.cpp:1023-1136
__device__ inline int bounding_start(const JacParams &P, double t) {
  const int N = P.n_clones;
  if (N < 4) return -1;
  const double *ct = P.clone_time;
  if (t < ct[0] - P.dt_exp || t > ct[N - 1] + P.dt_exp) return -1;
  if (t > ct[N - 1]) return -1;  // State.cpp:852-855
  int n_b = -1;
  for (int i = 0; i < N - 1; ++i)
    if (ct[i] - P.dt_exp <= t && t <= ct[i + 1] + P.dt_exp) {
      n_b = i;
      break;
    }
  if (n_b < 0) return -1;
  int start = n_b - 1;
  if (n_b - 1 < 0)
    start = 0;
  else if (n_b + 2 >= N)
    start = N - 4;
  if (start < 0 || start + 4 > N) return -1;
  return start;
}

struct Interp {
  M3 R;
  V3 p;
  M3 Ho[4];       // orientation blocks of dT/dx for the 4 poses
  double lam[4];  // position blocks are lam I  (lam[0] = 1 - sum)
  double dtj[6];
};

// polynomial through clones s0..s0+3 at time t.  REF: State.cpp:631-723, 881-958
__device__ inline void interpolate(const JacParams &P, int s0, double t, bool fej, bool want_jac, Interp &o) {
  const double *Rs = fej ? P.clone_R_fej : P.clone_R, *ps = fej ? P.clone_p_fej : P.clone_p;
  const M3 R0 = ldM(Rs + 9 * s0);
  const V3 p0 = ldV(ps + 3 * s0);
  V3 th[3], dp[3];
  M3 Rw[3], V;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    Rw[w] = mm(ldM(Rs + 9 * (s0 + 1 + w)), tp(R0));
    th[w] = log_so3(Rw[w]);
    dp[w] = vsub(ldV(ps + 3 * (s0 + 1 + w)), p0);
    const double d = P.clone_time[s0 + 1 + w] - P.clone_time[s0];
    V(w, 0) = d;  // REF uses std::pow(d, i); products differ from it by at most one rounding
    V(w, 1) = d * d;
    V(w, 2) = d * d * d;
  }
  const M3 Vi = inv3(V);
  const double dtm = t - P.clone_time[s0];
  const double pw[4] = {1.0, dtm, dtm * dtm, dtm * dtm * dtm};
  double lam[3], lamd[3];
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    lam[w] = lamd[w] = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      lam[w] += pw[i + 1] * Vi(i, w);
      lamd[w] += (double)(i + 1) * pw[i] * Vi(i, w);
    }
  }
  V3 A_ori{{0, 0, 0}}, A_pos{{0, 0, 0}};
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    A_ori = vadd(A_ori, vsc(th[w], lam[w]));
    A_pos = vadd(A_pos, vsc(dp[w], lam[w]));
  }
  const M3 Rio = exp_so3(A_ori);
  o.R = mm(Rio, R0);
  o.p = vadd(p0, A_pos);
  if (!want_jac) return;
  const M3 Jl = Jl_so3(A_ori);
  M3 H0o = Rio;
  double lsum = 0;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const M3 JinvW = inv3(Jl_so3(th[w]));
    H0o = ma(H0o, ms(mm(Jl, mm(JinvW, Rw[w])), -lam[w]));
    o.Ho[w + 1] = ms(mm(Jl, JinvW), lam[w]);
    o.lam[w + 1] = lam[w];
    lsum += lam[w];
  }
  o.Ho[0] = H0o;
  o.lam[0] = 1.0 - lsum;
  V3 dori{{0, 0, 0}}, dpos{{0, 0, 0}};
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    dori = vadd(dori, vsc(th[w], lamd[w]));
    dpos = vadd(dpos, vsc(dp[w], lamd[w]));
  }
  const V3 top = vsc(mv(Jl, dori), -1.0);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.dtj[i] = top[i];
    o.dtj[3 + i] = dpos[i];
  }
}

// where observation o's residual pose (res_R / res_p) and its covariance (res_Q / res_clone) sit: at o, or — poses per distinct
// observation time, JacParams::res_pose_of — at the entry of its time
__device__ __forceinline__ int res_index(const JacParams &P, int o) { return P.res_pose_of ? P.res_pose_of[o] : o; }

// The IMU pose of observation o, whose time tm = obs_time + cam_dt has the bounding clones s0 ..: the track's res_R / res_p, else the
// polynomial at tm (CamHelper::get_imu_poses)   REF: PL/update/cam/CamHelper.cpp:327-372
__device__ __forceinline__ void obs_imu_pose(const JacParams &P, int o, int s0, double tm, M3 &R_GtoI, V3 &p_IinG) {
  if (P.res_R) {
    const int ro = res_index(P, o);
    R_GtoI = ldM(P.res_R + 9 * ro);
    p_IinG = ldV(P.res_p + 3 * ro);
  } else {
    Interp est;
    interpolate(P, s0, tm, false, false, est);
    R_GtoI = est.R;
    p_IinG = est.p;
  }
}
// ... and the camera pose behind it (get_cam_poses)   REF: CamHelper.cpp:374-395, linefeat/LineHelper.cpp:190-196
__device__ __forceinline__ void obs_cam_pose(const JacParams &P, const M3 &R_GtoI, const V3 &p_IinG, M3 &R_GtoC, V3 &p_CinG) {
  R_GtoC = mm(ldM(P.R_ItoC), R_GtoI);
  p_CinG = vsub(p_IinG, mv(tp(R_GtoC), ldV(P.p_IinC)));
}
// Both for observation o: false when its time has no bounding clones (the view is dropped).
__device__ __forceinline__ bool obs_pose(const JacParams &P, int o, M3 &R_GtoC, V3 &p_CinG) {
  const double tm = P.obs_time[o] + P.cam_dt;
  const int s0 = bounding_start(P, tm);
  if (s0 < 0) return false;
  M3 R_GtoI;
  V3 p_IinG;
  obs_imu_pose(P, o, s0, tm, R_GtoI, p_IinG);
  obs_cam_pose(P, R_GtoI, p_IinG, R_GtoC, p_CinG);
  return true;
}

// ... stored for the triangulation kernels: poses [n_obs][12] = R_GtoC, p_CinG; imu (nullable) the same of the IMU pose
__device__ __forceinline__ void campose_one(const JacParams &P, int o, double *__restrict__ poses /*[n_obs][12]*/, unsigned char *__restrict__ valid,
                            double *__restrict__ imu) {
  const double tm = P.obs_time[o] + P.cam_dt;
  const int s0 = bounding_start(P, tm);
  valid[o] = s0 >= 0;
  if (s0 < 0) return;
  M3 R_GtoI;
  V3 p_IinG;
  obs_imu_pose(P, o, s0, tm, R_GtoI, p_IinG);
  if (imu) {
#pragma unroll
    for (int i = 0; i < 9; ++i) imu[12 * o + i] = R_GtoI.m[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) imu[12 * o + 9 + i] = p_IinG[i];
  }
  M3 R_GtoC;
  V3 p_CinG;
  obs_cam_pose(P, R_GtoI, p_IinG, R_GtoC, p_CinG);
#pragma unroll
  for (int i = 0; i < 9; ++i) poses[12 * o + i] = R_GtoC.m[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) poses[12 * o + 9 + i] = p_CinG[i];
}

}  // namespace plv
