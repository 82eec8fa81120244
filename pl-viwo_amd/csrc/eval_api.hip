// eval_api.hip — trajectory I/O and the ATE evaluator: the accuracy half of the metric.
//
//   State_Logger::save_trajectory_to_file          REF: PL-VIWO/src/utils/State_Logger.h:166-205
//   ov_eval::Loader::load_data / get_total_length  REF: open_vins/ov_eval/src/utils/Loader.cpp:26-90,388-398
//   AlignUtils::perform_association / align_umeyama REF: open_vins/ov_eval/src/alignment/AlignUtils.cpp:26-91,101-189
//   AlignUtils::get_best_yaw / get_mean            REF: open_vins/ov_eval/src/alignment/AlignUtils.h:53-72
//   AlignTrajectory::align_*                       REF: open_vins/ov_eval/src/alignment/AlignTrajectory.cpp:26-166
//   ResultTrajectory ctor / calculate_ate          REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:26-121
//   ResultTrajectory::calculate_ate_2d             REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:99-137
//   ResultTrajectory::calculate_rpe                REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:139-239
//   compute_comparison_indices_length              REF: open_vins/ov_eval/src/calc/ResultTrajectory.h:169-198
//   ResultTrajectory::calculate_nees               REF: open_vins/ov_eval/src/calc/ResultTrajectory.cpp:241-286
//   Statistics::calculate                          REF: open_vins/ov_eval/src/utils/Statistics.h:72-119
//
// File parsing, association and the order statistics are host logic; everything that touches every pose (the two
// Umeyama passes and the per-pose error) runs on the device: a KAIST sequence is ~1e4-1e5 poses, an evaluation
// sweep over many runs is where this is called in a loop.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "plv_ctx.hpp"
#include "so3.hpp"
#include "update_state.hpp"

namespace plv {
namespace {

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// block-wide sums of NV values per thread -> out[blockIdx.x][NV]
template <int NV> __device__ void block_sums(double (&v)[NV], double *out) {
  __shared__ double sh[4][NV];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double s = wsum(v[i]);
    if (lane == 0) sh[w][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) out[(size_t)blockIdx.x * NV + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

// pass 1: sums of the positions (get_mean)
__global__ void __launch_bounds__(256) traj_mean_kernel(int n, const double *__restrict__ data, const double *__restrict__ model,
                                                        double *__restrict__ partial) {
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] += data[7 * (size_t)i + c];
      v[3 + c] += model[7 * (size_t)i + c];
    }
  }
  block_sums<6>(v, partial);
}

// pass 2: C = sum (m - mu_M)(d - mu_D)^T and sigma2 = sum |d - mu_D|^2   (align_umeyama :33-52)
struct Means {
  double d[3], m[3];
};
__global__ void __launch_bounds__(256) traj_corr_kernel(int n, const double *__restrict__ data, const double *__restrict__ model, Means mu,
                                                        double *__restrict__ partial) {
  double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    double d[3], m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      d[c] = data[7 * (size_t)i + c] - mu.d[c];
      m[c] = model[7 * (size_t)i + c] - mu.m[c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * r + c] += m[r] * d[c];
    v[9] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  }
  block_sums<10>(v, partial);
}

struct Align {
  double R[9], t[3], s, qinv[4];  // qinv = Inv(rot_2_quat(R))
};

// quat_2_Rot as the evaluator has always formed it, on the device and on the host: each entry as (a or 0) - 2 q4 [q x] + 2 q q^T.  so3.hpp's
// quat_2_Rot scales whole matrices instead ((2 q4^2 - 1) * I has -0 off the diagonal), and the two differ in the sign of a zero entry,
// e.g. for q = (0, -1, 0, 0) in entry (1, 0): not merged.
__host__ __device__ inline void quat_2_rot(const double *q, double *R) {  // REF: quat_ops.h:152-157
  const double a = 2 * q[3] * q[3] - 1;
  const double sk[9] = {0, -q[2], q[1], q[2], 0, -q[0], -q[1], q[0], 0};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (r == c ? a : 0.0) - 2 * q[3] * sk[3 * r + c] + 2 * q[r] * q[c];
}

// ResultTrajectory ctor :72-82 (the aligned estimate) + calculate_ate :91-115 (errors), thread per pose.  TWO_D is calculate_ate_2d
// (:106-115): the signed z component of the log and the norm of the x-y difference; the 3-D instantiation is the kernel as it was.
template <bool TWO_D>
__global__ void __launch_bounds__(256) traj_ate_kernel(int n, const double *__restrict__ est, const double *__restrict__ gt, Align A,
                                                       double *__restrict__ aligned, double *__restrict__ ori_err,
                                                       double *__restrict__ pos_err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *e = est + 7 * (size_t)i, *g = gt + 7 * (size_t)i;
  double p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    // s * R * p + t: Eigen evaluates (s * R) * p
    p[r] = (A.s * A.R[3 * r] * e[0] + A.s * A.R[3 * r + 1] * e[1] + A.s * A.R[3 * r + 2] * e[2]) + A.t[r];
  }
  const Q4 q = quat_multiply(ldQ(e + 3), ldQ(A.qinv));
  double Re[9], Rg[9], eR[9];
  quat_2_rot(q.q, Re);
  quat_2_rot(g + 3, Rg);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) eR[3 * r + c] = Re[r] * Rg[c] + Re[3 + r] * Rg[3 + c] + Re[6 + r] * Rg[6 + c];  // Re^T Rg
  const V3 w = log_so3(ldM(eR));
  const double dx = g[0] - p[0], dy = g[1] - p[1], dz = g[2] - p[2];
  if constexpr (TWO_D) {
    ori_err[i] = 180.0 / M_PI * w[2];
    pos_err[i] = sqrt(dx * dx + dy * dy);
  } else {
    ori_err[i] = 180.0 / M_PI * sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    pos_err[i] = sqrt(dx * dx + dy * dy + dz * dz);
  }
  if (aligned) {
#pragma unroll
    for (int r = 0; r < 3; ++r) aligned[7 * (size_t)i + r] = p[r];
#pragma unroll
    for (int r = 0; r < 4; ++r) aligned[7 * (size_t)i + 3 + r] = q[r];
  }
}

// |acc[i] - (acc[start] + L)| with the reference's grouping (ResultTrajectory.h:184): ties fall where its scan lets them fall
__device__ __forceinline__ double seg_err(const double *__restrict__ acc, int i, double target) { return fabs(acc[i] - target); }

// compute_comparison_indices_length (ResultTrajectory.h:169-198) + the pair error of calculate_rpe (.cpp:180-228), one thread per
// (segment length, start).  The reference scans i = start .. n-1 and keeps the first i whose error is strictly below the best so
// far, beginning at max_dist_diff: the first minimiser of e(i) = |acc[i] - target|, if that minimum is below the limit.  acc is
// non-decreasing and rounding is monotone, so e(i) as computed never rises before j = the first acc[j] >= target and never falls
// after it.  The minimum right of j is therefore e(j) at j itself; left of j it is e(j - 1), first reached at the first i with
// e(i) <= e(j - 1) (a standing vehicle repeats acc values, and a subtraction may round neighbours to one error): a second
// bisection over the non-increasing stretch.  The left candidate precedes j, so it wins a tie.  A latency-bound gather: ~2 log2(n)
// dependent loads of acc through the cache, then four poses; no LDS, no atomics.
__global__ void __launch_bounds__(256) traj_rpe_kernel(int n, int n_seg, const double *__restrict__ acc, const double *__restrict__ seg,
                                                       double max_dist_diff, const double *__restrict__ aligned,
                                                       const double *__restrict__ gt, int *__restrict__ end_idx,
                                                       double *__restrict__ ori_err, double *__restrict__ pos_err) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (size_t)n_seg * n) return;
  const int start = (int)(k % n);
  const double target = acc[start] + seg[k / n];
  int lo = start, hi = n;  // j: the first index in [start, n) with acc[j] >= target, n when there is none
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (acc[mid] >= target)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int j = lo;
  int best = -1;
  double best_err = max_dist_diff;
  if (j > start) {
    const double e_left = seg_err(acc, j - 1, target);
    lo = start, hi = j - 1;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (seg_err(acc, mid, target) <= e_left)
        hi = mid;
      else
        lo = mid + 1;
    }
    if (e_left < best_err) best = lo, best_err = e_left;
  }
  if (j < n) {
    const double e_right = seg_err(acc, j, target);
    if (e_right < best_err) best = j;
  }
  end_idx[k] = best;
  if (best < 0) return;
  // T_c1_c2 = Inv_se3(T_c1) T_c2 with T = [quat_2_Rot(q)^T, p] (:183-194), likewise T_m1_m2 of the ground truth (:198-209)
  const double *c1 = aligned + 7 * (size_t)start, *c2 = aligned + 7 * (size_t)best, *m1 = gt + 7 * (size_t)start, *m2 = gt + 7 * (size_t)best;
  double Q1[9], Q2[9], G1[9], G2[9], Rc[9], Rm[9], tc[3], tm[3];
  quat_2_rot(c1 + 3, Q1);
  quat_2_rot(c2 + 3, Q2);
  quat_2_rot(m1 + 3, G1);
  quat_2_rot(m2 + 3, G2);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Rc[3 * r + c] = Q1[3 * r] * Q2[3 * c] + Q1[3 * r + 1] * Q2[3 * c + 1] + Q1[3 * r + 2] * Q2[3 * c + 2];  // Q1 Q2^T
      Rm[3 * r + c] = G1[3 * r] * G2[3 * c] + G1[3 * r + 1] * G2[3 * c + 1] + G1[3 * r + 2] * G2[3 * c + 2];
    }
    // Inv_se3's translation -R^T p, added last by the 4x4 product
    tc[r] = (Q1[3 * r] * c2[0] + Q1[3 * r + 1] * c2[1] + Q1[3 * r + 2] * c2[2]) + -(Q1[3 * r] * c1[0] + Q1[3 * r + 1] * c1[1] + Q1[3 * r + 2] * c1[2]);
    tm[r] = (G1[3 * r] * m2[0] + G1[3 * r + 1] * m2[1] + G1[3 * r + 2] * m2[2]) + -(G1[3 * r] * m1[0] + G1[3 * r + 1] * m1[1] + G1[3 * r + 2] * m1[2]);
  }
  // T_error_in_c2 = Inv_se3(T_m1_m2) T_c1_c2 (:213), then into the world by the end pose's rotation Q2^T (:215-222)
  double Re[9], te[3], RQ[9], Rw[9], tw[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Re[3 * r + c] = Rm[r] * Rc[c] + Rm[3 + r] * Rc[3 + c] + Rm[6 + r] * Rc[6 + c];  // Rm^T Rc
    te[r] = (Rm[r] * tc[0] + Rm[3 + r] * tc[1] + Rm[6 + r] * tc[2]) + -(Rm[r] * tm[0] + Rm[3 + r] * tm[1] + Rm[6 + r] * tm[2]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) RQ[3 * r + c] = Re[3 * r] * Q2[c] + Re[3 * r + 1] * Q2[3 + c] + Re[3 * r + 2] * Q2[6 + c];  // Re Q2
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rw[3 * r + c] = Q2[r] * RQ[c] + Q2[3 + r] * RQ[3 + c] + Q2[6 + r] * RQ[6 + c];  // Q2^T (Re Q2)
    tw[r] = Q2[r] * te[0] + Q2[3 + r] * te[1] + Q2[6 + r] * te[2];
  }
  const V3 w = log_so3(ldM(Rw));
  pos_err[k] = sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
  ori_err[k] = 180.0 / M_PI * sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
}

// e^T C^-1 e with the 3x3 inverse by cofactors over the determinant, as Eigen's fixed-size inverse() forms it
__device__ double quad_form_inv3(const double *__restrict__ m, const double *e) {
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
  };
  const double c0[3] = {cof(0, 0), cof(1, 0), cof(2, 0)};
  const double invdet = 1.0 / (c0[0] * m[0] + c0[1] * m[3] + c0[2] * m[6]);
  double v[3] = {0, 0, 0};  // e^T inv, inv(r, c) = cof(c, r) * invdet
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) v[c] += e[r] * ((r == 0 ? c0[c] : cof(c, r)) * invdet);
  return v[0] * e[0] + v[1] * e[1] + v[2] * e[2];
}

// calculate_nees :253-275, thread per pose: gt_in_est is the ground truth aligned to the estimate (the ctor's second alignment).
// A pose whose either value is NaN is skipped by the reference (:267-270): both outputs are NaN there.
__global__ void __launch_bounds__(256) traj_nees_kernel(int n, const double *__restrict__ est, const double *__restrict__ gt_in_est,
                                                        const double *__restrict__ cov_ori, const double *__restrict__ cov_pos,
                                                        double *__restrict__ nees_ori, double *__restrict__ nees_pos) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *e = est + 7 * (size_t)i, *g = gt_in_est + 7 * (size_t)i;
  double Rg[9], Re[9], eR[9];
  quat_2_rot(g + 3, Rg);
  quat_2_rot(e + 3, Re);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) eR[3 * r + c] = Rg[3 * r] * Re[3 * c] + Rg[3 * r + 1] * Re[3 * c + 1] + Rg[3 * r + 2] * Re[3 * c + 2];  // Rg Re^T
  const V3 w = log_so3(ldM(eR));
  const double eo[3] = {-w[0], -w[1], -w[2]}, ep[3] = {g[0] - e[0], g[1] - e[1], g[2] - e[2]};
  double no = quad_form_inv3(cov_ori + 9 * (size_t)i, eo), np = quad_form_inv3(cov_pos + 9 * (size_t)i, ep);
  if (isnan(no) || isnan(np)) no = np = NAN;
  nees_ori[i] = no;
  nees_pos[i] = np;
}

// ---------------------------------------------------------------------------------------- host 3x3 helpers
double det3(const double *a) {
  return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

// Singular value decomposition C = U diag(D) V^T of a 3x3 by one-sided Jacobi (Hestenes), singular values descending
// like Eigen::JacobiSVD.  A null singular direction is completed by the cross product; U S V^T with the reference's
// S = diag(1, 1, sign(det U det V)) does not depend on that choice.
void svd3(const double *C, double *U, double *D, double *V) {
  double A[9];
  std::copy(C, C + 9, A);
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 3; ++r) {
          al += A[3 * r + p] * A[3 * r + p];
          be += A[3 * r + q] * A[3 * r + q];
          ga += A[3 * r + p] * A[3 * r + q];
        }
        if (ga == 0.0 || std::fabs(ga) <= 1e-300) continue;
        off = std::max(off, std::fabs(ga) / std::sqrt(std::max(al * be, 1e-300)));
        const double zeta = (be - al) / (2 * ga);
        const double tt = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
        const double c = 1 / std::sqrt(1 + tt * tt), s = c * tt;
        for (int r = 0; r < 3; ++r) {
          const double ap = A[3 * r + p], aq = A[3 * r + q];
          A[3 * r + p] = c * ap - s * aq;
          A[3 * r + q] = s * ap + c * aq;
          const double vp = V[3 * r + p], vq = V[3 * r + q];
          V[3 * r + p] = c * vp - s * vq;
          V[3 * r + q] = s * vp + c * vq;
        }
      }
    if (off < 1e-16) break;
  }
  double sig[3];
  for (int c = 0; c < 3; ++c) sig[c] = std::sqrt(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
  int ord[3] = {0, 1, 2};
  std::sort(ord, ord + 3, [&](int a, int b) { return sig[a] > sig[b]; });
  double Vs[9];
  const double big = std::max(sig[ord[0]], 1e-300);
  for (int k = 0; k < 3; ++k) {
    const int c = ord[k];
    D[k] = sig[c];
    for (int r = 0; r < 3; ++r) {
      Vs[3 * r + k] = V[3 * r + c];
      U[3 * r + k] = sig[c] > 1e-14 * big ? A[3 * r + c] / sig[c] : 0.0;
    }
  }
  std::copy(Vs, Vs + 9, V);
  // complete null columns of U (rank-deficient C: planar or collinear trajectories)
  auto col = [&](double *M, int k, double *o) { o[0] = M[k], o[1] = M[3 + k], o[2] = M[6 + k]; };
  auto setc = [&](double *M, int k, const double *o) { M[k] = o[0], M[3 + k] = o[1], M[6 + k] = o[2]; };
  auto nrm = [](const double *o) { return std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]); };
  double u0[3], u1[3], u2[3];
  col(U, 0, u0), col(U, 1, u1);
  if (nrm(u0) == 0) u0[0] = 1, u0[1] = 0, u0[2] = 0, setc(U, 0, u0);
  if (nrm(u1) == 0) {  // any unit vector orthogonal to u0
    const double e[3] = {std::fabs(u0[0]) < 0.9 ? 1.0 : 0.0, std::fabs(u0[0]) < 0.9 ? 0.0 : 1.0, 0.0};
    u1[0] = u0[1] * e[2] - u0[2] * e[1], u1[1] = u0[2] * e[0] - u0[0] * e[2], u1[2] = u0[0] * e[1] - u0[1] * e[0];
    const double k = nrm(u1);
    for (double &x : u1) x /= k;
    setc(U, 1, u1);
  }
  col(U, 2, u2);
  if (nrm(u2) == 0) {
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1], u2[1] = u0[2] * u1[0] - u0[0] * u1[2], u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    setc(U, 2, u2);
  }
}

void stats_of(std::vector<double> v, plv_stats *st) {  // Statistics::calculate
  *st = plv_stats{0, 0, 0, 0, 0, 0, 0};
  std::sort(v.begin(), v.end());
  if (v.empty()) return;
  const size_t n = v.size();
  st->min = v.front();
  st->max = v.back();
  st->median = n == 1 ? v[0] : (n % 2 == 1 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]));
  double mean = 0, rmse = 0;
  for (double x : v) {
    mean += x;
    rmse += x * x;
  }
  mean /= n;
  st->mean = mean;
  st->rmse = std::sqrt(rmse / n);
  double sd = 0;
  for (double x : v) sd += std::pow(x - mean, 2);
  st->std = std::sqrt(sd / (n - 1));  // n == 1: 0 / 0 like the reference
  st->ninetynine = mean + 2.326 * st->std;
}

}  // namespace
}  // namespace plv

using namespace plv;

extern "C" {

int plv_traj_header(char *buf, int cap) {
  static const char *h = "# timestamp(s) tx ty tz qx qy qz qw Pr11 Pr12 Pr13 Pr22 Pr23 Pr33 Pt11 Pt12 Pt13 Pt22 Pt23 Pt33\n";
  const int need = (int)std::strlen(h);
  if (!buf || cap <= need) return PLV_E_BADARG;
  std::memcpy(buf, h, need + 1);
  return need;
}

int plv_traj_format(char *buf, int cap, double t, const double *p, const double *q, const double *P) {
  if (!buf || !p || !q || cap < 1) return PLV_E_BADARG;
  // ios::fixed, precision 6 for time / position / quaternion, precision 10 for the covariance terms (:192-204)
  int n = std::snprintf(buf, cap, "%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f", t, p[0], p[1], p[2], q[0], q[1], q[2], q[3]);
  if (n < 0 || n >= cap) return PLV_E_CAPACITY;
  if (P) {  // 6x6 row-major marginal of the IMU pose [ori; pos]
    auto at = [&](int r, int c) { return P[6 * r + c]; };
    const int m = std::snprintf(buf + n, cap - n, " %.10f %.10f %.10f %.10f %.10f %.10f %.10f %.10f %.10f %.10f %.10f %.10f", at(0, 0),
                                at(0, 1), at(0, 2), at(1, 1), at(1, 2), at(2, 2), at(3, 3), at(3, 4), at(3, 5), at(4, 4), at(4, 5), at(5, 5));
    if (m < 0 || m >= cap - n) return PLV_E_CAPACITY;
    n += m;
  }
  if (n + 1 >= cap) return PLV_E_CAPACITY;
  buf[n++] = '\n';
  buf[n] = 0;
  return n;
}

int plv_traj_load(const char *path, int cap, double *times, double *poses, double *cov_ori, double *cov_pos, int *n_out, int *n_cov_out) {
  if (!path || !n_out) return PLV_E_BADARG;
  std::ifstream file(path);
  if (!file.is_open()) {
    set_last_error("plv_traj_load: unable to open %s", path);
    return PLV_E_BADARG;
  }
  int n = 0, ncov = 0;
  std::string line;
  while (std::getline(file, line)) {
    if (!line.find("#")) continue;  // '#' in the first column only (:44-45)
    int i = 0;
    std::istringstream s(line);
    std::string field;
    double data[20] = {0};
    while (std::getline(s, field, ' ')) {
      if (field.empty() || i >= 20) continue;
      data[i++] = std::atof(field.c_str());
    }
    if (i < 8) continue;
    if (times && n < cap) {
      times[n] = data[0];
      if (poses) std::copy(data + 1, data + 8, poses + 7 * (size_t)n);
    }
    if (i >= 20) {
      if (cov_ori && cov_pos && ncov < cap) {
        // symmetric fill, then 0.5 (c + c^T) which leaves it unchanged
        const double o[9] = {data[8], data[9], data[10], data[9], data[11], data[12], data[10], data[12], data[13]};
        const double q[9] = {data[14], data[15], data[16], data[15], data[17], data[18], data[16], data[18], data[19]};
        std::copy(o, o + 9, cov_ori + 9 * (size_t)ncov);
        std::copy(q, q + 9, cov_pos + 9 * (size_t)ncov);
      }
      ++ncov;
    }
    ++n;
  }
  *n_out = n;
  if (n_cov_out) *n_cov_out = ncov;
  if (n == 0) {
    set_last_error("plv_traj_load: could not parse any data from %s", path);
    return PLV_E_BADARG;  // the reference exits (:78-82)
  }
  return (times && n > cap) ? PLV_E_CAPACITY : PLV_OK;
}

double plv_traj_length(int n, const double *poses) {
  double d = 0;
  for (int i = 1; i < n; ++i) {
    const double *a = poses + 7 * (size_t)i, *b = a - 7;
    d += std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
  }
  return d;
}

int plv_traj_associate(double offset, double max_difference, int n_est, const double *est_times, int n_gt, const double *gt_times,
                       int *est_idx, int *gt_idx, int *n_match) {
  if (n_est < 0 || n_gt < 0 || !n_match || (n_est && !est_times) || (n_gt && !gt_times) || !est_idx || !gt_idx) return PLV_E_BADARG;
  int gp = 0, m = 0;
  for (int i = 0; i < n_est; ++i) {
    double best = max_difference;
    int best_gt = -1;
    const double te = est_times[i] + offset;
    while (gp < n_gt && gt_times[gp] < te && std::fabs(gt_times[gp] - te) > max_difference) ++gp;
    while (gp < n_gt && std::fabs(gt_times[gp] - te) <= max_difference) {
      if (std::fabs(gt_times[gp] - te) >= best) break;
      best = std::fabs(gt_times[gp] - te);
      best_gt = gp;
      ++gp;
    }
    if (best_gt != -1) {
      est_idx[m] = i;
      gt_idx[m] = best_gt;
      ++m;
    }
  }
  *n_match = m;
  return PLV_OK;
}

static int device_align(plv_ctx *ctx, int method, int n, const double *d_est, const double *d_gt, const double *h_est, const double *h_gt,
                        int n_aligned, double *R, double *t, double *s) {
  *s = 1;
  auto single = [&](bool yaw) {  // align_posyaw_single / align_se3_single
    double g[9], e[9];
    quat_2_rot(h_gt + 3, g);
    quat_2_rot(h_est + 3, e);
    // g_rot = quat_2_Rot(q_gt)^T, est_rot = quat_2_Rot(q_es)^T
    if (yaw) {
      double CR[9];  // est_rot * g_rot^T = Re^T Rg
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) CR[3 * r + c] = e[r] * g[c] + e[3 + r] * g[3 + c] + e[6 + r] * g[6 + c];
      const double th = std::atan2(CR[1] - CR[3], CR[0] + CR[4]);
      const double ct = std::cos(th), st = std::sin(th);
      const double Rz[9] = {ct, -st, 0, st, ct, 0, 0, 0, 1};
      std::copy(Rz, Rz + 9, R);
    } else {
      for (int r = 0; r < 3; ++r)  // g_rot * est_rot^T = Rg^T Re
        for (int c = 0; c < 3; ++c) R[3 * r + c] = g[r] * e[c] + g[3 + r] * e[3 + c] + g[6 + r] * e[6 + c];
    }
    for (int r = 0; r < 3; ++r) t[r] = h_gt[r] - (R[3 * r] * h_est[0] + R[3 * r + 1] * h_est[1] + R[3 * r + 2] * h_est[2]);
  };
  if (method == PLV_ALIGN_NONE) {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::copy(I, I + 9, R);
    t[0] = t[1] = t[2] = 0;
    return PLV_OK;
  }
  if (method == PLV_ALIGN_POSYAW_SINGLE || (method == PLV_ALIGN_POSYAW && n_aligned == 1)) return single(true), PLV_OK;
  if (method == PLV_ALIGN_SE3_SINGLE || (method == PLV_ALIGN_SE3 && n_aligned == 1)) return single(false), PLV_OK;
  if (method != PLV_ALIGN_POSYAW && method != PLV_ALIGN_SE3 && method != PLV_ALIGN_SIM3) return PLV_E_BADARG;
  // ---- align_umeyama(data = est, model = gt)
  auto *us = plv_update_state(ctx);
  const int blocks = std::min(256, (n + 255) / 256);
  TRY(us->staging_of(3).tri.reserve((size_t)blocks * 16 * sizeof(double) + 64));
  double *d_part = us->staging_of(3).tri.as<double>();
  std::vector<double> part((size_t)blocks * 10);
  {
    ProfScope ps(ctx->prof, "traj_mean_kernel", ctx->stream);
    hipLaunchKernelGGL(traj_mean_kernel, dim3(blocks), dim3(256), 0, ctx->stream, n, d_est, d_gt, d_part);
  }
  PLV_HIP_CHECK(plv::memcpy_async(part.data(), d_part, (size_t)blocks * 6 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  Means mu{};
  for (int b = 0; b < blocks; ++b)
    for (int c = 0; c < 3; ++c) {
      mu.d[c] += part[6 * (size_t)b + c];
      mu.m[c] += part[6 * (size_t)b + 3 + c];
    }
  for (int c = 0; c < 3; ++c) {
    mu.d[c] /= n;
    mu.m[c] /= n;
  }
  {
    ProfScope ps(ctx->prof, "traj_corr_kernel", ctx->stream);
    hipLaunchKernelGGL(traj_corr_kernel, dim3(blocks), dim3(256), 0, ctx->stream, n, d_est, d_gt, mu, d_part);
  }
  PLV_HIP_CHECK(plv::memcpy_async(part.data(), d_part, (size_t)blocks * 10 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  double C[9] = {0}, sigma2 = 0;
  for (int b = 0; b < blocks; ++b) {
    for (int c = 0; c < 9; ++c) C[c] += part[10 * (size_t)b + c];
    sigma2 += part[10 * (size_t)b + 9];
  }
  for (double &x : C) x *= 1.0 / n;
  sigma2 *= 1.0 / n;
  double U[9], D[3], V[9];
  svd3(C, U, D, V);
  const double S22 = det3(U) * det3(V) < 0 ? -1.0 : 1.0;
  if (method == PLV_ALIGN_POSYAW) {
    // rot_C = n * C^T; theta = atan2(rot_C(0,1) - rot_C(1,0), rot_C(0,0) + rot_C(1,1))
    const double th = std::atan2(n * C[3] - n * C[1], n * C[0] + n * C[4]);
    const double ct = std::cos(th), st = std::sin(th);
    const double Rz[9] = {ct, -st, 0, st, ct, 0, 0, 0, 1};
    std::copy(Rz, Rz + 9, R);
  } else {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + S22 * U[3 * r + 2] * V[3 * c + 2];
  }
  if (method == PLV_ALIGN_SIM3) *s = 1.0 / sigma2 * (D[0] + D[1] + S22 * D[2]);
  for (int r = 0; r < 3; ++r) t[r] = mu.m[r] - (*s * R[3 * r] * mu.d[0] + *s * R[3 * r + 1] * mu.d[1] + *s * R[3 * r + 2] * mu.d[2]);
  return PLV_OK;
}

// The evaluator's common front: uploads the n pose pairs, aligns `from` to `to` (AlignTrajectory::align_trajectory(from, to, ...)) and
// runs traj_ate_kernel over them, which leaves `from` expressed in `to`'s frame (the ctor's loop :72-82) and the per-pose errors on
// the device.  extra_bytes more of the evaluation buffer are reserved behind them for the caller's own kernel.
struct EvalDev {
  double *from, *to, *aligned, *ori_err, *pos_err;
  void *extra;
};
static int align_on_device(plv_ctx *ctx, int method, bool two_d, int n, const double *from, const double *to, int n_aligned,
                           size_t extra_bytes, Align *A, EvalDev *d) {
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  const size_t bytes = (size_t)n * 7 * sizeof(double);
  TRY(us->eval.reserve(bytes * 3 + (size_t)n * 2 * sizeof(double) + extra_bytes));
  d->from = us->eval.as<double>(), d->to = d->from + (size_t)n * 7, d->aligned = d->to + (size_t)n * 7;
  d->ori_err = d->aligned + (size_t)n * 7, d->pos_err = d->ori_err + n, d->extra = d->pos_err + n;
  PLV_HIP_CHECK(plv::memcpy_async(d->from, from, bytes, hipMemcpyHostToDevice, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(d->to, to, bytes, hipMemcpyHostToDevice, ctx->stream));
  *A = Align{};
  TRY(device_align(ctx, method, n, d->from, d->to, from, to, n_aligned, A->R, A->t, &A->s));
  const Q4 q = rot_2_quat(ldM(A->R));
  A->qinv[0] = -q[0], A->qinv[1] = -q[1], A->qinv[2] = -q[2], A->qinv[3] = q[3];
  {
    ProfScope ps(ctx->prof, "traj_ate_kernel", ctx->stream);
    hipLaunchKernelGGL(two_d ? traj_ate_kernel<true> : traj_ate_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n,
                       d->from, d->to, *A, d->aligned, d->ori_err, d->pos_err);
  }
  PLV_HIP_CHECK(hipGetLastError());
  return PLV_OK;
}

// the per-pose errors of align_on_device back on the host, and their statistics
static int collect_errors(plv_ctx *ctx, int n, const EvalDev &d, double *aligned, double *ori_err, double *pos_err, plv_stats *ori,
                          plv_stats *pos) {
  std::vector<double> oe(n), pe(n);
  PLV_HIP_CHECK(plv::memcpy_async(oe.data(), d.ori_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(pe.data(), d.pos_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (aligned) PLV_HIP_CHECK(plv::memcpy_async(aligned, d.aligned, (size_t)n * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  if (ori_err) std::copy(oe.begin(), oe.end(), ori_err);
  if (pos_err) std::copy(pe.begin(), pe.end(), pos_err);
  if (ori) stats_of(oe, ori);
  if (pos) stats_of(pe, pos);
  return PLV_OK;
}

int plv_traj_ate(plv_ctx *ctx, int method, int n, const double *est_poses, const double *gt_poses, int n_aligned, double *R_out,
                 double *t_out, double *s_out, double *aligned, double *ori_err, double *pos_err, plv_stats *ori, plv_stats *pos) {
  if (!ctx || !est_poses || !gt_poses || n < 1) return PLV_E_BADARG;
  Align A;
  EvalDev d;
  TRY(align_on_device(ctx, method, false, n, est_poses, gt_poses, n_aligned, 0, &A, &d));
  TRY(collect_errors(ctx, n, d, aligned, ori_err, pos_err, ori, pos));
  if (R_out) std::copy(A.R, A.R + 9, R_out);
  if (t_out) std::copy(A.t, A.t + 3, t_out);
  if (s_out) *s_out = A.s;
  return PLV_OK;
}

int plv_traj_ate_2d(plv_ctx *ctx, int method, int n, const double *est_poses, const double *gt_poses, int n_aligned, double *ori_err,
                    double *pos_err, plv_stats *ori, plv_stats *pos) {
  if (!ctx || !est_poses || !gt_poses || n < 1) return PLV_E_BADARG;
  Align A;
  EvalDev d;
  TRY(align_on_device(ctx, method, true, n, est_poses, gt_poses, n_aligned, 0, &A, &d));
  return collect_errors(ctx, n, d, nullptr, ori_err, pos_err, ori, pos);
}

int plv_traj_rpe(plv_ctx *ctx, int method, int n, const double *est_poses, const double *gt_poses, int n_seg, const double *segments,
                 int *end_idx, double *ori_err, double *pos_err, int *n_valid, plv_stats *ori, plv_stats *pos) {
  if (!ctx || !est_poses || !gt_poses || n < 1 || n_seg < 0 || (n_seg && !segments)) return PLV_E_BADARG;
  const size_t total = (size_t)n_seg * n;
  if (total > (size_t)0x7fffffff) {
    set_last_error("plv_traj_rpe: %d segment lengths x %d poses exceed 2^31 - 1 (start, length) pairs", n_seg, n);
    return PLV_E_CAPACITY;
  }
  if (total == 0) return PLV_OK;
  // accum_distances :143-149: the reference's recurrence in its order, one addition per pose (a re-associated prefix sum rounds
  // differently and could move an end index at a tie or at the limit)
  std::vector<double> acc(n);
  acc[0] = 0;
  for (int i = 1; i < n; ++i) {
    const double *a = gt_poses + 7 * (size_t)i, *b = a - 7;
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    acc[i] = acc[i - 1] + std::sqrt(dx * dx + dy * dy + dz * dz);
  }
  Align A;
  EvalDev d;
  // behind the common block: acc [n], segments [n_seg], ori / pos errors [n_seg][n], end indices [n_seg][n]
  const size_t extra = ((size_t)n + n_seg + 2 * total) * sizeof(double) + total * sizeof(int);
  TRY(align_on_device(ctx, method, false, n, est_poses, gt_poses, -1, extra, &A, &d));
  double *d_acc = static_cast<double *>(d.extra), *d_seg = d_acc + n, *d_oe = d_seg + n_seg, *d_pe = d_oe + total;
  int *d_end = reinterpret_cast<int *>(d_pe + total);
  PLV_HIP_CHECK(plv::memcpy_async(d_acc, acc.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(d_seg, segments, (size_t)n_seg * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx->prof, "traj_rpe_kernel", ctx->stream);
    hipLaunchKernelGGL(traj_rpe_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, n, n_seg, d_acc, d_seg,
                       0.5 /* max_dist_diff :154 */, d.aligned, d.to, d_end, d_oe, d_pe);
  }
  PLV_HIP_CHECK(hipGetLastError());
  std::vector<int> end(total);
  std::vector<double> oe(total), pe(total);
  PLV_HIP_CHECK(plv::memcpy_async(end.data(), d_end, total * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(oe.data(), d_oe, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(pe.data(), d_pe, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  std::vector<double> vo, vp;
  for (int s = 0; s < n_seg; ++s) {
    vo.clear(), vp.clear();
    for (size_t k = (size_t)s * n; k < (size_t)(s + 1) * n; ++k) {
      if (end[k] < 0) continue;  // the device left ori / pos untouched there
      vo.push_back(oe[k]);       // start order, as the reference pushes them; Statistics sorts a copy
      vp.push_back(pe[k]);
      if (ori_err) ori_err[k] = oe[k];
      if (pos_err) pos_err[k] = pe[k];
    }
    if (n_valid) n_valid[s] = (int)vo.size();
    if (ori) stats_of(vo, ori + s);
    if (pos) stats_of(vp, pos + s);
  }
  if (end_idx) std::copy(end.begin(), end.end(), end_idx);
  return PLV_OK;
}

int plv_traj_nees(plv_ctx *ctx, int method, int n, const double *est_poses, const double *gt_poses, const double *cov_ori,
                  const double *cov_pos, double *nees_ori, double *nees_pos, int *n_valid, plv_stats *ori, plv_stats *pos) {
  if (!ctx || !est_poses || !gt_poses || n < 1) return PLV_E_BADARG;
  if (!cov_ori || !cov_pos) {  // the reference warns and returns (:244-250)
    set_last_error("plv_traj_nees: the estimate carries no covariance (cov_ori / cov_pos is NULL)");
    return PLV_E_BADARG;
  }
  Align A;
  EvalDev d;
  // the ctor's second alignment (:57): the ground truth aligned to the estimate, so `from` is gt and `aligned` is gt_poses_aignedtoEST
  const size_t cov_bytes = (size_t)n * 9 * sizeof(double);
  TRY(align_on_device(ctx, method, false, n, gt_poses, est_poses, -1, 2 * cov_bytes, &A, &d));
  double *d_co = static_cast<double *>(d.extra), *d_cp = d_co + (size_t)n * 9;
  PLV_HIP_CHECK(plv::memcpy_async(d_co, cov_ori, cov_bytes, hipMemcpyHostToDevice, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(d_cp, cov_pos, cov_bytes, hipMemcpyHostToDevice, ctx->stream));
  {
    // the 3-D errors of the alignment pass are not needed: their slots take the two NEES values
    ProfScope ps(ctx->prof, "traj_nees_kernel", ctx->stream);
    hipLaunchKernelGGL(traj_nees_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, d.to, d.aligned, d_co, d_cp, d.ori_err,
                       d.pos_err);
  }
  PLV_HIP_CHECK(hipGetLastError());
  std::vector<double> no(n), np(n);
  PLV_HIP_CHECK(plv::memcpy_async(no.data(), d.ori_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::memcpy_async(np.data(), d.pos_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  std::vector<double> vo, vp;
  for (int i = 0; i < n; ++i) {
    if (std::isnan(no[i])) continue;  // the kernel sets both when either is NaN
    vo.push_back(no[i]);
    vp.push_back(np[i]);
  }
  if (nees_ori) std::copy(no.begin(), no.end(), nees_ori);
  if (nees_pos) std::copy(np.begin(), np.end(), nees_pos);
  if (n_valid) *n_valid = (int)vo.size();
  if (ori) stats_of(vo, ori);
  if (pos) stats_of(vp, pos);
  return PLV_OK;
}

}  // extern "C"
