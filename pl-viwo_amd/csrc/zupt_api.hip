// zupt_api.hip — zero-velocity updater: the standstill measurement on the device, the detector and the update.
//
// The reference constructs a ZuptUpdater (REF: PL-VIWO/src/core/SystemManager.cpp:50-52, 116-121) whose class is not part of the
// published snapshot; the measurement is that of the upstream updater (open_vins UpdaterZeroVelocity::try_update): while the
// vehicle stands, every IMU interval i of length dt_i says
//   gyro            r = -sqrt(dt_i / a) / sigma_w * (wm_i - bg)                 H[bg] = -sqrt(dt_i / a) / sigma_w * I
//   accelerometer   r = -sqrt(dt_i / a) / sigma_a * (am_i - ba - R(q) g)        H[theta] = -sqrt(dt_i / a) / sigma_a * skew(R(q_fej) g)
//                                                                               H[ba]    = -sqrt(dt_i / a) / sigma_a * I
// (a = noise_mult; JPL-left error state, the Jacobian on the first estimate), and three rows pin the velocity: r = -v / sigma_v,
// H[v] = I / sigma_v.  Propagation and cloning keep running through a stop here, so velocity is a pseudo-measurement rather than
// a frozen state.  R = I.
//
// Every interval repeats one block pattern scaled by sqrt(dt_i), so the orthogonal compression of the stack (what
// measurement_compress_inplace would leave) has a closed form: with T = sum dt_i and the dt-weighted means w_bar, a_bar
//   rows 0-2   c_w = sqrt(T / a) / sigma_w    H[bg] = -c_w I                                   r = -c_w (w_bar - bg)
//   rows 3-5   c_a = sqrt(T / a) / sigma_a    H[theta] = -c_a skew(R(q_fej) g), H[ba] = -c_a I    r = -c_a (a_bar - ba - R(q) g)
//   rows 6-8   the velocity rows
// It has the stack's H^T H and H^T r, and its residual is Q1^T r for an orthonormal basis Q1 of the range of the stack's H: dx, the
// posterior P and the chi-square of the compressed rows are those of the full stack, whichever basis a QR would have picked.
//
// zupt_kernel: one workgroup of 64 lanes.  The lanes stride over the intervals and accumulate dt, dt * wm, dt * am; the seven sums go
// through the fixed-order DPP wave reduction (no atomics: a call is reproducible); lane 0 forms the nine residuals and the 3 x 3
// block, the lanes store the 9 x 12 system.  The gate and the update then run on the resident covariance (plv_chi2_batch /
// plv_ekf_update with P = NULL): P is never copied.
#include <algorithm>
#include <cmath>
#include <vector>

#include "plv_ctx.hpp"
#include "so3.hpp"
#include "update_state.hpp"
#include "wave_ops.hpp"

namespace plv {
namespace {

constexpr int kRows = 9, kCols = 12;

struct ZuptArgs {
  plv_imu_state imu;
  double sigma_w, sigma_a, gravity[3], noise_mult, sigma_v;
  int n;                        // samples (n - 1 intervals)
  const double *t, *wm, *am;    // device: [n], [n][3], [n][3]
  double *out;                  // [H 9 x 12 col-major][res 9]
};

__global__ void __launch_bounds__(64) zupt_kernel(ZuptArgs A) {
  __shared__ double blk[9], resv[9], cw_s, ca_s;
  const int tid = threadIdx.x;
  double s[7] = {0, 0, 0, 0, 0, 0, 0};   // dt, dt * wm, dt * am
  for (int i = tid; i < A.n - 1; i += 64) {
    const double dt = A.t[i + 1] - A.t[i];
    s[0] += dt;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[1 + c] += dt * A.wm[3 * i + c];
      s[4 + c] += dt * A.am[3 * i + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) s[c] = wave_sum_f64(s[c]);
  if (tid == 0) {
    const double T = s[0];
    const double cw = sqrt(T / A.noise_mult) / A.sigma_w, ca = sqrt(T / A.noise_mult) / A.sigma_a;
    const V3 g = ldV(A.gravity);
    const V3 w_bar = vsc(ldV(s + 1), 1.0 / T), a_bar = vsc(ldV(s + 4), 1.0 / T);
    const V3 g_I = mv(quat_2_Rot(ldQ(A.imu.q)), g);
    const V3 g_I_fej = mv(quat_2_Rot(ldQ(A.imu.q_fej)), g);
    stV(resv, vsc(vsub(w_bar, ldV(A.imu.bg)), -cw));
    stV(resv + 3, vsc(vsub(vsub(a_bar, ldV(A.imu.ba)), g_I), -ca));
    stV(resv + 6, vsc(ldV(A.imu.v), -1.0 / A.sigma_v));
    const M3 B = ms(skew3(g_I_fej), -ca);
#pragma unroll
    for (int e = 0; e < 9; ++e) blk[e] = B.m[e];
    cw_s = cw, ca_s = ca;
  }
  __syncthreads();
  // columns: theta 0-2, v 3-5, bg 6-8, ba 9-11
  for (int e = tid; e < kRows * kCols; e += 64) {
    const int c = e / kRows, r = e - c * kRows;
    const int rb = r / 3, cb = c / 3, ri = r % 3, ci = c % 3;
    double v = 0.0;
    if (rb == 0 && cb == 2) v = ri == ci ? -cw_s : 0.0;
    else if (rb == 1 && cb == 0) v = blk[3 * ri + ci];
    else if (rb == 1 && cb == 3) v = ri == ci ? -ca_s : 0.0;
    else if (rb == 2 && cb == 1) v = ri == ci ? 1.0 / A.sigma_v : 0.0;
    A.out[e] = v;
  }
  if (tid < kRows) A.out[kRows * kCols + tid] = resv[tid];
}

void zupt_columns(int imu_id, int *cols) {
  for (int i = 0; i < 3; ++i) {
    cols[i] = imu_id + i;
    cols[3 + i] = imu_id + 6 + i;
    cols[6 + i] = imu_id + 9 + i;
    cols[9 + i] = imu_id + 12 + i;
  }
}

// runs the kernel: H (9 x 12 col-major) and res (9) on the host
int zupt_system(plv_ctx *ctx, const plv_zupt_options *op, const plv_imu_state *imu, const plv_imu_noise *noise, int n, const double *t,
                const double *wm, const double *am, double *H, double *res) {
  if (!ctx || !op || !imu || !noise || !t || !wm || !am || !H || !res || n < 2) return PLV_E_BADARG;
  if (!(noise->sigma_w > 0.0) || !(noise->sigma_a > 0.0) || !(op->sigma_v > 0.0) || !(op->noise_mult > 0.0)) {
    set_last_error("plv_zupt: sigma_w, sigma_a, sigma_v and noise_mult must be positive");
    return PLV_E_BADARG;
  }
  for (int i = 0; i + 1 < n; ++i)
    if (!(t[i + 1] > t[i])) {
      set_last_error("plv_zupt: the sample times must increase (sample %d)", i + 1);
      return PLV_E_BADARG;
    }
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  const size_t nd = (size_t)n, n_out = kRows * kCols + kRows;
  TRY(us->eval.reserve((7 * nd + n_out) * 8));
  double *d = us->eval.as<double>();
  std::vector<double> h(7 * nd);   // the samples go up in one copy
  std::copy(t, t + nd, h.begin());
  std::copy(wm, wm + 3 * nd, h.begin() + nd);
  std::copy(am, am + 3 * nd, h.begin() + 4 * nd);
  PLV_HIP_CHECK(plv::memcpy_async(d, h.data(), 7 * nd * 8, hipMemcpyHostToDevice, ctx->stream));
  ZuptArgs A{};
  A.imu = *imu;
  A.sigma_w = noise->sigma_w, A.sigma_a = noise->sigma_a;
  std::copy(noise->gravity, noise->gravity + 3, A.gravity);
  A.noise_mult = op->noise_mult, A.sigma_v = op->sigma_v;
  A.n = n;
  A.t = d, A.wm = d + nd, A.am = d + 4 * nd;
  A.out = d + 7 * nd;
  {
    ProfScope ps(ctx->prof, "zupt_kernel", ctx->stream);
    hipLaunchKernelGGL(zupt_kernel, dim3(1), dim3(64), 0, ctx->stream, A);
  }
  PLV_HIP_CHECK(hipGetLastError());
  double out[kRows * kCols + kRows];
  PLV_HIP_CHECK(plv::memcpy_async(out, A.out, n_out * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  for (size_t i = 0; i < n_out; ++i)
    if (!std::isfinite(out[i])) {
      set_last_error("plv_zupt: the zero-velocity measurement is not finite");
      return PLV_E_NUMERIC;
    }
  std::copy(out, out + kRows * kCols, H);
  std::copy(out + kRows * kCols, out + n_out, res);
  return PLV_OK;
}

// the system and its chi-square on the resident covariance; nothing is changed
int zupt_gate(plv_ctx *ctx, const plv_zupt_options *op, const plv_imu_state *imu, const plv_imu_noise *noise, int n, const double *t,
              const double *wm, const double *am, int imu_id, double *H, double *res, int *cols, double *chi2) {
  if (!ctx || ctx->cov_n < 1) return PLV_E_BADARG;
  if (imu_id < 0 || imu_id + 15 > ctx->cov_n) {
    set_last_error("plv_zupt: the IMU block at %d lies outside the covariance (%d)", imu_id, ctx->cov_n);
    return PLV_E_BADARG;
  }
  TRY(zupt_system(ctx, op, imu, noise, n, t, wm, am, H, res));
  zupt_columns(imu_id, cols);
  const int rows = kRows, nst = ctx->cov_n;
  double chi = 0.0;
  TRY(plv_chi2_batch(ctx, nullptr, nst, nst, 1, kCols, kRows, &rows, H, res, cols, 1.0, &chi));  // R = I
  if (!std::isfinite(chi)) {
    set_last_error("plv_zupt: the chi-square of the zero-velocity measurement is not finite");
    return PLV_E_NUMERIC;
  }
  *chi2 = chi;
  return PLV_OK;
}

}  // namespace
}  // namespace plv

using namespace plv;

extern "C" {

int plv_zupt_system(plv_ctx *ctx, const plv_zupt_options *opt, const plv_imu_state *imu, const plv_imu_noise *noise, int n,
                    const double *t, const double *wm, const double *am, int imu_id, double *H, double *res, int *col_to_state) {
  if (!col_to_state || imu_id < 0) return PLV_E_BADARG;
  TRY(zupt_system(ctx, opt, imu, noise, n, t, wm, am, H, res));
  zupt_columns(imu_id, col_to_state);
  return PLV_OK;
}

int plv_zupt_update(plv_ctx *ctx, const plv_zupt_options *opt, const plv_imu_state *imu, const plv_imu_noise *noise, int n,
                    const double *t, const double *wm, const double *am, int imu_id, int force, double *chi2, uint8_t *accepted,
                    double *dx) {
  if (!ctx || !chi2 || !accepted || !dx || ctx->cov_n < 1) return PLV_E_BADARG;
  const int nst = ctx->cov_n;
  *accepted = 0;
  *chi2 = 0.0;
  std::fill(dx, dx + nst, 0.0);
  double H[kRows * kCols], res[kRows];
  int cols[kCols];
  TRY(zupt_gate(ctx, opt, imu, noise, n, t, wm, am, imu_id, H, res, cols, chi2));
  if (!force && !(*chi2 < opt->chi2_mult * plv_chi2_quantile95(kRows))) return PLV_OK;
  const int rc = plv_ekf_update(ctx, nullptr, nst, nst, H, kRows, kCols, kRows, cols, res, nullptr, dx);
  if (rc == PLV_OK) *accepted = 1;
  return rc;
}

int plv_zupt_try_update(plv_ctx *ctx, const plv_zupt_options *opt, const plv_imu_state *imu, const plv_imu_noise *noise, int n,
                        const double *t, const double *wm, const double *am, int imu_id, double cam_time0, double cam_time1,
                        double wheel_speed_max, plv_zupt_result *result, double *dx) {
  if (!ctx || !opt || !imu || !result || !dx || ctx->cov_n < 1) return PLV_E_BADARG;
  const int nst = ctx->cov_n;
  *result = plv_zupt_result{};
  std::fill(dx, dx + nst, 0.0);
  double H[kRows * kCols], res[kRows];
  int cols[kCols];
  TRY(zupt_gate(ctx, opt, imu, noise, n, t, wm, am, imu_id, H, res, cols, &result->chi2));
  TRY(plv_db_disparity(ctx, cam_time0, cam_time1, &result->disparity_mean, &result->disparity_std, &result->disparity_n));
  result->chi2_threshold = opt->chi2_mult * plv_chi2_quantile95(kRows);
  result->speed = std::sqrt(imu->v[0] * imu->v[0] + imu->v[1] * imu->v[1] + imu->v[2] * imu->v[2]);
  result->wheel_vetoed = wheel_speed_max >= 0.0 && wheel_speed_max > opt->max_wheel_speed;
  result->disparity_passed = result->disparity_n >= opt->min_disparity_feats && result->disparity_mean < opt->max_disparity;
  result->imu_passed = result->chi2 < result->chi2_threshold && result->speed <= opt->max_velocity;
  result->stationary = !result->wheel_vetoed && (result->disparity_passed || result->imu_passed);
  if (!result->stationary) return PLV_OK;
  // (with the disparity alone the update is applied whatever the gate says, as upstream does)
  const int rc = plv_ekf_update(ctx, nullptr, nst, nst, H, kRows, kCols, kRows, cols, res, nullptr, dx);
  if (rc == PLV_OK) result->updated = 1;
  return rc;
}

}  // extern "C"
