// wheel_api.hip — wheel odometry updater, 3D types.
//
//   UpdaterWheel::select_wheel_data / interpolate_data   REF: PL-VIWO/src/update/wheel/UpdaterWheel.cpp:142-215,784-794 (host)
//   UpdaterWheel::update                                 REF: UpdaterWheel.cpp:72-139
//   preintegration_3D / preintegration_intrinsics_3D     REF: UpdaterWheel.cpp:648-782, 472-500
//   compute_linear_system_3D                             REF: UpdaterWheel.cpp:327-424
//   Chi2Check + StateHelper::EKFUpdate with a full R     REF: UpdaterStatistics.cpp:94-117, StateHelper.cpp:94-173
//
// wheel_kernel: one workgroup.  The preintegration is a sequential recursion over the wheel samples between two clones
// (RK4 on a quaternion + a 6x6 covariance): lane 0 integrates the means, the 6x6 products Phi Cov Phi^T + Phi_n Q Phi_n^T
// are one element per lane.  The linear system is then laid down by lane 0 and rotated into the eigenbasis of the preintegrated
// covariance, Cov = V D V^T (Jacobi rotations on lane 0): V^T H, V^T res and the diagonal D are the same measurement with the
// full 6x6 (3x3) noise R = Cov, in the form plv_ekf_update takes.  Nothing divides by a pivot of Cov, so a covariance that is
// only positive SEMI-definite (the 2D types at standstill: no noise enters the lateral coordinate) is applied like any other.
// wheel_gate_kernel forms S = (V^T H) P (V^T H)^T + D on the resident P for the chi-square gate; the update uses the same S.
// Where every pivot of the Cholesky factorisation Cov = L L^T keeps more than kCholPivotMin of its diagonal entry, the kernels also
// leave the system whitened by L (H <- L^-1 H, res <- L^-1 res, R = I) and plv_wheel_update takes that one through the shared
// chi-square / EKF kernels: the same update again, and the arithmetic every well-conditioned covariance has always gone through.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "plv_ctx.hpp"
#include "so3.hpp"
#include "update_state.hpp"

namespace plv {
namespace {

struct WheelArgs {
  plv_wheel_options op;
  plv_wheel_state st;
  int n_data, k;
  const double *t, *m1, *m2;  // device
  double *out;                // [H 6*k col-major][res 6][Cov 36][R 9][p 3][Hw 6*k][resw 6][D 6][Hc 6*k][resc 6][chol 1]   (Hw = V^T H, Cov = V D V^T; Hc = L^-1 H, Cov = L L^T)
};

__device__ __forceinline__ void wheel_vel(const WheelArgs &A, double a1, double a2, V3 &w, V3 &v) {
  const double rl = A.st.intr[0], rr = A.st.intr[1], b = A.st.intr[2];
  if (A.op.type == PLV_WHEEL3D_ANG) {
    w = V3{{0, 0, (a2 * rr - a1 * rl) / b}};
    v = V3{{(a2 * rr + a1 * rl) / 2, 0, 0}};
  } else if (A.op.type == PLV_WHEEL3D_LIN) {
    w = V3{{0, 0, (a2 - a1) / b}};
    v = V3{{(a2 + a1) / 2, 0, 0}};
  } else {
    w = V3{{0, 0, a1}};
    v = V3{{a2, 0, 0}};
  }
}

__device__ __forceinline__ void put3w(double *M, int ldm_, int r0, int c0, const M3 &B) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[(r0 + r) * ldm_ + c0 + c] = B(r, c);
}

// Cyclic Jacobi on a symmetric M x M matrix (row-major, overwritten): A -> diagonal d, V's columns the eigenvectors, A = V d V^T.
// A zero off-diagonal entry takes no rotation, so a row / column of zeros keeps its exact zero eigenvalue and its unit vector.
// One thread.  REF for the rotation: Golub & Van Loan, Matrix Computations, alg. 8.4.1 (symmetric Schur 2 x 2).
template <int M>
__device__ void jacobi_eig(double *A, double *V, double *d) {
  for (int e = 0; e < M * M; ++e) V[e] = (e % (M + 1) == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < M; ++p)
      for (int q = p + 1; q < M; ++q) off += fabs(A[p * M + q]);
    if (off == 0.0) break;
    for (int p = 0; p < M; ++p)
      for (int q = p + 1; q < M; ++q) {
        const double apq = A[p * M + q];
        if (apq == 0.0) continue;
        const double app = A[p * M + p], aqq = A[q * M + q];
        // an entry that no longer moves either diagonal is done (it would only be chased through underflow otherwise)
        if (sweep > 3 && fabs(app) + 100.0 * fabs(apq) == fabs(app) && fabs(aqq) + 100.0 * fabs(apq) == fabs(aqq)) {
          A[p * M + q] = A[q * M + p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int i = 0; i < M; ++i) {  // A <- A J
          const double aip = A[i * M + p], aiq = A[i * M + q];
          A[i * M + p] = c * aip - sn * aiq;
          A[i * M + q] = sn * aip + c * aiq;
        }
        for (int i = 0; i < M; ++i) {  // A <- J^T A
          const double api = A[p * M + i], aqi = A[q * M + i];
          A[p * M + i] = c * api - sn * aqi;
          A[q * M + i] = sn * api + c * aqi;
        }
        A[p * M + q] = A[q * M + p] = 0.0;
        for (int i = 0; i < M; ++i) {  // V <- V J
          const double vip = V[i * M + p], viq = V[i * M + q];
          V[i * M + p] = c * vip - sn * viq;
          V[i * M + q] = sn * vip + c * viq;
        }
      }
  }
  // (a covariance is positive semi-definite: an eigenvalue below zero is rounding of a zero one)
  for (int i = 0; i < M; ++i) d[i] = A[i * M + i] < 0.0 ? 0.0 : A[i * M + i];
}

// A Cholesky pivot d^2 = Cov_jj - sum L_jq^2 is the variance of row j given the rows before it; whitening by L divides by its root
// and loses about eps * Cov_jj / d^2 of the result.  Below this fraction (and for a zero or non-finite entry) the eigenbasis is used.
constexpr double kCholPivotMin = 1e-6;

// Cov = L L^T (lower, row-major M x M); returns whether every pivot passed kCholPivotMin.  One thread.
template <int M>
__device__ bool cholesky_wellposed(const double *C, double *L) {
  bool ok = true;
  for (int e = 0; e < M * M; ++e) L[e] = 0.0;
  for (int j = 0; j < M; ++j) {
    double d = C[j * M + j];
    for (int q = 0; q < j; ++q) d -= L[j * M + q] * L[j * M + q];
    if (!(d > kCholPivotMin * C[j * M + j])) ok = false;
    d = sqrt(d);
    L[j * M + j] = d;
    for (int i2 = j + 1; i2 < M; ++i2) {
      double v = C[i2 * M + j];
      for (int q = 0; q < j; ++q) v -= L[i2 * M + q] * L[j * M + q];
      L[i2 * M + j] = v / d;
    }
  }
  return ok;
}

// Whitened system: forward substitution with L, one column per lane (column k = the residual)
template <int M>
__device__ __forceinline__ void whiten_columns(const double *L, const double *Hr, const double *resv, int k, int tid, double *oHc, double *oresc) {
  for (int col = tid; col <= k; col += 64) {
    double y[M];
#pragma unroll
    for (int i2 = 0; i2 < M; ++i2) {
      double v = col < k ? Hr[i2 * k + col] : resv[i2];
      for (int q = 0; q < i2; ++q) v -= L[i2 * M + q] * y[q];
      y[i2] = v / L[i2 * M + i2];
    }
#pragma unroll
    for (int i2 = 0; i2 < M; ++i2) {
      if (col < k) oHc[col * M + i2] = y[i2];
      else oresc[i2] = y[i2];
    }
  }
}

// Rotated system, one column per lane (column k = the residual): y = V^T x.  Hr row-major [M][k]; oHw col-major M x k.
template <int M>
__device__ __forceinline__ void rotate_columns(const double *V, const double *Hr, const double *resv, int k, int tid, double *oHw, double *oresw) {
  for (int col = tid; col <= k; col += 64) {
#pragma unroll
    for (int i2 = 0; i2 < M; ++i2) {
      double y = 0.0;
#pragma unroll
      for (int q = 0; q < M; ++q) y += V[q * M + i2] * (col < k ? Hr[q * k + col] : resv[q]);
      if (col < k) oHw[col * M + i2] = y;
      else oresw[i2] = y;
    }
  }
}

__global__ void __launch_bounds__(64) wheel_kernel(WheelArgs A) {
  __shared__ double Cov[36], Ptr[36], Pns[36], Qd[6], X[36], Y[36];
  __shared__ double R3[9], p3[3], dRdi[9], dpdi[9];
  __shared__ double Hr[6 * 24], resv[6], V[36], Dg[6], L[36], chol;
  const int tid = threadIdx.x, r = tid / 6, c = tid % 6;
  const bool el = tid < 36;
  if (el) Cov[tid] = 0.0;
  if (tid < 9) {
    R3[tid] = (tid % 4 == 0) ? 1.0 : 0.0;
    dRdi[tid] = 0.0;
    dpdi[tid] = 0.0;
  }
  if (tid < 3) p3[tid] = 0.0;
  __syncthreads();
  for (int i = 0; i < A.n_data - 1; ++i) {
    const double dt = A.t[i + 1] - A.t[i];
    if (tid == 0) {
      const M3 R_3D = ldM(R3);
      const V3 p_3D = ldV(p3);
      if (A.op.do_calib_int) {  // preintegration_intrinsics_3D
        const double rl = A.st.intr[0], rr = A.st.intr[1], b = A.st.intr[2];
        const double w_l = A.m1[i], w_r = A.m2[i];
        const V3 w{{0, 0, (w_r * rr - w_l * rl) / b}}, v{{(w_r * rr + w_l * rl) / 2, 0, 0}};
        M3 Hwx{{0, 0, 0, 0, 0, 0, -w_l / b, w_r / b, -(w_r * rr - w_l * rl) / (b * b)}};
        M3 Hvx{{w_l / 2, w_r / 2, 0, 0, 0, 0, 0, 0, 0}};
        const M3 R = exp_so3(vsc(w, -dt));
        const M3 Hth = ms(Jl_so3(vsc(w, -dt)), dt);
        const M3 dR = ldM(dRdi), dp = ldM(dpdi);
        const M3 ndp = ma(msb(dp, mm(mm(tp(R_3D), skew3(vsc(v, dt))), dR)), ms(mm(tp(R_3D), Hvx), dt));
        const M3 ndR = ma(mm(R, dR), mm(Hth, Hwx));
#pragma unroll
        for (int e = 0; e < 9; ++e) {
          dpdi[e] = ndp.m[e];
          dRdi[e] = ndR.m[e];
        }
      }
      // preintegration_3D: RK4 means
      V3 w1, v1, w2, v2;
      wheel_vel(A, A.m1[i], A.m2[i], w1, v1);
      wheel_vel(A, A.m1[i + 1], A.m2[i + 1], w2, v2);
      V3 w_hat = w1, v_hat = v1;
      const V3 w_alpha = vsc(vsub(w2, w1), 1.0 / dt), v_jerk = vsc(vsub(v2, v1), 1.0 / dt);
      const Q4 q_local = rot_2_quat(R_3D);
      const Q4 dq_0{{0, 0, 0, 1}};
      auto qdot = [&](const Q4 &dq) {
        const Q4 o = omega_times(w_hat, dq);
        return Q4{{dt * (0.5 * o[0]), dt * (0.5 * o[1]), dt * (0.5 * o[2]), dt * (0.5 * o[3])}};
      };
      auto pdot = [&](const Q4 &dq) { return vsc(mv(tp(quat_2_Rot(quat_multiply(dq, q_local))), v_hat), dt); };
      const Q4 k1_q = qdot(dq_0);
      const V3 k1_p = pdot(dq_0);
      w_hat = vadd(w_hat, vsc(w_alpha, 0.5 * dt));
      v_hat = vadd(v_hat, vsc(v_jerk, 0.5 * dt));
      const Q4 dq_1 = quatnorm(qaxpy(dq_0, 0.5, k1_q));
      const Q4 k2_q = qdot(dq_1);
      const V3 k2_p = pdot(dq_1);
      const Q4 dq_2 = quatnorm(qaxpy(dq_0, 0.5, k2_q));
      const Q4 k3_q = qdot(dq_2);
      const V3 k3_p = pdot(dq_2);
      w_hat = vadd(w_hat, vsc(w_alpha, 0.5 * dt));
      v_hat = vadd(v_hat, vsc(v_jerk, 0.5 * dt));
      const Q4 dq_3 = quatnorm(qaxpy(dq_0, 1.0, k3_q));
      const Q4 k4_q = qdot(dq_3);
      const V3 k4_p = pdot(dq_3);
      const Q4 dq = quatnorm(qaxpy(qaxpy(qaxpy(qaxpy(dq_0, 1.0 / 6.0, k1_q), 1.0 / 3.0, k2_q), 1.0 / 3.0, k3_q), 1.0 / 6.0, k4_q));
      const M3 R_new = quat_2_Rot(quat_multiply(dq, q_local));
      const V3 new_p = vadd(vadd(vadd(vadd(p_3D, vsc(k1_p, 1.0 / 6.0)), vsc(k2_p, 1.0 / 3.0)), vsc(k3_p, 1.0 / 3.0)), vsc(k4_p, 1.0 / 6.0));
      // Phi_tr, Phi_ns, Q
      const double nw = A.op.noise_w * A.op.noise_w, nv = A.op.noise_v * A.op.noise_v, np = A.op.noise_p * A.op.noise_p, b = A.st.intr[2];
      double q0, q3;
      if (A.op.type == PLV_WHEEL3D_ANG) {
        q0 = nw / dt, q3 = nw / dt;
      } else if (A.op.type == PLV_WHEEL3D_LIN) {
        q0 = nv / b / b / dt, q3 = nv / 2 / 2 / dt;
      } else {
        q0 = nw / dt, q3 = nv / dt;
      }
      Qd[0] = q0, Qd[3] = q3, Qd[1] = Qd[2] = Qd[4] = Qd[5] = np / dt;
      for (int e = 0; e < 36; ++e) Ptr[e] = Pns[e] = 0.0;
      const M3 RT = tp(R_3D);
      put3w(Ptr, 6, 0, 0, mm(R_new, RT));
      put3w(Ptr, 6, 3, 0, mm(ms(RT, -1.0), skew3(mv(RT, vsub(new_p, p_3D)))));
      put3w(Ptr, 6, 3, 3, eye3());
      put3w(Pns, 6, 0, 0, ms(eye3(), dt));
      put3w(Pns, 6, 3, 3, ms(RT, dt));
#pragma unroll
      for (int e = 0; e < 9; ++e) R3[e] = R_new.m[e];
      stV(p3, new_p);
    }
    __syncthreads();
    double a = 0.0, bq = 0.0;
    if (el) {  // X = Phi_tr Cov, Y = Phi_ns Q
#pragma unroll
      for (int k2 = 0; k2 < 6; ++k2) a += Ptr[r * 6 + k2] * Cov[k2 * 6 + c];
      bq = Pns[r * 6 + c] * Qd[c];
      X[tid] = a;
      Y[tid] = bq;
    }
    __syncthreads();
    double s = 0.0;
    if (el) {
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int k2 = 0; k2 < 6; ++k2) {
        s1 += X[r * 6 + k2] * Ptr[c * 6 + k2];
        s2 += Y[r * 6 + k2] * Pns[c * 6 + k2];
      }
      s = s1 + s2;
    }
    __syncthreads();
    if (el) X[tid] = s;
    __syncthreads();
    if (el) Cov[tid] = 0.5 * (X[tid] + X[c * 6 + r]);
    __syncthreads();
  }
  const int k = A.k;
  if (tid == 0) {  // compute_linear_system_3D
    const M3 R_3D = ldM(R3);
    const V3 p_3D = ldV(p3);
    V3 pI0 = ldV(A.st.p0), pI1 = ldV(A.st.p1);
    M3 RG0 = ldM(A.st.R0), RG1 = ldM(A.st.R1);
    const V3 pIinO = ldV(A.st.p_IinO);
    const M3 RItoO = ldM(A.st.R_ItoO);
    const V3 pOinI = mv(ms(tp(RItoO), -1.0), pIinO);
    M3 RO0toO1 = mm(mm(mm(RItoO, RG1), tp(RG0)), tp(RItoO));
    const V3 r_ori = vsc(log_so3(mm(R_3D, tp(RO0toO1))), -1.0);
    const V3 p_est = mv(mm(RItoO, RG0), vsub(vsub(vadd(pI1, mv(tp(RG1), pOinI)), pI0), mv(tp(RG0), pOinI)));
    const V3 r_pos = vsub(p_3D, p_est);
    stV(resv, r_ori);
    stV(resv + 3, r_pos);
    for (int e = 0; e < 6 * k; ++e) Hr[e] = 0.0;
    pI0 = ldV(A.st.p0_fej), pI1 = ldV(A.st.p1_fej), RG0 = ldM(A.st.R0_fej), RG1 = ldM(A.st.R1_fej);
    RO0toO1 = mm(mm(mm(RItoO, RG1), tp(RG0)), tp(RItoO));
    const M3 RO1toO0 = tp(RO0toO1);
    const M3 dzr_dth0 = mm(mm(ms(RItoO, -1.0), RG1), tp(RG0)), dzr_dth1 = RItoO;
    const M3 dzp_dth0 = mm(RItoO, skew3(vsub(vadd(mv(RG0, pI1), mv(mm(RG0, tp(RG1)), pOinI)), mv(RG0, pI0))));
    const M3 dzp_dp0 = mm(ms(RItoO, -1.0), RG0);
    const M3 dzp_dth1 = mm(mm(mm(ms(RItoO, -1.0), RG0), tp(RG1)), skew3(pOinI));
    const M3 dzp_dp1 = mm(RItoO, RG0);
    put3w(Hr, k, 0, 0, dzr_dth0), put3w(Hr, k, 0, 6, dzr_dth1);
    put3w(Hr, k, 3, 0, dzp_dth0), put3w(Hr, k, 3, 3, dzp_dp0), put3w(Hr, k, 3, 6, dzp_dth1), put3w(Hr, k, 3, 9, dzp_dp1);
    int hc = 12;
    if (A.op.do_calib_ext) {
      put3w(Hr, k, 0, hc, msb(eye3(), RO0toO1));
      put3w(Hr, k, 3, hc, ma(skew3(vsub(mv(mm(RItoO, RG0), vsub(pI1, pI0)), mv(RO1toO0, pIinO))), mm(RO1toO0, skew3(pIinO))));
      put3w(Hr, k, 3, hc + 3, ma(ms(RO1toO0, -1.0), eye3()));
      hc += 6;
    }
    if (A.op.do_calib_dt) {
      const V3 w0 = ldV(A.st.w0), v0 = ldV(A.st.v0), w1 = ldV(A.st.w1), v1 = ldV(A.st.v1);
      const V3 a = vadd(mv(dzr_dth0, w0), mv(dzr_dth1, w1));
      const V3 cc = vadd(vadd(vadd(mv(dzp_dth0, w0), mv(dzp_dp0, v0)), mv(dzp_dth1, w1)), mv(dzp_dp1, v1));
      Hr[0 * k + hc] = a[0], Hr[1 * k + hc] = a[1], Hr[2 * k + hc] = a[2];
      Hr[3 * k + hc] = cc[0], Hr[4 * k + hc] = cc[1], Hr[5 * k + hc] = cc[2];
      hc += 1;
    }
    if (A.op.do_calib_int) {
      put3w(Hr, k, 0, hc, ms(ldM(dRdi), -1.0));
      put3w(Hr, k, 3, hc, ms(ldM(dpdi), -1.0));
    }
    // eigenbasis of the preintegrated covariance (X is free after the recursion)
    for (int e = 0; e < 36; ++e) X[e] = Cov[e];
    jacobi_eig<6>(X, V, Dg);
    chol = cholesky_wellposed<6>(Cov, L) ? 1.0 : 0.0;
  }
  __syncthreads();
  double *oH = A.out, *ores = oH + 6 * k, *oC = ores + 6, *oR = oC + 36, *op = oR + 9, *oHw = op + 3, *oresw = oHw + 6 * k;
  for (int e = tid; e < 6 * k; e += 64) {
    const int cc = e / 6, rr = e % 6;
    oH[e] = Hr[rr * k + cc];  // col-major
  }
  if (tid < 6) ores[tid] = resv[tid];
  if (el) oC[tid] = Cov[tid];
  if (tid < 9) oR[tid] = R3[tid];
  if (tid < 3) op[tid] = p3[tid];
  if (tid < 6) oresw[6 + tid] = Dg[tid];
  rotate_columns<6>(V, Hr, resv, k, tid, oHw, oresw);
  double *oHc = oresw + 12, *oresc = oHc + 6 * k;
  if (tid == 0) oresc[6] = chol;
  whiten_columns<6>(L, Hr, resv, k, tid, oHc, oresc);
}

// Sensitivities of one constant-rate planar arc: heading `a`, turn rate `r` (the heading advances by -r dt) and forward speed `s`
// held over dt.  d(x, y) by the heading (_a), the rate (_r) and the speed (_s); below |r| = 1e-4 the straight-line limits.  The
// closed forms are the model's (REF: UpdaterWheel.cpp:449-461, 574-611, evaluated there twice: once per intrinsic chain and once
// for the covariance), written here once over the two differences every one of them contains; operation order as there.
struct ArcSens {
  double x_a, y_a, x_r, y_r, x_s, y_s;
};
__device__ inline ArcSens arc_sensitivities(double a, double r, double s, double dt) {
  ArcSens d;
  if (fabs(r) < 0.0001) {
    const double sa = sin(a), ca = cos(a);
    d.x_a = s * sa * dt, d.y_a = s * ca * dt;
    d.x_r = s * sa * dt * dt / 2, d.y_r = s * ca * dt * dt / 2;
    d.x_s = ca * dt, d.y_s = -sa * dt;
    return d;
  }
  const double a_end = a - r * dt;
  const double dcos = cos(a_end) - cos(a), dsin = sin(a_end) - sin(a);
  d.x_a = (s * dcos) / r;
  d.y_a = -(s * dsin) / r;
  d.x_r = (s * dsin) / r / r + (s * cos(a_end) * dt) / r;
  d.y_r = (s * dcos) / r / r - (s * sin(a_end) * dt) / r;
  d.x_s = -dsin / r;
  d.y_s = -dcos / r;
  return d;
}

// The 2D types (REF: preintegration_2D :502-646, preintegration_intrinsics_2D :426-470, compute_linear_system_2D :217-325):
// scalar recursions and a 3x3 covariance, all on lane 0; the lanes then rotate one column each.
// out: [H 3*k col-major][res 3][Cov 9][R 9 = I][meas 3 = theta x y][Hw 3*k][resw 3][D 3][Hc 3*k][resc 3][chol 1]
__global__ void __launch_bounds__(64) wheel2d_kernel(WheelArgs A) {
  __shared__ double Hr[3 * 24], resv[3], V[9], Dg[3], C2[9], meas[3], L[9], chol;
  const int tid = threadIdx.x, k = A.k;
  if (tid == 0) {
    double head = 0, px = 0, py = 0;   // the preintegrated planar pose: heading, position
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double g_head[3] = {0, 0, 0}, g_px[3] = {0, 0, 0}, g_py[3] = {0, 0, 0};   // its gradients by (r_left, r_right, base)
    const double rl = A.st.intr[0], rr = A.st.intr[1], b = A.st.intr[2];
    for (int i = 0; i < A.n_data - 1; ++i) {
      const double dt = A.t[i + 1] - A.t[i];
      if (A.op.do_calib_int) {
        const double enc_l = A.m1[i], enc_r = A.m2[i];
        const double rate = (enc_r * rr - enc_l * rl) / b, speed = (enc_r * rr + enc_l * rl) / 2;
        const double rate_by[3] = {-enc_l / b, enc_r / b, -(enc_r * rr - enc_l * rl) / (b * b)}, speed_by[3] = {enc_l / 2, enc_r / 2, 0};
        const ArcSens d = arc_sensitivities(head, rate, speed, dt);
        for (int c = 0; c < 3; ++c) {
          g_px[c] = ((g_px[c] + d.x_a * g_head[c]) + d.x_r * rate_by[c]) + d.x_s * speed_by[c];
          g_py[c] = ((g_py[c] + d.y_a * g_head[c]) + d.y_r * rate_by[c]) + d.y_s * speed_by[c];
        }
        for (int c = 0; c < 3; ++c) g_head[c] = g_head[c] + dt * rate_by[c];
      }
      // rate and speed at both ends of the interval, from what the type measures
      double rate0, rate1, speed0, speed1;
      if (A.op.type == PLV_WHEEL2D_ANG) {
        rate0 = (A.m2[i] * rr - A.m1[i] * rl) / b, speed0 = (A.m2[i] * rr + A.m1[i] * rl) / 2;
        rate1 = (A.m2[i + 1] * rr - A.m1[i + 1] * rl) / b, speed1 = (A.m2[i + 1] * rr + A.m1[i + 1] * rl) / 2;
      } else if (A.op.type == PLV_WHEEL2D_LIN) {
        rate0 = (A.m2[i] - A.m1[i]) / b, speed0 = (A.m2[i] + A.m1[i]) / 2;
        rate1 = (A.m2[i + 1] - A.m1[i + 1]) / b, speed1 = (A.m2[i + 1] + A.m1[i + 1]) / 2;
      } else {
        rate0 = A.m1[i], speed0 = A.m2[i], rate1 = A.m1[i + 1], speed1 = A.m2[i + 1];
      }
      // RK4 over the interval with rate and speed interpolated linearly; the stages' headings are relative to the interval's start
      const double rate_slope = (rate1 - rate0) / dt, speed_slope = (speed1 - speed0) / dt;
      double rate = rate0, speed = speed0;
      const double s1_head = -rate * dt, s1_x = speed * 1 * dt;
      const double mid_a = 0.5 * s1_head;
      rate += 0.5 * rate_slope * dt;
      speed += 0.5 * speed_slope * dt;
      const double s2_head = -rate * dt, s2_x = speed * cos(mid_a) * dt;
      const double mid_b = 0.5 * s2_head;
      const double s3_head = -rate * dt, s3_x = speed * cos(mid_b) * dt;
      const double end_c = s3_head;
      rate += 0.5 * rate_slope * dt;
      speed += 0.5 * speed_slope * dt;
      const double s4_head = -rate * dt, s4_x = speed * cos(end_c) * dt;
      const double head_next = head + (1.0 / 6.0) * (s1_head + 2 * s2_head + 2 * s3_head + s4_head);
      const double px_next = px + (1.0 / 6.0) * (s1_x + 2 * s2_x + 2 * s3_x + s4_x);
      double py_next;   // (the lateral coordinate takes the arc's closed form on the interval's first sample, as the reference does)
      if (fabs(rate0) < 0.0001)
        py_next = py - speed0 * sin(head - rate0 * dt) * dt;
      else
        py_next = py - (speed0 * (cos(head - rate0 * dt) - cos(head))) / rate0;
      // how the measurement noise enters rate and speed
      double rate_n[2], speed_n[2];
      if (A.op.type == PLV_WHEEL2D_ANG) {
        rate_n[0] = rl / b, rate_n[1] = -rr / b, speed_n[0] = -rl / 2, speed_n[1] = -rr / 2;
      } else if (A.op.type == PLV_WHEEL2D_LIN) {
        rate_n[0] = 1.0 / b, rate_n[1] = -1.0 / b, speed_n[0] = -1.0 / 2, speed_n[1] = -1.0 / 2;
      } else {
        rate_n[0] = 1, rate_n[1] = 0, speed_n[0] = 0, speed_n[1] = 1;
      }
      const ArcSens d = arc_sensitivities(head, rate0, speed0, dt);
      const double Ptr[9] = {1, 0, 0, d.x_a, 1, 0, d.y_a, 0, 1};
      double Pns[6];
      for (int c = 0; c < 2; ++c) {
        Pns[c] = dt * rate_n[c];
        Pns[2 + c] = d.x_r * rate_n[c] + d.x_s * speed_n[c];
        Pns[4 + c] = d.y_r * rate_n[c] + d.y_s * speed_n[c];
      }
      double Q0, Q1;
      if (A.op.type == PLV_WHEEL2D_ANG)
        Q0 = Q1 = A.op.noise_w * A.op.noise_w / dt;
      else if (A.op.type == PLV_WHEEL2D_LIN)
        Q0 = Q1 = A.op.noise_v * A.op.noise_v / dt;
      else
        Q0 = A.op.noise_w * A.op.noise_w / dt, Q1 = A.op.noise_v * A.op.noise_v / dt;
      double X[9], N[9];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          double a = 0;
          for (int q = 0; q < 3; ++q) a += Ptr[3 * r + q] * C[3 * q + c];
          X[3 * r + c] = a;
        }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          double a = 0;
          for (int q = 0; q < 3; ++q) a += X[3 * r + q] * Ptr[3 * c + q];
          const double nn = (Pns[2 * r] * Q0) * Pns[2 * c] + (Pns[2 * r + 1] * Q1) * Pns[2 * c + 1];
          N[3 * r + c] = a + nn;
        }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = 0.5 * (N[3 * r + c] + N[3 * c + r]);
      head = head_next, px = px_next, py = py_next;
    }
    // compute_linear_system_2D
    V3 pI0 = ldV(A.st.p0), pI1 = ldV(A.st.p1);
    M3 RG0 = ldM(A.st.R0), RG1 = ldM(A.st.R1);
    const V3 pIinO = ldV(A.st.p_IinO);
    const M3 RItoO = ldM(A.st.R_ItoO);
    const V3 pOinI = mv(ms(tp(RItoO), -1.0), pIinO);
    const double theta_est = log_so3(mm(mm(mm(RItoO, RG1), tp(RG0)), tp(RItoO)))[2];
    const V3 d_est = mv(mm(RItoO, RG0), vsub(vsub(vadd(pI1, mv(tp(RG1), pOinI)), pI0), mv(tp(RG0), pOinI)));
    resv[0] = theta_est - head;
    resv[1] = px - d_est[0];
    resv[2] = py - d_est[1];
    for (int e = 0; e < 3 * k; ++e) Hr[e] = 0.0;
    pI0 = ldV(A.st.p0_fej), pI1 = ldV(A.st.p1_fej), RG0 = ldM(A.st.R0_fej), RG1 = ldM(A.st.R1_fej);
    const M3 RO0toO1 = mm(mm(mm(RItoO, RG1), tp(RG0)), tp(RItoO)), RO1toO0 = tp(RO0toO1);
    const M3 A0 = mm(mm(ms(RItoO, -1.0), RG1), tp(RG0));
    const M3 Pth0 = mm(RItoO, skew3(mv(RG0, vsub(vadd(pI1, mv(tp(RG1), pOinI)), pI0))));
    const M3 Pp0 = mm(ms(RItoO, -1.0), RG0);
    const M3 Pth1 = mm(mm(mm(ms(RItoO, -1.0), RG0), tp(RG1)), skew3(pOinI));
    const M3 Pp1 = mm(RItoO, RG0);
    auto row_of = [&](int r, int c0, const M3 &B, int br) {
      for (int c = 0; c < 3; ++c) Hr[r * k + c0 + c] = B(br, c);
    };
    row_of(0, 0, A0, 2);
    row_of(0, 6, RItoO, 2);
    for (int r = 0; r < 2; ++r) {
      row_of(1 + r, 0, Pth0, r);
      row_of(1 + r, 3, Pp0, r);
      row_of(1 + r, 6, Pth1, r);
      row_of(1 + r, 9, Pp1, r);
    }
    int hc = 12;
    if (A.op.do_calib_ext) {
      row_of(0, hc, msb(eye3(), RO0toO1), 2);
      const M3 Dth = ma(skew3(vsub(mv(mm(RItoO, RG0), vsub(pI1, pI0)), mv(RO1toO0, pIinO))), mm(RO1toO0, skew3(pIinO)));
      const M3 Dp = ma(ms(RO1toO0, -1.0), eye3());
      for (int r = 0; r < 2; ++r) {
        row_of(1 + r, hc, Dth, r);
        row_of(1 + r, hc + 3, Dp, r);
      }
      hc += 6;
    }
    if (A.op.do_calib_dt) {
      const V3 w0 = ldV(A.st.w0), v0 = ldV(A.st.v0), w1 = ldV(A.st.w1), v1 = ldV(A.st.v1);
      const V3 a = vadd(mv(A0, w0), mv(RItoO, w1));
      const V3 cc = vadd(vadd(vadd(mv(Pth0, w0), mv(Pp0, v0)), mv(Pth1, w1)), mv(Pp1, v1));
      Hr[0 * k + hc] = a[2];
      Hr[1 * k + hc] = cc[0];
      Hr[2 * k + hc] = cc[1];
      hc += 1;
    }
    if (A.op.do_calib_int)
      for (int c = 0; c < 3; ++c) {
        Hr[0 * k + hc + c] = -g_head[c];
        Hr[1 * k + hc + c] = -g_px[c];
        Hr[2 * k + hc + c] = -g_py[c];
      }
    for (int e = 0; e < 9; ++e) C2[e] = C[e];
    chol = cholesky_wellposed<3>(C, L) ? 1.0 : 0.0;
    jacobi_eig<3>(C, V, Dg);
    meas[0] = head, meas[1] = px, meas[2] = py;
  }
  __syncthreads();
  double *oH = A.out, *ores = oH + 3 * k, *oC = ores + 3, *oR = oC + 9, *op = oR + 9, *oHw = op + 3, *oresw = oHw + 3 * k;
  for (int e = tid; e < 3 * k; e += 64) oH[e] = Hr[(e % 3) * k + e / 3];
  if (tid < 3) {
    ores[tid] = resv[tid];
    op[tid] = meas[tid];
  }
  if (tid < 9) {
    oC[tid] = C2[tid];
    oR[tid] = (tid % 4 == 0) ? 1.0 : 0.0;
  }
  if (tid < 3) oresw[3 + tid] = Dg[tid];
  rotate_columns<3>(V, Hr, resv, k, tid, oHw, oresw);
  double *oHc = oresw + 6, *oresc = oHc + 3 * k;
  if (tid == 0) oresc[3] = chol;
  whiten_columns<3>(L, Hr, resv, k, tid, oHc, oresc);
}

// Chi2Check on the rotated system: chi2 = r^T S^-1 r, S = H P[cols, cols] H^T + diag(D)   (REF: UpdaterStatistics.cpp:94-117).
// One workgroup: the M x k products one element per lane, the M x M Cholesky and the forward substitution on lane 0.
// H col-major M x k, P col-major n x n; chi2 is NaN when S is not positive definite (the caller then rejects).
struct WheelGateArgs {
  const double *P;
  int n, k, rows;
  int cols[24];
  const double *H, *res, *D;
  double *chi2;
};
__global__ void __launch_bounds__(64) wheel_gate_kernel(WheelGateArgs G) {
  __shared__ double T[6 * 24], S[36];
  const int tid = threadIdx.x, k = G.k, M = G.rows;
  for (int e = tid; e < M * k; e += 64) {  // T = H P[cols, cols]
    const int i = e / k, b = e - i * k;
    double s = 0.0;
    for (int a = 0; a < k; ++a) s += G.H[a * M + i] * G.P[(size_t)G.cols[b] * G.n + G.cols[a]];
    T[i * k + b] = s;
  }
  __syncthreads();
  if (tid < M * M) {
    const int i = tid / M, j = tid - i * M;
    double s = 0.0;
    for (int b = 0; b < k; ++b) s += T[i * k + b] * G.H[b * M + j];
    S[tid] = s + (i == j ? G.D[i] : 0.0);
  }
  __syncthreads();
  if (tid == 0) {
    double L[36], y[6], chi = 0.0;
    bool bad = false;
    for (int j = 0; j < M; ++j) {
      double d = S[j * M + j];
      for (int q = 0; q < j; ++q) d -= L[j * M + q] * L[j * M + q];
      if (!(d > 0.0)) bad = true;
      d = sqrt(d);
      L[j * M + j] = d;
      for (int i = j + 1; i < M; ++i) {
        double v = S[j * M + i];  // selfadjointView<Upper>
        for (int q = 0; q < j; ++q) v -= L[i * M + q] * L[j * M + q];
        L[i * M + j] = v / d;
      }
    }
    for (int i = 0; i < M; ++i) {
      double v = G.res[i];
      for (int q = 0; q < i; ++q) v -= L[i * M + q] * y[q];
      y[i] = v / L[i * M + i];
      chi += y[i] * y[i];
    }
    *G.chi2 = bad ? NAN : chi;
  }
}

int wheel_columns(const plv_wheel_options *op, const plv_wheel_state *st, int *cols) {
  int nc = 0;
  for (int i = 0; i < 6; ++i) cols[nc++] = st->pose0_id + i;
  for (int i = 0; i < 6; ++i) cols[nc++] = st->pose1_id + i;
  if (op->do_calib_ext)
    for (int i = 0; i < 6; ++i) cols[nc++] = st->ext_id + i;
  if (op->do_calib_dt) cols[nc++] = st->dt_id;
  if (op->do_calib_int)
    for (int i = 0; i < 3; ++i) cols[nc++] = st->intr_id + i;
  return nc;
}

// runs the kernel; host copies of every output block
int wheel_system(plv_ctx *ctx, const plv_wheel_options *op, const plv_wheel_state *st, int n_data, const double *t, const double *m1,
                 const double *m2, std::vector<double> &out, int &k, int &rows, double **d_out = nullptr) {
  if (!ctx || !op || !st || n_data < 2 || !t || !m1 || !m2 || op->type < 0 || op->type > PLV_WHEEL2D_CEN) return PLV_E_BADARG;
  k = 12 + (op->do_calib_ext ? 6 : 0) + (op->do_calib_dt ? 1 : 0) + (op->do_calib_int ? 3 : 0);
  rows = op->type >= PLV_WHEEL2D_ANG ? 3 : 6;
  (void)hipSetDevice(ctx->device);
  auto *us = plv_update_state(ctx);
  const size_t nd = (size_t)n_data, n_out = (size_t)3 * rows * k + rows + (size_t)rows * rows + 9 + 3 + 3 * rows + 1;
  TRY(us->eval.reserve((3 * nd + n_out + 1) * 8));  // (+ 1: the gate's chi2, plv_wheel_update)
  double *d = us->eval.as<double>();
  std::vector<double> h(3 * nd);
  std::copy(t, t + nd, h.begin());
  std::copy(m1, m1 + nd, h.begin() + nd);
  std::copy(m2, m2 + nd, h.begin() + 2 * nd);
  PLV_HIP_CHECK(plv::memcpy_async(d, h.data(), 3 * nd * 8, hipMemcpyHostToDevice, ctx->stream));
  WheelArgs A{};
  A.op = *op;
  A.st = *st;
  A.n_data = n_data;
  A.k = k;
  A.t = d, A.m1 = d + nd, A.m2 = d + 2 * nd;
  A.out = d + 3 * nd;
  {
    ProfScope ps(ctx->prof, "wheel_kernel", ctx->stream);
    if (rows == 6)
      hipLaunchKernelGGL(wheel_kernel, dim3(1), dim3(64), 0, ctx->stream, A);
    else
      hipLaunchKernelGGL(wheel2d_kernel, dim3(1), dim3(64), 0, ctx->stream, A);
  }
  PLV_HIP_CHECK(hipGetLastError());
  out.resize(n_out);
  PLV_HIP_CHECK(plv::memcpy_async(out.data(), A.out, n_out * 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  if (d_out) *d_out = A.out;
  return PLV_OK;
}

}  // namespace
}  // namespace plv

using namespace plv;

extern "C" {

int plv_select_wheel_data(int n, const double *t, const double *m1, const double *m2, double time0, double time1, int cap, double *ot,
                          double *o1, double *o2, int *n_out, int *ok) {
  if (!n_out || !ok || n < 0 || (n > 0 && (!t || !m1 || !m2))) return PLV_E_BADARG;
  *n_out = 0;
  *ok = 0;
  if (n < 1) return PLV_OK;                                  // :144-147
  if (t[n - 1] <= time1 || t[0] > time0) return PLV_OK;      // :150-154
  std::vector<double> vt, v1, v2;
  auto push = [&](double a, double b, double c) {
    vt.push_back(a);
    v1.push_back(b);
    v2.push_back(c);
  };
  auto interp = [&](int a, int b, double ts) {  // interpolate_data :784-794
    const double lambda = (ts - t[a]) / (t[b] - t[a]);
    push(ts, (1 - lambda) * m1[a] + lambda * m1[b], (1 - lambda) * m2[a] + lambda * m2[b]);
  };
  for (int i = 0; i < n - 1; i++) {
    if (t[i + 1] > time0 && t[i] < time0) {  // :162-166 split at time0
      interp(i, i + 1, time0);
      continue;
    }
    if (t[i] >= time0 && t[i + 1] <= time1) {  // :170-173 whole interval
      push(t[i], m1[i], m2[i]);
      continue;
    }
    if (t[i + 1] > time1) {  // :179-197 the last one, cut at time1
      if (t[i] > time1)
        interp(i - 1, i, time1);
      else
        push(t[i], m1[i], m2[i]);
      if (vt.back() != time1) interp(i, i + 1, time1);
      break;
    }
  }
  if (vt.size() < 2) return PLV_OK;  // :200-203
  for (size_t i = 0; i + 1 < vt.size(); i++)  // :207-212 zero-length steps removed
    if (std::fabs(vt[i + 1] - vt[i]) < 1e-12) {
      vt.erase(vt.begin() + i);
      v1.erase(v1.begin() + i);
      v2.erase(v2.begin() + i);
      i--;
    }
  *n_out = (int)vt.size();
  if ((int)vt.size() > cap) return PLV_E_CAPACITY;
  if (!ot || !o1 || !o2) return PLV_E_BADARG;
  std::copy(vt.begin(), vt.end(), ot);
  std::copy(v1.begin(), v1.end(), o1);
  std::copy(v2.begin(), v2.end(), o2);
  *ok = 1;
  return PLV_OK;
}

int plv_wheel_linear_system(plv_ctx *ctx, const plv_wheel_options *opt, const plv_wheel_state *st, int n_data, const double *t,
                            const double *m1, const double *m2, double *H, double *res, double *Cov, int *col_to_state, int *k_out,
                            int *rows_out, double *R_3D, double *p_3D) {
  if (!H || !res || !Cov || !col_to_state || !k_out) return PLV_E_BADARG;
  std::vector<double> out;
  int k = 0, rows = 0;
  TRY(wheel_system(ctx, opt, st, n_data, t, m1, m2, out, k, rows));
  const size_t o_res = (size_t)rows * k, o_cov = o_res + rows, o_R = o_cov + (size_t)rows * rows, o_p = o_R + 9;
  std::copy(out.begin(), out.begin() + o_res, H);
  std::copy(out.begin() + o_res, out.begin() + o_cov, res);
  std::copy(out.begin() + o_cov, out.begin() + o_R, Cov);
  if (R_3D) std::copy(out.begin() + o_R, out.begin() + o_p, R_3D);
  if (p_3D) std::copy(out.begin() + o_p, out.begin() + o_p + 3, p_3D);
  *k_out = wheel_columns(opt, st, col_to_state);
  if (rows_out) *rows_out = rows;
  return PLV_OK;
}

int plv_wheel_update(plv_ctx *ctx, const plv_wheel_options *opt, const plv_wheel_state *st, int n_data, const double *t,
                     const double *m1, const double *m2, uint8_t *accepted, double *dx) {
  if (!accepted || !dx || !ctx || ctx->cov_n < 1) return PLV_E_BADARG;
  std::vector<double> out;
  int k = 0, rows = 0;
  double *d_out = nullptr;
  TRY(wheel_system(ctx, opt, st, n_data, t, m1, m2, out, k, rows, &d_out));
  WheelGateArgs G{};
  wheel_columns(opt, st, G.cols);
  const int n = ctx->cov_n;
  for (int i = 0; i < k; ++i)
    if (G.cols[i] < 0 || G.cols[i] >= n) {
      set_last_error("plv_wheel_update: column %d maps to state %d outside the covariance (%d)", i, G.cols[i], n);
      return PLV_E_BADARG;
    }
  // the measurement in the eigenbasis of its noise: Hw = V^T H, resw = V^T res, R = diag(D)
  const size_t o_hw = (size_t)rows * k + rows + (size_t)rows * rows + 12, o_resw = o_hw + (size_t)rows * k, o_D = o_resw + rows;
  const size_t o_hc = o_D + rows, o_resc = o_hc + (size_t)rows * k, o_chol = o_resc + rows;
  const double *Hw = out.data() + o_hw, *resw = out.data() + o_resw, *D = out.data() + o_D;
  for (int i = 0; i < rows * k + 2 * rows; ++i)
    if (!std::isfinite(Hw[i])) {
      set_last_error("plv_wheel_update: the preintegrated measurement or its covariance is not finite");
      return PLV_E_NUMERIC;
    }
  if (out[o_chol] != 0.0) {
    // a well-conditioned covariance: Chi2Check + EKFUpdate on the system whitened by its Cholesky factor, R = I
    const double *Hc = out.data() + o_hc, *resc = out.data() + o_resc;
    for (int i = 0; i < rows * k + rows; ++i)
      if (!std::isfinite(Hc[i])) {
        set_last_error("plv_wheel_update: the whitened measurement is not finite");
        return PLV_E_NUMERIC;
      }
    return plv_slam_update(ctx, rows, k, rows, Hc, resc, G.cols, opt->chi2_mult, accepted, dx);
  }
  *accepted = 0;
  std::fill(dx, dx + n, 0.0);
  // Chi2Check(H, res, Cov): S = H P H^T + Cov, in the rotated basis
  G.P = ctx->d_P.as<double>();
  G.n = n, G.k = k, G.rows = rows;
  G.H = d_out + o_hw, G.res = d_out + o_resw, G.D = d_out + o_D;
  G.chi2 = d_out + o_chol + 1;
  {
    ProfScope ps(ctx->prof, "wheel_gate_kernel", ctx->stream);
    hipLaunchKernelGGL(wheel_gate_kernel, dim3(1), dim3(64), 0, ctx->stream, G);
  }
  PLV_HIP_CHECK(hipGetLastError());
  double chi = 0.0;
  PLV_HIP_CHECK(plv::memcpy_async(&chi, G.chi2, 8, hipMemcpyDeviceToHost, ctx->stream));
  PLV_HIP_CHECK(plv::stream_sync(ctx->stream));
  ctx->prof.collect();
  if (!(chi < opt->chi2_mult * plv_chi2_quantile95(rows))) return PLV_OK;  // REF: UpdaterWheel.cpp:126-131
  // EKFUpdate(H, res, Cov) == the rotated rows with the diagonal noise D
  const int rc = plv_ekf_update(ctx, nullptr, n, n, Hw, rows, k, rows, G.cols, resw, D, dx);
  if (rc == PLV_OK) *accepted = 1;
  return rc;
}

}  // extern "C"
