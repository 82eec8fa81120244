// so3.hpp — the one copy of the small fp64 arithmetic on 3-vectors, 3x3 matrices, SO(3) and JPL quaternions, for host and device.
// REF for every formula: open_vins/ov_core/src/utils/quat_ops.h (line ranges at the functions).
//
// The library is built -ffp-contract=off, so a result's bits depend on the order of operations alone: every function here keeps the
// order of the copy it replaced (tests/test_so3_header_cpu.py holds the exact ones to recorded bits), and host and device callers of
// one function form the same value.  Plain C++: a host-only file or a g++ program includes it without the HIP headers.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PLV_HD __host__ __device__
#else
#define PLV_HD
#endif

namespace plv {

struct V3 {
  double v[3];
  PLV_HD double &operator[](int i) { return v[i]; }
  PLV_HD double operator[](int i) const { return v[i]; }
};
struct M3 {  // row-major
  double m[9];
  PLV_HD double &operator()(int r, int c) { return m[3 * r + c]; }
  PLV_HD double operator()(int r, int c) const { return m[3 * r + c]; }
};
struct Q4 {  // JPL: x y z w
  double q[4];
  PLV_HD double &operator[](int i) { return q[i]; }
  PLV_HD double operator[](int i) const { return q[i]; }
};

PLV_HD inline M3 ldM(const double *p) {
  M3 m;
#pragma unroll
  for (int i = 0; i < 9; ++i) m.m[i] = p[i];
  return m;
}
PLV_HD inline V3 ldV(const double *p) { return V3{{p[0], p[1], p[2]}}; }
PLV_HD inline Q4 ldQ(const double *p) { return Q4{{p[0], p[1], p[2], p[3]}}; }
PLV_HD inline void stV(double *p, const V3 &a) { p[0] = a[0], p[1] = a[1], p[2] = a[2]; }

PLV_HD inline M3 eye3() { return M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
PLV_HD inline M3 mm(const M3 &a, const M3 &b) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c(i, j) = a(i, 0) * b(0, j) + a(i, 1) * b(1, j) + a(i, 2) * b(2, j);
  return c;
}
PLV_HD inline M3 tp(const M3 &a) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c(i, j) = a(j, i);
  return c;
}
PLV_HD inline V3 mv(const M3 &a, const V3 &x) {
  return V3{{a(0, 0) * x[0] + a(0, 1) * x[1] + a(0, 2) * x[2], a(1, 0) * x[0] + a(1, 1) * x[1] + a(1, 2) * x[2],
             a(2, 0) * x[0] + a(2, 1) * x[1] + a(2, 2) * x[2]}};
}
PLV_HD inline M3 ms(const M3 &a, double s) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 9; ++i) c.m[i] = a.m[i] * s;
  return c;
}
PLV_HD inline M3 ma(const M3 &a, const M3 &b) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 9; ++i) c.m[i] = a.m[i] + b.m[i];
  return c;
}
PLV_HD inline M3 msb(const M3 &a, const M3 &b) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 9; ++i) c.m[i] = a.m[i] - b.m[i];
  return c;
}
PLV_HD inline V3 vsub(const V3 &a, const V3 &b) { return V3{{a[0] - b[0], a[1] - b[1], a[2] - b[2]}}; }
PLV_HD inline V3 vadd(const V3 &a, const V3 &b) { return V3{{a[0] + b[0], a[1] + b[1], a[2] + b[2]}}; }
PLV_HD inline V3 vsc(const V3 &a, double s) { return V3{{a[0] * s, a[1] * s, a[2] * s}}; }
PLV_HD inline double vnorm(const V3 &a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
PLV_HD inline V3 cross3(const V3 &a, const V3 &b) {
  return V3{{a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}};
}
PLV_HD inline double dot3(const V3 &a, const V3 &b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PLV_HD inline M3 skew3(const V3 &w) { return M3{{0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0}}; }
PLV_HD inline M3 outer3(const V3 &a, const V3 &b) {
  return M3{{a[0] * b[0], a[0] * b[1], a[0] * b[2], a[1] * b[0], a[1] * b[1], a[1] * b[2], a[2] * b[0], a[2] * b[1], a[2] * b[2]}};
}
PLV_HD inline M3 inv3(const M3 &a) {  // cofactors over the determinant; a singular matrix gives non-finite entries
  double c00 = a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1), c01 = a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2),
         c02 = a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0);
  double det = a(0, 0) * c00 + a(0, 1) * c01 + a(0, 2) * c02;
  double id = 1.0 / det;
  M3 r;
  r(0, 0) = c00 * id;
  r(0, 1) = (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) * id;
  r(0, 2) = (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) * id;
  r(1, 0) = c01 * id;
  r(1, 1) = (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) * id;
  r(1, 2) = (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) * id;
  r(2, 0) = c02 * id;
  r(2, 1) = (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) * id;
  r(2, 2) = (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) * id;
  return r;
}

PLV_HD inline M3 exp_so3(const V3 &w) {  // REF: quat_ops.h:231-251
  const M3 wx = skew3(w);
  const double theta = vnorm(w);
  double A, B;
  if (theta < 1e-7) {
    A = 1;
    B = 0.5;
  } else {
    A = sin(theta) / theta;
    B = (1 - cos(theta)) / (theta * theta);
  }
  if (theta == 0) return eye3();
  return ma(ma(eye3(), ms(wx, A)), ms(mm(wx, wx), B));
}
PLV_HD inline V3 log_so3(const M3 &R) {  // REF: quat_ops.h:273-313
  const double R11 = R(0, 0), R12 = R(0, 1), R13 = R(0, 2), R21 = R(1, 0), R22 = R(1, 1), R23 = R(1, 2), R31 = R(2, 0),
               R32 = R(2, 1), R33 = R(2, 2);
  const double trc = R11 + R22 + R33;
  const double PI = 3.14159265358979323846;
  if (trc + 1.0 < 1e-10) {
    if (fabs(R33 + 1.0) > 1e-5) return vsc(V3{{R13, R23, 1.0 + R33}}, PI / sqrt(2.0 + 2.0 * R33));
    if (fabs(R22 + 1.0) > 1e-5) return vsc(V3{{R12, 1.0 + R22, R32}}, PI / sqrt(2.0 + 2.0 * R22));
    return vsc(V3{{1.0 + R11, R21, R31}}, PI / sqrt(2.0 + 2.0 * R11));
  }
  double magnitude;
  const double tr_3 = trc - 3.0;
  if (tr_3 < -1e-7) {
    const double theta = acos((trc - 1.0) / 2.0);
    magnitude = theta / (2.0 * sin(theta));
  } else {
    magnitude = 0.5 - tr_3 / 12.0;
  }
  return vsc(V3{{R32 - R23, R13 - R31, R21 - R12}}, magnitude);
}
PLV_HD inline M3 Jl_so3(const V3 &w) {  // REF: quat_ops.h:515-526
  const double theta = vnorm(w);
  if (theta < 1e-6) return eye3();
  const V3 a = vsc(w, 1.0 / theta);
  M3 aat;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) aat(i, j) = a[i] * a[j];
  return ma(ma(ms(eye3(), sin(theta) / theta), ms(aat, 1 - sin(theta) / theta)), ms(skew3(a), (1 - cos(theta)) / theta));
}
// exp_so3(w) and Jl_so3(w) for the same w with ONE sin / cos evaluation (the transcendental calls are the long poles of the
// per-observation chain); every other operation is the one of the two functions above, so the results are bit-identical.
PLV_HD inline void exp_and_Jl(const V3 &w, M3 &Rexp, M3 &J) {
  const M3 wx = skew3(w);
  const double theta = vnorm(w);
  const double st = sin(theta), ct = cos(theta);
  double A, B;
  if (theta < 1e-7) {
    A = 1;
    B = 0.5;
  } else {
    A = st / theta;
    B = (1 - ct) / (theta * theta);
  }
  Rexp = theta == 0 ? eye3() : ma(ma(eye3(), ms(wx, A)), ms(mm(wx, wx), B));
  if (theta < 1e-6) {
    J = eye3();
    return;
  }
  const V3 a = vsc(w, 1.0 / theta);
  M3 aat;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) aat(i, j) = a[i] * a[j];
  J = ma(ma(ms(eye3(), st / theta), ms(aat, 1 - st / theta)), ms(skew3(a), (1 - ct) / theta));
}

// (2 w^2 - 1) I - 2 w [q x] + 2 q q^T, formed as that matrix expression (jpl_left_update writes the entries out).
PLV_HD inline M3 quat_2_Rot(const Q4 &q) {  // REF: quat_ops.h:152-157
  const V3 v{{q[0], q[1], q[2]}};
  return ma(msb(ms(eye3(), 2 * q[3] * q[3] - 1), ms(skew3(v), 2 * q[3])), ms(outer3(v, v), 2.0));
}
PLV_HD inline Q4 quatnorm(Q4 q) {  // REF: quat_ops.h:496-501
  if (q[3] < 0) q = Q4{{-q[0], -q[1], -q[2], -q[3]}};
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  return Q4{{q[0] / n, q[1] / n, q[2] / n, q[3] / n}};
}
PLV_HD inline Q4 rot_2_quat(const M3 &R) {  // REF: quat_ops.h:88-130
  const double T = R(0, 0) + R(1, 1) + R(2, 2);
  Q4 q;
  if (R(0, 0) >= T && R(0, 0) >= R(1, 1) && R(0, 0) >= R(2, 2)) {
    q[0] = sqrt((1 + (2 * R(0, 0)) - T) / 4);
    q[1] = (1 / (4 * q[0])) * (R(0, 1) + R(1, 0));
    q[2] = (1 / (4 * q[0])) * (R(0, 2) + R(2, 0));
    q[3] = (1 / (4 * q[0])) * (R(1, 2) - R(2, 1));
  } else if (R(1, 1) >= T && R(1, 1) >= R(0, 0) && R(1, 1) >= R(2, 2)) {
    q[1] = sqrt((1 + (2 * R(1, 1)) - T) / 4);
    q[0] = (1 / (4 * q[1])) * (R(0, 1) + R(1, 0));
    q[2] = (1 / (4 * q[1])) * (R(1, 2) + R(2, 1));
    q[3] = (1 / (4 * q[1])) * (R(2, 0) - R(0, 2));
  } else if (R(2, 2) >= T && R(2, 2) >= R(0, 0) && R(2, 2) >= R(1, 1)) {
    q[2] = sqrt((1 + (2 * R(2, 2)) - T) / 4);
    q[0] = (1 / (4 * q[2])) * (R(0, 2) + R(2, 0));
    q[1] = (1 / (4 * q[2])) * (R(1, 2) + R(2, 1));
    q[3] = (1 / (4 * q[2])) * (R(0, 1) - R(1, 0));
  } else {
    q[3] = sqrt((1 + T) / 4);
    q[0] = (1 / (4 * q[3])) * (R(1, 2) - R(2, 1));
    q[1] = (1 / (4 * q[3])) * (R(2, 0) - R(0, 2));
    q[2] = (1 / (4 * q[3])) * (R(0, 1) - R(1, 0));
  }
  return quatnorm(q);
}
PLV_HD inline Q4 quat_multiply(const Q4 &q, const Q4 &p) {  // REF: quat_ops.h:180-195 (the code's L matrix: q4 I - [q x])
  Q4 r;
  r[0] = q[3] * p[0] + q[2] * p[1] - q[1] * p[2] + q[0] * p[3];
  r[1] = -q[2] * p[0] + q[3] * p[1] + q[0] * p[2] + q[1] * p[3];
  r[2] = q[1] * p[0] - q[0] * p[1] + q[3] * p[2] + q[2] * p[3];
  r[3] = -q[0] * p[0] - q[1] * p[1] - q[2] * p[2] + q[3] * p[3];
  return quatnorm(r);
}
PLV_HD inline Q4 omega_times(const V3 &w, const Q4 &q) {  // Omega(w) * q   REF: quat_ops.h:482-489
  return Q4{{-(-w[2] * q[1] + w[1] * q[2]) + w[0] * q[3], -(w[2] * q[0] - w[0] * q[2]) + w[1] * q[3], -(-w[1] * q[0] + w[0] * q[1]) + w[2] * q[3],
             -w[0] * q[0] - w[1] * q[1] - w[2] * q[2]}};
}
PLV_HD inline Q4 qaxpy(const Q4 &a, double s, const Q4 &b) { return Q4{{a[0] + s * b[0], a[1] + s * b[1], a[2] + s * b[2], a[3] + s * b[3]}}; }

// ov_type::JPLQuat::update (REF: open_vins/ov_core/src/types/JPLQuat.h:62-73, quat_ops.h:152-157, 232-252):
// q = quatnorm([dth / 2, 1]) (x) Q, w >= 0, renormalised; Qout (nullable, may be Q) receives q and R its rotation matrix, row-major
// (R is not optional: a null test on a pointer into LDS does not fold away in a kernel).  Host and device apply a correction through
// this one function, + - * / sqrt only: the state a chained launch forms on the device is bit for bit the one the host forms from
// the same dx.  The rotation is written out entry by entry, as this update always formed it; quat_2_Rot's matrix expression differs
// from it in the sign of a zero entry (q = (0, -0.6, 0, -0.8): entry (0, 1) is -0 here, +0 there).  Always inlined, with the entries
// in this body: the fused line launch then compiles to the instructions it had when the function lived beside it.
PLV_HD inline __attribute__((always_inline)) void jpl_left_update(const double *Q, const double *dth, double *Qout, double *R) {
  double a[3] = {0.5 * dth[0], 0.5 * dth[1], 0.5 * dth[2]}, b = 1.0;
  const double nd = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + 1.0);
  a[0] /= nd, a[1] /= nd, a[2] /= nd, b /= nd;
  const double v[3] = {Q[0], Q[1], Q[2]}, w0 = Q[3];
  double r[4];
  r[0] = b * v[0] - (a[1] * v[2] - a[2] * v[1]) + a[0] * w0;
  r[1] = b * v[1] - (a[2] * v[0] - a[0] * v[2]) + a[1] * w0;
  r[2] = b * v[2] - (a[0] * v[1] - a[1] * v[0]) + a[2] * w0;
  r[3] = -(a[0] * v[0] + a[1] * v[1] + a[2] * v[2]) + b * w0;
  if (r[3] < 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = -r[i];
  }
  const double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
  double q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = r[i] / nr;
  if (Qout) {
#pragma unroll
    for (int i = 0; i < 4; ++i) Qout[i] = q[i];
  }
  const double x = q[0], y = q[1], z = q[2], w = q[3], c = 2 * w * w - 1;
  R[0] = c + 2 * x * x, R[1] = 2 * w * z + 2 * x * y, R[2] = -2 * w * y + 2 * x * z;
  R[3] = -2 * w * z + 2 * y * x, R[4] = c + 2 * y * y, R[5] = 2 * w * x + 2 * y * z;
  R[6] = 2 * w * y + 2 * z * x, R[7] = -2 * w * x + 2 * z * y, R[8] = c + 2 * z * z;
}

}  // namespace plv
