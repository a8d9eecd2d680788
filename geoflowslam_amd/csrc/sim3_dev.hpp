// g2o's Sim3 arithmetic, host and device: Thirdparty/g2o/g2o/types/sim3.h:70-272 (exp, log, map, inverse, product),
// types_seven_dof_expmap.h:60-69 (VertexSim3Expmap::oplusImpl) and :106-114 (EdgeSim3::computeError), restated in the operation order of
// the sources with Eigen 3.4's quaternion <-> rotation-matrix conversions.  Double precision like the reference.  What is kept as
// written: the eps = 1e-5 branches on |sigma| and on theta (exp) or d (log); R = I + Omega + Omega^2 on the small-angle branch and
// Quaterniond(R) of that R, which is not orthonormal and never renormalised; W.lu().solve(t) as a 3 x 3 LU with partial pivoting.
// A Sim3 is eight doubles: the quaternion (x, y, z, w), the translation, the scale.
// Plain C++ (tests/host/pose_graph_restatement.cpp compiles it with g++); eg_dev.hpp calls it for the essential-graph kernels and
// host/gfs_adaptors.hpp for the edges' measurements.  The four quaternion helpers repeat g2o_se3_dev.hpp's, which are device-only and
// normalise where Sim3 does not; the bundle adjustments' kernels keep theirs untouched.
#pragma once
#include <cmath>

#include "glibc_math.hpp"

#if defined(__HIPCC__)
#define GFS_SIM3_HD __host__ __device__ inline
#else
#define GFS_SIM3_HD inline
#endif

namespace gfs_sim3 {

constexpr double kEps = 0.00001;        // sim3.h:90 and :165
constexpr double kNumericDelta = 1e-9;  // core/base_binary_edge.hpp:147

// which of the four (sigma, angle) branches an exp or a log took: bit 0 = |sigma| >= eps, bit 1 = the angle is not small
enum { kBranchSigma = 1, kBranchAngle = 2 };

GFS_SIM3_HD void quat_rotate(const double* q, const double* v, double* o) {  // Eigen _transformVector
  const double ux = 2 * (q[1] * v[2] - q[2] * v[1]), uy = 2 * (q[2] * v[0] - q[0] * v[2]), uz = 2 * (q[0] * v[1] - q[1] * v[0]);
  o[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
  o[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
  o[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
GFS_SIM3_HD void quat_mul(const double* a, const double* b, double* q) {  // Eigen quat_product (q may not alias a or b)
  q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
GFS_SIM3_HD void quat_to_R(const double* q, double* R) {  // toRotationMatrix, row-major
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1 - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1 - (txx + tyy);
}
GFS_SIM3_HD void R_to_quat(const double* m, double* q) {  // Quaterniond(R): no normalisation
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 0 ? m[0] : m[4])) i = 2;
    if (i == 0) {
      t = sqrt(m[0] - m[4] - m[8] + 1.0);
      q[0] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[7] - m[5]) * t;
      q[1] = (m[3] + m[1]) * t;
      q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
      t = sqrt(m[4] - m[8] - m[0] + 1.0);
      q[1] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[2] - m[6]) * t;
      q[2] = (m[7] + m[5]) * t;
      q[0] = (m[1] + m[3]) * t;
    } else {
      t = sqrt(m[8] - m[0] - m[4] + 1.0);
      q[2] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[3] - m[1]) * t;
      q[0] = (m[2] + m[6]) * t;
      q[1] = (m[5] + m[7]) * t;
    }
  }
}

// skew(om) and its square, row-major, products summed k ascending
GFS_SIM3_HD void skew_and_square(const double* om, double* O, double* O2) {
  O[0] = 0, O[1] = -om[2], O[2] = om[1];
  O[3] = om[2], O[4] = 0, O[5] = -om[0];
  O[6] = -om[1], O[7] = om[0], O[8] = 0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
}

// the coefficients of W = A Omega + B Omega^2 + C I, shared by exp (angle = theta, small = theta < eps) and log (angle = acos(d),
// small = d > 1 - eps): sim3.h:91-135 and :168-213
GFS_SIM3_HD void w_coefficients(double sigma, double s, double theta, bool small_angle, double* A, double* B, double* C) {
  if (fabs(sigma) < kEps) {
    *C = 1;
    if (small_angle) {
      *A = 1. / 2.;
      *B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      *A = (1 - gfs_glibc::cos(theta)) / (theta2);
      *B = (theta - gfs_glibc::sin(theta)) / (theta2 * theta);
    }
  } else {
    *C = (s - 1) / sigma;
    if (small_angle) {
      const double sigma2 = sigma * sigma;
      *A = ((sigma - 1) * s + 1) / sigma2;
      *B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * gfs_glibc::sin(theta);
      const double b = s * gfs_glibc::cos(theta);
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      *A = (a * sigma + (1 - b) * theta) / (theta * c);
      *B = (*C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
}

// Sim3(const Vector7d& update), sim3.h:70-142, with s = exp(sigma) handed in; returns the branch taken
GFS_SIM3_HD int sim3_exp_given_scale(const double* u, double s, double* S) {
  const double om[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
  const double sigma = u[6];
  const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
  double O[9], O2[9], R[9];
  skew_and_square(om, O, O2);
  const bool small_angle = theta < kEps;
  double A, B, C;
  w_coefficients(sigma, s, theta, small_angle, &A, &B, &C);
  if (small_angle) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i];
  } else {
    const double ca = gfs_glibc::sin(theta) / theta, cb = (1 - gfs_glibc::cos(theta)) / (theta * theta);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ca * O[i] + cb * O2[i];
  }
  R_to_quat(R, S);
  double W[9];
  for (int i = 0; i < 9; i++) W[i] = A * O[i] + B * O2[i] + C * (i % 4 == 0 ? 1.0 : 0.0);
  for (int r = 0; r < 3; r++) S[4 + r] = W[3 * r] * ups[0] + W[3 * r + 1] * ups[1] + W[3 * r + 2] * ups[2];
  S[7] = s;
  return (fabs(sigma) < kEps ? 0 : kBranchSigma) | (small_angle ? 0 : kBranchAngle);
}

// the scale by the library's exp: glibc's on the host, the device library's on the device (the essential-graph kernels)
GFS_SIM3_HD int sim3_exp(const double* u, double* S) { return sim3_exp_given_scale(u, ::exp(u[6]), S); }

// W.lu().solve(t): PartialPivLU of a 3 x 3 (the first largest |entry| of the column is the pivot), then the two column-oriented
// triangular solves
GFS_SIM3_HD void lu_solve3(const double* Win, const double* t, double* x) {
  double a00 = Win[0], a01 = Win[1], a02 = Win[2], a10 = Win[3], a11 = Win[4], a12 = Win[5], a20 = Win[6], a21 = Win[7], a22 = Win[8];
  double c0 = t[0], c1 = t[1], c2 = t[2];
#define GFS_SIM3_SWAP(p, q) { const double t_ = p; p = q; q = t_; }
  int p = 0;
  if (fabs(a10) > fabs(a00)) p = 1;
  if (fabs(a20) > fabs(p == 0 ? a00 : a10)) p = 2;
  if (p == 1) {
    GFS_SIM3_SWAP(a00, a10) GFS_SIM3_SWAP(a01, a11) GFS_SIM3_SWAP(a02, a12) GFS_SIM3_SWAP(c0, c1)
  } else if (p == 2) {
    GFS_SIM3_SWAP(a00, a20) GFS_SIM3_SWAP(a01, a21) GFS_SIM3_SWAP(a02, a22) GFS_SIM3_SWAP(c0, c2)
  }
  a10 /= a00;
  a20 /= a00;
  a11 -= a10 * a01;
  a12 -= a10 * a02;
  a21 -= a20 * a01;
  a22 -= a20 * a02;
  if (fabs(a21) > fabs(a11)) {
    GFS_SIM3_SWAP(a10, a20) GFS_SIM3_SWAP(a11, a21) GFS_SIM3_SWAP(a12, a22) GFS_SIM3_SWAP(c1, c2)
  }
#undef GFS_SIM3_SWAP
  a21 /= a11;
  a22 -= a21 * a12;
  c1 -= c0 * a10;
  c2 -= c0 * a20;
  c2 -= c1 * a21;
  x[2] = c2 / a22;
  c1 -= x[2] * a12;
  c0 -= x[2] * a02;
  x[1] = c1 / a11;
  c0 -= x[1] * a01;
  x[0] = c0 / a00;
}

// Sim3::log, sim3.h:148-230; returns the branch taken
GFS_SIM3_HD int sim3_log(const double* S, double* res) {
  const double s = S[7];
  const double sigma = ::log(s);
  double R[9];
  quat_to_R(S, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR(R), se3_ops.hpp
  const bool small_angle = d > 1 - kEps;
  double theta = 0, k = 0.5;
  if (!small_angle) {
    theta = ::acos(d);
    k = theta / (2 * sqrt(1 - d * d));
  }
  const double om[3] = {k * dR[0], k * dR[1], k * dR[2]};
  double A, B, C;
  w_coefficients(sigma, s, theta, small_angle, &A, &B, &C);
  double O[9], O2[9], W[9];
  skew_and_square(om, O, O2);
  for (int r = 0; r < 3; r++)  // A*Omega + B*Omega*Omega + C*I: the middle term is (B Omega) Omega here (:215), not B Omega^2 (:140)
    for (int c = 0; c < 3; c++) {
      const double boo = (B * O[3 * r]) * O[c] + (B * O[3 * r + 1]) * O[3 + c] + (B * O[3 * r + 2]) * O[6 + c];
      W[3 * r + c] = A * O[3 * r + c] + boo + C * (r == c ? 1.0 : 0.0);
    }
  lu_solve3(W, S + 4, res + 3);
  for (int i = 0; i < 3; i++) res[i] = om[i];
  res[6] = sigma;
  return (fabs(sigma) < kEps ? 0 : kBranchSigma) | (small_angle ? 0 : kBranchAngle);
}

GFS_SIM3_HD void sim3_mul(const double* a, const double* b, double* o) {  // operator*, sim3.h:266-272 (o may not alias a or b)
  double rt[3];
  quat_mul(a, b, o);
  quat_rotate(a, b + 4, rt);
  for (int i = 0; i < 3; i++) o[4 + i] = a[7] * rt[i] + a[4 + i];
  o[7] = a[7] * b[7];
}
GFS_SIM3_HD void sim3_inverse(const double* a, double* o) {  // sim3.h:233-236 (o may not alias a)
  o[0] = -a[0], o[1] = -a[1], o[2] = -a[2], o[3] = a[3];
  const double k = -1. / a[7];
  const double v[3] = {k * a[4], k * a[5], k * a[6]};
  quat_rotate(o, v, o + 4);
  o[7] = 1. / a[7];
}
GFS_SIM3_HD void sim3_map(const double* a, const double* xyz, double* o) {  // sim3.h:144-146
  double r[3];
  quat_rotate(a, xyz, r);
  for (int i = 0; i < 3; i++) o[i] = a[7] * r[i] + a[4 + i];
}
// VertexSim3Expmap::oplusImpl (out may not alias est)
GFS_SIM3_HD void sim3_oplus(const double* est, const double* update, bool fix_scale, double* out) {
  double u[7], e[8];
  for (int i = 0; i < 7; i++) u[i] = update[i];
  if (fix_scale) u[6] = 0;
  sim3_exp(u, e);
  sim3_mul(e, est, out);
}
// the same with glibc's exp restated (glibc_math.hpp): host and device give the same bits also when the scale is free (sim3_opt.hip)
GFS_SIM3_HD void sim3_oplus_glibc_exp(const double* est, const double* update, bool fix_scale, double* out) {
  double u[7], e[8];
  for (int i = 0; i < 7; i++) u[i] = update[i];
  if (fix_scale) u[6] = 0;
  sim3_exp_given_scale(u, gfs_glibc::exp(u[6]), e);
  sim3_mul(e, est, out);
}
// EdgeSim3::computeError: (C v0 v1^-1).log(); returns the log's branch
GFS_SIM3_HD int sim3_edge_residual(const double* C, const double* v0, const double* v1, double* err) {
  double a[8], b[8], c[8];
  sim3_mul(C, v0, a);
  sim3_inverse(v1, b);
  sim3_mul(a, b, c);
  return sim3_log(c, err);
}

}  // namespace gfs_sim3
