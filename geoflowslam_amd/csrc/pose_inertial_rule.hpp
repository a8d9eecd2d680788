// The rule of Optimizer::PoseInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:5899-6283, 6762-7171), the IMU
// pose step that ends Tracking::TrackLocalMap (src/Tracking.cc:3763-3798), stated once for the device (pose_inertial.hip) and the host
// (tests/host/pose_inertial_restatement.cpp); DESIGN.md section 25.  The two functions are one graph with two settings:
//
//   vertices   VP 0 (ImuCamPose, 6), VV 1, VG 2, VA 3 of the current frame; 4..7 the same of the other end of the inertial edge: the
//              last key frame, FIXED (mode kKeyFrame, 15 unknowns), or the previous frame, free (mode kFrame, 30 unknowns).  The
//              unknowns of the dense system are in vertex-id order: VP 0-5, VV 6-8, VG 9-11, VA 12-14, then 15-29 the same of 4..7.
//   edges      in insertion order, which is the order every sum below follows: the visual edges in index order
//              (EdgeMonoOnlyPose / EdgeStereoOnlyPose, Huber sqrt(5.991) / sqrt(7.815) as floats), EdgeInertial (Huber 6),
//              EdgeGyroRW, EdgeAccRW (no kernel), and in mode kFrame EdgePriorPoseImu (Huber 5).
//   schedule   n_rounds <= 4 rounds of initializeOptimization(0) + optimize(10) with OptimizationAlgorithmGaussNewton over
//              LinearSolverDense: computeActiveErrors, buildSystem, LDLT solve, update -- no gain ratio, no lambda; then the
//              re-classification of the visual edges against the round's gates, the recovery pass, the Hessian of the new prior.
//
// Quirks kept (each is the reference's behaviour, not a choice):
//   * STALE CHI2.  optimize() ends on an update and (not verbose) computes no errors after it: the error vectors that the
//     re-classification and chi2IMU read are those of the state BEFORE the round's last update (sparse_optimizer.cpp:376-414).  An edge
//     that was an outlier gets a fresh computeError() first (:6148-6150), so it alone is judged at the state after the update.
//     isDepthPositive() always reads the current state.  chi2() itself is e' (Omega e) at the time of the call: for the inertial edge
//     that is the stale error under the information as the earlier rounds left it.
//   * A FAILED SOLVE.  LinearSolverDense::solve leaves x untouched when the LDLT is not positive, OptimizationAlgorithmGaussNewton
//     applies x all the same and returns Fail, and optimize() stops the round there (sparse_optimizer.cpp:376,389).  x is the
//     solver's buffer: it holds the last successful solution of this call, from an earlier round too; before the first success the
//     reference reads memory it never wrote (solver.cpp:54, release build) -- stated here as zeros.  The rounds go on.
//   * optimizer.edges().size() < 10 counts ALL edges, those at level 1 too: n_obs + 3, or n_obs + 4 with the prior.
//   * In mode kKeyFrame chi2IMU > 15 gives the inertial edge a new Huber delta 2 and information *= 1e-2, compounding over rounds.
//   * The recovery pass compares the double chi2 with 18.f / 24.f and never sets an outlier flag; nInliers is the last round's.
//   * ConstraintPoseImu computes (H + H) / 2, not a symmetrisation: that is the adaptor's concern, H is returned as summed.
//
// Written rules stand where the reference's arithmetic comes from a library this project does not build against (Eigen, Sophus) or from
// the host's libm; device and host run the same text, built with -ffp-contract=off:
//   rule N   nearest rotation, for Eigen::JacobiSVD in NormalizeRotation (U V'): three Newton steps of the polar iteration
//            X <- (X + X^-T) / 2 in double, the inverse transpose by cofactors over the determinant.  The float NormalizeRotation
//            (src/ImuTypes.cc:35-39) runs the same three steps in double on the float entries and rounds to float once.  The inputs
//            here are rotations up to rounding or up to the O(d^3) of the small-angle branch, for which three steps reach the fixed
//            point.  A singular input divides by a zero determinant: inf / NaN entries, as IEEE 754 gives them.
//   rule E   Sophus::SO3f::exp(v).matrix(): the unit quaternion of v in double (Sophus's own branch at |v|^2 < 1e-10 with its Taylor
//            factors, else sin / cos of |v| / 2 from glibc_math.hpp), its matrix rounded to float once (so3_quat_rule.hpp, shared with
//            rule B of sim3_ransac_rule.hpp).
//   rule L   acos in LogSO3: acos_rule below, the rational approximation of Sun's fdlibm e_acos.c, plain double operations only
//            (tests/test_pose_inertial_restatement.py measures its distance to the host libm's acos).
//   sin/cos  in double: gfs_glibc::sin / cos where they restate glibc (|x| < 2.4); beyond, the argument is first reduced by the
//            nearest multiple of pi held in two doubles (sin_rule / cos_rule), so that no device libm is ever asked.
//   rule S   Eigen's fixed-size products and sums: the inner sum left to right, a chain A * B * C as (A * B) * C, sums of matrices
//            coefficient by coefficient left to right, as DESIGN.md section 9 pinned it.  The dynamic-size products of
//            BaseMultiEdge::computeQuadraticForm follow the same rule.
//
// Sums over the visual edges: a term of an edge that is skipped (level 1, an outlier) is added as +0.0, which changes no sum that
// is not -0.0; the restatement adds the same +0.0.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "glibc_math.hpp"
#include "so3_quat_rule.hpp"

// Small fixed-count loops over private arrays are unrolled on the device, where an array indexed at run time lives in scratch memory
#if defined(__HIPCC__)
#define GFS_PI_UNROLL _Pragma("unroll")
#else
#define GFS_PI_UNROLL
#endif

namespace gfs_pi {

constexpr int kKeyFrame = 0, kFrame = 1;  // GFS_POSE_INERTIAL_LAST_KEYFRAME / _LAST_FRAME
constexpr int kIterations = 10;           // its[4] = {10, 10, 10, 10}
constexpr int kMaxRounds = 4;
constexpr int kMinEdges = 10;             // optimizer.edges().size() < 10
constexpr int kFewInliers = 30;           // nInliers < 30 && !bRecInit
constexpr double kHuberInertial = 6.0, kHuberInertialWeak = 2.0, kHuberPrior = 5.0;
constexpr double kChi2ImuGate = 15.0, kInfoDown = 1e-2;
constexpr float kChi2MonoOut = 18.f, kChi2StereoOut = 24.f;
constexpr double kSmallAngle = 1e-5;  // ExpSO3, InverseRightJacobianSO3, RightJacobianSO3: d < 1e-5; LogSO3: fabs(s) < 1e-5
constexpr float kGravity = 9.81f;     // IMU::GRAVITY_VALUE
constexpr float kTrackDepthClose = 10.f;  // bClose = mTrackDepth < 10.f: the caller's `close` flag
constexpr int kNormalizeEvery = 3;    // ImuCamPose::Update: its >= 3

// chi2Mono[it] / chi2Stereo[it] (:6112-6113, :6993-6994) as the floats the arrays hold
GFS_HD float chi2_mono_gate(int mode, int it) {
  if (mode == kFrame) return 5.991f;
  return it == 0 ? 12.f : it == 1 ? 7.5f : 5.991f;
}
GFS_HD float chi2_stereo_gate(int it) { return it == 0 ? 15.6f : it == 1 ? 9.8f : 7.815f; }
GFS_HD float chi2_close_gate(int mode, int it) { return (float)(1.5 * (double)chi2_mono_gate(mode, it)); }  // float chi2close = 1.5 * chi2Mono[it]
GFS_HD double huber_delta_visual(bool stereo) { return stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991); }
// dbg = Eigen::Vector3f(1e-6, 1e-6, 1e-5) when the gyro bias difference is not finite (src/ImuTypes.cc:293-295)
GFS_HD float dbg_replacement(int k) { return k == 2 ? (float)1e-5 : (float)1e-6; }

struct Calib {  // the part of ImuCamPose that never changes; matrices row-major
  double fx, fy, cx, cy, bf;
  double Rcb[9], tcb[3], Rbc[9], tbc[3];
};
struct State {  // ImuCamPose's moving part and the three additive vertices of one end
  double Rwb[9], twb[3], Rcw[9], tcw[3];
  double v[3], bg[3], ba[3];
  int its, pad;
};
struct Preint {  // IMU::Preintegrated as the edges read it
  float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], bg[3], ba[3], dT;
};
struct Prior {  // ConstraintPoseImu
  double Rwb[9], twb[3], v[3], bg[3], ba[3], H[225];
};
struct Head {  // one problem without its visual edges
  int mode, n_obs, n_rounds, rec_init;
  Calib cam;
  State cur, oth;
  Preint pre;
  double info_i[81], info_g[9], info_a[9];
  Prior prior;
};

// ------------------------------------------------------------------------------------------------ small matrices (rule S)
GFS_HD void mul33(const double* A, const double* B, double* C) {  // C = A B
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
GFS_HD void mulT33(const double* A, const double* B, double* C) {  // C = A' B
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
GFS_HD void mul33T(const double* A, const double* B, double* C) {  // C = A B'
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[3 * r + c] = (A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1]) + A[3 * r + 2] * B[3 * c + 2];
}
GFS_HD void mv3(const double* A, const double* v, double* o) {  // o = A v
  for (int r = 0; r < 3; r++) o[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}
GFS_HD void mTv3(const double* A, const double* v, double* o) {  // o = A' v
  for (int r = 0; r < 3; r++) o[r] = (A[r] * v[0] + A[3 + r] * v[1]) + A[6 + r] * v[2];
}
GFS_HD void hat3(const double* v, double* W) {
  W[0] = 0.0, W[1] = -v[2], W[2] = v[1];
  W[3] = v[2], W[4] = 0.0, W[5] = -v[0];
  W[6] = -v[1], W[7] = v[0], W[8] = 0.0;
}
GFS_HD void huber(double e, double delta, double* rho0, double* rho1) {  // core/robust_kernel_impl.cpp:78-91
  const double dsqr = delta * delta;
  if (e <= dsqr) {
    *rho0 = e;
    *rho1 = 1.0;
  } else {
    const double sq = sqrt(e);
    *rho0 = 2 * sq * delta - dsqr;
    *rho1 = delta / sq;
  }
}

// ------------------------------------------------------------------------------------------------ sin / cos beyond glibc_math's range
constexpr double kPiHi = 0x1.921fb54442d18p+1, kPiLo = 0x1.1a62633145c07p-53, kInvPi = 0x1.45f306dc9c883p-2;
GFS_HD double reduce_pi(double x, bool* odd) {  // x - k pi, k the nearest integer to x / pi
  const double k = rint(x * kInvPi), half = k * 0.5;
  *odd = half != rint(half);
  return (x - k * kPiHi) - k * kPiLo;
}
GFS_HD double sin_rule(double x) {
  if (fabs(x) < 2.4) return gfs_glibc::sin(x);
  bool odd;
  const double r = reduce_pi(x, &odd);
  if (!(fabs(r) < 2.4)) return r - r;  // inf, NaN: NaN
  const double s = gfs_glibc::sin(r);
  return odd ? -s : s;
}
GFS_HD double cos_rule(double x) {
  if (fabs(x) < 2.4) return gfs_glibc::cos(x);
  bool odd;
  const double r = reduce_pi(x, &odd);
  if (!(fabs(r) < 2.4)) return r - r;
  const double c = gfs_glibc::cos(r);
  return odd ? -c : c;
}

// ------------------------------------------------------------------------------------------------ rule L
GFS_HD double acos_poly(double z) {
  const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
               qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
  const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
  return p / q;
}
GFS_HD double acos_rule(double x) {  // |x| <= 1 (LogSO3 returns before the call otherwise); NaN in, NaN out
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
  const double ax = fabs(x);
  if (!(ax < 1.0)) {
    if (x == 1.0) return 0.0;
    if (x == -1.0) return 2 * pio2_hi;
    return (x - x) / (x - x);
  }
  if (ax < 0.5) {
    if (ax < 0x1p-57) return pio2_hi;
    return pio2_hi - (x - (pio2_lo - x * acos_poly(x * x)));
  }
  if (x < 0) {
    const double z = (1.0 + x) * 0.5, s = sqrt(z), w = acos_poly(z) * s - pio2_lo;
    return 2 * (pio2_hi - (s + w));
  }
  const double z = (1.0 - x) * 0.5, s = sqrt(z);
  const double df = gfs_glibc::as_f64(gfs_glibc::as_u64(s) & 0xffffffff00000000ull);
  const double c = (z - df * df) / (s + df), w = acos_poly(z) * s + c;
  return 2 * (df + w);
}

// ------------------------------------------------------------------------------------------------ rule N
GFS_HD void polar_step(double* X) {
  const double C[9] = {X[4] * X[8] - X[5] * X[7], X[5] * X[6] - X[3] * X[8], X[3] * X[7] - X[4] * X[6],
                       X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                       X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};
  const double det = (X[0] * C[0] + X[1] * C[1]) + X[2] * C[2];
  for (int i = 0; i < 9; i++) X[i] = 0.5 * (X[i] + C[i] / det);
}
GFS_HD void nearest_rotation(double* R) {
  polar_step(R);
  polar_step(R);
  polar_step(R);
}
GFS_HD void nearest_rotation_f(float* R) {
  double X[9];
  for (int i = 0; i < 9; i++) X[i] = (double)R[i];
  nearest_rotation(X);
  for (int i = 0; i < 9; i++) R[i] = (float)X[i];
}

// ------------------------------------------------------------------------------------------------ rule E
GFS_HD void exp_so3f(const float* v, float* R) {
  const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
  const double t2 = (x * x + y * y) + z * z;
  double im, re;
  if (t2 < 1e-10) {
    const double t4 = t2 * t2;
    im = (0.5 - t2 / 48.0) + t4 / 3840.0;
    re = (1.0 - t2 / 8.0) + t4 / 384.0;
  } else {
    const double t = sqrt(t2), h = 0.5 * t;
    im = sin_rule(h) / t;
    re = cos_rule(h);
  }
  const double q[4] = {re, im * x, im * y, im * z};
  gfs_so3::quaternion_matrix(q, R);
}

// ------------------------------------------------------------------------------------------------ SO(3) in double (src/G2oTypes.cc:1007-1076)
GFS_HD void exp_so3(const double* w, double* R) {
  const double x = w[0], y = w[1], z = w[2];
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  double W[9], WW[9];
  hat3(w, W);
  if (d < kSmallAngle) {  // I + W + 0.5 * W * W: (0.5 W) W
    double hW[9];
    for (int i = 0; i < 9; i++) hW[i] = 0.5 * W[i];
    mul33(hW, W, WW);
    for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + W[i]) + WW[i];
  } else {  // I + W * sin(d) / d + W * W * (1.0 - cos(d)) / d2
    const double s = sin_rule(d), c1 = 1.0 - cos_rule(d);
    mul33(W, W, WW);
    for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + (W[i] * s) / d) + (WW[i] * c1) / d2;
  }
  nearest_rotation(R);
}
GFS_HD void log_so3(const double* R, double* w) {
  const double tr = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2, w[1] = (R[2] - R[6]) / 2, w[2] = (R[3] - R[1]) / 2;
  const double costheta = (tr - 1.0) * 0.5;
  if (costheta > 1 || costheta < -1) return;
  const double theta = acos_rule(costheta), s = sin_rule(theta);
  if (fabs(s) < kSmallAngle) return;
  for (int k = 0; k < 3; k++) w[k] = (theta * w[k]) / s;
}
GFS_HD void inverse_right_jacobian(const double* v, double* J) {
  const double x = v[0], y = v[1], z = v[2];
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  if (d < kSmallAngle) {
    for (int i = 0; i < 9; i++) J[i] = i % 4 == 0 ? 1.0 : 0.0;
    return;
  }
  double W[9], WW[9];
  hat3(v, W);
  mul33(W, W, WW);
  const double k = 1.0 / d2 - (1.0 + cos_rule(d)) / (2.0 * d * sin_rule(d));
  for (int i = 0; i < 9; i++) J[i] = ((i % 4 == 0 ? 1.0 : 0.0) + W[i] / 2) + WW[i] * k;
}
GFS_HD void right_jacobian(const double* v, double* J) {
  const double x = v[0], y = v[1], z = v[2];
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  if (d < kSmallAngle) {
    for (int i = 0; i < 9; i++) J[i] = i % 4 == 0 ? 1.0 : 0.0;
    return;
  }
  double W[9], WW[9];
  hat3(v, W);
  mul33(W, W, WW);
  const double a = 1.0 - cos_rule(d), b = d - sin_rule(d), d3 = d2 * d;
  for (int i = 0; i < 9; i++) J[i] = ((i % 4 == 0 ? 1.0 : 0.0) - (W[i] * a) / d2) + (WW[i] * b) / d3;
}

// ------------------------------------------------------------------------------------------------ vertex updates
// ImuCamPose::Update (src/G2oTypes.cc:193-217); the counter `its` lives in the state and survives the rounds
GFS_HD void pose_update(State& s, const Calib& c, const double* pu) {
  double d[3], E[9], R[9];
  mv3(s.Rwb, pu + 3, d);
  for (int k = 0; k < 3; k++) s.twb[k] += d[k];
  exp_so3(pu, E);
  mul33(s.Rwb, E, R);
  for (int i = 0; i < 9; i++) s.Rwb[i] = R[i];
  s.its++;
  if (s.its >= kNormalizeEvery) {
    nearest_rotation(s.Rwb);
    s.its = 0;
  }
  double nRbw[9], Rbw[9], tbw[3];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) {
      Rbw[3 * r + k] = s.Rwb[3 * k + r];
      nRbw[3 * r + k] = -s.Rwb[3 * k + r];
    }
  mv3(nRbw, s.twb, tbw);  // tbw = -Rbw * twb: the negated matrix times the vector
  mul33(c.Rcb, Rbw, s.Rcw);
  mv3(c.Rcb, tbw, d);
  for (int k = 0; k < 3; k++) s.tcw[k] = d[k] + c.tcb[k];
}
GFS_HD void add3(double* v, const double* u) {  // VertexVelocity / VertexGyroBias / VertexAccBias::oplusImpl
  for (int k = 0; k < 3; k++) v[k] += u[k];
}

// ------------------------------------------------------------------------------------------------ visual edges
// EdgeMonoOnlyPose / EdgeStereoOnlyPose::computeError through ImuCamPose::Project / ProjectStereo (double 1 / z)
GFS_HD void vis_error(const Calib& c, const double* Rcw, const double* tcw, const double* xw, const double* obs, bool stereo, double* e) {
  double X[3];
  mv3(Rcw, xw, X);
  for (int k = 0; k < 3; k++) X[k] += tcw[k];
  const double u = c.fx * X[0] / X[2] + c.cx, v = c.fy * X[1] / X[2] + c.cy;
  e[0] = obs[0] - u;
  e[1] = obs[1] - v;
  if (stereo) {
    const double invZ = 1 / X[2];
    e[2] = obs[2] - (u - c.bf * invZ);
  } else {
    e[2] = 0.0;
  }
}
GFS_HD double vis_chi2(const double* e, double w, bool stereo) {  // e . (Omega e), Omega = w I
  const double s = e[0] * (w * e[0]) + e[1] * (w * e[1]);
  return stereo ? s + e[2] * (w * e[2]) : s;
}
GFS_HD bool vis_depth_positive(const double* Rcw, const double* tcw, const double* xw) {  // ImuCamPose::isDepthPositive
  return ((Rcw[6] * xw[0] + Rcw[7] * xw[1]) + Rcw[8] * xw[2]) + tcw[2] > 0.0;
}
// linearizeOplus: proj_jac * Rcb * SE3deriv(Xb), Xb = Rbc Xc + tbc.  J row-major 3 x 6, the third row zero for a mono edge
GFS_HD void vis_jacobian(const Calib& c, const double* Rcw, const double* tcw, const double* xw, bool stereo, double (&J)[18]) {
  double X[3], Xb[3];
  mv3(Rcw, xw, X);
  for (int k = 0; k < 3; k++) X[k] += tcw[k];
  mv3(c.Rbc, X, Xb);
  for (int k = 0; k < 3; k++) Xb[k] += c.tbc[k];
  double P[9];  // Pinhole::projectJac, and for stereo the third row = the first with (2, 2) += bf / z^2
  P[0] = c.fx / X[2], P[1] = 0.0, P[2] = -c.fx * X[0] / (X[2] * X[2]);
  P[3] = 0.0, P[4] = c.fy / X[2], P[5] = -c.fy * X[1] / (X[2] * X[2]);
  const double inv_z2 = 1.0 / (X[2] * X[2]);
  P[6] = P[0], P[7] = P[1], P[8] = P[2] + c.bf * inv_z2;
  double M[9];
  mul33(P, c.Rcb, M);
  const double x = Xb[0], y = Xb[1], z = Xb[2];
  const double D[18] = {0.0, z, -y, 1.0, 0.0, 0.0, -z, 0.0, x, 0.0, 1.0, 0.0, y, -x, 0.0, 0.0, 0.0, 1.0};
  GFS_PI_UNROLL
  for (int r = 0; r < 3; r++)
    GFS_PI_UNROLL
    for (int k = 0; k < 6; k++) J[6 * r + k] = (r == 2 && !stereo) ? 0.0 : (M[3 * r] * D[k] + M[3 * r + 1] * D[6 + k]) + M[3 * r + 2] * D[12 + k];
}
// constructQuadraticForm of a unary edge (core/base_unary_edge.hpp:43-72) with Omega = w I: the 21 entries of the lower triangle of
// A' (rho1 Omega) A, packed a (a + 1) / 2 + c, then the 6 of -rho1 A' Omega e.  rho1 = 1 without the kernel: the same bits
constexpr int kSys = 27;
GFS_HD void vis_quadratic_form(const double (&J)[18], double w, bool stereo, double rho1, const double* e, double (&acc)[kSys]) {
  int o = 0;
  GFS_PI_UNROLL
  for (int a = 0; a < 6; a++) {
    double sb = 0;
    sb += ((rho1 * J[a]) * w) * e[0];
    sb += ((rho1 * J[6 + a]) * w) * e[1];
    const double sb3 = sb + ((rho1 * J[12 + a]) * w) * e[2];
    sb = stereo ? sb3 : sb;
    acc[21 + a] = -sb;
    GFS_PI_UNROLL
    for (int cc = 0; cc <= a; cc++) {
      double hh = 0;
      hh += (J[a] * (rho1 * w)) * J[cc];
      hh += (J[6 + a] * (rho1 * w)) * J[6 + cc];
      const double hh3 = hh + (J[12 + a] * (rho1 * w)) * J[12 + cc];
      acc[o++] = stereo ? hh3 : hh;
    }
  }
}
// GetHessian(): (J' Omega) J, all 36 entries (row a, column c at 6 a + c): the two triangles are rounded apart
GFS_HD double vis_hessian_entry(const double (&J)[18], double w, bool stereo, int a, int cc) {
  double hh = 0;
  hh += (J[a] * w) * J[cc];
  hh += (J[6 + a] * w) * J[6 + cc];
  const double hh3 = hh + (J[12 + a] * w) * J[12 + cc];
  return stereo ? hh3 : hh;
}
// The re-classification tests (:6155-6156, :6182): chi2 as a float against the round's gates
GFS_HD bool mono_is_outlier(float chi2, bool close, bool depth_positive, int mode, int it) {
  return (chi2 > chi2_mono_gate(mode, it) && !close) || (close && chi2 > chi2_close_gate(mode, it)) || !depth_positive;
}
GFS_HD bool stereo_is_outlier(float chi2, int it) { return chi2 > chi2_stereo_gate(it); }

// ------------------------------------------------------------------------------------------------ the small edges
// An edge with a dense Jacobian J (E x D, row-major, the columns in the order of the edge's vertices), as BaseMultiEdge /
// BaseBinaryEdge::constructQuadraticForm treat it: Om is the information the products use (rho1 Omega under a kernel), wr the
// weighted error -rho1 Omega e, AtO = J' Om.
template <int E_, int D_>
struct SmallEdge {
  static constexpr int E = E_, D = D_;
  double err[E_], Om[E_ * E_], wr[E_], J[E_ * D_], AtO[D_ * E_];
};
typedef SmallEdge<9, 24> InertialEdge;   // VPk 0-5, VVk 6-8, VGk 9-11, VAk 12-14, VP 15-20, VV 21-23
typedef SmallEdge<3, 6> RandomWalkEdge;  // the other end 0-2, the current frame 3-5
typedef SmallEdge<15, 15> PriorEdge;     // VPk 0-5, VVk 6-8, VGk 9-11, VAk 12-14

template <int E>
GFS_HD double edge_chi2(const double* e, const double* info) {  // BaseEdge::chi2: e . (Omega e)
  double s = 0;
  for (int r = 0; r < E; r++) {
    double oe = 0;
    for (int k = 0; k < E; k++) oe += info[E * r + k] * e[k];
    s += e[r] * oe;
  }
  return s;
}
// Om and wr for buildSystem.  delta > 0: under a Huber kernel of that width; delta == 0: no kernel
template <class Edge>
GFS_HD void edge_weights(Edge& ed, const double* info, double delta) {
  constexpr int E = Edge::E;
  double rho1 = 1.0;
  if (delta > 0) {
    double rho0;
    huber(edge_chi2<E>(ed.err, info), delta, &rho0, &rho1);
  }
  for (int r = 0; r < E; r++) {
    double oe = 0;
    for (int k = 0; k < E; k++) oe += info[E * r + k] * ed.err[k];
    ed.wr[r] = delta > 0 ? (-oe) * rho1 : -oe;
    for (int k = 0; k < E; k++) ed.Om[E * r + k] = delta > 0 ? rho1 * info[E * r + k] : info[E * r + k];
  }
}
template <class Edge>
GFS_HD void edge_plain_information(Edge& ed, const double* info) {  // Om = information(), for GetHessian*
  for (int i = 0; i < Edge::E * Edge::E; i++) ed.Om[i] = info[i];
}
template <class Edge>
GFS_HD void edge_AtO_entry(Edge& ed, int idx) {  // entry idx = r * E + k of AtO = J' Om
  constexpr int E = Edge::E, D = Edge::D;
  const int r = idx / E, k = idx % E;
  double s = 0;
  for (int m = 0; m < E; m++) s += ed.J[D * m + r] * ed.Om[E * m + k];
  ed.AtO[idx] = s;
}
template <class Edge>
GFS_HD double edge_H(const Edge& ed, int p, int q) {  // (AtO J)(p, q)
  constexpr int E = Edge::E, D = Edge::D;
  double s = 0;
  for (int k = 0; k < E; k++) s += ed.AtO[E * p + k] * ed.J[D * k + q];
  return s;
}
template <class Edge>
GFS_HD double edge_b(const Edge& ed, int r) {  // (J' wr)(r)
  constexpr int E = Edge::E, D = Edge::D;
  double s = 0;
  for (int m = 0; m < E; m++) s += ed.J[D * m + r] * ed.wr[m];
  return s;
}
// The Hessian block between two vertices of an edge is computed once, AtO_i A_j for i < j in the edge's vertex order, and the
// dense matrix holds it and its transpose; a vertex's own block is AtO_i A_i as it stands.  vertex_of: the vertex of a column
GFS_HD int inertial_vertex(int l) { return l < 6 ? 0 : l < 9 ? 1 : l < 12 ? 2 : l < 15 ? 3 : l < 21 ? 4 : 5; }
GFS_HD int rw_vertex(int l) { return l < 3 ? 0 : 1; }
GFS_HD int prior_vertex(int l) { return l < 6 ? 0 : l < 9 ? 1 : l < 12 ? 2 : 3; }
template <class Edge>
GFS_HD double edge_H_system(const Edge& ed, int p, int q, int vp, int vq) {
  if (vp == vq || p < q) return edge_H(ed, p, q);
  return edge_H(ed, q, p);
}
// The column of an edge that holds unknown g of the dense system, or -1
GFS_HD int inertial_column(int mode, int g) { return g < 9 ? 15 + g : (g >= 15 && mode == kFrame) ? g - 15 : -1; }
GFS_HD int gyro_column(int mode, int g) { return (g >= 9 && g < 12) ? g - 6 : (g >= 24 && g < 27 && mode == kFrame) ? g - 24 : -1; }
GFS_HD int acc_column(int mode, int g) { return (g >= 12 && g < 15) ? g - 9 : (g >= 27 && mode == kFrame) ? g - 27 : -1; }
GFS_HD int prior_column(int mode, int g) { return (g >= 15 && mode == kFrame) ? g - 15 : -1; }

// Bias-corrected deltas in float, as Preintegrated::GetDeltaRotation / Velocity / Position(b1) (src/ImuTypes.cc:289-313), then cast
GFS_HD void mv3f(const float* A, const float* v, float* o) {
  for (int r = 0; r < 3; r++) o[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}
GFS_HD void preint_deltas(const Preint& p, const double* bg, const double* ba, double* dR, double* dV, double* dP, double* dbg_d) {
  float dbg[3], dba[3], dbr[3];
  bool finite = true;
  for (int k = 0; k < 3; k++) {  // IMU::Bias holds floats
    dbg[k] = (float)bg[k] - p.bg[k];
    dba[k] = (float)ba[k] - p.ba[k];
    finite = finite && (dbg[k] - dbg[k] == 0.0f);
    dbg_d[k] = (double)dbg[k];  // GetDeltaBias for linearizeOplus: no replacement there
  }
  for (int k = 0; k < 3; k++) dbr[k] = finite ? dbg[k] : dbg_replacement(k);
  float v[3], Ex[9], M[9];
  mv3f(p.JRg, dbr, v);
  exp_so3f(v, Ex);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) M[3 * r + c] = (p.dR[3 * r] * Ex[c] + p.dR[3 * r + 1] * Ex[3 + c]) + p.dR[3 * r + 2] * Ex[6 + c];
  nearest_rotation_f(M);
  for (int i = 0; i < 9; i++) dR[i] = (double)M[i];
  float a[3], b[3];
  mv3f(p.JVg, dbg, a);
  mv3f(p.JVa, dba, b);
  for (int k = 0; k < 3; k++) dV[k] = (double)((p.dV[k] + a[k]) + b[k]);
  mv3f(p.JPg, dbg, a);
  mv3f(p.JPa, dba, b);
  for (int k = 0; k < 3; k++) dP[k] = (double)((p.dP[k] + a[k]) + b[k]);
}
GFS_HD void put_block(double* J, int D, int r0, int c0, const double* B, double scale_sign) {  // J(r0.., c0..) = sign * B
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) J[D * (r0 + r) + c0 + c] = scale_sign < 0 ? -B[3 * r + c] : B[3 * r + c];
}
// EdgeInertial::computeError + linearizeOplus (src/G2oTypes.cc:495-719).  s1: the other end (vertices 0-3), s2: the current frame
GFS_HD void inertial_linearize(const Preint& pre, const State& s1, const State& s2, InertialEdge& ed) {
  constexpr int D = 24;
  double dR[9], dV[3], dP[3], dbg[3];
  preint_deltas(pre, s1.bg, s1.ba, dR, dV, dP, dbg);
  const double dt = (double)pre.dT;
  const double g[3] = {0.0, 0.0, (double)(-kGravity)};
  double Rbw1[9], nRbw1[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Rbw1[3 * r + c] = s1.Rwb[3 * c + r], nRbw1[3 * r + c] = -s1.Rwb[3 * c + r];
  double T[9], eR[9], er[3];
  mulT33(dR, Rbw1, T);
  mul33(T, s2.Rwb, eR);
  log_so3(eR, er);
  double tv[3], tp[3], tp2[3], rv[3], rp[3], rp2[3];
  for (int k = 0; k < 3; k++) {
    tv[k] = (s2.v[k] - s1.v[k]) - g[k] * dt;
    tp[k] = ((s2.twb[k] - s1.twb[k]) - s1.v[k] * dt) - ((g[k] * dt) * dt) / 2;    // computeError: g * dt * dt / 2
    tp2[k] = ((s2.twb[k] - s1.twb[k]) - s1.v[k] * dt) - ((0.5 * g[k]) * dt) * dt;  // linearizeOplus: 0.5 * g * dt * dt
  }
  mv3(Rbw1, tv, rv);
  mv3(Rbw1, tp, rp);
  mv3(Rbw1, tp2, rp2);
  for (int k = 0; k < 3; k++) {
    ed.err[k] = er[k];
    ed.err[3 + k] = rv[k] - dV[k];
    ed.err[6 + k] = rp[k] - dP[k];
  }
  for (int i = 0; i < 9 * D; i++) ed.J[i] = 0.0;
  double invJr[9], nInvJr[9], A[9], B[9], W[9];
  inverse_right_jacobian(er, invJr);
  for (int i = 0; i < 9; i++) nInvJr[i] = -invJr[i];
  // pose 1
  mul33T(nInvJr, s2.Rwb, A);
  mul33(A, s1.Rwb, B);
  put_block(ed.J, D, 0, 0, B, 1);
  hat3(rv, W);
  put_block(ed.J, D, 3, 0, W, 1);
  hat3(rp2, W);
  put_block(ed.J, D, 6, 0, W, 1);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) ed.J[D * (6 + r) + 3 + c] = r == c ? -1.0 : -0.0;  // -Identity
  // velocity 1
  put_block(ed.J, D, 3, 6, nRbw1, 1);
  for (int i = 0; i < 9; i++) A[i] = nRbw1[i] * dt;
  put_block(ed.J, D, 6, 6, A, 1);
  // gyro bias 1: -invJr * eR' * RightJacobianSO3(JRg * dbg) * JRg
  double JRg[9], Md[9], jd[3], RJ[9];
  for (int i = 0; i < 9; i++) JRg[i] = (double)pre.JRg[i];
  mv3(JRg, dbg, jd);
  right_jacobian(jd, RJ);
  mul33T(nInvJr, eR, A);
  mul33(A, RJ, B);
  mul33(B, JRg, A);
  put_block(ed.J, D, 0, 9, A, 1);
  for (int i = 0; i < 9; i++) Md[i] = (double)pre.JVg[i];
  put_block(ed.J, D, 3, 9, Md, -1);
  for (int i = 0; i < 9; i++) Md[i] = (double)pre.JPg[i];
  put_block(ed.J, D, 6, 9, Md, -1);
  // accelerometer bias 1
  for (int i = 0; i < 9; i++) Md[i] = (double)pre.JVa[i];
  put_block(ed.J, D, 3, 12, Md, -1);
  for (int i = 0; i < 9; i++) Md[i] = (double)pre.JPa[i];
  put_block(ed.J, D, 6, 12, Md, -1);
  // pose 2
  put_block(ed.J, D, 0, 15, invJr, 1);
  mul33(Rbw1, s2.Rwb, A);
  put_block(ed.J, D, 6, 18, A, 1);
  // velocity 2
  put_block(ed.J, D, 3, 21, Rbw1, 1);
}
// EdgeGyroRW / EdgeAccRW: e = b2 - b1, J = [-I, I]
GFS_HD void random_walk_linearize(const double* b1, const double* b2, RandomWalkEdge& ed) {
  for (int k = 0; k < 3; k++) ed.err[k] = b2[k] - b1[k];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      ed.J[6 * r + c] = r == c ? -1.0 : -0.0;
      ed.J[6 * r + 3 + c] = r == c ? 1.0 : 0.0;
    }
}
// EdgePriorPoseImu::computeError + linearizeOplus (:945-985) at the other end's state
GFS_HD void prior_linearize(const Prior& c, const State& s, PriorEdge& ed) {
  constexpr int D = 15;
  double RtR[9], er[3], d[3], et[3], invJr[9];
  mulT33(c.Rwb, s.Rwb, RtR);
  log_so3(RtR, er);
  for (int k = 0; k < 3; k++) d[k] = s.twb[k] - c.twb[k];
  mTv3(c.Rwb, d, et);
  for (int k = 0; k < 3; k++) {
    ed.err[k] = er[k];
    ed.err[3 + k] = et[k];
    ed.err[6 + k] = s.v[k] - c.v[k];
    ed.err[9 + k] = s.bg[k] - c.bg[k];
    ed.err[12 + k] = s.ba[k] - c.ba[k];
  }
  for (int i = 0; i < 15 * D; i++) ed.J[i] = 0.0;
  inverse_right_jacobian(er, invJr);
  put_block(ed.J, D, 0, 0, invJr, 1);
  put_block(ed.J, D, 3, 3, RtR, 1);
  for (int k = 0; k < 9; k++) ed.J[D * (6 + k) + 6 + k] = 1.0;
}

// ------------------------------------------------------------------------------------------------ the dense system
// Everything that lives across the Gauss-Newton iterations of a call besides the visual edges
struct Persist {
  State s[2];           // [0] the current frame, [1] the other end
  double info_i[81];    // the inertial edge's information as the rounds leave it
  double delta_i;       // and its Huber width
  double err_i[9];      // its error vector as the last computeActiveErrors left it
  double x[30];         // the solver's x
  double vis[kSys];     // the ordered sums over the visual edges of one buildSystem
  int D, ok, pad[2];
};
struct Work {  // one linearisation: the small edges, the dense matrix (row-major, stride 30, lower triangle read), b, the LDLT's state
  InertialEdge ei;
  RandomWalkEdge gr, ar;
  PriorEdge ep;
  double A[900], b[30], y[30], temp[30];
  int tr[30], sign, positive;
};
GFS_HD void persist_init(const Head& h, Persist& P) {
  P.s[0] = h.cur;
  P.s[1] = h.oth;
  P.s[0].its = P.s[1].its = 0;
  for (int i = 0; i < 81; i++) P.info_i[i] = h.info_i[i];
  P.delta_i = kHuberInertial;
  for (int i = 0; i < 9; i++) P.err_i[i] = 0.0;
  for (int i = 0; i < 30; i++) P.x[i] = 0.0;
  for (int i = 0; i < kSys; i++) P.vis[i] = 0.0;
  P.D = h.mode == kFrame ? 30 : 15;
  P.ok = 1;
}
// computeError + linearizeOplus of small edge `which` (0 inertial, 1 gyro walk, 2 acc walk, 3 prior) and, with `build`, its weights
// for buildSystem; without, Om = information() for GetHessian*.  One lane each on the device
GFS_HD void small_edge_linearize(const Head& h, Persist& P, Work& W, int which, bool build) {
  if (which == 0) {
    inertial_linearize(h.pre, P.s[1], P.s[0], W.ei);
    if (build) {
      for (int k = 0; k < 9; k++) P.err_i[k] = W.ei.err[k];
      edge_weights(W.ei, P.info_i, P.delta_i);
    } else {
      edge_plain_information(W.ei, P.info_i);
    }
  } else if (which == 1) {
    random_walk_linearize(P.s[1].bg, P.s[0].bg, W.gr);
    if (build) edge_weights(W.gr, h.info_g, 0.0);
    else edge_plain_information(W.gr, h.info_g);
  } else if (which == 2) {
    random_walk_linearize(P.s[1].ba, P.s[0].ba, W.ar);
    if (build) edge_weights(W.ar, h.info_a, 0.0);
    else edge_plain_information(W.ar, h.info_a);
  } else if (h.mode == kFrame) {
    prior_linearize(h.prior, P.s[1], W.ep);
    if (build) edge_weights(W.ep, h.prior.H, kHuberPrior);
    else edge_plain_information(W.ep, h.prior.H);
  }
}
constexpr int kAtOInertial = 24 * 9, kAtOWalk = 6 * 3, kAtOPrior = 15 * 15;
constexpr int kAtOEntries = kAtOInertial + 2 * kAtOWalk + kAtOPrior;  // entries of all four AtO, one index space
GFS_HD void small_edge_AtO_entry(int mode, Work& W, int idx) {
  if (idx < kAtOInertial) return edge_AtO_entry(W.ei, idx);
  idx -= kAtOInertial;
  if (idx < kAtOWalk) return edge_AtO_entry(W.gr, idx);
  idx -= kAtOWalk;
  if (idx < kAtOWalk) return edge_AtO_entry(W.ar, idx);
  idx -= kAtOWalk;
  if (mode == kFrame) edge_AtO_entry(W.ep, idx);
}
// Entry (R, C), R >= C, of the system matrix: the visual sum, then the small edges in insertion order
GFS_HD double system_entry(int mode, const Persist& P, const Work& W, int R, int C) {
  double v = (R < 6 && C < 6) ? P.vis[R * (R + 1) / 2 + C] : 0.0;
  int p = inertial_column(mode, R), q = inertial_column(mode, C);
  if (p >= 0 && q >= 0) v += edge_H_system(W.ei, p, q, inertial_vertex(p), inertial_vertex(q));
  p = gyro_column(mode, R), q = gyro_column(mode, C);
  if (p >= 0 && q >= 0) v += edge_H_system(W.gr, p, q, rw_vertex(p), rw_vertex(q));
  p = acc_column(mode, R), q = acc_column(mode, C);
  if (p >= 0 && q >= 0) v += edge_H_system(W.ar, p, q, rw_vertex(p), rw_vertex(q));
  p = prior_column(mode, R), q = prior_column(mode, C);
  if (p >= 0 && q >= 0) v += edge_H_system(W.ep, p, q, prior_vertex(p), prior_vertex(q));
  return v;
}
GFS_HD double system_rhs(int mode, const Persist& P, const Work& W, int R) {
  double v = R < 6 ? P.vis[21 + R] : 0.0;
  int p = inertial_column(mode, R);
  if (p >= 0) v += edge_b(W.ei, p);
  p = gyro_column(mode, R);
  if (p >= 0) v += edge_b(W.gr, p);
  p = acc_column(mode, R);
  if (p >= 0) v += edge_b(W.ar, p);
  p = prior_column(mode, R);
  if (p >= 0) v += edge_b(W.ep, p);
  return v;
}

// Eigen::LDLT<MatrixXd>::compute + isPositive + solve (solvers/linear_solver_dense.h:104-112), the 6 x 6 statement of pose_lm_dev.hpp
// at size N in memory: A row-major with stride 30, the lower triangle in place.  The steps are separate functions so that the device
// can give the rows of a step to lanes; every entry is computed by the same text either way.
constexpr int kLd = 30;
GFS_HD void ldlt_pivot(double* A, int N, int k, int* tr, double* temp) {  // pivot search, transposition, temp = D L(k, :)'
  int p = k;
  double best = fabs(A[kLd * k + k]);
  for (int i = k + 1; i < N; i++)
    if (fabs(A[kLd * i + i]) > best) {
      best = fabs(A[kLd * i + i]);
      p = i;
    }
  tr[k] = p;
  if (p != k) {
    for (int j = 0; j < k; j++) {
      const double t = A[kLd * k + j];
      A[kLd * k + j] = A[kLd * p + j];
      A[kLd * p + j] = t;
    }
    for (int i = p + 1; i < N; i++) {
      const double t = A[kLd * i + k];
      A[kLd * i + k] = A[kLd * i + p];
      A[kLd * i + p] = t;
    }
    {
      const double t = A[kLd * k + k];
      A[kLd * k + k] = A[kLd * p + p];
      A[kLd * p + p] = t;
    }
    for (int i = k + 1; i < p; i++) {
      const double t = A[kLd * i + k];
      A[kLd * i + k] = A[kLd * p + i];
      A[kLd * p + i] = t;
    }
  }
  for (int j = 0; j < k; j++) temp[j] = A[kLd * j + j] * A[kLd * k + j];
}
GFS_HD void ldlt_row(double* A, int k, int i, const double* temp) {  // row i >= k of step k: A(i, k) -= A(i, 0..k) . temp
  if (k == 0) return;
  double acc = 0;
  for (int j = 0; j < k; j++) acc += A[kLd * i + j] * temp[j];
  A[kLd * i + k] -= acc;
}
GFS_HD void ldlt_scale(double* A, int k, int i) {  // row i > k: A(i, k) /= A(k, k) unless the pivot is zero
  const double akk = A[kLd * k + k];
  if (fabs(akk) > 0) A[kLd * i + k] /= akk;
}
GFS_HD void ldlt_sign(const double* A, int k, int* sign) {  // 0 zero, 1 positive, -1 negative, 2 indefinite
  const double akk = A[kLd * k + k];
  if (*sign == 1) {
    if (akk < 0) *sign = 2;
  } else if (*sign == -1) {
    if (akk > 0) *sign = 2;
  } else if (*sign == 0) {
    if (akk > 0) *sign = 1;
    else if (akk < 0) *sign = -1;
  }
}
GFS_HD void ldlt_substitute(const double* A, int N, const int* tr, const double* b, double* y, double* x) {
  for (int i = 0; i < N; i++) y[i] = b[i];
  for (int k = 0; k < N; k++) {
    const double t = y[k];
    y[k] = y[tr[k]];
    y[tr[k]] = t;
  }
  for (int i = 0; i < N; i++)
    for (int j = 0; j < i; j++) y[i] -= A[kLd * i + j] * y[j];
  for (int i = 0; i < N; i++) y[i] = fabs(A[kLd * i + i]) > 2.2250738585072014e-308 ? y[i] / A[kLd * i + i] : 0.0;
  for (int i = N - 1; i >= 0; i--)
    for (int j = i + 1; j < N; j++) y[i] -= A[kLd * j + i] * y[j];
  for (int k = N - 1; k >= 0; k--) {
    const double t = y[k];
    y[k] = y[tr[k]];
    y[tr[k]] = t;
  }
  for (int i = 0; i < N; i++) x[i] = y[i];
}
// SparseOptimizer::update: oplus of every vertex.  part 0: VP; 1: the current frame's additive vertices; 2: VPk; 3: the other end's
// additive vertices (parts 2 and 3 only in mode kFrame).  The parts touch disjoint state
GFS_HD void update_part(const Head& h, Persist& P, int part) {
  if (part == 0) {
    pose_update(P.s[0], h.cam, P.x);
  } else if (part == 1) {
    add3(P.s[0].v, P.x + 6);
    add3(P.s[0].bg, P.x + 9);
    add3(P.s[0].ba, P.x + 12);
  } else if (h.mode == kFrame && part == 2) {
    pose_update(P.s[1], h.cam, P.x + 15);
  } else if (h.mode == kFrame && part == 3) {
    add3(P.s[1].v, P.x + 21);
    add3(P.s[1].bg, P.x + 24);
    add3(P.s[1].ba, P.x + 27);
  }
}
// After a round in mode kKeyFrame (:6135-6141): chi2IMU as a float from the stale error under the current information
GFS_HD void inertial_after_round(const Head& h, Persist& P) {
  if (h.mode != kKeyFrame) return;
  const float chi2IMU = (float)edge_chi2<9>(P.err_i, P.info_i);
  if (chi2IMU > kChi2ImuGate) {
    P.delta_i = kHuberInertialWeak;
    for (int i = 0; i < 81; i++) P.info_i[i] = P.info_i[i] * kInfoDown;
  }
}
GFS_HD int edge_count(int mode, int n_obs) { return n_obs + (mode == kFrame ? 4 : 3); }

// Entry (R, C) of the returned Hessian WITHOUT the visual blocks (:6246-6251, :7119-7136): GetHessian2 / GetHessian of the small
// edges, re-linearised at the final state with Om = information(), added in the reference's order.  Mode kKeyFrame: 15 x 15 over
// (VP, VV, VG, VA); mode kFrame: 30 x 30 over (VPk, VVk, VGk, VAk, VP, VV, VG, VA)
GFS_HD double hessian_entry(int mode, const Work& W, int R, int C) {
  double v = 0.0;
  if (mode == kKeyFrame) {
    if (R < 9 && C < 9) v += edge_H(W.ei, 15 + R, 15 + C);
    if (R >= 9 && R < 12 && C >= 9 && C < 12) v += edge_H(W.gr, R - 6, C - 6);
    if (R >= 12 && C >= 12) v += edge_H(W.ar, R - 9, C - 9);
    return v;
  }
  if (R < 24 && C < 24) v += edge_H(W.ei, R, C);
  const int gr = (R >= 9 && R < 12) ? R - 9 : (R >= 24 && R < 27) ? R - 21 : -1, gc = (C >= 9 && C < 12) ? C - 9 : (C >= 24 && C < 27) ? C - 21 : -1;
  if (gr >= 0 && gc >= 0) v += edge_H(W.gr, gr, gc);
  const int ar = (R >= 12 && R < 15) ? R - 12 : R >= 27 ? R - 24 : -1, ac = (C >= 12 && C < 15) ? C - 12 : C >= 27 ? C - 24 : -1;
  if (ar >= 0 && ac >= 0) v += edge_H(W.ar, ar, ac);
  if (R < 15 && C < 15) v += edge_H(W.ep, R, C);
  return v;
}
GFS_HD int hessian_visual_offset(int mode) { return mode == kFrame ? 15 : 0; }  // where the inliers' 6 x 6 blocks go

// A problem of include/gfs_abi.h (any struct with its field names) into the rule's head
template <class Problem>
inline void fill_head(const Problem& p, Head& h) {
  memset(&h, 0, sizeof(h));
  h.mode = p.mode, h.n_obs = p.n_obs, h.n_rounds = p.n_rounds, h.rec_init = p.rec_init;
  h.cam.fx = p.fx, h.cam.fy = p.fy, h.cam.cx = p.cx, h.cam.cy = p.cy, h.cam.bf = p.bf;
  memcpy(h.cam.Rcb, p.Rcb, sizeof(p.Rcb)), memcpy(h.cam.tcb, p.tcb, sizeof(p.tcb));
  memcpy(h.cam.Rbc, p.Rbc, sizeof(p.Rbc)), memcpy(h.cam.tbc, p.tbc, sizeof(p.tbc));
  const auto state = [](const auto& a, State& s) {
    memcpy(s.Rwb, a.Rwb, sizeof(a.Rwb)), memcpy(s.twb, a.twb, sizeof(a.twb)), memcpy(s.Rcw, a.Rcw, sizeof(a.Rcw));
    memcpy(s.tcw, a.tcw, sizeof(a.tcw)), memcpy(s.v, a.v, sizeof(a.v)), memcpy(s.bg, a.bg, sizeof(a.bg)), memcpy(s.ba, a.ba, sizeof(a.ba));
  };
  state(p.cur, h.cur);
  state(p.other, h.oth);
  memcpy(h.pre.dR, p.dR, sizeof(p.dR)), memcpy(h.pre.dV, p.dV, sizeof(p.dV)), memcpy(h.pre.dP, p.dP, sizeof(p.dP));
  memcpy(h.pre.JRg, p.JRg, sizeof(p.JRg)), memcpy(h.pre.JVg, p.JVg, sizeof(p.JVg)), memcpy(h.pre.JVa, p.JVa, sizeof(p.JVa));
  memcpy(h.pre.JPg, p.JPg, sizeof(p.JPg)), memcpy(h.pre.JPa, p.JPa, sizeof(p.JPa));
  memcpy(h.pre.bg, p.preint_bg, sizeof(p.preint_bg)), memcpy(h.pre.ba, p.preint_ba, sizeof(p.preint_ba));
  h.pre.dT = p.dT;
  memcpy(h.info_i, p.info_inertial, sizeof(p.info_inertial)), memcpy(h.info_g, p.info_gyro_rw, sizeof(p.info_gyro_rw));
  memcpy(h.info_a, p.info_acc_rw, sizeof(p.info_acc_rw));
  memcpy(h.prior.Rwb, p.prior_Rwb, sizeof(p.prior_Rwb)), memcpy(h.prior.twb, p.prior_twb, sizeof(p.prior_twb));
  memcpy(h.prior.v, p.prior_vwb, sizeof(p.prior_vwb)), memcpy(h.prior.bg, p.prior_bg, sizeof(p.prior_bg));
  memcpy(h.prior.ba, p.prior_ba, sizeof(p.prior_ba)), memcpy(h.prior.H, p.prior_H, sizeof(p.prior_H));
}

}  // namespace gfs_pi
