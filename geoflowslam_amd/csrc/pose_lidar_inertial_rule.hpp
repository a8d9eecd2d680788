// The rule of Optimizer::PoseLidarVisualInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:6285-6760,
// 7173-7678), the pose step that ends Tracking::TrackLocalMap for IMU_RGBD with point-cloud observations (src/Tracking.cc:3763-3798),
// stated once for the device (pose_lidar_inertial.hip) and the host (tests/host/pose_lidar_inertial_restatement.cpp); DESIGN.md
// section 27.  The two functions are PoseInertialOptimizationLastKeyFrame / ...LastFrame with a block of point-to-plane edges
// (EdgeLidarPoint2Plane, include/G2oTypes.h:602-633) added to every round: the graph, the Gauss-Newton schedule, the
// re-classification, the recovery pass and the written rules N / E / L / S are pose_inertial_rule.hpp's, used unchanged.  This file
// holds what is new.
//
// Quirks kept (each is the reference's behaviour, not a choice):
//   * THE 0.1 SHIFT.  initPose of round 0 is Converter::toMatrix4d(pFrame->GetPose().inverse()) from the stored Sophus::SE3f; in mode
//     kFrame only, (0.1, 0.1, 0.1) is added to its translation in double (:7428).  Later rounds carry no shift.
//   * A ROUND WITHOUT LIDAR EDGES still optimises and classifies: there is no `continue` here, unlike PoseLidarVisualOptimization.
//   * chi2IMU IS READ AT THE TOP of a round, in BOTH modes (:6537, :7445): the inertial edge's stale error vector (zeros before the
//     first optimize) under the information as the earlier rounds left it.  Above 15: Huber 2 and information * 1e-2, compounding.
//     After the last round nothing reads it: the returned Hessian has the information the last round ran with.
//   * abs(pFrame->mTimeStamp - pKF->mTimeStamp > 0.8) (:6549) is the abs of a bool: the information is 1e2 * 1e2 when the SIGNED gap
//     exceeds 0.8, in mode kKeyFrame only.
//   * chi2Lidar is a float to which the doubles edge->chi2() are added one by one in cloud-index order, then divided by the edge count
//     as a float; valid_edge counts chi2 < 4.0.  nInliersLidar and residual are written after every round, also when they are 0.
//   * THE NUMERIC JACOBIAN.  linearizeOplus is commented out, so g2o differentiates numerically (core/base_unary_edge.hpp:82-123):
//     twelve ImuCamPose::Update by +-1e-9, scaled by 1 / (2e-9).  push() / pop() save `its` with the estimate: a perturbed pose has
//     its + 1 and goes through NormalizeRotation (rule N) exactly when the base state's `its` is 2.  The twelve perturbed poses are
//     the same for every edge of an iteration.
//   * THE ERROR goes through g2o::SE3Quat(Rcw, tcw).inverse(): the matrix is turned into a quaternion (Eigen's conversion, then
//     SE3Quat::normalizeRotation), conjugated, and the point is rotated by the quaternion.
//   * THE VISUAL EDGES' KERNEL is dropped after round 2 in mode kKeyFrame and after round n_rounds - 2 in mode kFrame (:7523): with
//     three rounds after round 1, with one round never (size_t it against int nIterations - 2 = -1).
//   * optimizer.edges().size() < 10 counts the round's lidar edges; the test sits before removeEdge and the last round removes
//     nothing, so the lidar edges of the last ENTERED round add J' Omega J to the pose block of the returned Hessian, re-linearised
//     numerically at the final estimate under information(), after the visual inliers.
//   * SOPHUS_ENSURE's abort on a matrix of non-positive determinant is not modelled.
//
// Sum order.  Lidar edges are inserted after every other edge and re-inserted each round: in the pose block and in b they come last --
// visual edges in index order, inertial, gyro walk, acc walk, the prior in mode kFrame, then the lidar edges in cloud-index order.
//
// The next initPose is the float Sophus chain (Thirdparty/Sophus/sophus/so3.hpp, se3.hpp), line by line:
//   Twb = SE3f(Rwb.cast<float>(), twb.cast<float>())   SO3(Matrix): Eigen's matrix-to-quaternion conversion in float, NOT normalised
//   Tbw = Twb.inverse()                                SO3(conjugate): normalised by the quaternion constructor; t = q' * (t * -1)
//   Tcw = mTcb * Tbw                                   the quaternion product written out in so3.hpp:334-338, then normalised by the
//                                                      same constructor (this Sophus has no squared-norm branch); t = t1 + q1 * t2
//   initPose = toMatrix4d(Tcw.inverse())               lidar_assoc.hpp's init_pose_f, restated here for host and device
// Float reductions (Quaternionf::norm) are added left to right, as DESIGN.md section 9 pinned them.
#pragma once
#include "pose_inertial_rule.hpp"

// The edge's functions are called a dozen times an edge with the point and the plane in private arrays: inlined on the device, so that
// those arrays stay in registers
#if defined(__HIPCC__)
#define GFS_PLI_EDGE __host__ __device__ __forceinline__
#else
#define GFS_PLI_EDGE inline
#endif

namespace gfs_pli {

using namespace gfs_pi;

constexpr int kMinCloud = 50;              // GenerateLidarEdge: mpPointCloudDownsampled->size() < 50 -> no edges
constexpr double kLidarInfo = 1e2;         // information(0, 0) = 1e2
constexpr double kLidarInfoFar = 1e2;      // setInformation(information * 1e2)
constexpr double kKfTimeGap = 0.8;         // pFrame->mTimeStamp - pKF->mTimeStamp > 0.8
constexpr double kLidarValidChi2 = 4.0;    // edge->chi2() < 4.0
constexpr double kInitShift = 0.1;         // initPose.block<3, 1>(0, 3) += Vector3d(0.1, 0.1, 0.1)
constexpr double kNumericDelta = 1e-9;     // core/base_unary_edge.hpp: const double delta = 1e-9
constexpr int kKernelDropRoundKeyFrame = 2;   // if (it == 2) e->setRobustKernel(0)
constexpr int kKernelDropFromEndFrame = 2;    // if (it == nIterations - 2) e->setRobustKernel(0)

GFS_HD double huber_delta_lidar() { return (double)(float)sqrt(1.0); }  // const float thHuberLidar = sqrt(1.0)
GFS_HD double lidar_information(int mode, double kf_time_gap) {
  double info = kLidarInfo;
  if (mode == kKeyFrame && kf_time_gap > kKfTimeGap) info = info * kLidarInfoFar;
  return info;
}
GFS_HD bool drops_visual_kernel(int mode, int it, int n_rounds) {
  return mode == kFrame ? (n_rounds >= kKernelDropFromEndFrame && it == n_rounds - kKernelDropFromEndFrame) : it == kKernelDropRoundKeyFrame;
}
GFS_HD int edge_count_with_lidar(int mode, int n_obs, int n_lidar) { return edge_count(mode, n_obs) + n_lidar; }

// ------------------------------------------------------------------------------------------------ Sophus::SE3f (float)
GFS_HD void so3f_normalize(float* q) {  // SO3::normalize: coeffs() /= norm(), the squared norm left to right
  float s = q[0] * q[0];
  s = s + q[1] * q[1];
  s = s + q[2] * q[2];
  s = s + q[3] * q[3];
  const float len = sqrtf(s);
  for (int i = 0; i < 4; i++) q[i] /= len;
}
GFS_HD void so3f_act(const float* q, const float* p, float* o) {  // SO3::operator*(point): uv = q.vec x p; uv += uv; p + w uv + q.vec x uv
  float uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int i = 0; i < 3; i++) uv[i] += uv[i];
  const float cr[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) o[i] = (p[i] + q[3] * uv[i]) + cr[i];
}
GFS_HD void so3f_product(const float* a, const float* b, float* q) {  // so3.hpp:334-338, then SO3(quaternion): normalised
  q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
  q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
  q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
  q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
  so3f_normalize(q);
}
GFS_HD void matrix_to_quat_f(const float* m, float* q) {  // Eigen quaternionbase_assign_impl<Matrix3f>: row-major m, q = (x, y, z, w)
  float t = (m[0] + m[4]) + m[8];
  if (t > 0.0f) {
    t = sqrtf(t + 1.0f);
    q[3] = 0.5f * t;
    t = 0.5f / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 0 ? m[0] : m[4])) i = 2;
    if (i == 0) {
      t = sqrtf(((m[0] - m[4]) - m[8]) + 1.0f);
      q[0] = 0.5f * t;
      t = 0.5f / t;
      q[3] = (m[7] - m[5]) * t;
      q[1] = (m[3] + m[1]) * t;
      q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
      t = sqrtf(((m[4] - m[8]) - m[0]) + 1.0f);
      q[1] = 0.5f * t;
      t = 0.5f / t;
      q[3] = (m[2] - m[6]) * t;
      q[2] = (m[7] + m[5]) * t;
      q[0] = (m[1] + m[3]) * t;
    } else {
      t = sqrtf(((m[8] - m[0]) - m[4]) + 1.0f);
      q[2] = 0.5f * t;
      t = 0.5f / t;
      q[3] = (m[3] - m[1]) * t;
      q[0] = (m[2] + m[6]) * t;
      q[1] = (m[5] + m[7]) * t;
    }
  }
}
// Converter::toMatrix4d(SE3f(q, t).inverse()): row-major 3 x 4 (the text of lidar_assoc.hpp's init_pose_f)
GFS_HD void init_pose_from(const float* q, const float* t, double* M) {
  float qi[4] = {-q[0], -q[1], -q[2], q[3]};
  so3f_normalize(qi);
  const float p[3] = {t[0] * -1.0f, t[1] * -1.0f, t[2] * -1.0f};
  float ti[3];
  so3f_act(qi, p, ti);
  const float x = qi[0], y = qi[1], z = qi[2], w = qi[3];
  const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const float R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * r + c] = (double)R[3 * r + c];
    M[4 * r + 3] = (double)ti[r];
  }
}
// initPose of round 0
GFS_HD void first_init_pose(int mode, const float* q, const float* t, double* M) {
  init_pose_from(q, t, M);
  if (mode == kFrame)
    for (int r = 0; r < 3; r++) M[4 * r + 3] += kInitShift;
}
// initPose after a round, from VP's estimate and the stored mTcb (its float quaternion and translation)
GFS_HD void next_init_pose(const double* Rwb, const double* twb, const float* tcb_q, const float* tcb_t, double* M) {
  float Rf[9], tf[3], q[4];
  for (int i = 0; i < 9; i++) Rf[i] = (float)Rwb[i];
  for (int i = 0; i < 3; i++) tf[i] = (float)twb[i];
  matrix_to_quat_f(Rf, q);  // Twb
  float qi[4] = {-q[0], -q[1], -q[2], q[3]};  // Tbw
  so3f_normalize(qi);
  const float nt[3] = {tf[0] * -1.0f, tf[1] * -1.0f, tf[2] * -1.0f};
  float tbw[3];
  so3f_act(qi, nt, tbw);
  float qc[4], rt[3], tcw[3];  // Tcw = mTcb * Tbw
  so3f_product(tcb_q, qi, qc);
  so3f_act(tcb_q, tbw, rt);
  for (int i = 0; i < 3; i++) tcw[i] = tcb_t[i] + rt[i];
  init_pose_from(qc, tcw, M);
}

// ------------------------------------------------------------------------------------------------ the edge (double)
GFS_HD void matrix_to_quat(const double* m, double* q) {  // Eigen::Quaterniond(R), as g2o_se3_dev.hpp's R_to_quat
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
GFS_PLI_EDGE void quat_rotate(const double* q, const double* v, double* o) {  // Eigen _transformVector
  const double ux = 2 * (q[1] * v[2] - q[2] * v[1]), uy = 2 * (q[2] * v[0] - q[0] * v[2]), uz = 2 * (q[0] * v[1] - q[1] * v[0]);
  o[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
  o[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
  o[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
// Twc = g2o::SE3Quat(Rcw, tcw).inverse() as (q', t') in W[7]: Quaterniond(R), normalizeRotation, conjugate, q' * (t * -1.)
GFS_HD void lidar_inverse_pose(const double* Rcw, const double* tcw, double* W) {
  double q[4];
  matrix_to_quat(Rcw, q);
  if (q[3] < 0)
    for (int i = 0; i < 4; i++) q[i] *= -1;
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= n;
  W[0] = -q[0], W[1] = -q[1], W[2] = -q[2], W[3] = q[3];
  const double nt[3] = {tcw[0] * -1., tcw[1] * -1., tcw[2] * -1.};
  quat_rotate(W, nt, W + 4);
}
// computeError: scale * (Twc.map(point_camera) . plane.head<3>() + plane(3)); the point, the plane and the scale are floats widened
GFS_PLI_EDGE double lidar_error(const double* W, const float* p, const float* plane, float s) {
  const double pc[3] = {(double)p[0], (double)p[1], (double)p[2]};
  double pw[3];
  quat_rotate(W, pc, pw);
  pw[0] += W[4];
  pw[1] += W[5];
  pw[2] += W[6];
  const double dot = pw[0] * (double)plane[0] + pw[1] * (double)plane[1] + pw[2] * (double)plane[2];
  return (double)s * (dot + (double)plane[3]);
}
GFS_PLI_EDGE double lidar_chi2(double e, double info) { return e * (info * e); }  // BaseEdge::chi2 of a 1 x 1 edge

// Perturbed pose k of an iteration's numeric Jacobian, inverted: k = 2 d for +delta along axis d, 2 d + 1 for -delta.  The copy
// carries `its`, as push() saves it
constexpr int kPerturbed = 12;
GFS_HD void perturbed_inverse_pose(const State& base, const Calib& cam, int k, double* W) {
  State s = base;
  constexpr double d = kNumericDelta;
  // (a table in constant memory: an update vector built per lane would live in the device's scratch memory)
  static constexpr double kUpdates[kPerturbed][6] = {{d, 0, 0, 0, 0, 0}, {-d, 0, 0, 0, 0, 0}, {0, d, 0, 0, 0, 0}, {0, -d, 0, 0, 0, 0},
                                                     {0, 0, d, 0, 0, 0}, {0, 0, -d, 0, 0, 0}, {0, 0, 0, d, 0, 0}, {0, 0, 0, -d, 0, 0},
                                                     {0, 0, 0, 0, d, 0}, {0, 0, 0, 0, -d, 0}, {0, 0, 0, 0, 0, d}, {0, 0, 0, 0, 0, -d}};
  pose_update(s, cam, kUpdates[k]);
  lidar_inverse_pose(s.Rcw, s.tcw, W);
}
// Wp: the twelve inverted perturbed poses, [12][7]
GFS_PLI_EDGE void lidar_jacobian(const double* Wp, const float* p, const float* plane, float s, double (&J)[6]) {
  GFS_PI_UNROLL
  for (int d = 0; d < 6; d++)
    J[d] = (1.0 / (2 * kNumericDelta)) * (lidar_error(Wp + 7 * (2 * d), p, plane, s) - lidar_error(Wp + 7 * (2 * d + 1), p, plane, s));
}
// constructQuadraticForm of the 1 x 1 unary edge under its Huber kernel: the packed lower triangle, then -rho1 J' Omega e
GFS_PLI_EDGE void lidar_quadratic_form(const double (&J)[6], double info, double e, double (&acc)[kSys]) {
  double rho0, rho1;
  gfs_pi::huber(lidar_chi2(e, info), huber_delta_lidar(), &rho0, &rho1);
  int o = 0;
  GFS_PI_UNROLL
  for (int a = 0; a < 6; a++) {
    acc[21 + a] = -(((rho1 * J[a]) * info) * e);
    GFS_PI_UNROLL
    for (int c = 0; c <= a; c++) acc[o++] = (J[a] * (rho1 * info)) * J[c];
  }
}
GFS_PLI_EDGE double lidar_hessian_entry(const double (&J)[6], double info, int a, int c) { return (J[a] * info) * J[c]; }  // GetHessian()

// Top of a round: chi2IMU (:6537-6543, :7445-7451), both modes.  Returns the float the reference reads
GFS_HD float inertial_before_round(Persist& P) {
  const float chi2IMU = (float)edge_chi2<9>(P.err_i, P.info_i);
  if (chi2IMU > kChi2ImuGate) {
    P.delta_i = kHuberInertialWeak;
    for (int i = 0; i < 81; i++) P.info_i[i] = P.info_i[i] * kInfoDown;
  }
  return chi2IMU;
}

}  // namespace gfs_pli
