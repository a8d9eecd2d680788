// The rule of Sim3Solver (reference src/Sim3Solver.cc), the RANSAC step of LoopClosing::DetectCommonRegionsFromBoW
// (src/LoopClosing.cc:742-759), stated once for the device and the host: the sampling of a minimal set
// (:233-246), ComputeSim3 (:289-392: Horn 1987, closed form from 3 point pairs), CheckInliers / Project (:394-440 with
// Pinhole::project, src/CameraModels/Pinhole.cpp:43-49), the outcome of the sequential loop as a pick over the scores of all
// hypotheses, and SetRansacParameters (:119-143).  float, every operation rounded once, double exactly where the source promotes; the
// translation units that include this are built with -ffp-contract=off.  Three written rules stand where the reference's arithmetic
// depends on a library (Eigen::EigenSolver, Sophus::SO3f::exp, Eigen's fixed-size reductions): rules A, B and C below.  The draws
// of DUtils::Random::RandomInt are an INPUT: the reference takes them from the process-global, never seeded rand().
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#if !defined(GFS_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFS_HD __host__ __device__ inline
#else
#define GFS_HD inline
#endif
#endif

#include "so3_quat_rule.hpp"

namespace gfs_s3r {

constexpr double kChi2 = 9.210;            // mvnMaxError = 9.210 * sigma2 (:95-96)
constexpr double kDefaultProbability = 0.99;  // SetRansacParameters' defaults (include/Sim3Solver.h:40-41)
constexpr int kDefaultMinInliers = 6, kDefaultMaxIterations = 300;
constexpr int kJacobiSweeps = 30;
constexpr double kJacobiEps = 2.220446049250313e-16;  // 2^-52

enum Status { kConverged = 0, kNoMore = 1, kTooFew = 2 };  // GFS_SIM3_RANSAC_* of include/gfs_abi.h

// One hypothesis as ComputeSim3 leaves it: mR12i, mt12i, ms12i and the upper three rows of mT12i = [sR | t], mT21i = [sRinv | tinv]
struct Hyp {
  float R[9], t[3], s;
  float T12[12], T21[12];  // row-major 3 x 4
};

// ---- Sampling (:233-246).  vAvailableIndices starts as 0 .. N-1; draw k takes position r_k of what is left, the back moves into the
// hole and the list shrinks.  Only two holes are ever filled, so the list is not kept: a1 / a2 are the list after one / two draws.
// r0 in [0, N-1], r1 in [0, N-2], r2 in [0, N-3]; N >= 3.
GFS_HD void resolve_draws(int N, int r0, int r1, int r2, int* idx) {
  const int back0 = N - 1;                          // vAvailableIndices.back() at the first draw
  idx[0] = r0;                                      // the list is still the identity
  const int a1_r1 = r1 == r0 ? back0 : r1;          // a1(p) = p == r0 ? N-1 : p   on [0, N-2]
  idx[1] = a1_r1;
  const int back1 = (N - 2) == r0 ? back0 : N - 2;  // a1(N-2): the back at the second draw
  const int a1_r2 = r2 == r0 ? back0 : r2;
  idx[2] = r2 == r1 ? back1 : a1_r2;                // a2(p) = p == r1 ? a1(N-2) : a1(p)   on [0, N-3]
}

GFS_HD bool draws_in_range(int N, int r0, int r1, int r2) {
  return r0 >= 0 && r0 <= N - 1 && r1 >= 0 && r1 <= N - 2 && r2 >= 0 && r2 <= N - 3;
}

// ---- Rule C (for Eigen's fixed-size float reductions: rowwise().sum(), the two .sum() of step 6, the dot of CheckInliers, the inner
// sums of the 3 x 3 products): added left to right in column-major storage order, as DESIGN.md section 9 pinned it.

// ---- Rule A (for Eigen::EigenSolver<Matrix4f>::compute + eigenvalues().real().maxCoeff + the eigenvector's column): the unit
// eigenvector of the largest eigenvalue of the SYMMETRIC float N by cyclic two-sided Jacobi in double: pairs in the fixed order
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most kJacobiSweeps sweeps, a pair is rotated while |a_pq| > kJacobiEps * (|a_pp| + |a_qq|),
// a sweep without a rotation ends it.  The largest diagonal entry wins, the lower column on ties.  Sign: the real part w >= 0; when
// w == 0 the first non-zero imaginary component is positive.  (NaN compares false everywhere: no rotation, column 0, NaN out.)
template <int P, int Q>
GFS_HD bool jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q], app = A[P][P], aqq = A[Q][Q];
  if (!(fabs(apq) > kJacobiEps * (fabs(app) + fabs(aqq)))) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double r = fabs(theta) + sqrt(1.0 + theta * theta);
  const double t = theta < 0.0 ? -1.0 / r : 1.0 / r;
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  A[P][P] = app - t * apq;
  A[Q][Q] = aqq + t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  for (int k = 0; k < 4; k++) {
    if (k != P && k != Q) {
      const double akp = A[k][P], akq = A[k][Q];
      A[k][P] = A[P][k] = c * akp - s * akq;
      A[k][Q] = A[Q][k] = s * akp + c * akq;
    }
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
  return true;
}

GFS_HD void largest_eigenvector(const float (&Nf)[4][4], double* q) {  // q = (w, x, y, z)
  double A[4][4], V[4][4];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      A[r][c] = (double)Nf[r][c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    bool rotated = jacobi_rotate<0, 1>(A, V);
    rotated |= jacobi_rotate<0, 2>(A, V);
    rotated |= jacobi_rotate<0, 3>(A, V);
    rotated |= jacobi_rotate<1, 2>(A, V);
    rotated |= jacobi_rotate<1, 3>(A, V);
    rotated |= jacobi_rotate<2, 3>(A, V);
    if (!rotated) break;
  }
  double best = A[0][0];
  double v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
  for (int c = 1; c < 4; c++)
    if (A[c][c] > best) {
      best = A[c][c];
      for (int k = 0; k < 4; k++) v[k] = V[k][c];
    }
  const double n = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
  const bool flip = v[0] < 0.0 || (v[0] == 0.0 && (v[1] < 0.0 || (v[1] == 0.0 && (v[2] < 0.0 || (v[2] == 0.0 && v[3] < 0.0)))));
  for (int k = 0; k < 4; k++) q[k] = flip ? -(v[k] / n) : v[k] / n;
}

// ---- Rule B (for ang = atan2(|vec|, w); vec = 2 ang vec / |vec|; Sophus::SO3f::exp(vec).matrix(), :339-350): R12 is the rotation
// matrix of the unit quaternion of rule A, computed in double and rounded to float once per entry: the same rotation, more
// accurate in the last bits.  The reference's vec.norm() == 0 branch (the vector of 1e-6) is the quaternion (1, 0, 0, 0): its matrix
// here is the identity exactly, which the formula below gives without a branch.
// (the formula lives in so3_quat_rule.hpp, shared with rule E of pose_inertial_rule.hpp)
using gfs_so3::quaternion_matrix;

// ComputeCentroid (:282-287): C = P.rowwise().sum() (rule C: columns left to right), C / P.cols() (the Index becomes a float: Eigen
// promotes a scalar operand to the expression's scalar type), Pr.col(i) = P.col(i) - C.  P[c] is column c, a point.
GFS_HD void centroid(const float (&P)[3][3], float (&Pr)[3][3], float* C) {
  for (int r = 0; r < 3; r++) C[r] = ((P[0][r] + P[1][r]) + P[2][r]) / 3.0f;
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) Pr[c][r] = P[c][r] - C[r];
}

// ---- ComputeSim3 (:289-392).  P1[c] / P2[c]: the c-th drawn point of set 1 / 2 (the columns of P3Dc1i / P3Dc2i).
GFS_HD void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, Hyp& h) {
  // Step 1: centroids and relative coordinates
  float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
  centroid(P1, Pr1, O1);
  centroid(P2, Pr2, O2);
  // Step 2: M = Pr2 * Pr1^T in float, M(i, j) = sum over the points k, left to right
  float M[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[i][j] = (Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j];
  // Step 3: the ten N.. are doubles OF float sums (the right-hand sides are float expressions), and `N << N11, ...` casts each back
  // to float: the float sums are what the 4 x 4 holds
  const float N11 = (M[0][0] + M[1][1]) + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const float N22 = (M[0][0] - M[1][1]) - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const float N33 = (-M[0][0] + M[1][1]) - M[2][2], N34 = M[1][2] + M[2][1], N44 = (-M[0][0] - M[1][1]) + M[2][2];
  const float Nf[4][4] = {{(float)(double)N11, (float)(double)N12, (float)(double)N13, (float)(double)N14},
                          {(float)(double)N12, (float)(double)N22, (float)(double)N23, (float)(double)N24},
                          {(float)(double)N13, (float)(double)N23, (float)(double)N33, (float)(double)N34},
                          {(float)(double)N14, (float)(double)N24, (float)(double)N34, (float)(double)N44}};
  // Step 4: rules A and B
  double q[4];
  largest_eigenvector(Nf, q);
  quaternion_matrix(q, h.R);
  const float* R = h.R;
  // Step 5: P3 = mR12i * Pr2 (float, inner sums left to right)
  float P3[3][3];
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) P3[c][r] = (R[3 * r] * Pr2[c][0] + R[3 * r + 1] * Pr2[c][1]) + R[3 * r + 2] * Pr2[c][2];
  // Step 6: nom and den are doubles of float sums over the nine entries in storage order (rule C); ms12i = nom / den is a double
  // divide stored to float
  if (!fix_scale) {
    float nomf = 0.0f, denf = 0.0f;
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) {
        const float a = Pr1[c][r] * P3[c][r], b = P3[c][r] * P3[c][r];
        nomf = (c == 0 && r == 0) ? a : nomf + a;
        denf = (c == 0 && r == 0) ? b : denf + b;
      }
    h.s = (float)((double)nomf / (double)denf);
  } else {
    h.s = 1.0f;
  }
  const float s = h.s;
  // Step 7: mt12i = O1 - ms12i * mR12i * O2 parses as (ms12i * mR12i) * O2: a float scalar times a float matrix, coefficient by
  // coefficient, then the matrix-vector product with its inner sum left to right
  // Step 8.1: sR = ms12i * mR12i, the same nine products
  float sR[9];
  for (int k = 0; k < 9; k++) sR[k] = s * R[k];
  for (int r = 0; r < 3; r++) h.t[r] = O1[r] - ((sR[3 * r] * O2[0] + sR[3 * r + 1] * O2[1]) + sR[3 * r + 2] * O2[2]);
  // Step 8.2: sRinv = (1.0 / ms12i) * mR12i.transpose().  1.0 / ms12i is a double divide; a double scalar times a float matrix:
  // Eigen 3.3 has no ScalarBinaryOpTraits<double, float>, so promote_scalar_arg converts the scalar to the expression's
  // NumTraits<float>::Literal, float, ONCE, and the nine products are float products.  (Eigen is not vendored by the reference;
  // this is the reading of Eigen 3.3's XprHelper.h.)  tinv = -sRinv * mt12i: the negated matrix times the vector
  const float inv_s = (float)(1.0 / (double)s);
  float sRinv[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) sRinv[3 * r + c] = inv_s * R[3 * c + r];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      h.T12[4 * r + c] = sR[3 * r + c];
      h.T21[4 * r + c] = sRinv[3 * r + c];
    }
    h.T12[4 * r + 3] = h.t[r];
    h.T21[4 * r + 3] = ((-sRinv[3 * r]) * h.t[0] + (-sRinv[3 * r + 1]) * h.t[1]) + (-sRinv[3 * r + 2]) * h.t[2];
  }
}

// Pinhole::project(Vector3f): u = fx * x / z + cx in that order; nothing guards z == 0 (IEEE 754 decides)
GFS_HD void project(const float* cam, const float* X, float* uv) {  // cam = fx, fy, cx, cy
  uv[0] = cam[0] * X[0] / X[2] + cam[2];
  uv[1] = cam[1] * X[1] / X[2] + cam[3];
}

// Project's P3Dc = Rcw * X + tcw (:436) for a 3 x 4 [R | t], then the camera
GFS_HD void transform_project(const float* T, const float* cam, const float* X, float* uv) {
  float P[3];
  for (int r = 0; r < 3; r++) P[r] = ((T[4 * r] * X[0] + T[4 * r + 1] * X[1]) + T[4 * r + 2] * X[2]) + T[4 * r + 3];
  project(cam, P, uv);
}

// CheckInliers for one pair (:401-413): dist1 = mvP1im1 - vP2im1, dist2 = vP1im2 - mvP2im2, err = d . d.  The comparison is strict,
// so a NaN error is an outlier.
GFS_HD bool pair_errors(const Hyp& h, const float* cam1, const float* cam2, const float* X1, const float* X2, const float* p1im1,
                        const float* p2im2, float max1, float max2, float* err1, float* err2) {
  float p2im1[2], p1im2[2];
  transform_project(h.T12, cam1, X2, p2im1);
  transform_project(h.T21, cam2, X1, p1im2);
  const float d1x = p1im1[0] - p2im1[0], d1y = p1im1[1] - p2im1[1];
  const float d2x = p1im2[0] - p2im2[0], d2y = p1im2[1] - p2im2[1];
  *err1 = d1x * d1x + d1y * d1y;
  *err2 = d2x * d2x + d2y * d2y;
  return *err1 < max1 && *err2 < max2;
}

// ---- The outcome of the sequential loop (:229-274) from the counts c[0 .. H) of all H = mRansacMaxIts hypotheses.
// The loop returns at the first i with c[i] > minInliers: the update test c[i] >= mnBestInliers in front of it cannot block that
// iteration, because every earlier iteration had c <= minInliers, so mnBestInliers <= minInliers < c[i].  Then the result is
// hypothesis i, iterations = i + 1, bConverge.  Otherwise every iteration ran; the best set is replaced whenever c[i] >=
// mnBestInliers, so of equal maxima the LAST one stays: the result is the last index that attains the maximum, iterations = H,
// bNoMore.  (mnBestInliers starts at 0 and counts are >= 0, so iteration 0 always replaces: the result is always a hypothesis.)
struct Pick {
  int index, iterations, status;
};
GFS_HD Pick pick(const int* c, int H, int min_inliers) {
  int best = 0, best_c = -1;
  for (int i = 0; i < H; i++) {
    if (c[i] > min_inliers) return Pick{i, i + 1, kConverged};
    if (c[i] >= best_c) {
      best_c = c[i];
      best = i;
    }
  }
  return Pick{best, H, kNoMore};
}

// ---- SetRansacParameters (:119-143), a host function: mRansacMaxIts for N correspondences, with the host's libm.  epsilon is a float; pow(epsilon,
// 3) promotes it to double.  N == 0 divides by zero as the reference does (epsilon = inf, the log of a NaN, the cast of a NaN is
// whatever the platform gives): callers with N < minInliers never iterate (iterate's first test), so that value is never used.
inline int ransac_iterations(int N, double probability, int min_inliers, int max_iterations) {
  const float epsilon = (float)min_inliers / N;
  int nIterations;
  if (min_inliers == N) {
    nIterations = 1;
  } else {
    // int = ceil(double): NaN (N < minInliers) and values beyond int are undefined in C++; x86-64's conversion answers INT_MIN for
    // both, which the max below turns into 1: stated here so that every platform gives the reference's x86-64 value
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
    nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
  }
  return std::max(1, std::min(nIterations, max_iterations));
}
}  // namespace gfs_s3r
