// The visual-edge and Levenberg-Marquardt bodies shared by the motion-only bundle adjustments (device side): k_pose_opt (pose.hip,
// Optimizer::PoseOptimization) and k_pl_round (pose_lidar.hip, Optimizer::PoseLidarVisualOptimization).  Restates
// EdgeSE3ProjectXYZOnlyPose (src/OptimizableTypes.cpp:49-63), g2o::EdgeStereoSE3ProjectXYZOnlyPose
// (Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:339-404), constructQuadraticForm (core/base_unary_edge.hpp:43-72), the dense
// 6x6 solve with Eigen::LDLT semantics (solvers/linear_solver_dense.h:64-112), the scalars of OptimizationAlgorithmLevenberg::solve
// (core/optimization_algorithm_levenberg.cpp:61-168) and the re-classification of src/Optimizer.cc:972-1060.  Both kernels are held
// to the bits of a sequential CPU restatement (oracle/pose_oracle.cpp, tests/host/pose_lidar_restatement.cpp).  Quirks kept: chi2
// values are compared as floats, the stereo projection uses a float 1/z.
// Only bodies live here: the loops, the LDS layout and where an edge is kept (registers in k_pose_opt, global memory in k_pl_round)
// stay with the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "g2o_se3_dev.hpp"
#include "lm_lambda_rule.hpp"

namespace gfs_pose_lm {

constexpr int kSys = 27;  // 21 (upper triangle of H) + 6 (b)

// deltaMono / deltaStereo are floats (src/Optimizer.cc:807-808)
__device__ __forceinline__ double huber_delta(bool stereo) { return stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991); }
// chi2Mono / chi2Stereo (:967-968): the mono list is re-classified in pass 0, the stereo list in pass 1
__device__ __forceinline__ float chi2_gate(int pass) { return pass ? 7.815f : 5.991f; }

__device__ __forceinline__ void map3(const double* q, const double* t, const double* X, double* o) {  // SE3Quat::map
  gfs_se3::quat_rotate(q, X, o);
  o[0] += t[0];
  o[1] += t[1];
  o[2] += t[2];
}

// computeError of a visual edge at pose (q, t) and its chi2.  Frame: fx, fy, cx, cy, bf
template <typename Frame>
__device__ __forceinline__ void vis_edge_error(const Frame& F, const double* xw, const double* obs, bool stereo, const double* q,
                                               const double* t, double* r) {
  double xc[3];
  map3(q, t, xw, xc);
  if (stereo) {  // cam_project (types_six_dof_expmap.cpp:339-346): float invz, double bf
    const float invz = (float)(1.0 / xc[2]);
    const double u = xc[0] * (double)invz * F.fx + F.cx, v = xc[1] * (double)invz * F.fy + F.cy;
    r[0] = obs[0] - u;
    r[1] = obs[1] - v;
    r[2] = obs[2] - (u - F.bf * (double)invz);
  } else {  // Pinhole::project(Vector3d), src/CameraModels/Pinhole.cpp:35-41
    r[0] = obs[0] - (F.fx * xc[0] / xc[2] + F.cx);
    r[1] = obs[1] - (F.fy * xc[1] / xc[2] + F.cy);
    r[2] = 0;
  }
}
__device__ __forceinline__ double vis_edge_chi2(const double* r, double w, bool stereo) {
  return stereo ? (r[0] * w * r[0] + r[1] * w * r[1] + r[2] * w * r[2]) : (r[0] * w * r[0] + r[1] * w * r[1]);
}
// computeError of a visual edge at pose T = (q, t), as computeActiveErrors and the re-classification run it: leaves the error vector
// and the chi2 in the edge (err, chi2) and returns the edge's term of activeRobustChi2 (robust: through the Huber kernel)
template <typename Frame>
__device__ __forceinline__ double vis_edge_update(const Frame& F, const double* xw, const double* obs, bool stereo, double w,
                                                 const double* T, bool robust, double* err, double& chi2) {
  double r[3];  // (not err itself: it may be global memory, which the reads of xw / obs would have to wait for)
  vis_edge_error(F, xw, obs, stereo, T, T + 4, r);
  const double c = vis_edge_chi2(r, w, stereo);
  for (int k = 0; k < 3; k++) err[k] = r[k];
  chi2 = c;
  double term = c, r1;
  if (robust) gfs_se3::huber(c, huber_delta(stereo), &term, &r1);
  return term;
}

// linearizeOplus + constructQuadraticForm of a visual edge at pose T = (q, t): its 21 + 6 terms of H and b in acc.  w: the edge's
// information; robust: with the Huber kernel; chi2, err: what computeError left in the edge.  (rho' is taken here, after the
// Jacobian, and not handed in by the caller: taken before it, k_pose_opt's tree instance spills 432 instead of 120 bytes a lane)
template <typename Frame>
__device__ __forceinline__ void vis_edge_quadratic_form(const Frame& F, const double* T, const double* xw, bool stereo, double w,
                                                        bool robust, double chi2, const double* err, double (&acc)[kSys]) {
  double xc[3];
  map3(T, T + 4, xw, xc);
  const double x = xc[0], y = xc[1], z = xc[2];
  double J[18];
  if (stereo) {  // types_six_dof_expmap.cpp:375-404
    const double invz = 1.0 / z, invz_2 = invz * invz;
    J[0] = x * y * invz_2 * F.fx;
    J[1] = -(1 + (x * x * invz_2)) * F.fx;
    J[2] = y * invz * F.fx;
    J[3] = -invz * F.fx;
    J[4] = 0;
    J[5] = x * invz_2 * F.fx;
    J[6] = (1 + y * y * invz_2) * F.fy;
    J[7] = -x * y * invz_2 * F.fy;
    J[8] = -x * invz * F.fy;
    J[9] = 0;
    J[10] = -invz * F.fy;
    J[11] = y * invz_2 * F.fy;
    J[12] = J[0] - F.bf * y * invz_2;
    J[13] = J[1] + F.bf * x * invz_2;
    J[14] = J[2];
    J[15] = J[3];
    J[16] = 0;
    J[17] = J[5] - F.bf * invz_2;
  } else {  // src/OptimizableTypes.cpp:49-63: -projectJac(xyz) * SE3deriv
    const double pj[6] = {F.fx / z, 0, -F.fx * x / (z * z), 0, F.fy / z, -F.fy * y / (z * z)};
    const double D[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int c = 0; c < 6; c++) J[6 * r + c] = -(pj[3 * r] * D[c] + pj[3 * r + 1] * D[6 + c] + pj[3 * r + 2] * D[12 + c]);
#pragma unroll
    for (int c = 0; c < 6; c++) J[12 + c] = 0;
  }
  double rho1 = 1.0;
  if (robust) {
    double r0;
    gfs_se3::huber(chi2, huber_delta(stereo), &r0, &rho1);
  }
  // the lower triangle, row a / column c <= a: the entries Eigen's LDLT reads (packed a (a + 1) / 2 + c)
  // (every index below is a compile-time constant: arrays indexed at run time would live in scratch memory.  The third
  //  row is added by a select, not as a zero term, so that a mono edge sums exactly its two terms)
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double sb = 0;
    sb += ((rho1 * J[a]) * w) * err[0];
    sb += ((rho1 * J[6 + a]) * w) * err[1];
    const double sb3 = sb + ((rho1 * J[12 + a]) * w) * err[2];
    sb = stereo ? sb3 : sb;
    acc[21 + a] = -sb;  // b -= ((rho1 A') Omega) e, Eigen's left-to-right association of base_unary_edge.hpp:62
#pragma unroll
    for (int c = 0; c <= a; c++) {
      double hh = 0;
      hh += (J[a] * (rho1 * w)) * J[c];  // (A' weightedOmega) A: H(a, c) = sum_k (J_ka w') J_kc, base_unary_edge.hpp:63
      hh += (J[6 + a] * (rho1 * w)) * J[6 + c];
      const double hh3 = hh + (J[12 + a] * (rho1 * w)) * J[12 + c];
      acc[o++] = stereo ? hh3 : hh;
    }
  }
}

// One dependent chain of cnt additions, s += v[0], v[1], ... in index order (S = float over double terms: each sum is rounded to
// float, as `float += double` does).  The terms of the NEXT batch are fetched from LDS while this batch is added (a plain loop
// waits for its eight reads, adds, and only then asks for the next eight: 250 cycles a batch instead of the 80 the adds take)
template <typename T, typename S>
__device__ __forceinline__ S ordered_sum(const T* __restrict__ v, int cnt, S s) {
  constexpr int kB = 8;
  T a[kB];
  int j = 0;
  if (cnt >= kB) {
#pragma unroll
    for (int u = 0; u < kB; u++) a[u] = v[u];
    for (; j + 2 * kB <= cnt; j += kB) {
      T b[kB];
#pragma unroll
      for (int u = 0; u < kB; u++) b[u] = v[j + kB + u];
#pragma unroll
      for (int u = 0; u < kB; u++) s += a[u];
#pragma unroll
      for (int u = 0; u < kB; u++) a[u] = b[u];
    }
#pragma unroll
    for (int u = 0; u < kB; u++) s += a[u];
    j += kB;
  }
  for (; j < cnt; j++) s += v[j];
  return s;
}

// Eigen::LDLT<MatrixXd>::compute + isPositive + solve on an N x N, N = 6 or 7 (see oracle/pose_oracle.cpp for the line-by-line restatement).
// The pivot search and the symmetric transpositions index the matrix at run time.  A private array indexed at run time lives in
// scratch memory, an LDS copy costs a round trip per access on the one lane everybody waits for (6.5 us a solve, a fifth of
// k_pose_opt): here every index is a compile-time constant -- the loops over k, i, j are unrolled and the run-time pivot p is matched
// against its (at most N - 1) possible values, each with its own statically indexed swaps -- so the entries of the lower
// triangle, y and the transpositions stay in registers.  The arithmetic, operation for operation, is the restatement's.
template <int N, int K, int PC>
__device__ __forceinline__ void ldlt_transpose(double (&A)[N][N]) {  // symmetric transposition k <-> p restricted to the lower triangle
#pragma unroll
  for (int j = 0; j < K; j++) {
    const double tmp = A[K][j];
    A[K][j] = A[PC][j];
    A[PC][j] = tmp;
  }
#pragma unroll
  for (int i = PC + 1; i < N; i++) {
    const double tmp = A[i][K];
    A[i][K] = A[i][PC];
    A[i][PC] = tmp;
  }
  {
    const double tmp = A[K][K];
    A[K][K] = A[PC][PC];
    A[PC][PC] = tmp;
  }
#pragma unroll
  for (int i = K + 1; i < PC; i++) {
    const double tmp = A[i][K];
    A[i][K] = A[PC][i];
    A[PC][i] = tmp;
  }
}
template <int N, int K>
__device__ __forceinline__ void ldlt_step(double (&A)[N][N], int (&tr)[N], int& sign) {
  int p = K;
  double best = fabs(A[K][K]);
#pragma unroll
  for (int i = K + 1; i < N; i++)
    if (fabs(A[i][i]) > best) {
      best = fabs(A[i][i]);
      p = i;
    }
  tr[K] = p;
  if constexpr (K + 1 < N) { if (p == K + 1) ldlt_transpose<N, K, K + 1 < N ? K + 1 : N - 1>(A); }
  if constexpr (K + 2 < N) { if (p == K + 2) ldlt_transpose<N, K, K + 2 < N ? K + 2 : N - 1>(A); }
  if constexpr (K + 3 < N) { if (p == K + 3) ldlt_transpose<N, K, K + 3 < N ? K + 3 : N - 1>(A); }
  if constexpr (K + 4 < N) { if (p == K + 4) ldlt_transpose<N, K, K + 4 < N ? K + 4 : N - 1>(A); }
  if constexpr (K + 5 < N) { if (p == K + 5) ldlt_transpose<N, K, K + 5 < N ? K + 5 : N - 1>(A); }
  if constexpr (K + 6 < N) { if (p == K + 6) ldlt_transpose<N, K, K + 6 < N ? K + 6 : N - 1>(A); }
  if constexpr (K > 0) {
    double temp[K];
#pragma unroll
    for (int j = 0; j < K; j++) temp[j] = A[j][j] * A[K][j];
    double acc = 0;
#pragma unroll
    for (int j = 0; j < K; j++) acc += A[K][j] * temp[j];
    A[K][K] -= acc;
#pragma unroll
    for (int i = K + 1; i < N; i++) {
      double a2 = 0;
#pragma unroll
      for (int j = 0; j < K; j++) a2 += A[i][j] * temp[j];
      A[i][K] -= a2;
    }
  }
  const double akk = A[K][K];
  if (fabs(akk) > 0) {
#pragma unroll
    for (int i = K + 1; i < N; i++) A[i][K] /= akk;
  }
  if (sign == 1) {
    if (akk < 0) sign = 2;
  } else if (sign == -1) {
    if (akk > 0) sign = 2;
  } else if (sign == 0) {
    if (akk > 0) sign = 1;
    else if (akk < 0) sign = -1;
  }
}
template <int N, int K>
__device__ __forceinline__ void ldlt_swap_y(double (&y)[N], int p) {  // y[K] <-> y[p], p >= K
  if constexpr (K + 1 < N) { if (p == K + 1) { const double t = y[K]; y[K] = y[K + 1 < N ? K + 1 : N - 1]; y[K + 1 < N ? K + 1 : N - 1] = t; } }
  if constexpr (K + 2 < N) { if (p == K + 2) { const double t = y[K]; y[K] = y[K + 2 < N ? K + 2 : N - 1]; y[K + 2 < N ? K + 2 : N - 1] = t; } }
  if constexpr (K + 3 < N) { if (p == K + 3) { const double t = y[K]; y[K] = y[K + 3 < N ? K + 3 : N - 1]; y[K + 3 < N ? K + 3 : N - 1] = t; } }
  if constexpr (K + 4 < N) { if (p == K + 4) { const double t = y[K]; y[K] = y[K + 4 < N ? K + 4 : N - 1]; y[K + 4 < N ? K + 4 : N - 1] = t; } }
  if constexpr (K + 5 < N) { if (p == K + 5) { const double t = y[K]; y[K] = y[K + 5 < N ? K + 5 : N - 1]; y[K + 5 < N ? K + 5 : N - 1] = t; } }
  if constexpr (K + 6 < N) { if (p == K + 6) { const double t = y[K]; y[K] = y[K + 6 < N ? K + 6 : N - 1]; y[K + 6 < N ? K + 6 : N - 1] = t; } }
}
// H: the N (N + 1) / 2 entries of the lower triangle, packed a (a + 1) / 2 + c; lambda is added to the diagonal.  false unless
// positive.  N = 6: the pose block of k_pose_opt and k_pl_round; N = 7: the Sim3 block of k_sim3_opt (sim3_opt.hip)
template <int N>
__device__ __forceinline__ bool ldlt_solve_positive(const double* Hp, double lambda, const double* b, double* x) {
  double A[N][N];
  {
    int o = 0;
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
      for (int c = 0; c <= a; c++) {
        A[a][c] = Hp[o];
        A[c][a] = Hp[o];
        o++;
      }
  }
#pragma unroll
  for (int a = 0; a < N; a++) A[a][a] += lambda;
  static_assert(N == 6 || N == 7, "the steps and transpositions below are written out for 6 and 7");
  int tr[N], sign = 0;
  ldlt_step<N, 0>(A, tr, sign);
  ldlt_step<N, 1>(A, tr, sign);
  ldlt_step<N, 2>(A, tr, sign);
  ldlt_step<N, 3>(A, tr, sign);
  ldlt_step<N, 4>(A, tr, sign);
  ldlt_step<N, 5>(A, tr, sign);
  if constexpr (N > 6) ldlt_step<N, 6>(A, tr, sign);
  if (sign != 1) return false;
  double y[N];
#pragma unroll
  for (int i = 0; i < N; i++) y[i] = b[i];
  ldlt_swap_y<N, 0>(y, tr[0]);
  ldlt_swap_y<N, 1>(y, tr[1]);
  ldlt_swap_y<N, 2>(y, tr[2]);
  ldlt_swap_y<N, 3>(y, tr[3]);
  ldlt_swap_y<N, 4>(y, tr[4]);
  if constexpr (N > 6) ldlt_swap_y<N, 5>(y, tr[5]);
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < i; j++) y[i] -= A[i][j] * y[j];
#pragma unroll
  for (int i = 0; i < N; i++) y[i] = fabs(A[i][i]) > 2.2250738585072014e-308 ? y[i] / A[i][i] : 0.0;
#pragma unroll
  for (int i = N - 1; i >= 0; i--)
#pragma unroll
    for (int j = i + 1; j < N; j++) y[i] -= A[j][i] * y[j];
  if constexpr (N > 6) ldlt_swap_y<N, 5>(y, tr[5]);
  ldlt_swap_y<N, 4>(y, tr[4]);
  ldlt_swap_y<N, 3>(y, tr[3]);
  ldlt_swap_y<N, 2>(y, tr[2]);
  ldlt_swap_y<N, 1>(y, tr[1]);
  ldlt_swap_y<N, 0>(y, tr[0]);
#pragma unroll
  for (int i = 0; i < N; i++) x[i] = y[i];
  return true;
}
__device__ __forceinline__ bool ldlt6_solve_positive(const double* H21, double lambda, const double* b, double* x) {
  return ldlt_solve_positive<6>(H21, lambda, b, x);
}

// The 6x6 solve of k_pose_opt's tree-sum mode (k_pl_round never calls it: its tree mode keeps the pivoted solve).  H + lambda I of
// an LM trial is symmetric positive definite unless the trial is hopeless, and for such a matrix Eigen's diagonal pivoting only
// re-orders the rounding: an UN-pivoted LDL^T (as k_gicp_solve uses for the same reason) gives the solution to rounding with ~150
// instead of ~1 000 instructions on the one lane everybody waits for (no pivot search, no transpositions, six reciprocals instead of
// 21 divisions).  "Not positive" (LinearSolverDense: the trial is rejected) = a pivot that is not > 0 -- the same matrices, up to
// those within rounding of singular.
__device__ __forceinline__ bool ldlt6_solve_spd_fast(const double* H21, double lambda, const double* b, double* x) {
#pragma clang fp contract(fast)
  double L[6][6], W[6][6], rd[6];  // L unit lower, W = L D, rd = 1 / d
  {
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c <= a; c++) L[a][c] = H21[o++];
  }
#pragma unroll
  for (int a = 0; a < 6; a++) L[a][a] += lambda;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double dj = L[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) dj -= L[j][k] * W[j][k];
    ok = ok && dj > 0.0;
    rd[j] = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) v -= L[i][k] * W[j][k];
      W[i][j] = v;
      L[i][j] = v * rd[j];
    }
  }
  if (!ok) return false;
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    y[i] = b[i];
#pragma unroll
    for (int j = 0; j < i; j++) y[i] -= L[i][j] * y[j];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) y[i] *= rd[i];
#pragma unroll
  for (int i = 5; i >= 0; i--) {
#pragma unroll
    for (int j = i + 1; j < 6; j++) y[i] -= L[j][i] * y[j];
    x[i] = y[i];
  }
  return true;
}

// The scalars of OptimizationAlgorithmLevenberg that live across the iterations of one optimize() call (one lane runs them)
struct LmState {
  double currentLambda, ni;
  int nBadLm;
};
__device__ __forceinline__ void lm_lambda_init(LmState& L, const double* H21) {  // computeLambdaInit: tau * max |diag(H)|
  L.currentLambda = 1e-5 * max_abs_diagonal6(H21);  // std::max's way with a NaN, not fmax's: lm_lambda_rule.hpp
  L.ni = 2;
  L.nBadLm = 0;
}
struct LmVerdict {
  bool again, accepted;  // try another lambda; the trial's estimate is kept (otherwise the caller pops the backup)
};
// Judges one trial of the lambda loop.  solved: the 6x6 solve was positive, x its solution (b: the right-hand side); tempChi: the
// activeRobustChi2 at the trial estimate.  Updates the gain ratio rho, lambda, currentChi and the trial count qmax.  plain_cube:
// g * g * g instead of glibc's pow(g, 3) (k_pose_opt's tree mode)
__device__ __forceinline__ LmVerdict lm_judge_trial(LmState& L, bool solved, double tempChi, const double* x, const double* b,
                                                    bool plain_cube, double& currentChi, double& rho, int& qmax) {
  if (!solved) tempChi = 1.79769313486231570e308;
  rho = currentChi - tempChi;
  double scale = 0;
  if (solved)
    for (int a = 0; a < 6; a++) scale += x[a] * (L.currentLambda * x[a] + b[a]);
  scale += 1e-3;
  rho /= scale;
  const bool accepted = rho > 0 && isfinite(tempChi);
  if (accepted) {
    const double g3 = 2 * rho - 1;
    double alpha = 1. - (plain_cube ? g3 * g3 * g3 : gfs_glibc::pow3(g3));
    alpha = fmin(alpha, 2. / 3.);
    const double scaleFactor = fmax(1. / 3., alpha);
    L.currentLambda *= scaleFactor;
    L.ni = 2;
    currentChi = tempChi;
  } else {
    L.currentLambda *= L.ni;
    L.ni *= 2;
  }
  qmax++;
  return {rho < 0 && qmax < 10, accepted};
}
// The stop rule at the end of an LM iteration: the lambda loop gave up, no gain at all, or three iterations in a row that gained
// less than a thousandth (the nBadLm rule of the reference's g2o)
__device__ __forceinline__ bool lm_stop(LmState& L, int qmax, double rho, double iniChi, double currentChi) {
  if (qmax == 10 || rho == 0) return true;
  if ((iniChi - currentChi) * 1e3 < iniChi) L.nBadLm++;
  else L.nBadLm = 0;
  return L.nBadLm >= 3;
}

// Re-classification of one visual edge in the pass of its list (pass 0: mono, pass 1: stereo; src/Optimizer.cc:972-1060): the chi2 is
// compared as a float, outlier edges leave the next round (level 1).  Returns the term of the inliers' float chi2 sum: +0 for an
// outlier and for an edge of the other list, which changes nothing.
template <typename Flag>
__device__ __forceinline__ float classify_edge(bool stereo, double chi2, int pass, Flag& outlier, Flag& level, int& n_bad, int& n_good) {
  if (stereo != (pass == 1)) return 0.0f;
  const float c = (float)chi2;
  const bool out = c > chi2_gate(pass);
  outlier = out ? 1 : 0;
  level = out ? 1 : 0;
  n_bad += out ? 1 : 0;
  n_good += out ? 0 : 1;
  return out ? 0.0f : c;
}

}  // namespace gfs_pose_lm
