// The rule of Optimizer::LocalInertialBA (reference src/Optimizer.cc:3056-3702), the inertial local bundle adjustment LocalMapping
// runs for every new key frame once the IMU is initialised, from optimizer.initializeOptimization() (:3589) to the end of the two
// classification loops (:3626); stated once for the device (lba_inertial.hip) and the host
// (tests/host/lba_inertial_restatement.cpp); DESIGN.md section 26.  The edges' arithmetic is pose_inertial_rule.hpp's, which this
// header includes and does not change.
//
//   vertices   the N window key frames, newest first, 15 unknowns each in the order VertexPose 0-5 (ImuCamPose, updated on the right
//              by pose_update), VertexVelocity 6-8, VertexGyroBias 9-11, VertexAccBias 12-14 (additive): unknown 15 i + r of the reduced
//              system.  Key-frame index N is the fixed key frame in front of the window (four fixed vertices), N + 1 + k the k-th
//              other fixed key frame (a pose only).  Every map point is a marginalised VertexSBAPointXYZ.
//   edges      in insertion order, the order of g2o's active edges: set i = EdgeInertial (Huber sqrt(16.0), information * 1e-2 for
//              i = N - 1), EdgeGyroRW, EdgeAccRW from key frame i + 1 to key frame i, for i = 0 .. N - 1; then the visual edges
//              (EdgeMono / EdgeStereo, Huber (float)sqrt(5.991) / (float)sqrt(7.815)) point by point, observation by observation.
//   schedule   ONE optimize(iterations) of the fork's OptimizationAlgorithmLevenberg (core/optimization_algorithm_levenberg.cpp
//              :61-169): lm_begin_iteration / lm_trial below.
//
// Quirks kept (each is the reference's behaviour, not a choice):
//   * NO STOP FLAG.  setForceStopFlag is called after optimize (:3594): nothing is polled, the call takes no flag.
//   * lambda_0 is the user's value (1e0, or 1e-2 with bLarge); computeLambdaInit's diagonal maximum is never read.  lambda is added to
//     EVERY diagonal entry, the landmarks' included.  Up to ten trials an iteration with _ni doubling; the gain ratio divides by
//     computeScale() + 1e-3; the `_nBad >= 3` stop marked "Raul" is kept; Terminate follows qmax == 10 || rho == 0.
//   * A comparison with a NaN rho is false: the trial is rejected, the trial loop ends (rho < 0 is false), the iteration returns OK and
//     the next one starts.
//   * err is the float cast of activeRobustChi2() after the first computeActiveErrors, err_end the float cast after optimize.  The
//     per-edge chi2 is what the edges hold then, i.e. after the LAST computeActiveErrors g2o ran: after an iteration that ended on a
//     rejected trial those are the REJECTED state's errors, while the estimate isDepthPositive() reads is the restored one.
//   * The erase tests compare the double chi2 with the floats 5.991f, 1.5f * 5.991f (close) and 7.815f.
//   * bRecInit is unused by the reference's function and is not part of the problem.
//
// Written rules, where the reference's arithmetic comes from a library this project does not build against:
//   rule D   g2o's LinearSolverEigen is a sparse SimplicialLDLT under an AMD ordering: its rounding cannot be reproduced and nothing
//            downstream depends on it.  In its place: a dense LDL' of the reduced 15 N system WITHOUT pivoting, in vertex order,
//            column by column (ldlt_* below); a zero, negative or non-finite pivot fails the solve.
//   rule F   after a failed solve g2o applies whatever its x buffer holds.  Here x is ZERO after a failed solve (poses and points);
//            tempChi = DBL_MAX as in the reference, so the gain ratio is -inf and the trial is rejected.
//   rule I   Eigen's 3 x 3 inverse of Hll + lambda I: cofactors over the determinant (inverse3).
//   rule P   pow(2 rho - 1, 3) is t * t * t.
//   rule S   as pose_inertial_rule.hpp: inner sums left to right.
//
// Every sum's order is a function of the problem alone -- no floating-point atomics, nothing depends on a grid:
//   * a landmark's Hll and bl: its edges in edge order;
//   * the pose block (21 + 6 entries) of key frame i: the small edges' contribution first (sets in insertion order), then the visual
//     edges of the key frame in ascending edge order;
//   * the reduced system's entry: that value (+ lambda on the diagonal), then the Schur terms SUBTRACTED one by one in
//     landmark-then-edge order (e1, then e2), as gba_lists.hpp states it; the right-hand side likewise over the key frame's edges;
//   * chi2 totals and computeScale(): per-landmark partials (edge order inside a landmark), the partials of kChunk = 256 consecutive
//     landmarks joined by the fixed pairwise tree of chunk_tree, the chunk sums added in chunk order onto the small edges' sum
//     (insertion order) respectively onto the poses' sum (unknown order).
#pragma once
#include <cfloat>

#include "pose_inertial_rule.hpp"

namespace gfs_li {

using namespace gfs_pi;

constexpr int kMaxWindow = 10, kMaxWindowLarge = 20;   // if (bLarge) maxOpt = 20 else 10 ... (:3064-3070)
constexpr int kOptIt = 8, kOptItLarge = 4;             // opt_it
constexpr double kLambdaInit = 1e0, kLambdaInitLarge = 1e-2;
constexpr double kInfoDownLast = 1e-2;                 // vei[N - 1]->information() * 1e-2
constexpr float kChi2Mono2 = 5.991f, kChi2Stereo2 = 7.815f, kCloseFactor = 1.5f;
constexpr int kMaxFixKF = 200, kMaxCovKF = 0;
constexpr double kFailGateFactor = 2.0;                // 2 * err < err_end: the adaptor's
constexpr int kMaxTrials = 10;                         // _maxTrialsAfterFailure
constexpr int kChunk = 256;                            // landmarks per chunk of the chi2 / scale sums
constexpr int kLdsRows = 180;                          // the packed triangle of up to 180 rows is factored in LDS
GFS_HD double huber_inertial_lba() { return sqrt(16.0); }

struct Set {  // one inertial edge set as the edges read it
  Preint pre;
  double info_i[81], info_g[9], info_a[9];
};
struct SetEdges {  // its linearisation
  InertialEdge ei;
  RandomWalkEdge gr, ar;
  double chi[3];  // what each edge adds to activeRobustChi2
};

// ------------------------------------------------------------------------------------------------ the Levenberg state machine
struct Ctl {
  double lambda, ni, current_chi, ini_chi, rho, last_total, first_total, scale_pose;
  int n_bad, qmax, iter_open, done, ok2, iterations_run, trials_run, accepted, started, pad;
};
GFS_HD void lm_init(Ctl& c, double lambda_init) {
  c.lambda = lambda_init, c.ni = 2.0, c.current_chi = c.ini_chi = c.rho = c.last_total = c.first_total = c.scale_pose = 0.0;
  c.n_bad = c.qmax = c.iter_open = c.done = c.iterations_run = c.trials_run = c.accepted = c.started = c.pad = 0;
  c.ok2 = 1;
}
// computeActiveErrors + activeRobustChi2 at the head of solve(): total is the robust chi2 at the current state
GFS_HD void lm_begin_iteration(Ctl& c, double total, bool open) {
  if (!c.started) c.first_total = total, c.started = 1;
  c.last_total = total;
  c.current_chi = c.ini_chi = total;
  c.rho = 0.0;
  c.qmax = 0;
  c.iter_open = open ? 1 : 0;
}
// One trial's decision.  lambda_used: the lambda the trial was solved with (c.lambda before the call).  Returns accepted
GFS_HD bool lm_trial(Ctl& c, double temp_raw, double scale_raw) {
  c.last_total = temp_raw;
  const double temp = c.ok2 ? temp_raw : DBL_MAX;
  double rho = c.current_chi - temp;
  const double scale = scale_raw + 1e-3;
  rho /= scale;
  c.rho = rho;
  const bool finite = temp - temp == 0.0;
  bool accepted = false;
  if (rho > 0 && finite) {
    const double t = 2 * rho - 1;
    double alpha = 1. - (t * t) * t;
    alpha = alpha < 2. / 3. ? alpha : 2. / 3.;       // (std::min)(alpha, _goodStepUpperScale)
    const double f = 1. / 3. < alpha ? alpha : 1. / 3.;  // (std::max)(_goodStepLowerScale, alpha)
    c.lambda *= f;
    c.ni = 2;
    c.current_chi = temp;
    accepted = true;
  } else {
    c.lambda *= c.ni;
    c.ni *= 2;
  }
  c.accepted = accepted ? 1 : 0;
  c.qmax++;
  c.trials_run++;
  if (rho < 0 && c.qmax < kMaxTrials) return accepted;  // the next trial
  c.iter_open = 0;
  c.iterations_run++;
  if (c.qmax == kMaxTrials || rho == 0) {
    c.done = 1;  // Terminate
    return accepted;
  }
  if ((c.ini_chi - c.current_chi) * 1e3 < c.ini_chi) c.n_bad++;
  else c.n_bad = 0;
  if (c.n_bad >= 3) c.done = 1;
  return accepted;
}

// ------------------------------------------------------------------------------------------------ sums over landmarks
// The partials of up to kChunk consecutive landmarks (missing ones +0.0) joined pairwise: s[i] += s[i + h] for h = 128, 64, .. 1
GFS_HD double chunk_tree(double* s) {
  for (int h = kChunk / 2; h >= 1; h >>= 1)
    for (int i = 0; i < h; i++) s[i] += s[i + h];
  return s[0];
}

// ------------------------------------------------------------------------------------------------ visual edges with a free point
// _jacobianOplusXi = -proj_jac * Rcw: the negated projection Jacobian times Rcw.  Row-major 3 x 3, the third row zero for a mono edge
GFS_HD void vis_point_jacobian(const Calib& c, const double* Rcw, const double* tcw, const double* xw, bool stereo, double (&Jl)[9]) {
  double X[3];
  mv3(Rcw, xw, X);
  for (int k = 0; k < 3; k++) X[k] += tcw[k];
  double P[9];
  P[0] = c.fx / X[2], P[1] = 0.0, P[2] = -c.fx * X[0] / (X[2] * X[2]);
  P[3] = 0.0, P[4] = c.fy / X[2], P[5] = -c.fy * X[1] / (X[2] * X[2]);
  const double inv_z2 = 1.0 / (X[2] * X[2]);
  P[6] = P[0], P[7] = P[1], P[8] = P[2] + c.bf * inv_z2;
  GFS_PI_UNROLL
  for (int r = 0; r < 3; r++)
    GFS_PI_UNROLL
    for (int k = 0; k < 3; k++)
      Jl[3 * r + k] = (r == 2 && !stereo) ? 0.0 : ((-P[3 * r]) * Rcw[k] + (-P[3 * r + 1]) * Rcw[3 + k]) + (-P[3 * r + 2]) * Rcw[6 + k];
}
// The point's share of constructQuadraticForm with Omega = w I: the 6 entries of the lower triangle of Jl' (rho1 Omega) Jl, then the
// 3 of -rho1 Jl' Omega e
GFS_HD void vis_point_form(const double (&Jl)[9], double w, bool stereo, double rho1, const double* e, double (&t)[9]) {
  int o = 0;
  GFS_PI_UNROLL
  for (int a = 0; a < 3; a++) {
    double sb = 0;
    sb += ((rho1 * Jl[a]) * w) * e[0];
    sb += ((rho1 * Jl[3 + a]) * w) * e[1];
    const double sb3 = sb + ((rho1 * Jl[6 + a]) * w) * e[2];
    t[6 + a] = -(stereo ? sb3 : sb);
    GFS_PI_UNROLL
    for (int cc = 0; cc <= a; cc++) {
      double hh = 0;
      hh += (Jl[a] * (rho1 * w)) * Jl[cc];
      hh += (Jl[3 + a] * (rho1 * w)) * Jl[3 + cc];
      const double hh3 = hh + (Jl[6 + a] * (rho1 * w)) * Jl[6 + cc];
      t[o++] = stereo ? hh3 : hh;
    }
  }
}
// Hpl (6 x 3, entry 3 a + k): (Jl' (rho1 Omega)) Jp transposed
GFS_HD void vis_hpl(const double (&Jp)[18], const double (&Jl)[9], double w, bool stereo, double rho1, double (&H)[18]) {
  GFS_PI_UNROLL
  for (int a = 0; a < 6; a++)
    GFS_PI_UNROLL
    for (int k = 0; k < 3; k++) {
      double hh = 0;
      hh += (Jl[k] * (rho1 * w)) * Jp[a];
      hh += (Jl[3 + k] * (rho1 * w)) * Jp[6 + a];
      const double hh3 = hh + (Jl[6 + k] * (rho1 * w)) * Jp[12 + a];
      H[3 * a + k] = stereo ? hh3 : hh;
    }
}
// rule I: the inverse of the symmetric 3 x 3 held as its lower triangle (0; 1 2; 3 4 5) with lambda on the diagonal
GFS_HD void inverse3(const double* h, double lambda, double* inv) {
  const double a = h[0] + lambda, b = h[1], c = h[3], d = h[2] + lambda, e = h[4], f = h[5] + lambda;  // [a b c; b d e; c e f]
  const double C0 = d * f - e * e, C1 = c * e - b * f, C2 = b * e - c * d;
  const double det = (a * C0 + b * C1) + c * C2;
  inv[0] = C0 / det, inv[1] = C1 / det, inv[2] = C2 / det;
  inv[3] = inv[1], inv[4] = (a * f - c * c) / det, inv[5] = (b * c - a * e) / det;
  inv[6] = inv[2], inv[7] = inv[5], inv[8] = (a * d - b * b) / det;
}
// Y (24): Hpl Inv (6 x 3, entry 3 a + m), then (Hpl Inv) bl (6)
GFS_HD void vis_y(const double* Hpl, const double* inv, const double* bl, double* Y) {
  for (int a = 0; a < 6; a++)
    for (int m = 0; m < 3; m++) Y[3 * a + m] = (Hpl[3 * a] * inv[m] + Hpl[3 * a + 1] * inv[3 + m]) + Hpl[3 * a + 2] * inv[6 + m];
  for (int a = 0; a < 6; a++) Y[18 + a] = (Y[3 * a] * bl[0] + Y[3 * a + 1] * bl[1]) + Y[3 * a + 2] * bl[2];
}
GFS_HD double schur_term(const double* Y1, const double* Hpl2, int a, int c) {  // ((Hpl1 Inv) Hpl2')(a, c)
  return (Y1[3 * a] * Hpl2[3 * c] + Y1[3 * a + 1] * Hpl2[3 * c + 1]) + Y1[3 * a + 2] * Hpl2[3 * c + 2];
}
// The landmark's step: cp = bl - sum over its free edges of Hpl' x_pose (edge order), x = Inv cp
GFS_HD void back_edge(const double* Hpl, const double* xp, double* cp) {
  for (int k = 0; k < 3; k++) {
    double s = 0;
    for (int a = 0; a < 6; a++) s += Hpl[3 * a + k] * xp[a];
    cp[k] -= s;
  }
}
GFS_HD bool erase_mono(double chi2, bool close, bool depth_positive) {
  return (chi2 > kChi2Mono2 && !close) || (chi2 > kCloseFactor * kChi2Mono2 && close) || !depth_positive;
}
GFS_HD bool erase_stereo(double chi2) { return chi2 > kChi2Stereo2; }

// ------------------------------------------------------------------------------------------------ the small edges
// Set s joins key frame s + 1 (the edge's vertices 0-3: columns 0-14) to key frame s (pose and velocity: columns 15-23); the random
// walks join the biases (columns 0-2 of key frame s + 1, 3-5 of key frame s).  The column of unknown (key frame i, r) or -1
GFS_HD int set_inertial_column(int s, int i, int r) { return i == s ? (r < 9 ? 15 + r : -1) : i == s + 1 ? r : -1; }
GFS_HD int set_gyro_column(int s, int i, int r) { return (r < 9 || r >= 12) ? -1 : i == s ? r - 6 : i == s + 1 ? r - 9 : -1; }
GFS_HD int set_acc_column(int s, int i, int r) { return r < 12 ? -1 : i == s ? r - 9 : i == s + 1 ? r - 12 : -1; }
// computeError + linearizeOplus + the weights of set s.  prev / cur: the states of key frames s + 1 and s.  Lane 0 of the device
GFS_HD void set_inertial(const Set& st, const State& prev, const State& cur, SetEdges& E, bool build) {
  inertial_linearize(st.pre, prev, cur, E.ei);
  double rho0, rho1;
  huber(edge_chi2<9>(E.ei.err, st.info_i), huber_inertial_lba(), &rho0, &rho1);
  E.chi[0] = rho0;
  if (build) edge_weights(E.ei, st.info_i, huber_inertial_lba());
}
GFS_HD void set_walks(const Set& st, const State& prev, const State& cur, SetEdges& E, bool build) {
  random_walk_linearize(prev.bg, cur.bg, E.gr);
  random_walk_linearize(prev.ba, cur.ba, E.ar);
  E.chi[1] = edge_chi2<3>(E.gr.err, st.info_g);
  E.chi[2] = edge_chi2<3>(E.ar.err, st.info_a);
  if (build) {
    edge_weights(E.gr, st.info_g, 0.0);
    edge_weights(E.ar, st.info_a, 0.0);
  }
}
constexpr int kSetAtO = kAtOInertial + 2 * kAtOWalk;
GFS_HD void set_AtO_entry(SetEdges& E, int idx) {
  if (idx < kAtOInertial) return edge_AtO_entry(E.ei, idx);
  idx -= kAtOInertial;
  if (idx < kAtOWalk) return edge_AtO_entry(E.gr, idx);
  edge_AtO_entry(E.ar, idx - kAtOWalk);
}
// What the small edges add to entry (R, C), R >= C, of the 15 N system, sets in insertion order
GFS_HD double small_entry(int N, const SetEdges* E, int R, int C) {
  const int iR = R / 15, r = R % 15, iC = C / 15, c = C % 15;
  double v = 0.0;
  for (int s = iR - 1; s <= iR; s++) {
    if (s < 0 || s >= N) continue;
    int p = set_inertial_column(s, iR, r), q = set_inertial_column(s, iC, c);
    if (p >= 0 && q >= 0) v += edge_H_system(E[s].ei, p, q, inertial_vertex(p), inertial_vertex(q));
    p = set_gyro_column(s, iR, r), q = set_gyro_column(s, iC, c);
    if (p >= 0 && q >= 0) v += edge_H_system(E[s].gr, p, q, rw_vertex(p), rw_vertex(q));
    p = set_acc_column(s, iR, r), q = set_acc_column(s, iC, c);
    if (p >= 0 && q >= 0) v += edge_H_system(E[s].ar, p, q, rw_vertex(p), rw_vertex(q));
  }
  return v;
}
GFS_HD double small_rhs(int N, const SetEdges* E, int R) {
  const int iR = R / 15, r = R % 15;
  double v = 0.0;
  for (int s = iR - 1; s <= iR; s++) {
    if (s < 0 || s >= N) continue;
    int p = set_inertial_column(s, iR, r);
    if (p >= 0) v += edge_b(E[s].ei, p);
    p = set_gyro_column(s, iR, r);
    if (p >= 0) v += edge_b(E[s].gr, p);
    p = set_acc_column(s, iR, r);
    if (p >= 0) v += edge_b(E[s].ar, p);
  }
  return v;
}
// Entry q of key frame i's pose block before its visual edges: q < 21 the packed lower triangle a (a + 1) / 2 + c, then the 6 of b
GFS_HD double pose_block_start(int N, const SetEdges* E, int i, int q) {
  if (q >= 21) return small_rhs(N, E, 15 * i + q - 21);
  int a = 0;
  while ((a + 1) * (a + 2) / 2 <= q) a++;
  return small_entry(N, E, 15 * i + a, 15 * i + q - a * (a + 1) / 2);
}
// Entry (R, C), R >= C, of H before lambda and the Schur terms; vis [N][27]: the pose blocks' finished sums
GFS_HD double system_base(int N, const SetEdges* E, const double* vis, int R, int C) {
  const int iR = R / 15, r = R % 15, iC = C / 15, c = C % 15;
  if (iR == iC && r < 6) return vis[27 * iR + r * (r + 1) / 2 + c];
  return small_entry(N, E, R, C);
}
GFS_HD double rhs_base(int N, const SetEdges* E, const double* vis, int R) {
  return R % 15 < 6 ? vis[27 * (R / 15) + 21 + R % 15] : small_rhs(N, E, R);
}

// ------------------------------------------------------------------------------------------------ rule D
// The packed lower triangle A (row i at i (i + 1) / 2), column k: temp = D L(k, :)', then every row i >= k, then the pivot test, then
// the rows below divided.  The device gives the entries of a step to lanes; every entry is computed by the same text
GFS_HD int64_t tri(int64_t i, int64_t j) { return i * (i + 1) / 2 + j; }
template <class P>
GFS_HD void ldlt_temp(P A, int k, int j, double* temp) { temp[j] = A[tri(j, j)] * A[tri(k, j)]; }
template <class P>
GFS_HD void ldlt_row_packed(P A, int k, int i, const double* temp) {
  if (k == 0) return;
  double acc = 0;
  for (int j = 0; j < k; j++) acc += A[tri(i, j)] * temp[j];
  A[tri(i, k)] -= acc;
}
GFS_HD bool pivot_ok(double d) { return d > 0 && d - d == 0.0; }
// y = b; forward in column order j ascending: y[i] -= L(i, j) y[j]; y[i] /= d_i; backward j descending: y[i] -= L(j, i) y[j]
template <class P>
GFS_HD void ldlt_forward(P A, int j, int i, double* y) { y[i] -= A[tri(i, j)] * y[j]; }
template <class P>
GFS_HD void ldlt_backward(P A, int j, int i, double* y) { y[i] -= A[tri(j, i)] * y[j]; }

// ------------------------------------------------------------------------------------------------ the problem
// The window's camera and one set out of a problem of include/gfs_abi.h (any struct with its field names)
template <class Problem>
inline void fill_calib(const Problem& p, Calib& c) {
  c.fx = p.fx, c.fy = p.fy, c.cx = p.cx, c.cy = p.cy, c.bf = p.bf;
  memcpy(c.Rcb, p.Rcb, sizeof(p.Rcb)), memcpy(c.tcb, p.tcb, sizeof(p.tcb));
  memcpy(c.Rbc, p.Rbc, sizeof(p.Rbc)), memcpy(c.tbc, p.tbc, sizeof(p.tbc));
}
template <class Edge>
inline void fill_set(const Edge& e, bool last, Set& s) {
  memset(&s, 0, sizeof(s));
  memcpy(s.pre.dR, e.dR, sizeof(e.dR)), memcpy(s.pre.dV, e.dV, sizeof(e.dV)), memcpy(s.pre.dP, e.dP, sizeof(e.dP));
  memcpy(s.pre.JRg, e.JRg, sizeof(e.JRg)), memcpy(s.pre.JVg, e.JVg, sizeof(e.JVg)), memcpy(s.pre.JVa, e.JVa, sizeof(e.JVa));
  memcpy(s.pre.JPg, e.JPg, sizeof(e.JPg)), memcpy(s.pre.JPa, e.JPa, sizeof(e.JPa));
  memcpy(s.pre.bg, e.preint_bg, sizeof(e.preint_bg)), memcpy(s.pre.ba, e.preint_ba, sizeof(e.preint_ba));
  s.pre.dT = e.dT;
  for (int k = 0; k < 81; k++) s.info_i[k] = last ? e.info_inertial[k] * kInfoDownLast : e.info_inertial[k];
  memcpy(s.info_g, e.info_gyro_rw, sizeof(s.info_g)), memcpy(s.info_a, e.info_acc_rw, sizeof(s.info_a));
}
template <class ImuState>
inline void fill_state(const ImuState& a, State& s) {
  memcpy(s.Rwb, a.Rwb, sizeof(a.Rwb)), memcpy(s.twb, a.twb, sizeof(a.twb)), memcpy(s.Rcw, a.Rcw, sizeof(a.Rcw));
  memcpy(s.tcw, a.tcw, sizeof(a.tcw)), memcpy(s.v, a.v, sizeof(a.v)), memcpy(s.bg, a.bg, sizeof(a.bg)), memcpy(s.ba, a.ba, sizeof(a.ba));
  s.its = 0, s.pad = 0;
}
// SparseOptimizer::update of key frame i: its four vertices
GFS_HD void keyframe_update(State& s, const Calib& c, const double* x) {
  pose_update(s, c, x);
  add3(s.v, x + 6);
  add3(s.bg, x + 9);
  add3(s.ba, x + 12);
}

}  // namespace gfs_li
