// Optimizer::PoseInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:5899-6283, 6762-7171) as ONE sequential
// loop over one problem of include/gfs_abi.h section 19: what gfs_pose_inertial_optimize is held to, byte for byte.  The arithmetic
// is geoflowslam_amd/csrc/pose_inertial_rule.hpp's; the loops below are written the way the reference runs them -- edge after edge,
// iteration after iteration -- and share nothing with the kernel (csrc/pose_inertial.hip).
// Built by tests/pose_inertial_support.py: g++ -O2 -std=c++17 -ffp-contract=off -shared.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../geoflowslam_amd/csrc/pose_inertial_rule.hpp"
#include "../../include/gfs_abi.h"

using namespace gfs_pi;

namespace {

struct VisEdge {
  double err[3];
  int level, outlier;
};

// What the tests look at besides the solution.  Every pointer may be NULL
struct Trace {
  double* round_chi2;      // [4][n] the chi2 (double) the re-classification read for every edge
  uint8_t* round_fresh;    // [4][n] 1 where it was re-computed first (the edge was an outlier)
  double* pose_before;     // [4][12] Rcw, tcw of the current frame before the round's last update
  double* pose_after;      // [4][12] ... after it
  float* chi2_imu;         // [4] chi2IMU as the round read it (key-frame mode)
  double* info_scale;      // [4] info_i[0] / the problem's info_inertial[0] after the round
  int32_t* iterations;     // [4] Gauss-Newton iterations the round ran
  int32_t* solve_failed;   // [4] 1 where the round ended on a failed solve
  int32_t* recovery_ran;   // [1]
};

void build_system(const Head& h, const gfs_pose_inertial_problem& p, Persist& P, Work& W, std::vector<VisEdge>& ve, bool robust) {
  const int n = h.n_obs;
  double sums[kSys];
  for (int k = 0; k < kSys; k++) sums[k] = 0.0;
  for (int e = 0; e < n; e++) {
    double term[kSys];
    for (int k = 0; k < kSys; k++) term[k] = 0.0;
    if (ve[e].level == 0) {
      const bool st = p.stereo[e] != 0;
      const double w = (double)p.inv_sigma2[e];
      vis_error(h.cam, P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e, p.obs + 3 * e, st, ve[e].err);  // computeActiveErrors
      double J[18], rho0, rho1 = 1.0;
      vis_jacobian(h.cam, P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e, st, J);
      if (robust) huber(vis_chi2(ve[e].err, w, st), huber_delta_visual(st), &rho0, &rho1);
      vis_quadratic_form(J, w, st, rho1, ve[e].err, term);
    }
    for (int k = 0; k < kSys; k++) sums[k] += term[k];
  }
  for (int k = 0; k < kSys; k++) P.vis[k] = sums[k];
  for (int which = 0; which < 4; which++) small_edge_linearize(h, P, W, which, true);
  for (int idx = 0; idx < kAtOEntries; idx++) small_edge_AtO_entry(h.mode, W, idx);
  for (int R = 0; R < P.D; R++) {
    for (int C = 0; C <= R; C++) W.A[kLd * R + C] = system_entry(h.mode, P, W, R, C);
    W.b[R] = system_rhs(h.mode, P, W, R);
  }
}

bool solve_system(Persist& P, Work& W) {
  const int N = P.D;
  W.sign = 0;
  for (int k = 0; k < N; k++) {
    ldlt_pivot(W.A, N, k, W.tr, W.temp);
    for (int i = k; i < N; i++) ldlt_row(W.A, k, i, W.temp);
    for (int i = k + 1; i < N; i++) ldlt_scale(W.A, k, i);
    ldlt_sign(W.A, k, &W.sign);
  }
  if (W.sign != 1) return false;
  ldlt_substitute(W.A, N, W.tr, W.b, W.y, P.x);
  return true;
}

void snapshot(const Persist& P, double* out) {
  if (!out) return;
  memcpy(out, P.s[0].Rcw, 9 * sizeof(double));
  memcpy(out + 9, P.s[0].tcw, 3 * sizeof(double));
}

void estimate_out(const State& s, gfs_imu_estimate& o) {
  memcpy(o.Rwb, s.Rwb, sizeof(o.Rwb)), memcpy(o.twb, s.twb, sizeof(o.twb)), memcpy(o.v, s.v, sizeof(o.v));
  memcpy(o.bg, s.bg, sizeof(o.bg)), memcpy(o.ba, s.ba, sizeof(o.ba));
}

}  // namespace

extern "C" {

int pir_optimize(const gfs_pose_inertial_problem* pp, gfs_pose_inertial_solution* S, Trace* t) {
  const gfs_pose_inertial_problem& p = *pp;
  if (p.n_obs < 0 || p.n_rounds < 1 || p.n_rounds > kMaxRounds || (p.mode != kKeyFrame && p.mode != kFrame)) return GFS_ERR_INVALID_ARG;
  Head h;
  fill_head(p, h);
  Persist P;
  persist_init(h, P);
  static thread_local Work W;
  const int n = h.n_obs;
  std::vector<VisEdge> ve(n);
  for (auto& e : ve) e.err[0] = e.err[1] = e.err[2] = 0.0, e.level = 0, e.outlier = 0;
  bool robust = true;
  int nBad = 0, nInliers = 0, rounds_run = 0;
  float avg = 0.0f;
  for (int it = 0; it < h.n_rounds; it++) {
    P.ok = 1;
    int iters = 0;
    for (int i = 0; i < kIterations && P.ok; i++) {
      build_system(h, p, P, W, ve, robust);
      if (!solve_system(P, W)) P.ok = 0;  // x keeps what it held
      if (t) snapshot(P, t->pose_before ? t->pose_before + 12 * it : nullptr);
      for (int part = 0; part < 4; part++) update_part(h, P, part);
      iters++;
    }
    if (t) snapshot(P, t->pose_after ? t->pose_after + 12 * it : nullptr);
    if (t && t->iterations) t->iterations[it] = iters;
    if (t && t->solve_failed) t->solve_failed[it] = !P.ok;
    if (t && t->chi2_imu) t->chi2_imu[it] = (float)edge_chi2<9>(P.err_i, P.info_i);
    inertial_after_round(h, P);
    if (t && t->info_scale) t->info_scale[it] = P.info_i[0] / h.info_i[0];
    // the re-classification: the mono list, then the stereo list; the float sum of the inliers' chi2 in that order
    nBad = 0, nInliers = 0, avg = 0.0f;
    for (int pass = 0; pass < 2; pass++)
      for (int e = 0; e < n; e++) {
        const bool st = p.stereo[e] != 0;
        float term = 0.0f;
        if (st == (pass == 1)) {
          if (ve[e].outlier) vis_error(h.cam, P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e, p.obs + 3 * e, st, ve[e].err);
          const double c2 = vis_chi2(ve[e].err, (double)p.inv_sigma2[e], st);
          if (t && t->round_chi2) t->round_chi2[(size_t)it * n + e] = c2;
          if (t && t->round_fresh) t->round_fresh[(size_t)it * n + e] = ve[e].outlier ? 1 : 0;
          const float chi2 = (float)c2;
          const bool bad = st ? stereo_is_outlier(chi2, it)
                              : mono_is_outlier(chi2, p.close[e] != 0, vis_depth_positive(P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e), h.mode, it);
          ve[e].outlier = ve[e].level = bad ? 1 : 0;
          if (bad) nBad++;
          else nInliers++, term = chi2;
        }
        avg += term;
      }
    avg /= (float)nInliers;
    if (it == 2) robust = false;
    rounds_run = it + 1;
    if (edge_count(h.mode, n) < kMinEdges) break;
  }
  // recover not too bad points
  if (t && t->recovery_ran) t->recovery_ran[0] = 0;
  if (nInliers < kFewInliers && !h.rec_init) {
    if (t && t->recovery_ran) t->recovery_ran[0] = 1;
    nBad = 0;
    for (int pass = 0; pass < 2; pass++)
      for (int e = 0; e < n; e++) {
        const bool st = p.stereo[e] != 0;
        if (st != (pass == 1)) continue;
        vis_error(h.cam, P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e, p.obs + 3 * e, st, ve[e].err);
        if (vis_chi2(ve[e].err, (double)p.inv_sigma2[e], st) < (st ? kChi2StereoOut : kChi2MonoOut)) ve[e].outlier = 0;
        else nBad++;
      }
  }
  // the Hessian of the new prior, re-linearised at the final state
  for (int which = 0; which < 4; which++) small_edge_linearize(h, P, W, which, false);
  for (int idx = 0; idx < kAtOEntries; idx++) small_edge_AtO_entry(h.mode, W, idx);
  const int Dh = P.D, off = hessian_visual_offset(h.mode);
  for (int i = 0; i < 900; i++) S->H[i] = 0.0;
  for (int R = 0; R < Dh; R++)
    for (int C = 0; C < Dh; C++) S->H[Dh * R + C] = hessian_entry(h.mode, W, R, C);
  for (int pass = 0; pass < 2; pass++)
    for (int e = 0; e < n; e++) {
      const bool st = p.stereo[e] != 0, in = st == (pass == 1) && !ve[e].outlier;
      double J[18];
      if (in) vis_jacobian(h.cam, P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e, st, J);
      for (int a = 0; a < 6; a++)
        for (int c = 0; c < 6; c++) S->H[Dh * (off + a) + off + c] += in ? vis_hessian_entry(J, (double)p.inv_sigma2[e], st, a, c) : 0.0;
    }
  estimate_out(P.s[0], S->cur);
  estimate_out(P.s[1], S->other);
  for (int e = 0; e < n; e++) S->outlier[e] = (uint8_t)ve[e].outlier;
  S->n_good = n - nBad;
  S->n_inliers = nInliers;
  S->rounds_run = rounds_run;
  S->avg_reproj = avg;
  return GFS_OK;
}

// B problems one after the other on the calling thread (tools/bench_pose_inertial.py times this)
int pir_optimize_batch(const gfs_pose_inertial_problem* pp, int B, gfs_pose_inertial_solution* S) {
  for (int f = 0; f < B; f++)
    if (int rc = pir_optimize(pp + f, S + f, nullptr)) return rc;
  return GFS_OK;
}

// One Gauss-Newton step from the problem's state, every edge active, the kernels on: dx [D], the assembled matrix [D][D] (both
// triangles), b [D], the error vector and chi2 of every visual edge ([n][3], [n]) and of the four small edges (err [9 + 3 + 3 + 15],
// chi2 [4]).  Returns 1 when the LDLT was positive
int pir_gn_step(const gfs_pose_inertial_problem* pp, double* dx, double* Hs, double* b, double* vis_err, double* vis_c2, double* small_err,
                double* small_c2) {
  const gfs_pose_inertial_problem& p = *pp;
  Head h;
  fill_head(p, h);
  Persist P;
  persist_init(h, P);
  static thread_local Work W;
  std::vector<VisEdge> ve(h.n_obs);
  for (auto& e : ve) e.level = 0, e.outlier = 0;
  build_system(h, p, P, W, ve, true);
  const int D = P.D;
  for (int R = 0; R < D; R++) {
    for (int C = 0; C <= R; C++) Hs[D * R + C] = Hs[D * C + R] = W.A[kLd * R + C];
    b[R] = W.b[R];
  }
  for (int e = 0; e < h.n_obs; e++) {
    for (int k = 0; k < 3; k++) vis_err[3 * e + k] = ve[e].err[k];
    vis_c2[e] = vis_chi2(ve[e].err, (double)p.inv_sigma2[e], p.stereo[e] != 0);
  }
  memcpy(small_err, W.ei.err, 9 * sizeof(double)), memcpy(small_err + 9, W.gr.err, 3 * sizeof(double));
  memcpy(small_err + 12, W.ar.err, 3 * sizeof(double));
  small_c2[0] = edge_chi2<9>(W.ei.err, h.info_i), small_c2[1] = edge_chi2<3>(W.gr.err, h.info_g), small_c2[2] = edge_chi2<3>(W.ar.err, h.info_a);
  small_c2[3] = 0.0;
  for (int k = 0; k < 15; k++) small_err[15 + k] = h.mode == kFrame ? W.ep.err[k] : 0.0;
  if (h.mode == kFrame) small_c2[3] = edge_chi2<15>(W.ep.err, h.prior.H);
  const bool ok = solve_system(P, W);
  for (int k = 0; k < D; k++) dx[k] = P.x[k];
  return ok ? 1 : 0;
}

// The Hessian of the new prior at the problem's state with every edge an inlier: [D][D]
void pir_final_hessian(const gfs_pose_inertial_problem* pp, double* H) {
  const gfs_pose_inertial_problem& p = *pp;
  Head h;
  fill_head(p, h);
  Persist P;
  persist_init(h, P);
  static thread_local Work W;
  for (int which = 0; which < 4; which++) small_edge_linearize(h, P, W, which, false);
  for (int idx = 0; idx < kAtOEntries; idx++) small_edge_AtO_entry(h.mode, W, idx);
  const int Dh = P.D, off = hessian_visual_offset(h.mode);
  for (int R = 0; R < Dh; R++)
    for (int C = 0; C < Dh; C++) H[Dh * R + C] = hessian_entry(h.mode, W, R, C);
  for (int pass = 0; pass < 2; pass++)
    for (int e = 0; e < h.n_obs; e++) {
      const bool st = p.stereo[e] != 0;
      if (st != (pass == 1)) continue;
      double J[18];
      vis_jacobian(h.cam, P.s[0].Rcw, P.s[0].tcw, p.xw + 3 * e, st, J);
      for (int a = 0; a < 6; a++)
        for (int c = 0; c < 6; c++) H[Dh * (off + a) + off + c] += vis_hessian_entry(J, (double)p.inv_sigma2[e], st, a, c);
    }
}

// ---- the written rules alone
void pir_nearest_rotation(const double* in, double* out) {
  memcpy(out, in, 9 * sizeof(double));
  nearest_rotation(out);
}
void pir_nearest_rotation_f(const float* in, float* out) {
  memcpy(out, in, 9 * sizeof(float));
  nearest_rotation_f(out);
}
void pir_exp_so3f(const float* v, float* R) { exp_so3f(v, R); }
void pir_exp_so3(const double* w, double* R) { exp_so3(w, R); }
void pir_log_so3(const double* R, double* w) { log_so3(R, w); }
void pir_acos(const double* x, double* y, int64_t n) {
  for (int64_t i = 0; i < n; i++) y[i] = acos_rule(x[i]);
}
void pir_sincos(const double* x, double* s, double* c, int64_t n) {
  for (int64_t i = 0; i < n; i++) s[i] = sin_rule(x[i]), c[i] = cos_rule(x[i]);
}
void pir_inverse_right_jacobian(const double* v, double* J) { inverse_right_jacobian(v, J); }
void pir_right_jacobian(const double* v, double* J) { right_jacobian(v, J); }
void pir_pose_update(const gfs_pose_inertial_problem* pp, const double* u, int times, double* Rwb, double* twb, double* Rcw, double* tcw) {
  Head h;
  fill_head(*pp, h);
  State s = h.cur;
  s.its = 0;
  for (int k = 0; k < times; k++) pose_update(s, h.cam, u + 6 * k);
  memcpy(Rwb, s.Rwb, sizeof(s.Rwb)), memcpy(twb, s.twb, sizeof(s.twb)), memcpy(Rcw, s.Rcw, sizeof(s.Rcw)), memcpy(tcw, s.tcw, sizeof(s.tcw));
}
void pir_preint_deltas(const gfs_pose_inertial_problem* pp, const double* bg, const double* ba, double* dR, double* dV, double* dP) {
  Head h;
  fill_head(*pp, h);
  double dbg[3];
  preint_deltas(h.pre, bg, ba, dR, dV, dP, dbg);
}
// The dense solve alone: A [N][N] symmetric, b [N] -> x; returns isPositive()
int pir_ldlt(const double* Ain, const double* b, int N, double* x) {
  Persist P;
  static thread_local Work W;
  P.D = N;
  for (int k = 0; k < 30; k++) P.x[k] = 0.0;
  for (int R = 0; R < N; R++)
    for (int C = 0; C < N; C++) W.A[kLd * R + C] = Ain[N * R + C];
  for (int R = 0; R < N; R++) W.b[R] = b[R];
  const bool ok = solve_system(P, W);
  for (int k = 0; k < N; k++) x[k] = P.x[k];
  return ok ? 1 : 0;
}

void pir_constants(double* out) {
  int o = 0;
  for (int it = 0; it < 4; it++) out[o++] = chi2_mono_gate(kKeyFrame, it);
  for (int it = 0; it < 4; it++) out[o++] = chi2_mono_gate(kFrame, it);
  for (int it = 0; it < 4; it++) out[o++] = chi2_stereo_gate(it);
  out[o++] = kHuberInertial, out[o++] = kHuberInertialWeak, out[o++] = kHuberPrior, out[o++] = kChi2ImuGate, out[o++] = kInfoDown;
  out[o++] = kChi2MonoOut, out[o++] = kChi2StereoOut, out[o++] = kFewInliers, out[o++] = kMinEdges, out[o++] = kIterations;
  out[o++] = kSmallAngle, out[o++] = kGravity;
  for (int k = 0; k < 3; k++) out[o++] = dbg_replacement(k);
  out[o++] = huber_delta_visual(false), out[o++] = huber_delta_visual(true), out[o++] = kNormalizeEvery, out[o++] = kTrackDepthClose;  // 32 values
}

}  // extern "C"
