// Optimizer::LocalInertialBA's numeric core (reference src/Optimizer.cc:3589-3626) as ONE sequential loop over one problem of
// include/gfs_abi.h section 20: what gfs_lba_inertial_solve is held to, byte for byte.  The arithmetic is
// geoflowslam_amd/csrc/lba_inertial_rule.hpp's; the loops below are written the way g2o runs them -- edge after edge, trial after
// trial -- and share nothing with the kernels (csrc/lba_inertial.hip).
// Built by tests/lba_inertial_support.py: g++ -O2 -std=c++17 -ffp-contract=off -shared.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../geoflowslam_amd/csrc/lba_inertial_rule.hpp"
#include "../../include/gfs_abi.h"

using namespace gfs_li;

extern "C" {

// What the tests look at besides the solution.  Every pointer may be NULL
struct LirTrace {
  int32_t cap;             // rows of the per-trial arrays
  int32_t* n_trials;       // [1] rows written
  double* lambda;          // [cap] the lambda the trial was solved with
  double* temp_chi;        // [cap] tempChi (DBL_MAX after a failed solve)
  double* rho;             // [cap]
  int32_t* accepted;       // [cap]
  int32_t* ok2;            // [cap]
  int32_t* iteration;      // [cap] the iteration the trial belongs to
  // the first trial's linear step
  double* vis_err;         // [n_edges][3]
  double* edge_rho;        // [n_edges][2] rho0, rho1
  double* small_err;       // [n_opt][15] inertial 9, gyro 3, acc 3
  double* small_chi;       // [n_opt][3]
  double* Hll;             // [n_points][6]
  double* bl;              // [n_points][3]
  double* Hpl;             // [n_edges][18]
  double* H;               // [D][D] both triangles, before lambda and the Schur terms
  double* b;               // [D]
  double* M;               // [D][D] the reduced system, both triangles
  double* bs;              // [D]
  double* dx;              // [D]
  double* dxl;             // [n_points][3]
  double* trial_state;     // [n_opt][21] Rwb twb v bg ba after the first trial's update
  double* trial_chi;       // [1] the robust chi2 at the first trial's state
};

}  // extern "C"

namespace {

struct Solver {
  const gfs_lba_inertial_problem& p;
  int N, F, P, E, D;
  Calib cam;
  std::vector<Set> sets;
  std::vector<State> cur, trial;            // [N + 1]: N is prev
  std::vector<double> pts, pts_trial;       // [P][3]
  std::vector<SetEdges> se, se_trial;
  std::vector<double> echi2, Hll, bl, Hpl, T, vis, Y, inv, bfull, M, bs, x, xl, cp;
  std::vector<double> err3, rho01;
  std::vector<std::vector<int>> kf_edges;  // a window key frame's edges, ascending
  Ctl ctl;

  explicit Solver(const gfs_lba_inertial_problem& pp) : p(pp) {
    N = p.n_opt, F = p.n_fixed, P = p.n_points, E = p.n_edges, D = 15 * N;
    fill_calib(p, cam);
    sets.resize(N);
    for (int i = 0; i < N; i++) fill_set(p.inertial[i], i == N - 1, sets[i]);
    cur.resize(N + 1);
    for (int i = 0; i < N; i++) fill_state(p.window[i], cur[i]);
    fill_state(p.prev, cur[N]);
    trial = cur;
    pts.assign(p.points, p.points + (size_t)3 * P);
    pts_trial = pts;
    se.resize(N), se_trial.resize(N);
    echi2.assign(E, 0.0), Hll.assign((size_t)6 * P, 0.0), bl.assign((size_t)3 * P, 0.0), Hpl.assign((size_t)18 * E, 0.0);
    T.assign((size_t)27 * E, 0.0), vis.assign((size_t)27 * N, 0.0), Y.assign((size_t)24 * E, 0.0), inv.assign((size_t)9 * P, 0.0);
    bfull.assign(D, 0.0), M.assign((size_t)tri(D, 0), 0.0), bs.assign(D, 0.0), x.assign(D, 0.0), xl.assign((size_t)3 * P, 0.0);
    err3.assign((size_t)3 * E, 0.0), rho01.assign((size_t)2 * E, 0.0);
    kf_edges.resize(N);
    for (int e = 0; e < E; e++)
      if (p.edge_kf[e] < N) kf_edges[p.edge_kf[e]].push_back(e);
    lm_init(ctl, p.lambda_init);
  }
  void camera(const std::vector<State>& st, int kf, const double*& Rcw, const double*& tcw) const {
    if (kf <= N) Rcw = st[kf].Rcw, tcw = st[kf].tcw;
    else Rcw = p.fixed_Rcw + 9 * (size_t)(kf - N - 1), tcw = p.fixed_tcw + 3 * (size_t)(kf - N - 1);
  }
  // computeActiveErrors + activeRobustChi2 at a state; with build, linearizeOplus and constructQuadraticForm too
  double evaluate(const std::vector<State>& st, const std::vector<double>& xw, std::vector<SetEdges>& S, bool build) {
    double total = 0.0;
    for (int s = 0; s < N; s++) {
      set_inertial(sets[s], st[s + 1], st[s], S[s], build);
      set_walks(sets[s], st[s + 1], st[s], S[s], build);
      if (build)
        for (int idx = 0; idx < kSetAtO; idx++) set_AtO_entry(S[s], idx);
      for (int k = 0; k < 3; k++) total += S[s].chi[k];
    }
    double slab[kChunk];
    for (int base = 0; base < P; base += kChunk) {
      for (int t = 0; t < kChunk; t++) {
        const int l = base + t;
        double part = 0.0;
        if (l < P) {
          double hl[9];
          for (int k = 0; k < 9; k++) hl[k] = 0.0;
          for (int e = p.point_edge_begin[l]; e < p.point_edge_begin[l + 1]; e++) {
            const int kf = p.edge_kf[e];
            const bool stv = p.stereo[e] != 0;
            const double w = (double)p.inv_sigma2[e];
            const double *Rcw, *tcw;
            camera(st, kf, Rcw, tcw);
            double er[3], rho0, rho1;
            vis_error(cam, Rcw, tcw, &xw[3 * (size_t)l], p.obs + 3 * (size_t)e, stv, er);
            const double c2 = vis_chi2(er, w, stv);
            huber(c2, huber_delta_visual(stv), &rho0, &rho1);
            echi2[e] = c2;
            part += rho0;
            if (!build) continue;
            for (int k = 0; k < 3; k++) err3[3 * (size_t)e + k] = er[k];
            rho01[2 * (size_t)e] = rho0, rho01[2 * (size_t)e + 1] = rho1;
            double Jl[9], t9[9];
            vis_point_jacobian(cam, Rcw, tcw, &xw[3 * (size_t)l], stv, Jl);
            vis_point_form(Jl, w, stv, rho1, er, t9);
            for (int k = 0; k < 9; k++) hl[k] += t9[k];
            if (kf < N) {
              double Jp[18], acc[kSys], H18[18];
              vis_jacobian(cam, Rcw, tcw, &xw[3 * (size_t)l], stv, Jp);
              vis_quadratic_form(Jp, w, stv, rho1, er, acc);
              vis_hpl(Jp, Jl, w, stv, rho1, H18);
              for (int k = 0; k < kSys; k++) T[27 * (size_t)e + k] = acc[k];
              for (int k = 0; k < 18; k++) Hpl[18 * (size_t)e + k] = H18[k];
            }
          }
          if (build) {
            for (int k = 0; k < 6; k++) Hll[6 * (size_t)l + k] = hl[k];
            for (int k = 0; k < 3; k++) bl[3 * (size_t)l + k] = hl[6 + k];
          }
        }
        slab[t] = part;
      }
      total += chunk_tree(slab);
    }
    if (build) {  // the pose blocks: the small edges first, then the key frame's visual edges in edge order
      for (int i = 0; i < N; i++)
        for (int q = 0; q < 27; q++) {
          double run = pose_block_start(N, se.data(), i, q);
          for (int e : kf_edges[i]) run += T[27 * (size_t)e + q];
          vis[27 * (size_t)i + q] = run;
        }
    }
    return total;
  }
  // setLambda + solve + update + computeActiveErrors: returns the raw robust chi2 at the trial state, the raw computeScale in *scale
  double trial_step(double* scale, LirTrace* t, bool dump) {
    const double lambda = ctl.lambda;
    for (int l = 0; l < P; l++) {
      inverse3(&Hll[6 * (size_t)l], lambda, &inv[9 * (size_t)l]);
      for (int e = p.point_edge_begin[l]; e < p.point_edge_begin[l + 1]; e++)
        if (p.edge_kf[e] < N) vis_y(&Hpl[18 * (size_t)e], &inv[9 * (size_t)l], &bl[3 * (size_t)l], &Y[24 * (size_t)e]);
    }
    for (int R = 0; R < D; R++) {
      for (int C = 0; C <= R; C++) {
        double v = system_base(N, se.data(), vis.data(), R, C);
        if (dump && t->H) t->H[(size_t)D * R + C] = t->H[(size_t)D * C + R] = v;
        if (R == C) v += lambda;
        M[tri(R, C)] = v;
      }
      bfull[R] = bs[R] = rhs_base(N, se.data(), vis.data(), R);
    }
    for (int l = 0; l < P; l++)  // the Schur terms, landmark by landmark, e1 then e2
      for (int e1 = p.point_edge_begin[l]; e1 < p.point_edge_begin[l + 1]; e1++) {
        const int i = p.edge_kf[e1];
        if (i >= N) continue;
        for (int e2 = p.point_edge_begin[l]; e2 < p.point_edge_begin[l + 1]; e2++) {
          const int j = p.edge_kf[e2];
          if (j >= N || j > i) continue;
          for (int a = 0; a < 6; a++)
            for (int c = 0; c < 6; c++)
              if (15 * i + a >= 15 * j + c) M[tri(15 * i + a, 15 * j + c)] -= schur_term(&Y[24 * (size_t)e1], &Hpl[18 * (size_t)e2], a, c);
        }
        for (int a = 0; a < 6; a++) bs[15 * i + a] -= Y[24 * (size_t)e1 + 18 + a];
      }
    if (dump) {
      for (int R = 0; R < D && t->M; R++)
        for (int C = 0; C <= R; C++) t->M[(size_t)D * R + C] = t->M[(size_t)D * C + R] = M[tri(R, C)];
      if (t->bs) memcpy(t->bs, bs.data(), D * sizeof(double));
      if (t->b) memcpy(t->b, bfull.data(), D * sizeof(double));
    }
    // rule D
    std::vector<double> temp(D);
    bool ok = true;
    for (int k = 0; k < D && ok; k++) {
      for (int j = 0; j < k; j++) ldlt_temp(M.data(), k, j, temp.data());
      for (int i = k; i < D; i++) ldlt_row_packed(M.data(), k, i, temp.data());
      const double d = M[tri(k, k)];
      if (!pivot_ok(d)) ok = false;
      else
        for (int i = k + 1; i < D; i++) M[tri(i, k)] /= d;
    }
    ctl.ok2 = ok ? 1 : 0;
    if (ok) {
      for (int i = 0; i < D; i++) x[i] = bs[i];
      for (int j = 0; j < D; j++)
        for (int i = j + 1; i < D; i++) ldlt_forward(M.data(), j, i, x.data());
      for (int i = 0; i < D; i++) x[i] /= M[tri(i, i)];
      for (int j = D - 1; j >= 0; j--)
        for (int i = 0; i < j; i++) ldlt_backward(M.data(), j, i, x.data());
    } else {
      for (int i = 0; i < D; i++) x[i] = 0.0;  // rule F
    }
    double sc = 0.0;
    for (int j = 0; j < D; j++) sc += x[j] * (lambda * x[j] + bfull[j]);
    trial = cur;
    for (int i = 0; i < N; i++) keyframe_update(trial[i], cam, &x[15 * (size_t)i]);
    double slab[kChunk];
    for (int base = 0; base < P; base += kChunk) {
      for (int tt = 0; tt < kChunk; tt++) {
        const int l = base + tt;
        double part = 0.0;
        if (l < P) {
          double c3[3] = {bl[3 * (size_t)l], bl[3 * (size_t)l + 1], bl[3 * (size_t)l + 2]}, d3[3] = {0.0, 0.0, 0.0};
          if (ok) {
            for (int e = p.point_edge_begin[l]; e < p.point_edge_begin[l + 1]; e++)
              if (p.edge_kf[e] < N) back_edge(&Hpl[18 * (size_t)e], &x[15 * (size_t)p.edge_kf[e]], c3);
            mv3(&inv[9 * (size_t)l], c3, d3);
          }
          for (int k = 0; k < 3; k++) {
            xl[3 * (size_t)l + k] = d3[k];
            pts_trial[3 * (size_t)l + k] = pts[3 * (size_t)l + k] + d3[k];
            part += d3[k] * (lambda * d3[k] + bl[3 * (size_t)l + k]);
          }
        }
        slab[tt] = part;
      }
      sc += chunk_tree(slab);
    }
    *scale = sc;
    return evaluate(trial, pts_trial, se_trial, false);
  }
};

}  // namespace

extern "C" {

int lir_solve(const gfs_lba_inertial_problem* pp, gfs_lba_inertial_solution* S, LirTrace* t) {
  const gfs_lba_inertial_problem& p = *pp;
  if (p.n_opt < 1 || p.iterations < 0 || p.n_points < 0 || p.n_edges < 0 || p.n_fixed < 0) return GFS_ERR_INVALID_ARG;
  Solver s(p);
  Ctl& c = s.ctl;
  int row = 0;
  for (int it = 0; it < p.iterations || it == 0; it++) {
    const double total = s.evaluate(s.cur, s.pts, s.se, true);
    lm_begin_iteration(c, total, it < p.iterations);
    if (it == 0 && t) {
      if (t->vis_err) memcpy(t->vis_err, s.err3.data(), s.err3.size() * sizeof(double));
      if (t->edge_rho) memcpy(t->edge_rho, s.rho01.data(), s.rho01.size() * sizeof(double));
      if (t->Hll) memcpy(t->Hll, s.Hll.data(), s.Hll.size() * sizeof(double));
      if (t->bl) memcpy(t->bl, s.bl.data(), s.bl.size() * sizeof(double));
      if (t->Hpl) memcpy(t->Hpl, s.Hpl.data(), s.Hpl.size() * sizeof(double));
      for (int i = 0; i < s.N; i++) {
        if (t->small_err) {
          memcpy(t->small_err + 15 * i, s.se[i].ei.err, 9 * sizeof(double));
          memcpy(t->small_err + 15 * i + 9, s.se[i].gr.err, 3 * sizeof(double));
          memcpy(t->small_err + 15 * i + 12, s.se[i].ar.err, 3 * sizeof(double));
        }
        if (t->small_chi) memcpy(t->small_chi + 3 * i, s.se[i].chi, 3 * sizeof(double));
      }
    }
    while (c.iter_open) {
      const double lambda = c.lambda;
      const bool dump = t && row == 0;
      double scale;
      const double temp = s.trial_step(&scale, t, dump);
      if (dump) {
        if (t->dx) memcpy(t->dx, s.x.data(), s.D * sizeof(double));
        if (t->dxl) memcpy(t->dxl, s.xl.data(), s.xl.size() * sizeof(double));
        if (t->trial_chi) t->trial_chi[0] = temp;
        for (int i = 0; i < s.N && t->trial_state; i++) {
          const State& st = s.trial[i];
          double* o = t->trial_state + 21 * i;
          memcpy(o, st.Rwb, 72), memcpy(o + 9, st.twb, 24), memcpy(o + 12, st.v, 24), memcpy(o + 15, st.bg, 24), memcpy(o + 18, st.ba, 24);
        }
      }
      const bool accepted = lm_trial(c, temp, scale);
      if (accepted) s.cur = s.trial, s.pts = s.pts_trial;
      if (t && row < t->cap) {
        if (t->lambda) t->lambda[row] = lambda;
        if (t->temp_chi) t->temp_chi[row] = c.ok2 ? temp : DBL_MAX;
        if (t->rho) t->rho[row] = c.rho;
        if (t->accepted) t->accepted[row] = accepted;
        if (t->ok2) t->ok2[row] = c.ok2;
        if (t->iteration) t->iteration[row] = it;
      }
      row++;
    }
    if (c.done) break;
  }
  if (t && t->n_trials) t->n_trials[0] = row;
  for (int i = 0; i < s.N; i++) {
    const State& st = s.cur[i];
    gfs_imu_state& o = S->window[i];
    memcpy(o.Rwb, st.Rwb, sizeof(o.Rwb)), memcpy(o.twb, st.twb, sizeof(o.twb)), memcpy(o.Rcw, st.Rcw, sizeof(o.Rcw));
    memcpy(o.tcw, st.tcw, sizeof(o.tcw)), memcpy(o.v, st.v, sizeof(o.v)), memcpy(o.bg, st.bg, sizeof(o.bg)), memcpy(o.ba, st.ba, sizeof(o.ba));
  }
  for (int l = 0; l < s.P; l++) {
    for (int k = 0; k < 3; k++) S->points[3 * (size_t)l + k] = s.pts[3 * (size_t)l + k];
    for (int e = p.point_edge_begin[l]; e < p.point_edge_begin[l + 1]; e++) {
      const double *Rcw, *tcw;
      s.camera(s.cur, p.edge_kf[e], Rcw, tcw);
      const bool dp = vis_depth_positive(Rcw, tcw, &s.pts[3 * (size_t)l]);
      S->edge_chi2[e] = s.echi2[e];
      S->edge_depth_positive[e] = dp ? 1 : 0;
      S->edge_erase[e] = (p.stereo[e] ? erase_stereo(s.echi2[e]) : erase_mono(s.echi2[e], p.close[e] != 0, dp)) ? 1 : 0;
    }
  }
  S->err = (float)c.first_total;
  S->err_end = (float)c.last_total;
  S->iterations_run = c.iterations_run;
  S->trials_run = c.trials_run;
  S->final_lambda = c.lambda;
  return GFS_OK;
}

void lir_constants(double* out) {
  int o = 0;
  out[o++] = kMaxWindow, out[o++] = kMaxWindowLarge, out[o++] = kOptIt, out[o++] = kOptItLarge, out[o++] = kLambdaInit, out[o++] = kLambdaInitLarge;
  out[o++] = huber_inertial_lba(), out[o++] = kInfoDownLast, out[o++] = kChi2Mono2, out[o++] = kChi2Stereo2, out[o++] = kCloseFactor;
  out[o++] = kTrackDepthClose, out[o++] = kMaxFixKF, out[o++] = kMaxCovKF, out[o++] = kFailGateFactor, out[o++] = kMaxTrials;
  out[o++] = huber_delta_visual(false), out[o++] = huber_delta_visual(true), out[o++] = kChunk, out[o++] = kLdsRows;  // 20 values
}

}  // extern "C"
