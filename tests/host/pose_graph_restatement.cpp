// Host build of geoflowslam_amd/csrc/sim3_dev.hpp (g++, -ffp-contract=off) for tests/test_pose_graph_restatement.py: the arithmetic the
// device runs, called on batches and compared bit for bit with the numpy float64 restatement (tests/pose_graph_support.py); and
// pgr_optimize, a sequential host statement of gfs_essential_graph_optimize on the same structs (dense system, dense L D L^T), which
// tests/host/essential_graph_adaptor_test.cpp uses as the adaptor's solve.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../geoflowslam_amd/csrc/sim3_dev.hpp"
#include "../../include/gfs_abi.h"

using namespace gfs_sim3;

extern "C" {

void pgr_constants(double* out /* eps, numeric delta */) {
  out[0] = kEps;
  out[1] = kNumericDelta;
}
void pgr_exp(int n, const double* u, double* S, int32_t* branch) {
  for (int k = 0; k < n; k++) branch[k] = sim3_exp(u + 7 * k, S + 8 * k);
}
void pgr_log(int n, const double* S, double* u, int32_t* branch) {
  for (int k = 0; k < n; k++) branch[k] = sim3_log(S + 8 * k, u + 7 * k);
}
void pgr_mul(int n, const double* a, const double* b, double* o) {
  for (int k = 0; k < n; k++) sim3_mul(a + 8 * k, b + 8 * k, o + 8 * k);
}
void pgr_inverse(int n, const double* a, double* o) {
  for (int k = 0; k < n; k++) sim3_inverse(a + 8 * k, o + 8 * k);
}
void pgr_map(int n, const double* a, const double* xyz, double* o) {
  for (int k = 0; k < n; k++) sim3_map(a + 8 * k, xyz + 3 * k, o + 3 * k);
}
void pgr_oplus(int n, const double* est, const double* upd, int fix_scale, double* o) {
  for (int k = 0; k < n; k++) sim3_oplus(est + 8 * k, upd + 7 * k, fix_scale != 0, o + 8 * k);
}
void pgr_residual(int n, const double* C, const double* v0, const double* v1, double* err, int32_t* branch) {
  for (int k = 0; k < n; k++) branch[k] = sim3_edge_residual(C + 8 * k, v0 + 8 * k, v1 + 8 * k, err + 7 * k);
}

}  // extern "C"

// linearizeOplus of one edge: J [7][dim] row-major with row stride 7, of vertex `side`
static void numeric_jacobian(const double* C, const double* v0, const double* v1, int side, bool fix_scale, int dim, double* J) {
  const double delta = kNumericDelta, scalar = 1.0 / (2 * delta);
  for (int d = 0; d < dim; d++) {
    double add[7] = {0, 0, 0, 0, 0, 0, 0}, moved[8], ep[7], em[7];
    add[d] = delta;
    sim3_oplus(side ? v1 : v0, add, fix_scale, moved);
    sim3_edge_residual(C, side ? v0 : moved, side ? moved : v1, ep);
    add[d] = -delta;
    sim3_oplus(side ? v1 : v0, add, fix_scale, moved);
    sim3_edge_residual(C, side ? v0 : moved, side ? moved : v1, em);
    for (int k = 0; k < 7; k++) J[7 * k + d] = scalar * (ep[k] - em[k]);
  }
}

extern "C" void pgr_jacobians(int n, const double* C, const double* v0, const double* v1, int fix_scale, double* Ji, double* Jj) {
  const int dim = fix_scale ? 6 : 7;
  memset(Ji, 0, sizeof(double) * 49 * n);
  memset(Jj, 0, sizeof(double) * 49 * n);
  for (int k = 0; k < n; k++) {
    numeric_jacobian(C + 8 * k, v0 + 8 * k, v1 + 8 * k, 0, fix_scale != 0, dim, Ji + 49 * k);
    numeric_jacobian(C + 8 * k, v0 + 8 * k, v1 + 8 * k, 1, fix_scale != 0, dim, Jj + 49 * k);
  }
}

namespace {

struct HostGraph {
  const gfs_essential_graph_problem* p;
  int V, E, F, dim, n;
  std::vector<int> free_index;
  std::vector<double> meas;

  explicit HostGraph(const gfs_essential_graph_problem* p_) : p(p_), V(p_->n_vertices), E(p_->n_edges) {
    free_index.assign(V, -1);
    F = 0;
    for (int v = 0; v < V; v++)
      if (!p->vertex_fixed[v]) free_index[v] = F++;
    dim = p->fix_scale ? 6 : 7;
    n = dim * F;
    meas.resize(8 * (size_t)E);
    for (int e = 0; e < E; e++) {
      for (int c = 0; c < 4; c++) meas[8 * e + c] = p->edge_q[4 * e + c];
      for (int c = 0; c < 3; c++) meas[8 * e + 4 + c] = p->edge_t[3 * e + c];
      meas[8 * e + 7] = p->edge_s[e];
    }
  }
  double errors(const std::vector<double>& est, std::vector<double>& chi, std::vector<double>* err) const {
    double total = 0;
    chi.resize(E);
    if (err) err->resize(7 * (size_t)E);
    for (int e = 0; e < E; e++) {
      double r[7];
      sim3_edge_residual(&meas[8 * e], &est[8 * p->edge_i[e]], &est[8 * p->edge_j[e]], r);
      double c = 0;
      for (int k = 0; k < 7; k++) c += r[k] * (p->edge_w[e] * r[k]);
      chi[e] = c;
      total += c;
      if (err) memcpy(&(*err)[7 * e], r, sizeof(r));
    }
    return total;
  }
  // H (n x n, both triangles, no lambda) and b, the edges' terms added in edge order
  void system(const std::vector<double>& est, const std::vector<double>& err, std::vector<double>& H, std::vector<double>& b) const {
    H.assign((size_t)n * n, 0.0);
    b.assign(n, 0.0);
    for (int e = 0; e < E; e++) {
      const int vi = p->edge_i[e], vj = p->edge_j[e], fi = free_index[vi], fj = free_index[vj];
      if (fi < 0 && fj < 0) continue;
      const double w = p->edge_w[e];
      double A[49] = {0}, B[49] = {0}, omega_r[7];
      if (fi >= 0) numeric_jacobian(&meas[8 * e], &est[8 * vi], &est[8 * vj], 0, p->fix_scale != 0, dim, A);
      if (fj >= 0) numeric_jacobian(&meas[8 * e], &est[8 * vi], &est[8 * vj], 1, p->fix_scale != 0, dim, B);
      for (int k = 0; k < 7; k++) omega_r[k] = -(w * err[7 * e + k]);
      for (int a = 0; a < dim; a++) {
        for (int c = 0; c < dim; c++) {
          double hii = 0, hij = 0, hjj = 0;
          for (int k = 0; k < 7; k++) {
            hii += (A[7 * k + a] * w) * A[7 * k + c];
            hij += (A[7 * k + a] * w) * B[7 * k + c];
            hjj += (B[7 * k + a] * w) * B[7 * k + c];
          }
          if (fi >= 0) H[(size_t)(dim * fi + a) * n + dim * fi + c] += hii;
          if (fj >= 0) H[(size_t)(dim * fj + a) * n + dim * fj + c] += hjj;
          if (fi >= 0 && fj >= 0) {
            H[(size_t)(dim * fi + a) * n + dim * fj + c] += hij;
            H[(size_t)(dim * fj + c) * n + dim * fi + a] += hij;
          }
        }
        double bi = 0, bj = 0;
        for (int k = 0; k < 7; k++) {
          bi += A[7 * k + a] * omega_r[k];
          bj += B[7 * k + a] * omega_r[k];
        }
        if (fi >= 0) b[dim * fi + a] += bi;
        if (fj >= 0) b[dim * fj + a] += bj;
      }
    }
  }
};

// dense L D L^T without pivoting on the lower triangle; false on a zero or non-finite pivot
bool ldlt_solve(std::vector<double> A, int n, const std::vector<double>& b, std::vector<double>& x) {
  std::vector<double> w(n);
  x = b;
  for (int c = 0; c < n; c++) {
    const double d = A[(size_t)c * n + c];
    if (d == 0.0 || !std::isfinite(d)) return false;
    for (int i = c + 1; i < n; i++) {
      w[i] = A[(size_t)i * n + c];
      A[(size_t)i * n + c] = w[i] / d;
    }
    for (int i = c + 1; i < n; i++)
      for (int k = c + 1; k <= i; k++) A[(size_t)i * n + k] -= A[(size_t)i * n + c] * w[k];
    for (int i = c + 1; i < n; i++) x[i] -= A[(size_t)i * n + c] * x[c];
  }
  for (int c = 0; c < n; c++) x[c] /= A[(size_t)c * n + c];
  for (int c = n - 1; c >= 0; c--)
    for (int i = 0; i < c; i++) x[i] -= A[(size_t)c * n + i] * x[c];
  return true;
}

}  // namespace

// gfs_essential_graph_optimize on the host (optimization_algorithm_levenberg.cpp:61-168 with the user's first lambda)
extern "C" int pgr_optimize(const gfs_essential_graph_problem* p, gfs_essential_graph_solution* sol) {
  HostGraph G(p);
  const int V = G.V, n = G.n, dim = G.dim;
  std::vector<double> est(8 * (size_t)V), trial, chi, err, H, Hl, b, x;
  for (int v = 0; v < V; v++) {
    for (int c = 0; c < 4; c++) est[8 * v + c] = p->vertex_q[4 * v + c];
    for (int c = 0; c < 3; c++) est[8 * v + 4 + c] = p->vertex_t[3 * v + c];
    est[8 * v + 7] = p->vertex_s[v];
  }
  const std::vector<double> before = est;
  double lambda = p->lambda_init, ni = 2, last_chi = 0;
  int n_bad = 0, iters = 0;
  const bool runs = p->iterations > 0 && G.F > 0;
  for (int it = 0; runs && it < p->iterations; it++) {
    double current = G.errors(est, chi, &err);
    const double ini = current;
    G.system(est, err, H, b);
    double rho = 0;
    int qmax = 0;
    do {
      Hl = H;
      for (int k = 0; k < n; k++) Hl[(size_t)k * n + k] += lambda;
      const bool ok = ldlt_solve(Hl, n, b, x);
      trial = est;
      double scale = 0, temp = std::numeric_limits<double>::max();
      if (ok) {
        for (int f = 0, v = 0; v < V; v++) {
          if (G.free_index[v] < 0) continue;
          double u[7] = {0, 0, 0, 0, 0, 0, 0}, loc = 0;
          for (int a = 0; a < dim; a++) {
            u[a] = x[dim * f + a];
            loc += u[a] * (lambda * u[a] + b[dim * f + a]);
          }
          scale += loc;
          sim3_oplus(&est[8 * v], u, p->fix_scale != 0, &trial[8 * v]);
          f++;
        }
        temp = G.errors(trial, chi, nullptr);
      }
      rho = (current - temp) / (scale + 1e-3);
      if (rho > 0 && std::isfinite(temp)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        current = temp;
        est = trial;
      } else {
        lambda *= ni;
        ni *= 2;
      }
      qmax++;
    } while (rho < 0 && qmax < 10);
    iters++;
    last_chi = current;
    if (qmax == 10 || rho == 0) break;
    if ((ini - current) * 1e3 < ini)
      n_bad++;
    else
      n_bad = 0;
    if (n_bad >= 3) break;
  }
  const double total = G.errors(est, chi, nullptr);
  for (int v = 0; v < V; v++) {
    for (int c = 0; c < 4; c++) sol->vertex_q[4 * v + c] = est[8 * v + c];
    for (int c = 0; c < 3; c++) sol->vertex_t[3 * v + c] = est[8 * v + 4 + c];
    sol->vertex_s[v] = est[8 * v + 7];
  }
  if (sol->edge_chi2) memcpy(sol->edge_chi2, chi.data(), sizeof(double) * chi.size());
  sol->iterations_run = iters;
  sol->final_chi2 = runs ? last_chi : total;
  sol->final_lambda = runs ? lambda : 0.0;
  for (int m = 0; m < p->n_points && sol->points; m++) {
    const int r = p->point_ref[m];
    const float* P = p->points + 3 * (size_t)m;
    float* o = sol->points + 3 * (size_t)m;
    if (r < 0) {
      o[0] = P[0], o[1] = P[1], o[2] = P[2];
      continue;
    }
    double Swr[8], Pd[3] = {P[0], P[1], P[2]}, Pr[3], Pw[3];
    sim3_inverse(&est[8 * r], Swr);
    sim3_map(&before[8 * r], Pd, Pr);
    sim3_map(Swr, Pr, Pw);
    for (int k = 0; k < 3; k++) o[k] = (float)Pw[k];
  }
  return 0;
}
