// Essential-graph optimisation (Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:2042-2413): gfs_essential_graph and its entry
// points.  Included last by lba.hip.  The kernels in front of and behind the factorisation are eg_dev.hpp's, the structure lists
// eg_lists.hpp's; the factorisation (gba_factor_and_solve), the LM state and k_lba_init / k_lba_decide / k_lba_finish are the bundle
// adjustments', driven through an LbaDev that carries only what those kernels read.
#pragma once

extern "C" {

struct gfs_essential_graph {
  int device = 0, max_vertices = 0, max_edges = 0, max_points = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int* h_flags = nullptr;  // host-mapped, one slot of kFlagInts ints written by k_lba_decide
  gfs::DevBuf<double> d_v0, d_est, d_meas, d_w, d_chi2, d_J, d_blocks, d_b, d_scale, d_xp, d_tiles, d_W, d_rhs, d_stats, d_after;
  gfs::DevBuf<int> d_free_index, d_free_vert, d_ei, d_ej, d_blk_i, d_blk_j, d_contrib, d_info, d_ref;
  gfs::DevBuf<long long> d_blk_begin;
  gfs::DevBuf<LbaState> d_state;
  gfs::DevBuf<float> d_pts, d_pts_out;
  eg_sys::Lists lists;
  std::vector<double> v0, meas;  // the estimates and measurements as eight doubles each
  gfs_essential_graph_info info = {};
};

int gfs_essential_graph_create(int device, int max_vertices, int max_edges, int max_points, gfs_essential_graph** out) {
  GFS_REQUIRE(out && max_vertices > 0 && max_edges > 0 && max_points >= 0, GFS_ERR_INVALID_ARG, "gfs_essential_graph_create: invalid argument");
  GFS_REQUIRE(max_edges < (1 << 29), GFS_ERR_INVALID_ARG, "gfs_essential_graph_create: more than 2^29 edges");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_essential_graph> g(new gfs_essential_graph);
  g->device = device;
  int rc = gba_raise_lds_limits(device);
  if (rc) return rc;
  const size_t V = max_vertices, E = max_edges, M = std::max(max_points, 1), n = 7 * V, T = gba_sys::panels(n);
  {  // the tiled system and the panel workspace have to fit: refused here, not in the middle of a call
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t need = gba_sys::storage_bytes(n) + T * gba_sys::kP * gba_sys::kP * sizeof(double) + E * (kEgEdgeDoubles + 98 + 32) * sizeof(double);
      if (need > free_b) {
        gfs::set_error("gfs_essential_graph_create: the system of %d vertices needs %zu bytes, %zu are free", max_vertices, need, free_b);
        return GFS_ERR_CAPACITY;
      }
    }
  }
  GFS_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
  if (hipHostMalloc((void**)&g->h_flags, kFlagInts * sizeof(int), hipHostMallocMapped) != hipSuccess) {
    g->h_flags = nullptr;
    gfs::set_error("gfs_essential_graph_create: hipHostMalloc failed");
    rc = GFS_ERR_HIP;
  }
#define A(x) if (!rc) rc = (x)
  A(g->d_v0.alloc(8 * V));
  A(g->d_est.alloc(16 * V));
  A(g->d_after.alloc(8 * V));
  A(g->d_meas.alloc(8 * E));
  A(g->d_w.alloc(E));
  A(g->d_chi2.alloc(E));
  A(g->d_J.alloc(98 * E));
  A(g->d_blocks.alloc(kEgEdgeDoubles * E));
  A(g->d_b.alloc(n));
  A(g->d_scale.alloc(V));
  A(g->d_xp.alloc(n));
  A(g->d_tiles.alloc(gba_sys::storage_doubles(n)));
  A(g->d_W.alloc(T * gba_sys::kP * gba_sys::kP));
  A(g->d_rhs.alloc(T * gba_sys::kP));
  A(g->d_stats.alloc(2));
  A(g->d_info.alloc(2));
  A(g->d_state.alloc(1));
  A(g->d_free_index.alloc(V));
  A(g->d_free_vert.alloc(V));
  A(g->d_ei.alloc(E));
  A(g->d_ej.alloc(E));
  A(g->d_blk_i.alloc(V + E));  // every diagonal block and at most one pair an edge
  A(g->d_blk_j.alloc(V + E));
  A(g->d_blk_begin.alloc(V + E + 1));
  A(g->d_contrib.alloc(3 * E));
  A(g->d_ref.alloc(M));
  A(g->d_pts.alloc(3 * M));
  A(g->d_pts_out.alloc(3 * M));
#undef A
  if (rc) {
    gfs_essential_graph_destroy(g.release());
    return rc;
  }
  g->max_vertices = max_vertices;
  g->max_edges = max_edges;
  g->max_points = max_points;
  *out = g.release();
  return GFS_OK;
}

void gfs_essential_graph_destroy(gfs_essential_graph* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) {
    (void)hipStreamSynchronize(g->stream);
    (void)hipStreamDestroy(g->stream);
  }
  if (g->h_flags) (void)hipHostFree(g->h_flags);
  delete g;
}

}  // extern "C"

namespace {

// a call's descriptors and its launch count (LM_LAUNCH's queue)
struct EgRun {
  gfs_essential_graph* g;
  hipStream_t s;
  LbaDev D;
  EgDev E;
  GbaDev G;
  int* d_flags = nullptr;
  int launches = 0, trials = 0;
};

int eg_check(const gfs_essential_graph* g, const gfs_essential_graph_problem* p, const char* who) {
  const int V = p->n_vertices, E = p->n_edges, M = p->n_points;
  GFS_REQUIRE(V > 0 && E >= 0 && M >= 0, GFS_ERR_INVALID_ARG, "%s: negative count or no vertex", who);
  GFS_REQUIRE(p->vertex_q && p->vertex_t && p->vertex_s && p->vertex_fixed, GFS_ERR_INVALID_ARG, "%s: NULL vertex array", who);
  GFS_REQUIRE(E == 0 || (p->edge_i && p->edge_j && p->edge_q && p->edge_t && p->edge_s && p->edge_w), GFS_ERR_INVALID_ARG, "%s: NULL edge array", who);
  GFS_REQUIRE(M == 0 || (p->points && p->point_ref), GFS_ERR_INVALID_ARG, "%s: NULL point array", who);
  GFS_REQUIRE(V <= g->max_vertices && E <= g->max_edges && M <= g->max_points, GFS_ERR_CAPACITY,
              "%s: %d vertices, %d edges, %d points exceed the handle's %d, %d, %d", who, V, E, M, g->max_vertices, g->max_edges, g->max_points);
  GFS_REQUIRE(std::isfinite(p->lambda_init) && p->lambda_init > 0, GFS_ERR_INVALID_ARG, "%s: lambda_init must be positive", who);
  for (int v = 0; v < V; v++)
    GFS_REQUIRE(std::isfinite(p->vertex_s[v]) && p->vertex_s[v] > 0, GFS_ERR_INVALID_ARG, "%s: the scale of vertex %d is not positive and finite", who, v);
  for (int e = 0; e < E; e++) {
    const int i = p->edge_i[e], j = p->edge_j[e];
    GFS_REQUIRE(i >= 0 && i < V && j >= 0 && j < V, GFS_ERR_INVALID_ARG, "%s: edge %d references an unknown vertex", who, e);
    GFS_REQUIRE(i != j, GFS_ERR_INVALID_ARG, "%s: edge %d joins vertex %d to itself", who, e, i);
    GFS_REQUIRE(std::isfinite(p->edge_s[e]) && p->edge_s[e] > 0 && std::isfinite(p->edge_w[e]) && p->edge_w[e] > 0, GFS_ERR_INVALID_ARG,
                "%s: the scale or the weight of edge %d is not positive and finite", who, e);
  }
  for (int m = 0; m < M; m++)
    GFS_REQUIRE(p->point_ref[m] < V, GFS_ERR_INVALID_ARG, "%s: point %d references an unknown vertex", who, m);
  return GFS_OK;
}

void eg_pack8(const double* q, const double* t, const double* s, size_t n, std::vector<double>& out) {
  out.resize(8 * n);
  for (size_t k = 0; k < n; k++) {
    for (int c = 0; c < 4; c++) out[8 * k + c] = q[4 * k + c];
    for (int c = 0; c < 3; c++) out[8 * k + 4 + c] = t[3 * k + c];
    out[8 * k + 7] = s[k];
  }
}

// the checked graph listed, uploaded and described; the LM state and both estimate buffers set
int eg_start(gfs_essential_graph* g, const gfs_essential_graph_problem* p, EgRun& R) {
  GFS_HIP(hipSetDevice(g->device));
  hipStream_t s = g->stream;
  const int V = p->n_vertices, E = p->n_edges;
  eg_sys::Lists& L = g->lists;
  eg_sys::build_lists(V, E, p->vertex_fixed, p->edge_i, p->edge_j, L);
  const int F = (int)L.n_free(), dim = p->fix_scale ? 6 : 7;
  eg_pack8(p->vertex_q, p->vertex_t, p->vertex_s, V, g->v0);
  eg_pack8(p->edge_q, p->edge_t, p->edge_s, E, g->meas);
  auto up = [&](void* d, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
  GFS_HIP(up(g->d_v0.p, g->v0.data(), g->v0.size() * 8));
  GFS_HIP(up(g->d_meas.p, g->meas.data(), g->meas.size() * 8));
  GFS_HIP(up(g->d_w.p, p->edge_w, (size_t)E * 8));
  GFS_HIP(up(g->d_ei.p, p->edge_i, (size_t)E * 4));
  GFS_HIP(up(g->d_ej.p, p->edge_j, (size_t)E * 4));
  GFS_HIP(up(g->d_free_index.p, L.free_index.data(), (size_t)V * 4));
  GFS_HIP(up(g->d_free_vert.p, L.free_vert.data(), (size_t)F * 4));
  GFS_HIP(up(g->d_blk_i.p, L.blk_i.data(), L.blk_i.size() * 4));
  GFS_HIP(up(g->d_blk_j.p, L.blk_j.data(), L.blk_j.size() * 4));
  static_assert(sizeof(long long) == sizeof(int64_t), "the lists' 64-bit counts go up as they are");
  GFS_HIP(up(g->d_blk_begin.p, L.blk_begin.data(), L.blk_begin.size() * 8));
  GFS_HIP(up(g->d_contrib.p, L.contrib.data(), L.contrib.size() * 4));
  GFS_HIP(hipStreamSynchronize(s));  // (the host vectors are pageable: the copies have read them)

  R.g = g;
  R.s = s;
  EgDev& Ed = R.E;
  Ed = EgDev{};
  Ed.n_vert = V;
  Ed.n_edges = E;
  Ed.n_free = F;
  Ed.dim = dim;
  Ed.fix_scale = p->fix_scale ? 1 : 0;
  Ed.lambda_init = p->lambda_init;
  bind(Ed.free_index, g->d_free_index.p);
  bind(Ed.free_vert, g->d_free_vert.p);
  bind(Ed.e_i, g->d_ei.p);
  bind(Ed.e_j, g->d_ej.p);
  bind(Ed.e_meas, g->d_meas.p);
  bind(Ed.e_w, g->d_w.p);
  bind(Ed.est, g->d_est.p);
  bind(Ed.chi2, g->d_chi2.p);
  bind(Ed.J, g->d_J.p);
  bind(Ed.blocks, g->d_blocks.p);
  bind(Ed.b, g->d_b.p);
  bind(Ed.scale, g->d_scale.p);
  Ed.n_blocks = L.n_blocks();
  bind(Ed.blk_i, g->d_blk_i.p);
  bind(Ed.blk_j, g->d_blk_j.p);
  bind(Ed.blk_begin, g->d_blk_begin.p);
  bind(Ed.contrib, g->d_contrib.p);
  // what k_lba_init (no pose, no point, no edge: the LM state alone), k_gba_*, k_lba_decide and k_lba_finish read
  LbaDev& D = R.D;
  D = LbaDev{};
  bind(D.S, g->d_state.p);
  bind(D.xp, g->d_xp.p);
  bind(D.part_chi, g->d_chi2.p);    // k_lba_decide's sums: the edges' chi2 in edge order ...
  D.n_err_blocks = E;
  bind(D.part_scale, g->d_scale.p);  // ... and the vertices' computeScale terms in vertex order
  D.n_upd_blocks = F;
  bind(D.out_info, g->d_info.p);
  bind(D.out_stats, g->d_stats.p);
  GbaDev& G = R.G;
  G = GbaDev{};
  G.n = dim * F;
  G.T = (int)gba_sys::panels((size_t)G.n);
  bind(G.tiles, g->d_tiles.p);
  bind(G.W, g->d_W.p);
  bind(G.rhs, g->d_rhs.p);
  GFS_HIP(hipHostGetDevicePointer((void**)&R.d_flags, g->h_flags, 0));
  gfs_essential_graph_info& I = g->info;
  I = gfs_essential_graph_info{};
  I.n_free = F;
  I.dimension = dim;
  I.panels = G.T;
  I.blocks = L.n_blocks();
  I.system_bytes = (int64_t)gba_sys::storage_bytes((size_t)G.n);
  LM_LAUNCH(R, "k_lba_init", k_lba_init, dim3(1), dim3(kMk), 0, D);
  LM_LAUNCH(R, "k_eg_init", k_eg_init, dim3(std::min(gfs::div_up(8 * V, kMk), 256)), dim3(kMk), 0, Ed, g->d_v0.p);
  return GFS_OK;
}

int eg_errors(EgRun& R, int trial) {
  if (R.E.n_edges > 0) LM_LAUNCH(R, "k_eg_errors", k_eg_errors, dim3(gfs::div_up(R.E.n_edges, kEgWg)), dim3(kEgWg), 0, R.D, R.E, trial);
  return GFS_OK;
}
// the top of an iteration: the edges linearised at the estimate, the LM bookkeeping
int eg_build(EgRun& R, int iteration) {
  if (R.E.n_edges > 0) LM_LAUNCH(R, "k_eg_linearize", k_eg_linearize, dim3(gfs::div_up(R.E.n_edges, kEgWg)), dim3(kEgWg), 0, R.D, R.E);
  LM_LAUNCH(R, "k_eg_begin", k_eg_begin, dim3(1), dim3(64), 0, R.D, R.E, iteration);
  return GFS_OK;
}
// one trial up to the errors at the trial estimate; d_tap: the assembled system packed there ahead of the factorisation
int eg_trial(EgRun& R, double* d_tap) {
  const GbaDev& G = R.G;
  R.trials++;
  GFS_HIP(hipMemsetAsync(G.tiles, 0, gba_sys::storage_bytes((size_t)G.n), R.s));
  LM_LAUNCH(R, "k_eg_assemble", k_eg_assemble, dim3((unsigned)((R.E.n_blocks + kMk / 64 - 1) / (kMk / 64))), dim3(kMk), 0, R.D, R.E, G);
  if (d_tap) {
    const size_t n = (size_t)G.n;
    GFS_LAUNCH("k_gba_pack_lower", k_gba_pack_lower, dim3(256), dim3(kMk), 0, R.s, G, d_tap, d_tap + n * (n + 1) / 2);
  }
  if (int rc = gba_factor_and_solve(R, R.D, G)) return rc;
  LM_LAUNCH(R, "k_eg_update", k_eg_update, dim3(gfs::div_up(R.E.n_free, kEgWg)), dim3(kEgWg), 0, R.D, R.E);
  return eg_errors(R, 1);
}

// optimize(iterations): the host waits for every trial's verdict, as gfs_gba_solve does -- next to a factorisation of the whole
// system the round trip is nothing.  There is no stop flag (src/Optimizer.cc:2042-2413 sets none).
int eg_solve(gfs_essential_graph* g, const gfs_essential_graph_problem* p, EgRun& R) {
  int rc = eg_start(g, p, R);
  if (rc) return rc;
  const bool runs = p->iterations > 0 && R.E.n_free > 0;
  for (int iteration = 0; runs && iteration < p->iterations; iteration++) {
    if ((rc = eg_build(R, iteration))) return rc;
    const int* f = g->h_flags;
    for (;;) {
      if ((rc = eg_trial(R, nullptr))) return rc;
      LM_LAUNCH(R, "k_lba_decide", k_lba_decide, dim3(1), dim3(64), 0, R.D, 0, R.d_flags, 0);
      GFS_HIP(hipStreamSynchronize(R.s));
      if (!f[0]) break;  // accepted, or the iteration's last trial
    }
    if (f[1]) break;  // qmax == 10 || rho == 0
  }
  // e->chi2() at the estimate that is returned; without an iteration also the chi2 the run reports, and lambda 0
  if ((rc = eg_errors(R, 0))) return rc;
  if (!runs) LM_LAUNCH(R, "k_eg_begin", k_eg_begin, dim3(1), dim3(64), 0, R.D, R.E, 1);
  LbaDev Df = R.D;
  Df.mode = runs ? 0 : 1;
  LM_LAUNCH(R, "k_lba_finish", k_lba_finish, dim3(1), dim3(64), 0, Df);
  GFS_HIP(hipStreamSynchronize(R.s));
  g->info.trials = R.trials;
  g->info.launches = R.launches;
  return GFS_OK;
}

// correctedSwr.map(Srw.map(P)) for m points on the handle's stream, drained
int eg_correct(gfs_essential_graph* g, int m, const float* points, const int32_t* ref, const double* d_before, const double* d_after, float* out) {
  if (m <= 0 || !out) return GFS_OK;
  hipStream_t s = g->stream;
  GFS_HIP(hipMemcpyAsync(g->d_pts.p, points, (size_t)m * 12, hipMemcpyHostToDevice, s));
  GFS_HIP(hipMemcpyAsync(g->d_ref.p, ref, (size_t)m * 4, hipMemcpyHostToDevice, s));
  GFS_LAUNCH("k_eg_correct_points", k_eg_correct_points, dim3(gfs::div_up(m, kMk)), dim3(kMk), 0, s, m, g->d_pts.p, g->d_ref.p, d_before, d_after,
             g->d_pts_out.p);
  GFS_HIP(hipMemcpyAsync(out, g->d_pts_out.p, (size_t)m * 12, hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  return GFS_OK;
}

}  // namespace

extern "C" {

int gfs_essential_graph_optimize(gfs_essential_graph* g, const gfs_essential_graph_problem* p, gfs_essential_graph_solution* sol) {
  GFS_REQUIRE(g && p && sol, GFS_ERR_INVALID_ARG, "gfs_essential_graph_optimize: NULL argument");
  GFS_REQUIRE(sol->vertex_q && sol->vertex_t && sol->vertex_s, GFS_ERR_INVALID_ARG, "gfs_essential_graph_optimize: NULL output array");
  std::lock_guard<std::mutex> lk(g->mu);
  int rc = eg_check(g, p, "gfs_essential_graph_optimize");
  if (rc) return rc;
  EgRun R;
  if ((rc = eg_solve(g, p, R))) return rc;
  const int V = p->n_vertices, E = p->n_edges;
  int info[2];
  double stats[2];
  GFS_HIP(hipMemcpy(info, g->d_info.p, sizeof(info), hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(stats, g->d_stats.p, sizeof(stats), hipMemcpyDeviceToHost));
  const double* d_est = g->d_est.p + (size_t)info[1] * 8 * V;
  std::vector<double>& est = g->meas;  // (the staging vector is free again)
  est.resize(8 * (size_t)V);
  GFS_HIP(hipMemcpy(est.data(), d_est, est.size() * 8, hipMemcpyDeviceToHost));
  for (int v = 0; v < V; v++) {
    for (int c = 0; c < 4; c++) sol->vertex_q[4 * (size_t)v + c] = est[8 * (size_t)v + c];
    for (int c = 0; c < 3; c++) sol->vertex_t[3 * (size_t)v + c] = est[8 * (size_t)v + 4 + c];
    sol->vertex_s[v] = est[8 * (size_t)v + 7];
  }
  if (sol->edge_chi2 && E) GFS_HIP(hipMemcpy(sol->edge_chi2, g->d_chi2.p, (size_t)E * 8, hipMemcpyDeviceToHost));
  sol->iterations_run = info[0];
  sol->final_chi2 = stats[0];
  sol->final_lambda = stats[1];
  return eg_correct(g, p->n_points, p->points, p->point_ref, g->d_v0.p, d_est, sol->points);
}

int gfs_essential_graph_correct_points(gfs_essential_graph* g, int n_vertices, const double* before, const double* after, int n_points,
                                       const float* points, const int32_t* point_ref, float* out) {
  GFS_REQUIRE(g && n_vertices > 0 && n_points >= 0 && before && after, GFS_ERR_INVALID_ARG, "gfs_essential_graph_correct_points: invalid argument");
  GFS_REQUIRE(n_points == 0 || (points && point_ref && out), GFS_ERR_INVALID_ARG, "gfs_essential_graph_correct_points: NULL point array");
  std::lock_guard<std::mutex> lk(g->mu);
  GFS_REQUIRE(n_vertices <= g->max_vertices && n_points <= g->max_points, GFS_ERR_CAPACITY,
              "gfs_essential_graph_correct_points: %d vertices, %d points exceed the handle's %d, %d", n_vertices, n_points, g->max_vertices, g->max_points);
  for (int m = 0; m < n_points; m++)
    GFS_REQUIRE(point_ref[m] < n_vertices, GFS_ERR_INVALID_ARG, "gfs_essential_graph_correct_points: point %d references an unknown vertex", m);
  GFS_HIP(hipSetDevice(g->device));
  GFS_HIP(hipMemcpyAsync(g->d_v0.p, before, (size_t)n_vertices * 64, hipMemcpyHostToDevice, g->stream));
  GFS_HIP(hipMemcpyAsync(g->d_after.p, after, (size_t)n_vertices * 64, hipMemcpyHostToDevice, g->stream));
  return eg_correct(g, n_points, points, point_ref, g->d_v0.p, g->d_after.p, out);
}

int gfs_essential_graph_last_info(const gfs_essential_graph* g, gfs_essential_graph_info* info) {
  GFS_REQUIRE(g && info, GFS_ERR_INVALID_ARG, "gfs_essential_graph_last_info: NULL argument");
  *info = g->info;  // (not under the handle's lock: for the thread that made the call, after it returned)
  return GFS_OK;
}

int gfs_test_essential_graph_first_trial(gfs_essential_graph* g, const gfs_essential_graph_problem* p, gfs_test_essential_graph_trial* out) {
  GFS_REQUIRE(g && p && out, GFS_ERR_INVALID_ARG, "gfs_test_essential_graph_first_trial: NULL argument");
  GFS_REQUIRE(out->H && out->b && out->x, GFS_ERR_INVALID_ARG, "gfs_test_essential_graph_first_trial: NULL output array");
  std::lock_guard<std::mutex> lk(g->mu);
  int rc = eg_check(g, p, "gfs_test_essential_graph_first_trial");
  if (rc) return rc;
  EgRun R;
  if ((rc = eg_start(g, p, R)) || (rc = eg_build(R, 0))) return rc;
  const size_t n = (size_t)R.G.n, nt = n * (n + 1) / 2;
  gfs::DevBuf<double> d_tap;
  if ((rc = d_tap.alloc(nt + n + 1))) return rc;
  if (n > 0 && (rc = eg_trial(R, d_tap.p))) return rc;
  GFS_HIP(hipStreamSynchronize(R.s));
  LbaState S;
  GFS_HIP(hipMemcpy(&S, g->d_state.p, sizeof(S), hipMemcpyDeviceToHost));
  if (n) {
    GFS_HIP(hipMemcpy(out->H, d_tap.p, nt * 8, hipMemcpyDeviceToHost));
    GFS_HIP(hipMemcpy(out->b, d_tap.p + nt, n * 8, hipMemcpyDeviceToHost));
    GFS_HIP(hipMemcpy(out->x, g->d_xp.p, n * 8, hipMemcpyDeviceToHost));
  }
  std::vector<double> chi(p->n_edges), part(R.E.n_free);
  if (!chi.empty()) GFS_HIP(hipMemcpy(chi.data(), g->d_chi2.p, chi.size() * 8, hipMemcpyDeviceToHost));
  if (!part.empty() && n) GFS_HIP(hipMemcpy(part.data(), g->d_scale.p, part.size() * 8, hipMemcpyDeviceToHost));
  double trial_chi = 0, scale = 0;
  for (double v : chi) trial_chi += v;  // k_lba_decide's orders
  for (double v : part) scale += v;
  out->chi2 = S.current_chi;
  out->trial_chi2 = trial_chi;
  out->scale = scale;
  out->n_free = R.E.n_free;
  out->dimension = R.E.dim;
  out->solve_ok = S.solve_ok;
  g->info.trials = R.trials;
  g->info.launches = R.launches;
  return GFS_OK;
}

// host-only: the structure lists of eg_lists.hpp
int gfs_test_essential_graph_lists(int n_vertices, int n_edges, const uint8_t* vertex_fixed, const int32_t* edge_i, const int32_t* edge_j,
                                   int64_t* counts, int32_t* free_index, int32_t* blk_ij, int64_t* blk_begin, int64_t cap_blocks,
                                   int32_t* contrib, int64_t cap_contrib) {
  GFS_REQUIRE(n_vertices >= 0 && n_edges >= 0 && counts && (n_vertices == 0 || vertex_fixed) && (n_edges == 0 || (edge_i && edge_j)),
              GFS_ERR_INVALID_ARG, "gfs_test_essential_graph_lists: invalid argument");
  for (int e = 0; e < n_edges; e++)
    GFS_REQUIRE(edge_i[e] >= 0 && edge_i[e] < n_vertices && edge_j[e] >= 0 && edge_j[e] < n_vertices && edge_i[e] != edge_j[e], GFS_ERR_INVALID_ARG,
                "gfs_test_essential_graph_lists: edge %d references an unknown vertex or joins a vertex to itself", e);
  eg_sys::Lists L;
  eg_sys::build_lists(n_vertices, n_edges, vertex_fixed, edge_i, edge_j, L);
  counts[0] = L.n_free();
  counts[1] = L.n_blocks();
  counts[2] = L.n_contrib();
  if (L.n_blocks() > cap_blocks || L.n_contrib() > cap_contrib) return GFS_ERR_CAPACITY;
  if (free_index) std::copy(L.free_index.begin(), L.free_index.end(), free_index);
  for (int64_t b = 0; b < L.n_blocks() && blk_ij; b++) {
    blk_ij[2 * b] = L.blk_i[(size_t)b];
    blk_ij[2 * b + 1] = L.blk_j[(size_t)b];
  }
  if (blk_begin) std::copy(L.blk_begin.begin(), L.blk_begin.end(), blk_begin);
  if (contrib) std::copy(L.contrib.begin(), L.contrib.end(), contrib);
  return GFS_OK;
}

}  // extern "C"
