// Global bundle adjustment (Optimizer::BundleAdjustment, src/Optimizer.cc:56-363): gfs_gba and its entry points.  Included last by
// lba.hip.  A gfs_gba is a gfs_lba (the problem staging, the LM state and every phase kernel but the Schur products and the reduced
// solve are gfs_lba_solve's: lba_host.hpp) plus the structure lists, the tiled reduced system and the panel workspace of gba_dev.hpp.
#pragma once

extern "C" {

struct gfs_gba {
  gfs_lba* lba = nullptr;
  int max_poses = 0;
  gfs::DevBuf<double> d_tiles, d_W, d_rhs;
  gfs::DevBuf<int> d_blk_i, d_blk_j, d_contrib, d_pose_edges;  // (d_contrib grows on demand)
  gfs::DevBuf<long long> d_blk_begin, d_pose_begin;
  gba_sys::Lists lists;
  std::vector<int32_t> e_free;
  gfs_gba_info info = {};
};

static int gba_raise_lds_limits(int device) {
  static std::mutex mu;
  static bool done[64] = {};
  std::lock_guard<std::mutex> lk(mu);
  if (device >= 0 && device < 64 && done[device]) return GFS_OK;
  // (what each kernel is launched with: the sizes are compile-time constants, and the kernels hold static LDS besides)
  GFS_HIP(hipFuncSetAttribute((const void*)k_gba_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGbaTileLds));
  GFS_HIP(hipFuncSetAttribute((const void*)k_gba_back, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGbaTileLds));
  GFS_HIP(hipFuncSetAttribute((const void*)k_gba_panel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * kGbaTileLds)));
  if (device >= 0 && device < 64) done[device] = true;
  return GFS_OK;
}

int gfs_gba_create(int device, int max_poses, int max_points, int max_edges, gfs_gba** out) {
  GFS_REQUIRE(out && max_poses > 0 && max_points > 0 && max_edges > 0, GFS_ERR_INVALID_ARG, "gfs_gba_create: invalid argument");
  std::unique_ptr<gfs_gba> g(new gfs_gba);
  int rc = lba_create_impl(device, max_poses, max_points, max_edges, true, &g->lba);
  if (!rc) rc = gba_raise_lds_limits(device);
  const size_t n = 6 * (size_t)max_poses, T = gba_sys::panels(n), F = max_poses;
  {  // the reduced system plus workspaces have to fit: refused here, not in the middle of a solve
    size_t free_b = 0, total_b = 0;
    if (!rc && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      // the tiles, the panel workspace and the block tables (one entry per block of the packed lower triangle: F (F + 1) / 2 is the
      // most a map can list, ~100 MB at 4 000 poses); the contribution list is sized by the map and grows in gba_lists_upload
      const size_t need = gba_sys::storage_bytes(n) + T * gba_sys::kP * gba_sys::kP * sizeof(double) + F * (F + 1) / 2 * 16;
      if (need > free_b) {
        gfs::set_error("gfs_gba_create: the reduced system of %d poses needs %zu bytes, %zu are free", max_poses, need, free_b);
        rc = GFS_ERR_CAPACITY;
      }
    }
  }
#define A(x) if (!rc) rc = (x)
  A(g->d_tiles.alloc(gba_sys::storage_doubles(n)));
  A(g->d_W.alloc(T * gba_sys::kP * gba_sys::kP));
  A(g->d_rhs.alloc(T * gba_sys::kP));
  A(g->d_blk_i.alloc(F * (F + 1) / 2));
  A(g->d_blk_j.alloc(g->d_blk_i.n));
  A(g->d_blk_begin.alloc(g->d_blk_i.n + 1));
  A(g->d_pose_begin.alloc(F + 1));
  A(g->d_pose_edges.alloc(max_edges));
#undef A
  if (rc) {
    if (g->lba) gfs_lba_destroy(g->lba);
    return rc;
  }
  g->max_poses = max_poses;
  *out = g.release();
  return GFS_OK;
}

void gfs_gba_destroy(gfs_gba* g) {
  if (!g) return;
  if (g->lba) {
    (void)hipSetDevice(g->lba->device);
    (void)hipStreamSynchronize(g->lba->stream);
  }
  g->d_tiles.free();
  g->d_W.free();
  g->d_rhs.free();
  g->d_blk_i.free();
  g->d_blk_j.free();
  g->d_contrib.free();
  g->d_pose_edges.free();
  g->d_blk_begin.free();
  g->d_pose_begin.free();
  gfs_lba_destroy(g->lba);
  delete g;
}

// the structure lists of a prepared problem, uploaded on the handle's stream
static int gba_lists_upload(gfs_gba* g, const gfs_lba_problem* p, const HostPrep& P, GbaDev& G) {
  gfs_lba* h = g->lba;
  hipStream_t s = h->stream;
  const int E = p->n_edges, F = P.n_free;
  g->e_free.resize(E);
  for (int k = 0; k < E; k++) g->e_free[k] = P.free_index[P.e_pose[k]];
  gba_sys::Lists& L = g->lists;
  gba_sys::build_lists(F, p->n_points, P.pt_begin, g->e_free.data(), L);
  GFS_REQUIRE((size_t)L.n_blocks() <= g->d_blk_i.n, GFS_ERR_CAPACITY, "gfs_gba: %lld block pairs exceed the handle's %zu",
              (long long)L.n_blocks(), g->d_blk_i.n);
  if (g->d_contrib.n < L.contrib.size()) {  // (before anything of this solve is queued; a handle settles after its largest map)
    GFS_HIP(hipStreamSynchronize(s));
    if (int rc = g->d_contrib.alloc(L.contrib.size() + L.contrib.size() / 4)) return rc;
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "the lists' 64-bit counts go up as they are");
  auto up = [&](void* d, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  GFS_HIP(up(g->d_blk_i.p, L.blk_i.data(), L.blk_i.size() * 4));
  GFS_HIP(up(g->d_blk_j.p, L.blk_j.data(), L.blk_j.size() * 4));
  GFS_HIP(up(g->d_blk_begin.p, L.blk_begin.data(), L.blk_begin.size() * 8));
  GFS_HIP(up(g->d_contrib.p, L.contrib.data(), L.contrib.size() * 4));
  GFS_HIP(up(g->d_pose_begin.p, L.pose_begin.data(), L.pose_begin.size() * 8));
  GFS_HIP(up(g->d_pose_edges.p, L.pose_edges.data(), L.pose_edges.size() * 4));
  GFS_HIP(hipStreamSynchronize(s));  // (the host vectors are pageable: the copies have read them)
  G = GbaDev{};
  G.n = 6 * F;
  G.T = (int)gba_sys::panels(6 * (size_t)F);
  G.n_blocks = L.n_blocks();
  bind(G.blk_i, g->d_blk_i.p);
  bind(G.blk_j, g->d_blk_j.p);
  bind(G.blk_begin, g->d_blk_begin.p);
  bind(G.contrib, g->d_contrib.p);
  bind(G.pose_begin, g->d_pose_begin.p);
  bind(G.pose_edges, g->d_pose_edges.p);
  bind(G.tiles, g->d_tiles.p);
  bind(G.W, g->d_W.p);
  bind(G.rhs, g->d_rhs.p);
  return GFS_OK;
}

// What a call starts with: the prepared map uploaded and described (no Schur path: the reduced system is the tiles'), its structure
// lists -> the two descriptors and the call's info.
static int gba_map(gfs_gba* g, const gfs_lba_problem* p, const HostPrep& P, LbaDev& D, GbaDev& G) {
  gfs_lba* h = g->lba;
  int rc;
  if ((rc = upload(h, P, h->stream))) return rc;
  describe(h, p, P, 0, D);
  if ((rc = gba_lists_upload(g, p, P, G))) return rc;
  h->last_desc = D;
  gfs_gba_info& I = g->info;
  I = gfs_gba_info{};
  I.n_free = P.n_free;
  I.panel_rows = kP;
  I.panels = G.T;
  I.block_pairs = G.n_blocks;
  I.contributions = g->lists.n_contrib();
  I.system_bytes = (int64_t)gba_sys::storage_bytes((size_t)G.n);
  return GFS_OK;
}

// The tiled L D L^T of an assembled system and its substitutions, queued on `ph` (anything with a stream `s` and a `launches` count):
// panel by panel, then z = D^-1 y, then the back substitution from the last panel.  The kernels read D.S and D.xp and G's n, T, tiles,
// W and rhs, nothing else: gfs_gba_solve and gfs_essential_graph_optimize (eg_host.hpp) both come through here.
extern "C++" template <class Queue>
int gba_factor_and_solve(Queue& ph, const LbaDev& D, const GbaDev& G) {
  const int T = G.T;
  for (int q = 0; q < T; q++) {
    LM_LAUNCH(ph, "k_gba_diag", k_gba_diag, dim3(1), dim3(kMk), kGbaTileLds, D, G, q);
    const int m = T - 1 - q;
    if (m > 0) {
      LM_LAUNCH(ph, "k_gba_panel", k_gba_panel, dim3(m), dim3(kMk), 2 * kGbaTileLds, D, G, q);
      LM_LAUNCH(ph, "k_gba_trail", k_gba_trail, dim3((unsigned)((size_t)m * (m + 1) / 2)), dim3(kMk), 0, D, G, q);
    }
  }
  LM_LAUNCH(ph, "k_gba_scale", k_gba_scale, dim3(gfs::div_up(T * kP, kMk)), dim3(kMk), 0, D, G);
  for (int q = T; q >= 1; q--) LM_LAUNCH(ph, "k_gba_back", k_gba_back, dim3(q == T ? 1 : q), dim3(kMk), kGbaTileLds, D, G, q);
  return GFS_OK;
}

// The reduced system of a global trial (LmPhases::trial), gba_dev.hpp's: the tiles cleared and assembled from the lists, factored
// panel by panel, the substitutions.  Nothing is ever queued ahead of a verdict here, so there is no gate.
struct GbaReduced {
  gfs_gba* g;
  LmPhases& ph;
  const GbaDev& G;
  gfs::DevBuf<double>* d_tap;  // the test hook's: the reduced system packed the way the local one is stored
  int operator()(int, const TrialTap* tap) const {
    const LbaDev& D = ph.D;
    const int T = G.T;
    if (T <= 0) return GFS_OK;
    GFS_HIP(hipMemsetAsync(g->d_tiles.p, 0, gba_sys::storage_bytes((size_t)G.n), ph.s));
    LM_LAUNCH(ph, "k_gba_assemble", k_gba_assemble, dim3((unsigned)((G.n_blocks + kMk / 64 - 1) / (kMk / 64))), dim3(kMk), 0, D, G);
    if (tap) {
      const size_t n = (size_t)G.n, nt = n * (n + 1) / 2;
      if (int rc = d_tap->alloc(nt + n)) return rc;
      GFS_LAUNCH("k_gba_pack_lower", k_gba_pack_lower, dim3(256), dim3(kMk), 0, ph.s, G, d_tap->p, d_tap->p + nt);
      GFS_HIP(hipMemcpyAsync(tap->Hs, d_tap->p, nt * sizeof(double), hipMemcpyDeviceToHost, ph.s));
      GFS_HIP(hipMemcpyAsync(tap->bs, d_tap->p + nt, n * sizeof(double), hipMemcpyDeviceToHost, ph.s));
    }
    return gba_factor_and_solve(ph, D, G);
  }
};

// The LM loop of gfs_gba_solve.  The host waits for every trial's verdict (no iteration is queued ahead: next to a map-sized
// factorisation the round trip is nothing), so the caller's flag is looked at exactly where g2o looks: at the top of every iteration
// -- the first look is the top of iteration 0, Optimizer::BundleAdjustment has no entry check -- and after every rejected trial that
// would be retried.
static int gba_solve_map(gfs_gba* g, const gfs_lba_problem* p, const HostPrep& P, StopFlag stop) {
  LbaDev D;
  GbaDev G;
  int rc = gba_map(g, p, P, D, G);
  if (rc) return rc;
  LmPhases ph(g->lba, D);
  GbaReduced reduced{g, ph, G, nullptr};
  if ((rc = ph.init())) return rc;
  bool stopped = false, began = false;
  for (int iteration = 0; iteration < p->iterations && !stopped; iteration++) {
    if (stop && *stop) break;
    if ((rc = ph.build(iteration, 0))) return rc;
    began = true;
    const int* f = nullptr;
    for (;;) {
      if ((rc = ph.trial(0, reduced, nullptr)) || (rc = ph.verdict(ph.n_decides - 1, f))) return rc;
      if (!f[0]) break;         // accepted, or the iteration's last trial
      if (stop && *stop) {      // a rejected trial that would be retried
        if ((rc = ph.force_decide())) return rc;
        stopped = true;
        break;
      }
    }
    if (!stopped && f[1]) break;
  }
  // e->chi2() at the estimate that is returned (after an accepted trial the arrays hold it already and the kernel leaves at once)
  if ((rc = ph.errors(0, 0))) return rc;
  // no iteration at all (the flag was up at the first look, or iterations <= 0): the robust chi2 of the estimate as it came and
  // lambda 0, what gfs_lba_solve reports for iterations <= 0
  if (!began && (rc = ph.begin(1, 0))) return rc;
  if ((rc = ph.finish(began ? 0 : 1))) return rc;
  g->info.trials = ph.trials;
  g->info.launches = ph.launches;
  return GFS_OK;
}

static int gba_solve_impl(gfs_gba* g, const gfs_lba_problem* p, gfs_lba_solution* sol, StopFlag stop) {
  StopScriptCall script_call;
  GFS_REQUIRE(g && p && sol, GFS_ERR_INVALID_ARG, "gfs_gba_solve: NULL argument");
  gfs_lba* h = g->lba;
  std::lock_guard<std::mutex> lk(h->mu);
  HostPrep* P;
  int rc = prepare_call(h, p, false, P);
  if (rc) return rc;
  if ((rc = gba_solve_map(g, p, *P, stop)) || (rc = fetch_solution(h, p, *P, sol))) return rc;
  // a run without an iteration hands the caller's estimate back as it came (the device holds the quaternions normalised)
  if (sol->iterations_run == 0 && p->n_poses && sol->pose_q) memcpy(sol->pose_q, p->pose_q, (size_t)p->n_poses * 32);
  return GFS_OK;
}

int gfs_gba_solve(gfs_gba* h, const gfs_lba_problem* p, gfs_lba_solution* sol, volatile const int* stop) {
  return gba_solve_impl(h, p, sol, StopFlag(stop));
}
int gfs_gba_solve_bool(gfs_gba* h, const gfs_lba_problem* p, gfs_lba_solution* sol, const volatile unsigned char* stop) {
  return gba_solve_impl(h, p, sol, StopFlag(stop));
}
int gfs_gba_last_info(const gfs_gba* h, gfs_gba_info* info) {
  GFS_REQUIRE(h && info, GFS_ERR_INVALID_ARG, "gfs_gba_last_info: NULL argument");
  *info = h->info;  // (not under the handle's lock: for the thread that made the call, after it returned)
  return GFS_OK;
}

int gfs_test_gba_panel_rows(void) { return kP; }

int gfs_test_gba_first_trial(gfs_gba* g, const gfs_lba_problem* p, gfs_test_lba_trial* out) {
  GFS_REQUIRE(g && p && out, GFS_ERR_INVALID_ARG, "gfs_test_gba_first_trial: NULL argument");
  GFS_REQUIRE(out->Dinv && out->Hs && out->bs && out->xp && out->xl, GFS_ERR_INVALID_ARG, "gfs_test_gba_first_trial: NULL output array");
  gfs_lba* h = g->lba;
  std::lock_guard<std::mutex> lk(h->mu);
  HostPrep* P;
  int rc = prepare_call(h, p, false, P);
  if (rc) return rc;
  LbaDev D;
  GbaDev G;
  if ((rc = gba_map(g, p, *P, D, G))) return rc;
  LmPhases ph(h, D);
  gfs::DevBuf<double> d_tap;
  GbaReduced reduced{g, ph, G, &d_tap};
  const TrialTap tap{out->Hs, out->bs};
  if ((rc = first_trial(ph, reduced, &tap))) return rc;
  g->info.trials = ph.trials;
  g->info.launches = ph.launches;
  return first_trial_download(h, p, *P, out);
}

// host-only: the structure lists of a caller-order problem (gba_lists.hpp), in the landmark-major edge numbering `order` gives
int gfs_test_gba_lists(int n_poses, int n_points, int n_edges, const uint8_t* pose_fixed, const int32_t* edge_pose, const int32_t* edge_point,
                       int64_t* counts /* n_free, blocks, contributions */, int32_t* order, int32_t* blk_ij, int64_t* blk_begin,
                       int64_t cap_blocks, int32_t* contrib, int64_t cap_contrib, int64_t* pose_begin, int32_t* pose_edges) {
  GFS_REQUIRE(n_poses >= 0 && n_points >= 0 && n_edges >= 0 && counts, GFS_ERR_INVALID_ARG, "gfs_test_gba_lists: invalid argument");
  for (int e = 0; e < n_edges; e++)
    GFS_REQUIRE(edge_point[e] >= 0 && edge_point[e] < n_points && edge_pose[e] >= 0 && edge_pose[e] < n_poses, GFS_ERR_INVALID_ARG,
                "gfs_test_gba_lists: edge %d references an unknown vertex", e);
  std::vector<int32_t> ord, ptb, ef;
  gba_sys::Lists L;
  const int64_t F = gba_sys::landmark_major(n_poses, n_points, n_edges, pose_fixed, edge_pose, edge_point, ord, ptb, ef);
  gba_sys::build_lists(F, n_points, ptb.data(), ef.data(), L);
  counts[0] = F;
  counts[1] = L.n_blocks();
  counts[2] = L.n_contrib();
  if (L.n_blocks() > cap_blocks || L.n_contrib() > cap_contrib) return GFS_ERR_CAPACITY;
  if (order) std::copy(ord.begin(), ord.end(), order);
  for (int64_t b = 0; b < L.n_blocks() && blk_ij; b++) {
    blk_ij[2 * b] = L.blk_i[(size_t)b];
    blk_ij[2 * b + 1] = L.blk_j[(size_t)b];
  }
  if (blk_begin) std::copy(L.blk_begin.begin(), L.blk_begin.end(), blk_begin);
  if (contrib) std::copy(L.contrib.begin(), L.contrib.end(), contrib);
  if (pose_begin) std::copy(L.pose_begin.begin(), L.pose_begin.end(), pose_begin);
  if (pose_edges) std::copy(L.pose_edges.begin(), L.pose_edges.end(), pose_edges);
  return GFS_OK;
}

// host-only: gba_tiles.hpp's arithmetic for n rows and the element (r, c), r >= c
int gfs_test_gba_tile_layout(int64_t n, int64_t r, int64_t c, uint64_t* out /* panels, storage bytes, tile index, element byte offset */) {
  GFS_REQUIRE(n >= 0 && c >= 0 && r >= c && out, GFS_ERR_INVALID_ARG, "gfs_test_gba_tile_layout: invalid argument");
  out[0] = gba_sys::panels((size_t)n);
  out[1] = gba_sys::storage_bytes((size_t)n);
  out[2] = gba_sys::tile_index((size_t)r / kP, (size_t)c / kP);
  out[3] = gba_sys::elem_offset((size_t)r, (size_t)c) * sizeof(double);
  return GFS_OK;
}

}  // extern "C"
