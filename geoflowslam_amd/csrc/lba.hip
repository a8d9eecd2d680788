// Local bundle adjustment for gfx950 (MI355X): the numeric core of Optimizer::LocalBundleAdjustment
// (reference src/Optimizer.cc:1588-2040): g2o BlockSolver_6_3 + OptimizationAlgorithmLevenberg on
// VertexSE3Expmap / VertexSBAPointXYZ with EdgeSE3ProjectXYZ (mono) and EdgeStereoSE3ProjectXYZ (RGB-D) edges,
// Huber kernels, Schur complement on the landmarks, 10 LM iterations with up to 10 lambda trials each.
//
// MI355X design: a window (tens of free poses, a few thousand landmarks, ~50 k edges) is small and windows of one map cannot
// be sharded ("replicas only"), so the work is spread over the chip phase by phase: one launch per phase of
// a Levenberg-Marquardt trial (edge errors, landmark blocks with 16 lanes per landmark, pose blocks, Schur products with one
// workgroup per pose pair, the reduced solve, back-substitution / update, the LM decision), the LM state lives in HBM
// (LbaState) and the host only reads two mapped flags per trial.  The reduced pose system is factored by one workgroup with a
// blocked 6-wide LDL^T: in LDS while its packed triangle fits (<= 30 free poses, 130 KB), in place in HBM / L2 with the
// current panel staged in LDS for larger windows.  All sums are taken in a fixed order (deterministic, unlike atomics).
//
// Edge order: edges are stably re-ordered landmark-major on the host so each landmark's observations are
// contiguous (the reference builds them that way, src/Optimizer.cc:1816-1952); a second CSR lists each free
// pose's edges; edge_of[free pose][landmark] gives O(1) co-visibility lookups for the Schur products.
//
// Files: lba_dev.hpp (the device code), gba_dev.hpp (the global bundle adjustment's reduced system), lba_host.hpp (what both handles
// share on the host: preparation, descriptor, stop flag, the queue of LM phases, the download), this file (the local entry points:
// single window, lidar, batch, linearize, test hooks) and gba_host.hpp (gfs_gba and its entry points).  One translation unit: the
// kernels live in an anonymous namespace and both handles launch them.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <thread>

#include "lba_dev.hpp"
#include "gba_dev.hpp"  // the global bundle adjustment's assembly, tiled factorisation and substitutions (gfs_gba_solve)
#include "gba_lists.hpp"
#include "eg_dev.hpp"  // the essential graph's linearisation, assembly, update and point correction (gfs_essential_graph_optimize)
#include "eg_lists.hpp"
#include "lba_host.hpp"

namespace {

// The lidar key-frames of a window (lidar_prepare): their association and compaction are queued on the handle's stream
struct LidarRun {
  int n_kf = 0, n_free = 0, total = 0;
  std::vector<int> kf_of_pose;  // [n_poses] lidar key-frame or -1
};

// What every local call starts with: the prepared window uploaded and described, its Schur path chosen, the lidar key-frames attached
// -> the descriptor (kept as the handle's last) and the dynamic LDS of the reduced solve.
int local_window(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, int mode, const LidarRun* lid, LbaDev& D, size_t& solve_lds) {
  int rc;
  if ((rc = upload(h, P, h->stream))) return rc;
  describe(h, p, P, mode, D);
  if ((rc = choose_schur(h, p, P, h->stream, D))) return rc;
  if (lid && lid->n_kf > 0) {  // LocalVisualLidarBA: the lidar key-frames' workgroups go ahead of the reprojection edges' in k_lba_errors
    D.n_lidar_kf = lid->n_kf;
    D.n_lidar_free = lid->n_free;
    bind(D.lkf, h->d_lkf.p);
    bind(D.lkf_free, h->d_lkf_free.p);
    bind(D.lcloud, h->d_lcloud.p);
    bind(D.l_cnt, h->d_lcnt.p);
    bind(D.l_idx, h->d_lidx.p);
    bind(D.l_plane, h->d_leplane.p);
    bind(D.l_s, h->d_les.p);
    bind(D.l_chi2, h->d_lchi2.p);
    D.l_info = gfs_lidar::edge_information();
    D.l_huber = gfs_lidar::edge_huber_delta();
    D.n_err_blocks += lid->n_kf;
  }
  const size_t n = 6 * (size_t)P.n_free;
  solve_lds = (P.n_free <= kMaxFreeLds ? n * (n + 1) / 2 + 8 * n + 8 : 7 * n + 8) * sizeof(double);
  GFS_REQUIRE(solve_lds <= 160 * 1024, GFS_ERR_CAPACITY, "gfs_lba: %d free poses exceed the solver's workspace", P.n_free);
  h->last_desc = D;
  return GFS_OK;
}

// The reduced system of a local trial (LmPhases::trial): the Schur products by the path choose_schur took, then one workgroup factors
// and solves -- in LDS while the packed triangle fits, in place in HBM beyond.
struct SchurAndSolve {
  LmPhases& ph;
  size_t solve_lds;
  int operator()(int gate, const TrialTap* tap) const {
    const LbaDev& D = ph.D;
    const int n = 6 * D.n_free, npairs = D.n_free * (D.n_free + 1) / 2;
    if (npairs > 0 && D.schur_mfma) {
      if (D.n_pair_tiles == 1)
        LM_LAUNCH(ph, "k_lba_schur_mfma", k_lba_schur_mfma<true>, dim3(D.n_schur_chunks), dim3(kMk), schur_mfma_lds_bytes(D), D, gate);
      else
        LM_LAUNCH(ph, "k_lba_schur_mfma", k_lba_schur_mfma<false>, dim3(D.n_schur_chunks * D.n_pair_tiles), dim3(kMk), schur_mfma_lds_bytes(D), D, gate);
      LM_LAUNCH(ph, "k_lba_schur_reduce", k_lba_schur_reduce_mfma, dim3(gfs::div_up(n * (n + 1) / 2 + n, kMk)), dim3(kMk), 0, D, gate);
    } else if (npairs > 0 && D.schur_sub) {
      LM_LAUNCH(ph, "k_lba_schur_chunks", k_lba_schur_chunks, dim3(D.n_schur_chunks * D.n_pair_tiles), dim3(kMk), schur_lds_bytes(D), D, gate);
      LM_LAUNCH(ph, "k_lba_schur_reduce", k_lba_schur_reduce, dim3(gfs::div_up(n * (n + 1) / 2 + n, kMk)), dim3(kMk), 0, D, gate);
    } else if (npairs > 0) {
      LM_LAUNCH(ph, "k_lba_schur", k_lba_schur, dim3(npairs), dim3(kMk), 0, D, gate);
    }
    if (tap && n > 0) {  // stream-ordered: behind the Schur launches, ahead of the factorisation
      GFS_HIP(hipMemcpyAsync(tap->Hs, ph.h->d_Hs.p, (size_t)n * (n + 1) / 2 * sizeof(double), hipMemcpyDeviceToHost, ph.s));
      GFS_HIP(hipMemcpyAsync(tap->bs, ph.h->d_bs.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ph.s));
    }
    if (D.n_free <= kMaxFreeLds)
      LM_LAUNCH(ph, "k_lba_solve", k_lba_solve<true>, dim3(1), dim3(kThreads), solve_lds, D, gate);
    else
      LM_LAUNCH(ph, "k_lba_solve", k_lba_solve<false>, dim3(1), dim3(kThreads), solve_lds, D, gate);
    return GFS_OK;
  }
};

// No LM loop: the errors of the estimate as it came -- with `blocks` (gfs_lba_linearize) the system's blocks too -- and the results,
// drained.
int linearize_only(LmPhases& ph, bool blocks) {
  int rc = ph.init();
  if (!rc) rc = blocks ? ph.build(1, 0) : ph.errors(0, 0);
  if (!rc && !blocks) rc = ph.begin(1, 0);
  if (!rc) rc = ph.finish(1);
  if (rc) return rc;
  GFS_HIP(hipStreamSynchronize(ph.s));
  return GFS_OK;
}

// The LM loop of gfs_lba_solve / gfs_lba_solve_lidar: the host runs ONE ITERATION AHEAD of what it knows.  Behind the decide kernel of
// iteration k's trial it queues the whole of iteration k + 1 -- build group and first trial -- GATED on the device by what that kernel
// decides (LbaState::spec_ok: trial accepted, loop goes on; every kernel of a gated launch leaves at once otherwise), and only then
// waits for decide k's flags (an event behind it, the flags in host-mapped memory).  An accepted trial -- the rule -- finds the GPU
// already at work on the next iteration while the host wakes up and queues the one after: the ~24 us round trip and the ~40 us of
// launch calls per iteration are off the critical path.  A rejected trial costs the launches of one gated iteration (~35 us) and is
// retried ungated.  Same kernels in the same order per executed trial: bit-identical results.  The caller's stop flag is looked at
// where g2o looks (top of an iteration, end of a rejected trial); if it is up when an iteration is already running ahead, that
// iteration is DISCARDED: its trial wrote only the other estimate buffer, the scalar state decide k left is put back from its snapshot
// (k_lba_restore) and the errors are evaluated again at that estimate -- what the loop without the look-ahead would have left.
int solve_window(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, StopFlag stop, const LidarRun* lid) {
  LbaDev D;
  size_t solve_lds;
  int rc = local_window(h, p, P, 0, lid, D, solve_lds);
  if (rc) return rc;
  static const bool timing = getenv("GFS_LBA_TIMING") != nullptr;
  if (timing) GFS_HIP(hipStreamSynchronize(h->stream));
  const auto Ta = std::chrono::steady_clock::now();
  LmPhases ph(h, D);
  if (p->iterations <= 0) return linearize_only(ph, false);
  SchurAndSolve reduced{ph, solve_lds};
  if ((rc = ph.init())) return rc;
  if (!(stop && *stop)) {
    int iteration = 0;
    if ((rc = ph.build(0, 0)) || (rc = ph.trial(0, reduced, nullptr))) return rc;
    int waiting = ph.n_decides - 1;  // the decide whose verdict the host waits for next
    for (;;) {
      const bool ahead = iteration + 1 < p->iterations;
      if (ahead && ((rc = ph.build(iteration + 1, 1)) || (rc = ph.trial(1, reduced, nullptr)))) return rc;  // gated on decide `waiting`
      const int* f;
      if ((rc = ph.verdict(waiting, f))) return rc;
      const bool again = f[0] != 0, terminate = f[1] != 0;
      if (again) {  // rejected: what was queued ahead has left (or is leaving) untouched
        if (stop && *stop) {
          if ((rc = ph.force_decide())) return rc;
          tl_stop_script.ahead = ahead ? 1 : 0;
          break;
        }
        if ((rc = ph.trial(0, reduced, nullptr))) return rc;
        waiting = ph.n_decides - 1;
        continue;
      }
      if (terminate || !ahead) break;
      iteration++;  // accepted, the loop goes on: iteration `iteration` is already running (decide waiting + 1)
      if (stop && *stop) {  // ... but g2o would not have started it: put decide `waiting`'s state back
        const int cur = f[2], iters = f[3];
        const double* snap = reinterpret_cast<const double*>(f + 4);
        const double lambda = snap[0], last_chi = snap[1];
        GFS_HIP(hipStreamSynchronize(ph.s));  // (the iteration running ahead: let it finish, nothing reads the snapshot slot meanwhile)
        LM_LAUNCH(ph, "k_lba_restore", k_lba_restore, dim3(1), dim3(64), 0, D, cur, iters, lambda, last_chi);
        if ((rc = ph.errors(0, 0))) return rc;
        tl_stop_script.discarded++;
        tl_stop_script.ahead = 1;
        break;
      }
      waiting = waiting + 1;
    }
  }
  if ((rc = ph.finish(0))) return rc;
  if (timing) {
    GFS_HIP(hipStreamSynchronize(ph.s));
    fprintf(stderr, "  run: LM loop %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - Ta).count());
  }
  return GFS_OK;
}

// pKFi->mnMatchesInliers > 75 -> no lidar edges for this key-frame (src/Optimizer.cc:1338)
constexpr int kLbaLidarMaxInliers = 75;

// The lidar key-frames of a window: local (lLocalKeyFrames, the fixed initial key-frame included), at most 75 inliers, a cloud of at
// least GenerateLidarEdge's minimum.  Their clouds go up concatenated in pose order; the association (one launch) and the compaction
// are queued on the handle's stream.
int lidar_prepare(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* L, LidarRun& R) {
  h->last_lkf_of_pose.clear();  // the device edge lists are about to change: nothing to fetch until this call succeeds
  GFS_REQUIRE(!L->two_camera, GFS_ERR_UNSUPPORTED, "gfs_lba_solve_lidar: key-frames with a second camera are not supported");
  GFS_REQUIRE(L->map && L->map->n >= 5, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: no lidar map, or a map that was never set");
  GFS_REQUIRE(L->map->device == h->device, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: the lidar map lives on device %d, the handle on %d",
              L->map->device, h->device);
  const int NQ = p->n_poses;
  GFS_REQUIRE(NQ == 0 || (L->pose_local && L->matches_inliers && L->cloud_begin), GFS_ERR_INVALID_ARG,
              "gfs_lba_solve_lidar: NULL key-frame arrays");
  GFS_REQUIRE(NQ == 0 || L->cloud_begin[0] == 0, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: cloud_begin[0] must be 0");
  const int min_cloud = gfs_lidar::min_cloud();
  R = LidarRun{};
  R.kf_of_pose.assign(NQ, -1);
  long long total = 0;
  for (int i = 0; i < NQ; i++) {
    const int n = L->cloud_begin[i + 1] - L->cloud_begin[i];
    GFS_REQUIRE(n >= 0, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: cloud_begin decreases at pose %d", i);
    if (L->pose_local[i] && L->matches_inliers[i] <= kLbaLidarMaxInliers && n >= min_cloud) {
      R.kf_of_pose[i] = R.n_kf++;
      total += n;
    }
  }
  GFS_REQUIRE(total <= h->lidar_cap, GFS_ERR_CAPACITY, "gfs_lba_solve_lidar: %lld cloud points of lidar key-frames exceed the reserved %d",
              total, h->lidar_cap);
  GFS_REQUIRE(total == 0 || L->cloud, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: NULL cloud");
  R.total = (int)total;
  if (R.n_kf == 0) return GFS_OK;
  int at = 0, max_n = 0;
  for (int i = 0; i < NQ; i++) {
    const int k = R.kf_of_pose[i];
    if (k < 0) continue;
    gfs_lidar::WindowKF& K = h->h_lkf.p[k];
    K.pose = i;
    K.begin = at;
    K.n = L->cloud_begin[i + 1] - L->cloud_begin[i];
    for (int c = 0; c < 4; c++) K.q[c] = (float)p->pose_q[4 * (size_t)i + c];  // exact for poses that come from Sophus::SE3f
    for (int c = 0; c < 3; c++) K.t[c] = (float)p->pose_t[3 * (size_t)i + c];
    bool finite = true;
    for (int c = 0; c < 4; c++) finite = finite && std::isfinite(K.q[c]);
    for (int c = 0; c < 3; c++) finite = finite && std::isfinite(K.t[c]);
    GFS_REQUIRE(finite, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: the float pose of key-frame %d is not finite", i);
    memcpy(h->h_lcloud.p + 3 * (size_t)at, L->cloud + 3 * (size_t)L->cloud_begin[i], (size_t)K.n * 12);
    if (!p->pose_fixed[i]) h->h_lkf_free.p[R.n_free++] = k;
    at += K.n;
    max_n = std::max(max_n, K.n);
  }
  hipStream_t s = h->stream;
  GFS_HIP(hipMemcpyAsync(h->d_lkf.p, h->h_lkf.p, (size_t)R.n_kf * sizeof(gfs_lidar::WindowKF), hipMemcpyHostToDevice, s));
  if (R.n_free) GFS_HIP(hipMemcpyAsync(h->d_lkf_free.p, h->h_lkf_free.p, (size_t)R.n_free * sizeof(int), hipMemcpyHostToDevice, s));
  GFS_HIP(hipMemcpyAsync(h->d_lcloud.p, h->h_lcloud.p, (size_t)at * 12, hipMemcpyHostToDevice, s));
  int rc = gfs_lidar::launch_window_assoc(L->map, h->d_lkf.p, R.n_kf, max_n, h->d_lcloud.p, h->d_lflag.p, h->d_lplane.p, h->d_ls.p, s);
  if (rc) return rc;
  GFS_LAUNCH("k_lba_lidar_compact", k_lba_lidar_compact, dim3(R.n_kf), dim3(kMk), 0, s, h->d_lkf.p, h->d_lflag.p, h->d_lplane.p, h->d_ls.p,
             h->d_lcnt.p, h->d_lidx.p, h->d_leplane.p, h->d_les.p);
  return GFS_OK;
}

// the edge counts of the last lidar call, kept for gfs_lba_fetch_lidar_edges (h_lcnt holds them once the stream is done)
void lidar_keep(gfs_lba* h, const gfs_lba_problem* p, const LidarRun& R, int32_t* pose_lidar_edges) {
  h->last_lkf_of_pose = R.kf_of_pose;
  h->last_lbegin.assign(R.n_kf, 0);
  h->last_lcnt.assign(R.n_kf, 0);
  for (int k = 0; k < R.n_kf; k++) {
    h->last_lbegin[k] = h->h_lkf.p[k].begin;
    h->last_lcnt[k] = h->h_lcnt.p[k];
  }
  if (pose_lidar_edges)
    for (int i = 0; i < p->n_poses; i++) pose_lidar_edges[i] = R.kf_of_pose[i] >= 0 ? h->last_lcnt[R.kf_of_pose[i]] : 0;
}

}  // namespace

extern "C" {

// gba: the handle inside a gfs_gba -- no co-visibility table in the staging arena, no packed reduced system
static int lba_create_impl(int device, int max_poses, int max_points, int max_edges, bool gba, gfs_lba** out) {
  GFS_REQUIRE(out && max_poses > 0 && max_points > 0 && max_edges > 0, GFS_ERR_INVALID_ARG, "gfs_lba_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_lba> h(new gfs_lba);
  h->device = device;
  h->max_poses = max_poses;
  h->max_points = max_points;
  h->max_edges = max_edges;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  if (int rc0 = lba_raise_lds_limits(device)) return rc0;
  GFS_HIP(hipHostMalloc((void**)&h->h_flags, 2 * kFlagInts * sizeof(int), hipHostMallocMapped));
  for (int k = 0; k < 2; k++) GFS_HIP(hipEventCreateWithFlags(&h->ev_decide[k], hipEventDisableTiming));
  const size_t NP = max_points, E = max_edges, NQ = max_poses, F = max_poses;
  int rc = 0;
#define A(x) if (!rc) rc = (x)
  A(h->d_q.alloc(NQ * 4));
  A(h->d_t.alloc(NQ * 3));
  A(h->d_X.alloc(NP * 3));
  A(h->d_qt.alloc(NQ * 4));
  A(h->d_tt.alloc(NQ * 3));
  A(h->d_Xt.alloc(NP * 3));
  A(h->d_chi2.alloc(E));
  A(h->d_err.alloc(E * 3));
  A(h->d_Hpl.alloc(E * 18));
  A(h->d_Hll.alloc(NP * 6));
  A(h->d_bl.alloc(NP * 3));
  A(h->d_Dinv.alloc(NP * 6));
  A(h->d_Hpp.alloc(F * 21));
  A(h->d_bp.alloc(F * 6));
  A(h->d_xl.alloc(NP * 3));
  A(h->d_xp.alloc(F * 6));
  A(h->d_stats.alloc(2));
  A(h->d_info.alloc(2));
  A(h->d_state.alloc(1));
  A(h->h_stage.alloc(NQ * (32 + 24 + 4) + NP * (24 + 4) + E * (4 + 4 + 24 + 8 + 1 + 4 + 4) + F * (4 + 4 + (gba ? 0 : NP * 4)) + (NP + 2) * 4 + 4096));
  A(h->d_in.alloc(h->h_stage.n));
  A(h->d_out.alloc(E + 7 * NQ + 3 * NP + 4));
  A(h->h_out.alloc(E + 7 * NQ + 3 * NP + 4));
  A(h->d_part_chi.alloc(E / kMk + 2));
  A(h->d_part_scale.alloc(NP / kMk + 2));
  A(h->d_Hs.alloc(gba ? 8 : (size_t)(6 * F) * (6 * F + 1) / 2 + 8));
  A(h->d_bs.alloc(6 * F + 8));
#undef A
  if (rc) return rc;
  *out = h.release();
  return GFS_OK;
}
int gfs_lba_create(int device, int max_poses, int max_points, int max_edges, gfs_lba** out) {
  return lba_create_impl(device, max_poses, max_points, max_edges, false, out);
}

void gfs_lba_destroy(gfs_lba* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  if (h->h_flags) (void)hipHostFree(h->h_flags);
  for (int k = 0; k < 2; k++)
    if (h->ev_decide[k]) (void)hipEventDestroy(h->ev_decide[k]);
  delete h;
}

static int lba_solve_lidar_impl(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* L, gfs_lba_solution* sol,
                                int32_t* pose_lidar_edges, StopFlag stop) {
  StopScriptCall script_call;
  GFS_REQUIRE(h && p && L && sol, GFS_ERR_INVALID_ARG, "gfs_lba_solve_lidar: NULL argument");
  if (stop && *stop) {  // if (pbStopFlag) if (*pbStopFlag) return;  (src/Optimizer.cc:1502-1503)
    gfs::set_error("gfs_lba_solve_lidar: stop flag raised before optimisation");
    return GFS_ERR_STOPPED;
  }
  std::lock_guard<std::mutex> lk(h->mu);
  HostPrep* P;
  static thread_local LidarRun tl_lidar;
  LidarRun& R = tl_lidar;
  int rc = prepare_call(h, p, true, P);
  if (rc) return rc;
  if ((rc = lidar_prepare(h, p, L, R))) return rc;
  if ((rc = solve_window(h, p, *P, stop, &R))) return rc;
  rc = fetch_solution(h, p, *P, sol, [&]() -> int {
    if (R.n_kf) GFS_HIP(hipMemcpyAsync(h->h_lcnt.p, h->d_lcnt.p, (size_t)R.n_kf * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return GFS_OK;
  });
  if (rc) return rc;
  lidar_keep(h, p, R, pose_lidar_edges);
  return GFS_OK;
}
static int lba_solve_impl(gfs_lba* h, const gfs_lba_problem* p, gfs_lba_solution* sol, StopFlag stop) {
  StopScriptCall script_call;
  GFS_REQUIRE(h && p && sol, GFS_ERR_INVALID_ARG, "gfs_lba_solve: NULL argument");
  if (stop && *stop) {  // if (pbStopFlag) if (*pbStopFlag) return;  (src/Optimizer.cc:1955-1956)
    gfs::set_error("gfs_lba_solve: stop flag raised before optimisation");
    return GFS_ERR_STOPPED;
  }
  std::lock_guard<std::mutex> lk(h->mu);
  static const bool timing = getenv("GFS_LBA_TIMING") != nullptr;
  const auto T0 = std::chrono::steady_clock::now();
  HostPrep* P;
  int rc = prepare_call(h, p, true, P);
  if (rc) return rc;
  const auto T1 = std::chrono::steady_clock::now();
  if ((rc = solve_window(h, p, *P, stop, nullptr))) return rc;
  const auto T2 = std::chrono::steady_clock::now();
  if (timing)
    fprintf(stderr, "gfs_lba_solve: prepare %.2f ms, upload + solve %.2f ms\n", std::chrono::duration<double, std::milli>(T1 - T0).count(),
            std::chrono::duration<double, std::milli>(T2 - T1).count());
  return fetch_solution(h, p, *P, sol);
}

// ---- batched windows -----------------------------------------------------------------------------------------------
struct gfs_lba_batch {
  int device = 0, max_windows = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::vector<gfs_lba*> win;       // one workspace per window (their kernels run together: window index = blockIdx.y)
  gfs::DevBuf<LbaDev> d_desc;
  gfs::PinBuf<LbaDev> h_desc;
  gfs::DevBuf<int> d_flags, d_done;
  int* h_done = nullptr;           // pinned copy targets of the done counter (two rounds in flight)
  hipEvent_t ev_round[2] = {nullptr, nullptr};
  gfs::PinBuf<int> h_cur;          // per window: which estimate buffer holds the result
  std::vector<HostPrep> prep;
};

int gfs_lba_batch_create(int device, int max_windows, int max_poses, int max_points, int max_edges, gfs_lba_batch** out) {
  GFS_REQUIRE(out && max_windows > 0, GFS_ERR_INVALID_ARG, "gfs_lba_batch_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_lba_batch> b(new gfs_lba_batch);
  b->device = device;
  b->max_windows = max_windows;
  GFS_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  for (int w = 0; w < max_windows; w++) {
    gfs_lba* h = nullptr;
    const int rc = gfs_lba_create(device, max_poses, max_points, max_edges, &h);
    if (rc) {
      gfs_lba_batch_destroy(b.release());
      return rc;
    }
    b->win.push_back(h);
  }
  int rc = 0;
  if ((rc = b->d_desc.alloc(max_windows)) || (rc = b->h_desc.alloc(max_windows)) || (rc = b->d_flags.alloc(4 * (size_t)max_windows)) ||
      (rc = b->d_done.alloc(1)) || (rc = b->h_cur.alloc(max_windows))) {
    gfs_lba_batch_destroy(b.release());  // the windows (tens of MB of HBM and pinned arenas each) and the stream go with it
    return rc;
  }
  if (hipHostMalloc((void**)&b->h_done, 2 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    b->h_done = nullptr;
    gfs::set_error("gfs_lba_batch_create: hipHostMalloc failed");
    gfs_lba_batch_destroy(b.release());
    return GFS_ERR_HIP;
  }
  for (int k = 0; k < 2; k++)
    if (hipEventCreateWithFlags(&b->ev_round[k], hipEventDisableTiming) != hipSuccess) {
      gfs::set_error("gfs_lba_batch_create: hipEventCreate failed");
      gfs_lba_batch_destroy(b.release());
      return GFS_ERR_HIP;
    }
  b->prep.resize(max_windows);
  *out = b.release();
  return GFS_OK;
}

void gfs_lba_batch_destroy(gfs_lba_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (gfs_lba* x : b->win) gfs_lba_destroy(x);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  for (int k = 0; k < 2; k++)
    if (b->ev_round[k]) (void)hipEventDestroy(b->ev_round[k]);
  if (b->h_done) (void)hipHostFree(b->h_done);
  delete b;
}

// n independent windows (replicas of the single-window solve: "LBA of one map does not shard") solved
// together: per window exactly the arithmetic of gfs_lba_solve, the launches shared by all of them.
static int lba_solve_batch_impl(gfs_lba_batch* b, const gfs_lba_problem* problems, gfs_lba_solution* solutions, int n, StopFlag stop) {
  StopScriptCall script_call;
  GFS_REQUIRE(b && problems && solutions && n > 0, GFS_ERR_INVALID_ARG, "gfs_lba_solve_batch: invalid argument");
  GFS_REQUIRE(n <= b->max_windows, GFS_ERR_CAPACITY, "gfs_lba_solve_batch: %d windows exceed the handle's %d", n, b->max_windows);
  if (stop && *stop) {
    gfs::set_error("gfs_lba_solve_batch: stop flag raised before optimisation");
    return GFS_ERR_STOPPED;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  GFS_HIP(hipSetDevice(b->device));
  hipStream_t s = b->stream;
  static const bool timing = getenv("GFS_LBA_TIMING") != nullptr;
  auto now = []() { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) {
    return std::chrono::duration<double, std::milli>(c - a).count();
  };
  const auto T0 = now();
  // ---- host preparation of every window (edge re-ordering, CSR tables), on a few threads
  std::vector<int> rcs((size_t)n, 0);
  std::vector<std::string> msgs((size_t)n);  // gfs_last_error() is per thread: a worker's message is carried back to the caller's
  {
    static const int cap = getenv("GFS_LBA_THREADS") ? atoi(getenv("GFS_LBA_THREADS")) : 32;
    const int nthreads = std::max(1, std::min(n, std::min(cap, (int)std::thread::hardware_concurrency())));
    auto work = [&](int t) {
      (void)hipSetDevice(b->device);
      for (int w = t; w < n; w += nthreads) {
        rcs[w] = prepare(b->win[w], &problems[w], b->prep[w]);
        if (!rcs[w]) rcs[w] = upload(b->win[w], b->prep[w], s);  // the copy leaves as soon as the window is ready
        if (rcs[w]) msgs[w] = gfs_last_error();
      }
    };
    if (nthreads == 1) {
      work(0);  // one window: no thread to start
    } else {
      std::vector<std::thread> th;
      for (int t = 0; t < nthreads; t++) th.emplace_back(work, t);
      for (auto& x : th) x.join();
    }
  }
  for (int w = 0; w < n; w++)
    if (rcs[w]) {
      gfs::set_error("gfs_lba_solve_batch: window %d: %s", w, msgs[w].c_str());
      return rcs[w];
    }
  const auto T1 = now();
  int max_free = 0, max_err = 1, max_upd = 1, max_lm = 1, max_iter = 0, max_chunk_blocks = 0, max_pair_blocks = 0;
  size_t schur_lds = 0, mfma_lds = 0;
  int max_mfma_blocks = 0;
  bool any_one_block = false, any_multi_block = false;
  for (int w = 0; w < n; w++) {
    LbaDev D;
    describe(b->win[w], &problems[w], b->prep[w], 0, D);  // (uploaded by the workers above)
    if (int rc = choose_schur(b->win[w], &problems[w], b->prep[w], s, D)) return rc;
    b->h_desc.p[w] = D;
    max_free = std::max(max_free, D.n_free);
    max_err = std::max(max_err, D.n_err_blocks);
    max_upd = std::max(max_upd, D.n_upd_blocks);
    max_lm = std::max(max_lm, D.n_lm_wg);
    max_iter = std::max(max_iter, problems[w].iterations);
    if (D.schur_mfma) {
      max_mfma_blocks = std::max(max_mfma_blocks, D.n_schur_chunks * D.n_pair_tiles);
      any_one_block = any_one_block || D.n_pair_tiles == 1;
      any_multi_block = any_multi_block || D.n_pair_tiles != 1;
      mfma_lds = std::max(mfma_lds, schur_mfma_lds_bytes(D));
    } else if (D.schur_sub) {
      max_chunk_blocks = std::max(max_chunk_blocks, D.n_schur_chunks * D.n_pair_tiles);
      schur_lds = std::max(schur_lds, schur_lds_bytes(D));
    } else {
      max_pair_blocks = std::max(max_pair_blocks, D.n_free * (D.n_free + 1) / 2);
    }
  }
  GFS_HIP(hipMemcpyAsync(b->d_desc.p, b->h_desc.p, (size_t)n * sizeof(LbaDev), hipMemcpyHostToDevice, s));
  GFS_HIP(hipMemsetAsync(b->d_done.p, 0, sizeof(int), s));
  const int nmax = 6 * max_free;
  int free_small = 0, free_large = 0;  // largest window solved in LDS / in HBM
  for (int w = 0; w < n; w++) {
    const int f = b->h_desc.p[w].n_free;
    if (f <= kMaxFreeLds)
      free_small = std::max(free_small, f);
    else
      free_large = std::max(free_large, f);
  }
  const size_t lds_small = ((size_t)(6 * free_small) * (6 * free_small + 1) / 2 + 8 * (6 * free_small) + 8) * sizeof(double);
  const size_t lds_large = ((size_t)7 * 6 * free_large + 8) * sizeof(double);
  GFS_REQUIRE(lds_large <= 160 * 1024 - 1024, GFS_ERR_CAPACITY, "gfs_lba_solve_batch: %d free poses exceed the solver's workspace", max_free);
  const LbaDev* DD = b->d_desc.p;
  const auto T2 = now();
  int rounds_run = 0;
  GFS_LAUNCH("kb_lba_init", kb_lba_init, dim3(64, n), dim3(kMk), 0, s, DD);
  const int max_rounds = std::max(max_iter, 0) * 11 + 1;  // (windows with iterations <= 0 leave in the first round, after the errors)
  for (int round = 0; round < max_rounds; round++) {
    GFS_LAUNCH("kb_lba_errors", kb_lba_errors, dim3(max_err, n), dim3(kMk), 0, s, DD, 0);
    GFS_LAUNCH("kb_lba_build_landmarks", kb_lba_build_landmarks, dim3(max_lm, n), dim3(kMk), 0, s, DD);
    if (max_free > 0) GFS_LAUNCH("kb_lba_build_poses", kb_lba_build_poses, dim3(max_free, n), dim3(kPoseWg), 0, s, DD);
    GFS_LAUNCH("kb_lba_begin", kb_lba_begin, dim3(1, n), dim3(kThreads), 0, s, DD, b->d_done.p);
    GFS_LAUNCH("kb_lba_dinv", kb_lba_dinv, dim3(max_upd, n), dim3(kMk), 0, s, DD);
    if (max_mfma_blocks > 0) {
      if (any_one_block) GFS_LAUNCH("kb_lba_schur_mfma", kb_lba_schur_mfma<true>, dim3(max_mfma_blocks, n), dim3(kMk), mfma_lds, s, DD);
      if (any_multi_block) GFS_LAUNCH("kb_lba_schur_mfma", kb_lba_schur_mfma<false>, dim3(max_mfma_blocks, n), dim3(kMk), mfma_lds, s, DD);
      GFS_LAUNCH("kb_lba_schur_reduce", kb_lba_schur_reduce_mfma, dim3(gfs::div_up(nmax * (nmax + 1) / 2 + nmax, kMk), n), dim3(kMk), 0, s, DD);
    }
    if (max_chunk_blocks > 0) {
      GFS_LAUNCH("kb_lba_schur_chunks", kb_lba_schur_chunks, dim3(max_chunk_blocks, n), dim3(kMk), schur_lds, s, DD);
      GFS_LAUNCH("kb_lba_schur_reduce", kb_lba_schur_reduce, dim3(gfs::div_up(nmax * (nmax + 1) / 2 + nmax, kMk), n), dim3(kMk), 0, s, DD);
    }
    if (max_pair_blocks > 0) GFS_LAUNCH("kb_lba_schur", kb_lba_schur, dim3(max_pair_blocks, n), dim3(kMk), 0, s, DD);
    bool any_small = false;
    for (int w = 0; w < n; w++) any_small = any_small || b->h_desc.p[w].n_free <= kMaxFreeLds;
    if (any_small) GFS_LAUNCH("kb_lba_solve", kb_lba_solve<true>, dim3(1, n), dim3(kThreads), lds_small, s, DD);
    if (free_large > 0) GFS_LAUNCH("kb_lba_solve", kb_lba_solve<false>, dim3(1, n), dim3(kThreads), lds_large, s, DD);
    GFS_LAUNCH("kb_lba_update", kb_lba_update, dim3(max_upd, n), dim3(kMk), 0, s, DD);
    GFS_LAUNCH("kb_lba_errors", kb_lba_errors, dim3(max_err, n), dim3(kMk), 0, s, DD, 1);
    const bool force_end = stop && *stop;  // setForceStopFlag: the running iteration is closed, nothing further starts
    GFS_LAUNCH("kb_lba_decide", kb_lba_decide, dim3(n), dim3(64), 0, s, DD, force_end ? 1 : 0, b->d_flags.p, b->d_done.p);
    // The done counter is polled ONE ROUND BEHIND the round just queued: the GPU never idles on the host round trip (a window's
    // state machine lives on the device, a round queued for windows that are all done finds every kernel leaving at once).
    GFS_HIP(hipMemcpyAsync(b->h_done + (round & 1), b->d_done.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GFS_HIP(hipEventRecord(b->ev_round[round & 1], s));
    rounds_run++;
    if (force_end) {
      tl_stop_script.forced++;
      tl_stop_script.ahead = 0;
      GFS_HIP(hipStreamSynchronize(s));
      break;
    }
    if (round >= 1) {
      GFS_HIP(hipEventSynchronize(b->ev_round[(round - 1) & 1]));
      if (b->h_done[(round - 1) & 1] >= n) break;
    }
  }
  const auto T3 = now();
  GFS_LAUNCH("kb_lba_finish", kb_lba_finish, dim3(n), dim3(64), 0, s, DD);
  GFS_LAUNCH("kb_lba_pack", kb_lba_pack, dim3(8, n), dim3(kMk), 0, s, DD);
  std::vector<LbaFetch> F((size_t)n);
  for (int w = 0; w < n; w++) {
    const int rc = lba_fetch_issue(b->win[w], &problems[w], s, F[w]);
    if (rc) return rc;
  }
  GFS_HIP(hipStreamSynchronize(s));
  const auto T4 = now();
  {
    const int nthreads = std::max(1, std::min(n, std::min(32, (int)std::thread::hardware_concurrency())));
    if (nthreads == 1) {
      for (int w = 0; w < n; w++) lba_fetch_finish(&problems[w], b->prep[w], F[w], &solutions[w]);
    } else {
      std::vector<std::thread> th;
      for (int t = 0; t < nthreads; t++)
        th.emplace_back([&, t]() {
          for (int w = t; w < n; w += nthreads) lba_fetch_finish(&problems[w], b->prep[w], F[w], &solutions[w]);
        });
      for (auto& x : th) x.join();
    }
  }
  if (timing)
    fprintf(stderr, "gfs_lba_solve_batch(%d): prepare %.2f, upload %.2f, %d rounds %.2f, download %.2f, scatter %.2f ms\n", n, ms(T0, T1),
            ms(T1, T2), rounds_run, ms(T2, T3), ms(T3, T4), ms(T4, now()));
  return GFS_OK;
}

static int lba_linearize_impl(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* L, double* Hpp, double* Hll, double* Hpl,
                              double* bp, double* bl, double* edge_chi2, double* chi2, double* lidar_chi2, int lidar_cap,
                              int32_t* pose_lidar_edges) {
  GFS_REQUIRE(h && p, GFS_ERR_INVALID_ARG, "gfs_lba_linearize: NULL argument");
  std::lock_guard<std::mutex> lk(h->mu);
  HostPrep* Pp;
  int rc = prepare_call(h, p, true, Pp);
  if (rc) return rc;
  const HostPrep& P = *Pp;
  LidarRun R;
  if (L && (rc = lidar_prepare(h, p, L, R))) return rc;
  LbaDev D;
  size_t solve_lds;
  if ((rc = local_window(h, p, P, 1, L ? &R : nullptr, D, solve_lds))) return rc;
  LmPhases ph(h, D);
  if ((rc = linearize_only(ph, true))) return rc;
  if (L) {  // the per-edge chi2 of the lidar edges, in g2o's order (key-frames in pose order, then cloud order)
    if (R.n_kf) GFS_HIP(hipMemcpyAsync(h->h_lcnt.p, h->d_lcnt.p, (size_t)R.n_kf * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GFS_HIP(hipStreamSynchronize(h->stream));
    lidar_keep(h, p, R, pose_lidar_edges);
    int at = 0;
    for (int k = 0; k < R.n_kf && lidar_chi2; k++) {
      const int m = std::min(h->last_lcnt[k], lidar_cap - at);
      if (m > 0) GFS_HIP(hipMemcpy(lidar_chi2 + at, h->d_lchi2.p + h->last_lbegin[k], (size_t)m * 8, hipMemcpyDeviceToHost));
      at += std::max(m, 0);
    }
  }
  const int E = p->n_edges, NP = p->n_points, F = P.n_free;
  std::vector<double> hpp((size_t)F * 21), hll((size_t)NP * 6), hpl((size_t)E * 18), chi(E);
  if (F) GFS_HIP(hipMemcpy(hpp.data(), h->d_Hpp.p, hpp.size() * 8, hipMemcpyDeviceToHost));
  if (NP) GFS_HIP(hipMemcpy(hll.data(), h->d_Hll.p, hll.size() * 8, hipMemcpyDeviceToHost));
  if (E) GFS_HIP(hipMemcpy(hpl.data(), h->d_Hpl.p, hpl.size() * 8, hipMemcpyDeviceToHost));
  if (E) GFS_HIP(hipMemcpy(chi.data(), h->d_chi2.p, chi.size() * 8, hipMemcpyDeviceToHost));
  if (bp && F) GFS_HIP(hipMemcpy(bp, h->d_bp.p, (size_t)F * 48, hipMemcpyDeviceToHost));
  if (bl && NP) GFS_HIP(hipMemcpy(bl, h->d_bl.p, (size_t)NP * 24, hipMemcpyDeviceToHost));
  double stats[2];
  GFS_HIP(hipMemcpy(stats, h->d_stats.p, sizeof(stats), hipMemcpyDeviceToHost));
  if (chi2) *chi2 = stats[0];
  if (Hpp)
    for (int f = 0; f < F; f++) {
      int o = 0;
      for (int a = 0; a < 6; a++)
        for (int c = a; c < 6; c++) {
          Hpp[36 * (size_t)f + a + 6 * c] = hpp[21 * (size_t)f + o];
          Hpp[36 * (size_t)f + c + 6 * a] = hpp[21 * (size_t)f + o];
          o++;
        }
    }
  if (Hll)
    for (int l = 0; l < NP; l++) {
      const double* s6 = &hll[6 * (size_t)l];
      double* o = Hll + 9 * (size_t)l;
      o[0] = s6[0];
      o[1] = o[3] = s6[1];
      o[2] = o[6] = s6[2];
      o[4] = s6[3];
      o[5] = o[7] = s6[4];
      o[8] = s6[5];
    }
  for (int k = 0; k < E; k++) {
    const int e = P.order[k];
    if (edge_chi2) edge_chi2[e] = chi[k];
    if (Hpl)
      for (int a = 0; a < 6; a++)
        for (int c = 0; c < 3; c++) Hpl[18 * (size_t)e + a + 6 * c] = hpl[18 * (size_t)k + 3 * a + c];
  }
  return GFS_OK;
}

int gfs_lba_linearize(gfs_lba* h, const gfs_lba_problem* p, double* Hpp, double* Hll, double* Hpl, double* bp, double* bl,
                      double* edge_chi2, double* chi2) {
  return lba_linearize_impl(h, p, nullptr, Hpp, Hll, Hpl, bp, bl, edge_chi2, chi2, nullptr, 0, nullptr);
}

int gfs_lba_linearize_lidar(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* lidar, double* Hpp, double* Hll, double* Hpl,
                            double* bp, double* bl, double* edge_chi2, double* chi2, double* lidar_edge_chi2, int cap,
                            int32_t* pose_lidar_edges) {
  GFS_REQUIRE(lidar && cap >= 0, GFS_ERR_INVALID_ARG, "gfs_lba_linearize_lidar: invalid argument");
  return lba_linearize_impl(h, p, lidar, Hpp, Hll, Hpl, bp, bl, edge_chi2, chi2, lidar_edge_chi2, cap, pose_lidar_edges);
}

int gfs_lba_lidar_reserve(gfs_lba* h, int max_cloud_points) {
  GFS_REQUIRE(h && max_cloud_points >= 0, GFS_ERR_INVALID_ARG, "gfs_lba_lidar_reserve: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipStreamSynchronize(h->stream));
  const size_t N = std::max(max_cloud_points, 1), NQ = h->max_poses;
  int rc = 0;
#define A(x) if (!rc) rc = (x)
  A(h->h_lcloud.alloc(3 * N));
  A(h->d_lcloud.alloc(3 * N));
  A(h->d_lflag.alloc(N));
  A(h->d_lplane.alloc(N));
  A(h->d_ls.alloc(N));
  A(h->d_lidx.alloc(N));
  A(h->d_leplane.alloc(N));
  A(h->d_les.alloc(N));
  A(h->d_lchi2.alloc(N));
  A(h->h_lkf.alloc(NQ));
  A(h->d_lkf.alloc(NQ));
  A(h->h_lkf_free.alloc(NQ));
  A(h->d_lkf_free.alloc(NQ));
  A(h->h_lcnt.alloc(NQ));
  A(h->d_lcnt.alloc(NQ));
#undef A
  // + one partial sum of k_lba_errors per lidar key-frame.  The plain solve uses this buffer too: it only grows, and the old one is
  // kept until the new one exists.
  const size_t need_chi = (size_t)h->max_edges / kMk + 2 + NQ;
  if (!rc && h->d_part_chi.n < need_chi) {
    double* np_ = nullptr;
    if (hipMalloc((void**)&np_, need_chi * sizeof(double)) != hipSuccess) {
      gfs::set_error("gfs_lba_lidar_reserve: hipMalloc of %zu partial sums failed", need_chi);
      rc = GFS_ERR_HIP;
    } else {
      (void)hipFree(h->d_part_chi.p);
      h->d_part_chi.p = np_;
      h->d_part_chi.n = need_chi;
    }
  }
  h->lidar_cap = rc ? 0 : max_cloud_points;
  h->last_lkf_of_pose.clear();
  return rc;
}

int gfs_lba_solve(gfs_lba* h, const gfs_lba_problem* p, gfs_lba_solution* sol, volatile const int* stop) {
  return lba_solve_impl(h, p, sol, StopFlag(stop));
}
int gfs_lba_solve_bool(gfs_lba* h, const gfs_lba_problem* p, gfs_lba_solution* sol, const volatile unsigned char* stop) {
  return lba_solve_impl(h, p, sol, StopFlag(stop));
}
int gfs_lba_solve_batch(gfs_lba_batch* b, const gfs_lba_problem* problems, gfs_lba_solution* solutions, int n, volatile const int* stop) {
  return lba_solve_batch_impl(b, problems, solutions, n, StopFlag(stop));
}
int gfs_lba_solve_lidar(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* lidar, gfs_lba_solution* sol,
                        int32_t* pose_lidar_edges, volatile const int* stop) {
  return lba_solve_lidar_impl(h, p, lidar, sol, pose_lidar_edges, StopFlag(stop));
}
int gfs_lba_solve_lidar_bool(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* lidar, gfs_lba_solution* sol,
                             int32_t* pose_lidar_edges, const volatile unsigned char* stop) {
  return lba_solve_lidar_impl(h, p, lidar, sol, pose_lidar_edges, StopFlag(stop));
}

int gfs_lba_fetch_lidar_edges(gfs_lba* h, int pose, int32_t* index, float* plane, float* s, int cap, int32_t* n) {
  GFS_REQUIRE(h && n && cap >= 0 && (cap == 0 || (index && plane && s)), GFS_ERR_INVALID_ARG, "gfs_lba_fetch_lidar_edges: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_REQUIRE(pose >= 0 && pose < (int)h->last_lkf_of_pose.size(), GFS_ERR_INVALID_ARG,
              "gfs_lba_fetch_lidar_edges: pose %d outside the last lidar call", pose);
  GFS_HIP(hipSetDevice(h->device));
  const int k = h->last_lkf_of_pose[pose];
  const int cnt = k >= 0 ? h->last_lcnt[k] : 0;
  *n = cnt;
  const int m = std::min(cnt, cap);
  if (m == 0) return GFS_OK;
  const size_t o = h->last_lbegin[k];
  GFS_HIP(hipMemcpy(index, h->d_lidx.p + o, (size_t)m * 4, hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(plane, h->d_leplane.p + o, (size_t)m * 16, hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(s, h->d_les.p + o, (size_t)m * 4, hipMemcpyDeviceToHost));
  return GFS_OK;
}

int gfs_test_lba_stop_at_look(int look) {
  tl_stop_script.at = look < 0 ? -1 : look;
  return GFS_OK;
}
int gfs_test_lba_last_looks(int32_t* looks, int32_t* discarded, int32_t* forced_decides, int32_t* ahead_at_stop) {
  const StopScript& T = tl_stop_script;
  if (looks) *looks = T.looks;
  if (discarded) *discarded = T.discarded;
  if (forced_decides) *forced_decides = T.forced;
  if (ahead_at_stop) *ahead_at_stop = T.ahead;
  return GFS_OK;
}

int gfs_test_lba_first_trial(gfs_lba* h, const gfs_lba_problem* p, gfs_test_lba_trial* out) {
  GFS_REQUIRE(h && p && out, GFS_ERR_INVALID_ARG, "gfs_test_lba_first_trial: NULL argument");
  GFS_REQUIRE(out->Dinv && out->Hs && out->bs && out->xp && out->xl, GFS_ERR_INVALID_ARG, "gfs_test_lba_first_trial: NULL output array");
  std::lock_guard<std::mutex> lk(h->mu);
  HostPrep* P;
  int rc = prepare_call(h, p, true, P);
  if (rc) return rc;
  LbaDev D;
  size_t solve_lds;
  if ((rc = local_window(h, p, *P, 0, nullptr, D, solve_lds))) return rc;
  LmPhases ph(h, D);
  SchurAndSolve reduced{ph, solve_lds};
  const TrialTap tap{out->Hs, out->bs};
  if ((rc = first_trial(ph, reduced, &tap))) return rc;
  return first_trial_download(h, p, *P, out);
}

}  // extern "C"

#include "gba_host.hpp"
#include "eg_host.hpp"
