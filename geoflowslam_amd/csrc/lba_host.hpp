// Host code that the local and the global bundle adjustment share (lba.hip, gba_host.hpp): the handle, the host preparation of a
// problem, its upload and descriptor, the stop flag, the queue of LM phases and the result download.  Included behind lba_dev.hpp.
#pragma once

struct gfs_lba {
  int device, max_poses, max_points, max_edges;
  hipStream_t stream;
  std::mutex mu;
  int* h_flags = nullptr;  // host-mapped, two slots of kFlagInts ints: {again, terminate, cur, iters | lambda, last_chi (doubles)} written by k_lba_decide
  hipEvent_t ev_decide[2] = {nullptr, nullptr};  // behind decide i: event i & 1 -- the host waits for THIS, not for what is queued behind it
  LbaDev last_desc;        // the window of the last call
  gfs::DevBuf<LbaState> d_state;
  gfs::PinBuf<unsigned char> h_stage;  // pinned staging arena for the problem upload (pageable copies cost ~2 ms each)
  gfs::DevBuf<double> d_part_chi, d_part_scale, d_Hs, d_bs;
  gfs::DevBuf<double> d_schur_part, d_schur_part_b;  // grown on demand (choose_schur)
  gfs::DevBuf<unsigned char> d_in;      // the window's inputs, same layout as h_stage (Stager)
  gfs::DevBuf<double> d_out;            // the window's results (b_pack)
  gfs::PinBuf<double> h_out;
  gfs::DevBuf<double> d_q, d_t, d_X, d_qt, d_tt, d_Xt, d_chi2, d_err, d_Hpl, d_Hll, d_bl, d_Dinv, d_Hpp, d_bp, d_xl, d_xp, d_stats;
  gfs::DevBuf<int> d_info;
  // LocalVisualLidarBA (gfs_lba_lidar_reserve): the concatenated clouds of a window's lidar key-frames and their edges
  int lidar_cap = 0;
  gfs::PinBuf<float> h_lcloud;
  gfs::DevBuf<float> d_lcloud, d_ls, d_les;
  gfs::PinBuf<gfs_lidar::WindowKF> h_lkf;
  gfs::DevBuf<gfs_lidar::WindowKF> d_lkf;
  gfs::PinBuf<int> h_lkf_free, h_lcnt;
  gfs::DevBuf<int> d_lkf_free, d_lcnt, d_lidx;
  gfs::DevBuf<uint8_t> d_lflag;
  gfs::DevBuf<float4> d_lplane, d_leplane;
  gfs::DevBuf<double> d_lchi2;
  // the last lidar call's key-frames, for gfs_lba_fetch_lidar_edges: lidar key-frame of each pose (-1: none), its offset and edges
  std::vector<int> last_lkf_of_pose, last_lbegin, last_lcnt;
};

namespace {

// Host preparation of a window, written straight into the handle's pinned arena (the device block d_in has the same layout, one
// copy moves it): landmark-major edge order, the CSR tables, the co-visibility table.
struct HostPrep {
  std::vector<int> order;  // landmark-major position -> original edge
  int n_free = 0;
  double *q0 = nullptr, *t0 = nullptr, *X0 = nullptr, *obs = nullptr, *w = nullptr;
  int *free_index = nullptr, *free_pose = nullptr, *e_pose = nullptr, *e_point = nullptr, *pt_begin = nullptr, *pose_begin = nullptr,
      *pose_edges = nullptr, *edge_of = nullptr;
  unsigned char* stereo = nullptr;
  int* e_dup = nullptr;  // NULL when the window has no duplicate (pose, landmark) edges
  int* lm_wg = nullptr;  // landmark ranges of b_build_landmarks' workgroups
  int n_lm_wg = 0;
  size_t used = 0;  // bytes of the arena in use
};

// covis = false (gfs_gba_solve): no [free pose][landmark] table -- at map size it would be gigabytes, and the structure lists take its
// place; the duplicate table comes from the landmark-major order itself (a pose's edges on one landmark are neighbours in it)
int prepare(gfs_lba* h, const gfs_lba_problem* p, HostPrep& P, bool covis = true) {
  GFS_REQUIRE(p && p->n_poses >= 0 && p->n_points >= 0 && p->n_edges >= 0, GFS_ERR_INVALID_ARG, "gfs_lba: invalid problem");
  GFS_REQUIRE(p->n_poses <= h->max_poses && p->n_points <= h->max_points && p->n_edges <= h->max_edges, GFS_ERR_CAPACITY,
              "gfs_lba: problem (%d poses, %d points, %d edges) exceeds handle capacity (%d, %d, %d)", p->n_poses,
              p->n_points, p->n_edges, h->max_poses, h->max_points, h->max_edges);
  const int E = p->n_edges, NP = p->n_points, NQ = p->n_poses;
  int nf = 0;
  for (int i = 0; i < NQ; i++) nf += p->pose_fixed[i] ? 0 : 1;
  P.n_free = nf;
  {  // carve the arena
    unsigned char* base = h->h_stage.p;
    size_t at = 0;
    auto take = [&](size_t bytes) {
      unsigned char* r = base + at;
      at = (at + bytes + 63) & ~(size_t)63;
      return r;
    };
    P.q0 = (double*)take((size_t)NQ * 32);
    P.t0 = (double*)take((size_t)NQ * 24);
    P.X0 = (double*)take((size_t)NP * 24);
    P.obs = (double*)take((size_t)E * 24);
    P.w = (double*)take((size_t)E * 8);
    P.free_index = (int*)take((size_t)NQ * 4);
    P.free_pose = (int*)take((size_t)nf * 4);
    P.e_pose = (int*)take((size_t)E * 4);
    P.e_point = (int*)take((size_t)E * 4);
    P.pt_begin = (int*)take((size_t)(NP + 1) * 4);
    P.pose_begin = (int*)take((size_t)(nf + 1) * 4);
    P.pose_edges = (int*)take((size_t)E * 4);
    P.edge_of = covis ? (int*)take((size_t)nf * NP * 4) : nullptr;
    P.stereo = take((size_t)E);
    P.lm_wg = (int*)take((size_t)(NP + 2) * 4);
    P.used = at;  // (grows by the duplicate table below when the window has any)
    P.e_dup = (int*)take((size_t)E * 4);
    GFS_REQUIRE(at <= h->h_stage.n, GFS_ERR_CAPACITY, "gfs_lba: staging arena too small");
  }
  bool any_dup = false;
  if (NQ) memcpy(P.q0, p->pose_q, (size_t)NQ * 32);
  if (NQ) memcpy(P.t0, p->pose_t, (size_t)NQ * 24);
  if (NP) memcpy(P.X0, p->points, (size_t)NP * 24);
  nf = 0;
  for (int i = 0; i < NQ; i++) {
    P.free_index[i] = -1;
    if (!p->pose_fixed[i]) {
      P.free_index[i] = nf;
      P.free_pose[nf++] = i;
    }
  }
  std::fill(P.pt_begin, P.pt_begin + NP + 1, 0);
  for (int e = 0; e < E; e++) {
    GFS_REQUIRE(p->edge_point[e] >= 0 && p->edge_point[e] < NP && p->edge_pose[e] >= 0 && p->edge_pose[e] < NQ,
                GFS_ERR_INVALID_ARG, "gfs_lba: edge %d references an unknown vertex", e);
    P.pt_begin[p->edge_point[e] + 1]++;
  }
  for (int l = 0; l < NP; l++) P.pt_begin[l + 1] += P.pt_begin[l];
  {  // whole landmarks packed into workgroups of at most kMk edges (b_build_landmarks)
    int nw = 0, l = 0;
    while (l < NP) {
      P.lm_wg[nw++] = l;
      const int base = P.pt_begin[l];
      int l2 = l + 1;
      while (l2 < NP && P.pt_begin[l2 + 1] - base <= kMk) l2++;
      l = l2;
    }
    P.lm_wg[nw] = NP;
    P.n_lm_wg = nw;
  }
  P.order.assign(E, 0);
  {
    std::vector<int> pos(P.pt_begin, P.pt_begin + NP);
    for (int e = 0; e < E; e++) P.order[pos[p->edge_point[e]]++] = e;  // stable
  }
  std::fill(P.pose_begin, P.pose_begin + P.n_free + 1, 0);
  if (covis) std::fill(P.edge_of, P.edge_of + (size_t)P.n_free * NP, -1);
  static thread_local std::vector<int> tl_first;  // covis = false: the first edge of free pose f on the last landmark it was met on
  if (!covis) tl_first.assign(P.n_free, -1);
  for (int k = 0; k < E; k++) {
    const int e = P.order[k];
    P.e_pose[k] = p->edge_pose[e];
    P.e_point[k] = p->edge_point[e];
    for (int c = 0; c < 3; c++) P.obs[3 * (size_t)k + c] = p->edge_obs[3 * (size_t)e + c];
    P.w[k] = p->edge_inv_sigma2[e];
    P.stereo[k] = p->edge_stereo[e] ? 1 : 0;
    const int f = P.free_index[P.e_pose[k]];
    P.e_dup[k] = -1;
    if (f >= 0) {
      P.pose_begin[f + 1]++;
      int& slot = covis ? P.edge_of[(size_t)f * NP + P.e_point[k]] : tl_first[f];
      if (!covis && slot >= 0 && P.e_point[slot] != P.e_point[k]) slot = -1;  // (that edge was on an earlier landmark)
      if (slot < 0) {
        slot = k;
      } else {  // a second edge between this pose and this landmark
        P.e_dup[k] = slot;
        any_dup = true;
      }
    }
  }
  if (any_dup)
    P.used = (size_t)((unsigned char*)(P.e_dup + E) - h->h_stage.p);
  else
    P.e_dup = nullptr;
  for (int f = 0; f < P.n_free; f++) P.pose_begin[f + 1] += P.pose_begin[f];
  {
    std::vector<int> pos(P.pose_begin, P.pose_begin + P.n_free);
    for (int k = 0; k < E; k++) {
      const int f = P.free_index[P.e_pose[k]];
      if (f >= 0) P.pose_edges[pos[f]++] = k;
    }
  }
  return GFS_OK;
}

// a single-problem call, under the handle's lock: the device, the problem prepared in this thread's HostPrep (its vectors keep their
// capacity between calls: no allocation on the hot path)
int prepare_call(gfs_lba* h, const gfs_lba_problem* p, bool covis, HostPrep*& P) {
  GFS_HIP(hipSetDevice(h->device));
  static thread_local HostPrep tl_prep;
  P = &tl_prep;
  return prepare(h, p, tl_prep, covis);
}

// the arena of a prepared window -> the device block (one copy, on stream s)
int upload(gfs_lba* h, const HostPrep& P, hipStream_t s) {
  if (P.used) GFS_HIP(hipMemcpyAsync(h->d_in.p, h->h_stage.p, P.used, hipMemcpyHostToDevice, s));
  return GFS_OK;
}

// a descriptor member takes a pointer (the members carry the GLOBAL address space in the device pass: lba_dev.hpp)
template <class M, class T>
void bind(M& m, T* p) { m = (M)p; }

// describes a prepared window for the kernels (no HIP call); the Schur path is choose_schur's
void describe(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, int mode, LbaDev& D) {
  const int E = p->n_edges, NP = p->n_points;
  D = LbaDev{};
  auto dev = [&](const void* host) -> const void* { return host ? h->d_in.p + ((const unsigned char*)host - h->h_stage.p) : nullptr; };
  bind(D.pose_q0, dev(P.q0));
  bind(D.pose_t0, dev(P.t0));
  bind(D.points0, dev(P.X0));
  bind(D.free_index, dev(P.free_index));
  bind(D.free_pose, dev(P.free_pose));
  bind(D.e_pose, dev(P.e_pose));
  bind(D.e_point, dev(P.e_point));
  bind(D.e_obs, dev(P.obs));
  bind(D.e_w, dev(P.w));
  bind(D.pt_begin, dev(P.pt_begin));
  bind(D.pose_begin, dev(P.pose_begin));
  bind(D.pose_edges, dev(P.pose_edges));
  bind(D.edge_of, dev(P.edge_of));
  bind(D.e_stereo, dev(P.stereo));
  bind(D.e_dup, dev(P.e_dup));
  bind(D.lm_wg, dev(P.lm_wg));
  D.n_lm_wg = P.n_lm_wg;
  D.n_poses = p->n_poses;
  D.n_points = NP;
  D.n_edges = E;
  D.n_free = P.n_free;
  D.fx = p->fx;
  D.fy = p->fy;
  D.cx = p->cx;
  D.cy = p->cy;
  D.bf = p->bf;
  D.huber_mono = p->huber_mono;
  D.huber_stereo = p->huber_stereo;
  D.iterations = p->iterations;
  bind(D.q, h->d_q.p);
  bind(D.t, h->d_t.p);
  bind(D.X, h->d_X.p);
  bind(D.q_try, h->d_qt.p);
  bind(D.t_try, h->d_tt.p);
  bind(D.X_try, h->d_Xt.p);
  bind(D.chi2, h->d_chi2.p);
  bind(D.err, h->d_err.p);
  bind(D.Hpl, h->d_Hpl.p);
  bind(D.Hll, h->d_Hll.p);
  bind(D.bl, h->d_bl.p);
  bind(D.Dinv, h->d_Dinv.p);
  bind(D.Hpp, h->d_Hpp.p);
  bind(D.bp, h->d_bp.p);
  bind(D.xl, h->d_xl.p);
  bind(D.xp, h->d_xp.p);
  bind(D.out_info, h->d_info.p);
  bind(D.out_stats, h->d_stats.p);
  bind(D.out_pack, h->d_out.p);
  D.mode = mode;
  bind(D.S, h->d_state.p);
  bind(D.part_chi, h->d_part_chi.p);
  bind(D.part_scale, h->d_part_scale.p);
  bind(D.Hs, h->d_Hs.p);
  bind(D.bs, h->d_bs.p);
  D.n_err_blocks = gfs::div_up(std::max(E, 1), kMk);
  D.n_upd_blocks = gfs::div_up(std::max(NP, 1), kMk);
}

// Schur products: on the matrix cores by landmark chunks (b_schur_mfma), GFS_LBA_SCHUR=chunks | pairs select the vector kernels
// (b_schur_chunks; one workgroup per pose pair, which also takes the windows too wide for the others' staging)
int choose_schur(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, hipStream_t s, LbaDev& D) {
  const int NP = p->n_points, F = P.n_free;
  int rc;
  static const char* mode = getenv("GFS_LBA_SCHUR");
  static const bool by_pairs = mode && !strcmp(mode, "pairs"), by_chunks = mode && !strcmp(mode, "chunks");
  size_t need = 0, need_b = 0;
  if (F > 0 && !by_pairs && !by_chunks) {
    const size_t NB = (6 * (size_t)F + 1 + 127) / 128, ld = 128 * NB, chunks = gfs::div_up(std::max(NP, 1), kSchurMPts);
    need = chunks * ld * ld;
    if (need * sizeof(double) <= ((size_t)2 << 30) && p->n_poses <= 4096) {
      D.schur_mfma = 1;
      D.n_schur_chunks = (int)chunks;
      D.n_pair_tiles = (int)(NB * (NB + 1) / 2);
    }
  }
  if (F > 0 && !by_pairs && !D.schur_mfma) {
    const size_t per_landmark = (size_t)F * (kSchurSlot * sizeof(double) + sizeof(int)) + 4 * sizeof(double);
    const int sub = (int)std::min<size_t>(8, (96 * 1024) / per_landmark);
    const size_t npairs = (size_t)F * (F + 1) / 2, chunks = gfs::div_up(std::max(NP, 1), kSchurPts);
    need = chunks * npairs * 36;
    need_b = chunks * (size_t)F * 6;
    if (sub >= 1 && need * sizeof(double) <= ((size_t)1 << 30)) {
      D.schur_sub = sub;
      D.n_schur_chunks = (int)chunks;
      D.n_pair_tiles = (int)gfs::div_up((int)npairs, kMk);
    }
  }
  if (D.schur_sub || D.schur_mfma) {
    if (h->d_schur_part.n < need) {
      GFS_HIP(hipStreamSynchronize(s));
      if ((rc = h->d_schur_part.alloc(need + need / 4))) return rc;
    }
    if (h->d_schur_part_b.n < need_b) {
      GFS_HIP(hipStreamSynchronize(s));
      if ((rc = h->d_schur_part_b.alloc(need_b + need_b / 4))) return rc;
    }
    bind(D.schur_part, h->d_schur_part.p);
    bind(D.schur_part_b, h->d_schur_part_b.p);
  }
  return GFS_OK;
}

inline size_t schur_mfma_lds_bytes(const LbaDev& D) {
  return (size_t)(2 * 3 * kSchurSub * kSchurLd + 9 * kSchurMPts) * sizeof(double) + (size_t)(kSchurMPts + 1 + D.n_poses) * sizeof(int);
}
inline size_t schur_lds_bytes(const LbaDev& D) {
  return (size_t)D.schur_sub * ((size_t)D.n_free * (kSchurSlot * sizeof(double) + sizeof(int)) + 4 * sizeof(double));
}

// The dynamic-LDS ceiling of a kernel is one global setting per function: raising it per call to that call's need would let
// two host threads with different windows undercut each other.  Set once per device to the hardware limit instead.
int lba_raise_lds_limits(int device) {
  static std::mutex mu;
  static bool done[64] = {};
  std::lock_guard<std::mutex> lk(mu);
  if (device >= 0 && device < 64 && done[device]) return GFS_OK;
  const int lim = 160 * 1024 - 1024;
  const void* fns[] = {(const void*)k_lba_solve<true>, (const void*)k_lba_solve<false>, (const void*)kb_lba_solve<true>,
                       (const void*)kb_lba_solve<false>, (const void*)k_lba_schur_chunks, (const void*)kb_lba_schur_chunks,
                       (const void*)k_lba_schur_mfma<true>, (const void*)k_lba_schur_mfma<false>, (const void*)kb_lba_schur_mfma<true>,
                       (const void*)kb_lba_schur_mfma<false>};
  for (const void* f : fns) GFS_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
  if (device >= 0 && device < 64) done[device] = true;
  return GFS_OK;
}

// The caller's force-stop flag, read LIVE every time the host loop looks at it: an int (gfs_lba_solve) or the C++ bool the
// reference hands in (Optimizer::LocalBundleAdjustment's pbStopFlag = &mbAbortBA, one byte: gfs_lba_solve_bool).
// Test hook (include/gfs_abi_test.h: gfs_test_lba_stop_at_look): a SCRIPTED flag.  Every evaluation of the flag by the calling thread's
// solve is a "look" (0 = the entry check); armed with `at`, looks at, at + 1, ... read as raised whatever the caller's memory holds.
// Nothing else changes: the same kernels are queued in the same order as for a flag that another thread raises at that moment.
struct StopScript {
  int at = -1;         // < 0: not armed
  int looks = 0;       // looks made by this thread's current / last call
  int discarded = 0;   // iterations that had run ahead of a raised flag and were put back (k_lba_restore)
  int forced = 0;      // forced decides queued (k_lba_decide / kb_lba_decide with force_end = 1)
  int ahead = -1;      // was a gated iteration queued behind the decide the host waited for when it saw the flag up?  -1: never saw it
};
static thread_local StopScript tl_stop_script;
struct StopScriptCall {  // one solve call: the counters start at zero, the script disarms itself when the call returns
  StopScriptCall() {
    StopScript& T = tl_stop_script;
    T.looks = T.discarded = T.forced = 0;
    T.ahead = -1;
  }
  ~StopScriptCall() { tl_stop_script.at = -1; }
};

struct StopFlag {
  volatile const int* i = nullptr;
  volatile const unsigned char* b = nullptr;
  StopFlag() = default;
  StopFlag(volatile const int* flag) : i(flag) {}
  StopFlag(const volatile unsigned char* flag) : b(flag) {}
  explicit operator bool() const { return i || b; }
  bool operator*() const {
    StopScript& T = tl_stop_script;
    const int look = T.looks++;
    if (T.at >= 0 && look >= T.at) return true;
    return (i && *i) || (b && *b);
  }
};

// Test hooks (include/gfs_abi_test.h: gfs_test_lba_first_trial, gfs_test_gba_first_trial): a tap in the trial sequence.  first_trial()
// queues init, the build group of iteration 0 and ONE trial up to and including k_lba_update -- the launches, grids and LDS sizes of the
// product -- with the reduced system copied to the tap's host arrays between its assembly and its factorisation (which works in place).
struct TrialTap {
  double *Hs, *bs;  // host: packed lower triangle (6F (6F + 1) / 2) and right-hand side (6F) as the Schur stage left them
};

// a launch on the stream of the LmPhases `ph`, counted
#define LM_LAUNCH(ph, name, kernel, grid, block, shmem, ...)                \
  do {                                                                      \
    GFS_LAUNCH(name, kernel, grid, block, shmem, (ph).s, __VA_ARGS__);      \
    (ph).launches++;                                                        \
  } while (0)

// The phases of a Levenberg-Marquardt run over a described problem, one launch each on the handle's stream.  The control flow is the
// caller's, and so is the reduced system between k_lba_dinv and k_lba_update: int reduced(int gate, const TrialTap* tap).
// gate = 1: queued speculatively behind a decide, every kernel leaves at once unless that trial was accepted and the loop goes on.
struct LmPhases {
  gfs_lba* h;
  hipStream_t s;
  const LbaDev D;
  const dim3 g_err, g_lm, g_upd;
  int* d_flags = nullptr;
  int launches = 0, trials = 0;
  int n_decides = 0;  // decide kernels queued so far: number i writes slot i & 1 of h_flags and is followed by event i & 1

  LmPhases(gfs_lba* h_, const LbaDev& D_)
      : h(h_), s(h_->stream), D(D_), g_err(D_.n_err_blocks), g_lm(std::max(D_.n_lm_wg, 1)), g_upd(D_.n_upd_blocks) {}

  int init() {
    GFS_HIP(hipHostGetDevicePointer((void**)&d_flags, h->h_flags, 0));
    LM_LAUNCH(*this, "k_lba_init", k_lba_init, dim3(64), dim3(kMk), 0, D);
    return GFS_OK;
  }
  int errors(int trial, int gate) {
    LM_LAUNCH(*this, "k_lba_errors", k_lba_errors, g_err, dim3(kMk), 0, D, trial, gate);
    return GFS_OK;
  }
  int begin(int iteration, int gate) {
    LM_LAUNCH(*this, "k_lba_begin", k_lba_begin, dim3(1), dim3(kThreads), 0, D, iteration, gate);
    return GFS_OK;
  }
  // the top of an iteration: the errors at the accepted estimate, the blocks of the system, the LM bookkeeping
  int build(int iteration, int gate) {
    if (int rc = errors(0, gate)) return rc;
    if (D.n_lm_wg > 0) LM_LAUNCH(*this, "k_lba_build_landmarks", k_lba_build_landmarks, g_lm, dim3(kMk), 0, D, gate);
    if (D.n_free > 0) LM_LAUNCH(*this, "k_lba_build_poses", k_lba_build_poses, dim3(D.n_free), dim3(kPoseWg), 0, D, gate);
    if (D.n_lidar_free > 0) LM_LAUNCH(*this, "k_lba_lidar_build", k_lba_lidar_build, dim3(D.n_lidar_free), dim3(kMk), 0, D, gate);
    return begin(iteration, gate);
  }
  // one trial of the iteration; with a tap it ends with the step: no errors at the trial estimate, no decision
  template <class Reduced>
  int trial(int gate, Reduced& reduced, const TrialTap* tap) {
    trials++;
    LM_LAUNCH(*this, "k_lba_dinv", k_lba_dinv, g_upd, dim3(kMk), 0, D, gate);
    if (int rc = reduced(gate, tap)) return rc;
    LM_LAUNCH(*this, "k_lba_update", k_lba_update, g_upd, dim3(kMk), 0, D, gate);
    if (tap) return GFS_OK;
    if (int rc = errors(1, gate)) return rc;
    LM_LAUNCH(*this, "k_lba_decide", k_lba_decide, dim3(1), dim3(64), 0, D, 0, d_flags + kFlagInts * (n_decides & 1), gate);
    GFS_HIP(hipEventRecord(h->ev_decide[n_decides & 1], s));
    n_decides++;
    return GFS_OK;
  }
  // waits for decide i (not for what is queued behind it) -> its flags: {again, terminate, cur, iters | lambda, last_chi}
  int verdict(int i, const int*& flags) {
    GFS_HIP(hipEventSynchronize(h->ev_decide[i & 1]));
    flags = h->h_flags + kFlagInts * (i & 1);
    return GFS_OK;
  }
  // the flag went up behind a rejected trial that would be retried: the iteration ends here, counted (terminate())
  int force_decide() {
    LM_LAUNCH(*this, "k_lba_decide", k_lba_decide, dim3(1), dim3(64), 0, D, 1, d_flags + kFlagInts * (n_decides & 1), 0);
    n_decides++;
    tl_stop_script.forced++;
    return GFS_OK;
  }
  // the results of the run; mode 1: no iteration ran, the robust chi2 of the estimate as it came and lambda 0
  int finish(int mode) {
    LbaDev Df = D;
    Df.mode = mode;
    LM_LAUNCH(*this, "k_lba_finish", k_lba_finish, dim3(1), dim3(64), 0, Df);
    return GFS_OK;
  }
};

// init, the build group of iteration 0 and one tapped trial, drained (the test hooks)
template <class Reduced>
int first_trial(LmPhases& ph, Reduced& reduced, const TrialTap* tap) {
  int rc;
  if ((rc = ph.init()) || (rc = ph.build(0, 0)) || (rc = ph.trial(0, reduced, tap))) return rc;
  GFS_HIP(hipStreamSynchronize(ph.s));
  return GFS_OK;
}

// ... and what the hooks report of it besides the tap's arrays
int first_trial_download(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, gfs_test_lba_trial* out) {
  const size_t NP = p->n_points, n = 6 * (size_t)P.n_free;
  LbaState S;
  GFS_HIP(hipMemcpy(&S, h->d_state.p, sizeof(S), hipMemcpyDeviceToHost));
  if (NP) GFS_HIP(hipMemcpy(out->Dinv, h->d_Dinv.p, NP * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (NP) GFS_HIP(hipMemcpy(out->xl, h->d_xl.p, NP * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (n) GFS_HIP(hipMemcpy(out->xp, h->d_xp.p, n * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> part(h->last_desc.n_upd_blocks);
  GFS_HIP(hipMemcpy(part.data(), h->d_part_scale.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
  double scale = 0;
  for (double v : part) scale += v;  // k_lba_decide's order
  out->lambda = S.lambda;
  out->scale = scale;
  out->solve_ok = S.solve_ok;
  return GFS_OK;
}

// result download of one window, in two halves so that a batch can queue all copies before one synchronisation: the packed
// block of b_pack comes back in one copy
struct LbaFetch {
  const double *chi, *q, *t, *X, *stats;
};
int lba_fetch_issue(gfs_lba* h, const gfs_lba_problem* p, hipStream_t s, LbaFetch& F) {
  const size_t E = p->n_edges, NP = p->n_points, NQ = p->n_poses, total = E + 7 * NQ + 3 * NP + 4;
  GFS_REQUIRE(total <= h->h_out.n, GFS_ERR_CAPACITY, "gfs_lba: result arena too small");
  const double* base = h->h_out.p;
  F.chi = base;
  F.q = base + E;
  F.t = F.q + 4 * NQ;
  F.X = F.t + 3 * NQ;
  F.stats = F.X + 3 * NP;
  GFS_HIP(hipMemcpyAsync(h->h_out.p, h->d_out.p, total * sizeof(double), hipMemcpyDeviceToHost, s));
  return GFS_OK;
}
void lba_fetch_finish(const gfs_lba_problem* p, const HostPrep& P, const LbaFetch& F, gfs_lba_solution* sol) {
  const int E = p->n_edges, NP = p->n_points;
  const double *chi = F.chi, *q = F.q, *t = F.t, *X = F.X, *stats = F.stats;
  if (p->n_poses && sol->pose_q) memcpy(sol->pose_q, q, (size_t)p->n_poses * 32);
  if (p->n_poses && sol->pose_t) memcpy(sol->pose_t, t, (size_t)p->n_poses * 24);
  if (NP && sol->points) memcpy(sol->points, X, (size_t)NP * 24);
  for (int k = 0; k < E; k++) {
    const int e = P.order[k];
    if (sol->edge_chi2) sol->edge_chi2[e] = chi[k];
    if (sol->edge_depth_positive) {  // isDepthPositive() at the final estimates (host side, trivial)
      const double* qq = &q[4 * (size_t)p->edge_pose[e]];
      const double* v = &X[3 * (size_t)p->edge_point[e]];
      const double ux = 2 * (qq[1] * v[2] - qq[2] * v[1]), uy = 2 * (qq[2] * v[0] - qq[0] * v[2]);
      const double uz = 2 * (qq[0] * v[1] - qq[1] * v[0]);
      const double z = v[2] + qq[3] * uz + (qq[0] * uy - qq[1] * ux) + t[3 * (size_t)p->edge_pose[e] + 2];
      sol->edge_depth_positive[e] = z > 0.0;
    }
  }
  sol->iterations_run = (int)stats[2];
  sol->final_chi2 = stats[0];
  sol->final_lambda = stats[1];
}

// the end of a single-problem solve: the last window's results packed, copied back (with what `more` queues besides), scattered
template <class More>
int fetch_solution(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, gfs_lba_solution* sol, More more) {
  LbaFetch F;
  int rc;
  GFS_LAUNCH("k_lba_pack", k_lba_pack, dim3(16), dim3(kMk), 0, h->stream, h->last_desc);
  if ((rc = lba_fetch_issue(h, p, h->stream, F)) || (rc = more())) return rc;
  GFS_HIP(hipStreamSynchronize(h->stream));
  lba_fetch_finish(p, P, F, sol);
  return GFS_OK;
}
int fetch_solution(gfs_lba* h, const gfs_lba_problem* p, const HostPrep& P, gfs_lba_solution* sol) {
  return fetch_solution(h, p, P, sol, [] { return (int)GFS_OK; });
}

}  // namespace
