// gfs_sim3_search on the gfs_sbp handle (gfs_sbp_reserve_sim3_search allocates its workspace): the three Sim3 searches of loop
// closing -- ORBmatcher::Fuse(KeyFrame*, Sim3f&, ...) (reference src/ORBmatcher.cc:1550-1654) and the two
// SearchByProjection(KeyFrame*, Sim3f&, ...) (:432-529, :531-636) -- for every listed map point (the rule
// itself is sim3_search_rule.hpp, shared with the host).
// Grid (min(ceil(n / 256), groups), B), blockIdx.y = the (list, problem) pair.  k_sim3_search keeps k_fuse's structure: every
// workgroup builds its key frame's 64 x 48 grid in LDS (load_keyframe_grid_lds, sbp_dev.hpp) with the positions and octaves of the
// key-points next to it -- bit 7 of the octave byte says that the key-point is taken at entry, which is the whole taken mask -- and
// then a lane owns one map point: projection, gates, PredictScale and the walk of its window (walk_window, sbp_dev.hpp).
// A workgroup that has its grid walks the chunks blockIdx.x,
// blockIdx.x + gridDim.x, ... of its list (no barrier inside that loop).
// What a lane delivers is not a match but a LIST: its first kListed candidates in (distance, visiting order) and the count of all of
// them.  A candidate lies in the window, passes the level filter, is not taken at entry, and has a distance below what bestDist starts
// at.  The dependency between the points of a projection search (a match takes its key-point from every later point) is resolved on
// the host after the download, in point order, from these lists (gfs_sim3_search below); so nothing is resolved across lanes on the
// device: no atomics on global memory, no waiting between workgroups, results independent of scheduling.
// LDS: 6 146 (cell starts) + 8 192 (items) + 2 x 16 384 (x, y) + 4 096 (octave | taken) + 12 288 (the cell counters of the build) +
// the header = 63 776 B, two workgroups a CU (160 KB).

#include "point_search.hpp"
#include "sim3_search_rule.hpp"

using namespace gfs;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kListed = gfs_sim3::kListed;
constexpr uint8_t kTakenBit = 0x80;  // of the staged octave byte (octaves are below 16)

struct Sim3Problem {
  gfs_fuse::KeyFrame K;
  int n_mp, list_base, out_base;  // the list's length and its first point in the point arrays; the problem's first output slot
  int cand_base, cand_stride;     // candidate k of point i is slot cand_base + k * cand_stride + i
  int mode;
};

static_assert(gfs_sim3::kFuse == GFS_SIM3_FUSE && gfs_sim3::kSbp == GFS_SIM3_SBP && gfs_sim3::kSbpKfs == GFS_SIM3_SBP_KFS &&
                  gfs_sim3::kSkipped == GFS_FUSE_SKIPPED && gfs_sim3::kListed == GFS_SIM3_SEARCH_LISTED, "the rule's modes and codes are the ABI's");
static_assert(gfs_fuse::kMatched == GFS_FUSE_MATCHED && gfs_fuse::kEmptyWindow == GFS_FUSE_EMPTY_WINDOW, "the rule's exits are the ABI's");

__host__ __device__ inline int listed_of(int mode) { return mode == gfs_sim3::kFuse ? 1 : kListed; }

__global__ __launch_bounds__(kThreads) void k_sim3_search(const Sim3Problem* __restrict__ problems, const float* __restrict__ mp_xw,
                                                          const float* __restrict__ mp_normal, const float* __restrict__ mp_min,
                                                          const float* __restrict__ mp_max, const uint8_t* __restrict__ mp_desc,
                                                          const float2* __restrict__ kf_xy, const uint8_t* __restrict__ kf_oct,
                                                          const uint8_t* __restrict__ kf_desc, int SC, uint8_t* __restrict__ o_exit,
                                                          int* __restrict__ o_level, int* __restrict__ o_count, int* __restrict__ o_cidx,
                                                          int* __restrict__ o_cdist) {
  __shared__ unsigned short s_start[kCells + 1];
  __shared__ unsigned short s_items[kSbpMaxCur];
  __shared__ float s_kx[kSbpMaxCur], s_ky[kSbpMaxCur];
  __shared__ uint8_t s_oct[kSbpMaxCur];
  __shared__ int s_cnt[kCells];
  __shared__ int s_scan[kWaves];
  __shared__ Sim3Problem s_P;
  const int f = blockIdx.y, tid = threadIdx.x;
  if ((int)blockIdx.x * kThreads >= problems[f].n_mp) return;  // (uniform: the grid is sized by the call's longest list)
  if (tid == 0) s_P = problems[f];
  __syncthreads();
  const gfs_fuse::KeyFrame& K = s_P.K;
  const int N = K.n_kp, mode = s_P.mode, n_mp = s_P.n_mp;
  const size_t kf_at = (size_t)f * SC;
  load_keyframe_grid_lds<kThreads>(K, N, kf_xy + kf_at, kf_oct + kf_at, s_kx, s_ky, s_oct, s_start, s_items, s_cnt, s_scan);
  const uint8_t* kd = kf_desc + 32 * kf_at;
  const int first = gfs_sim3::first_best_dist(mode), n_listed = listed_of(mode);
  // ---- a lane per map point, chunk after chunk
  for (int base = blockIdx.x * kThreads; base < n_mp; base += gridDim.x * kThreads) {
    const int i = base + tid;
    if (i >= n_mp) continue;
    const size_t at = (size_t)s_P.list_base + i, to = (size_t)s_P.out_base + i;
    const float P[3] = {mp_xw[3 * at], mp_xw[3 * at + 1], mp_xw[3 * at + 2]};
    const float Pn[3] = {mp_normal[3 * at], mp_normal[3 * at + 1], mp_normal[3 * at + 2]};
    const gfs_fuse::Proj R = gfs_sim3::project(K, mode, P, Pn, mp_min[at], mp_max[at]);
    int c_dist[kListed], c_idx[kListed], count = 0, ex = R.exit;
#pragma unroll
    for (int k = 0; k < kListed; k++) {
      c_dist[k] = first;
      c_idx[k] = -1;
    }
    if (R.exit < 0) {
      bool any = false;
      walk_window(
          R.x0, R.x1, R.y0, R.y1, s_start, s_items, mp_desc + 32 * at, kd,
          [&](int j) {
            if (!gfs_fuse::in_window(R, s_kx[j], s_ky[j])) return false;
            any = true;
            const int o = s_oct[j];
            if (o & kTakenBit) return false;  // vpMatched[idx] (:506, :612), ahead of the level filter
            return gfs_sim3::level_ok(R, o);
          },
          [&](int j, int d) {
            if (d >= first) return;  // 256 in the projection searches: `dist < bestDist` never holds
            count++;
            if (d < c_dist[kListed - 1]) {  // strict, and strict on the way up: the first visited of equal distances stays ahead
              c_dist[kListed - 1] = d;
              c_idx[kListed - 1] = j;
#pragma unroll
              for (int s = kListed - 1; s > 0; s--) {
                if (c_dist[s] < c_dist[s - 1]) {
                  const int td = c_dist[s], ti = c_idx[s];
                  c_dist[s] = c_dist[s - 1];
                  c_idx[s] = c_idx[s - 1];
                  c_dist[s - 1] = td;
                  c_idx[s - 1] = ti;
                }
              }
            }
          });
      ex = any ? gfs_fuse::kNoCandidate : gfs_fuse::kEmptyWindow;  // (matched or not: the host's replay decides)
    }
    o_exit[to] = (uint8_t)ex;
    o_level[to] = R.level;
    o_count[to] = count;
    const size_t ct = (size_t)s_P.cand_base + i;
#pragma unroll
    for (int s = 0; s < kListed; s++) {
      if (s < n_listed) {
        o_cidx[ct + (size_t)s * s_P.cand_stride] = c_idx[s];
        o_cdist[ct + (size_t)s * s_P.cand_stride] = c_dist[s];
      }
    }
  }
}

using Layout = gfs::Sim3SearchLayout<Sim3Problem>;

}  // namespace

struct gfs_sim3_workspace : gfs::PointSearchWorkspace {
  int resident = 0;    // workgroups the device holds at once: two a CU
  int max_groups = 0;  // gfs_test_sim3_search_groups: 0 = resident, < 0 = a workgroup a chunk
};

extern "C" {

int gfs_sbp_reserve_sim3_search(gfs_sbp* h, int max_lists, int max_points_per_list, int max_problems) {
  GFS_REQUIRE(h && max_lists > 0 && max_points_per_list > 0 && max_problems > 0, GFS_ERR_INVALID_ARG,
              "gfs_sbp_reserve_sim3_search: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_REQUIRE(h->max_cur <= kSbpMaxCur, GFS_ERR_CAPACITY, "gfs_sbp_reserve_sim3_search: max_cur %d exceeds the LDS tables (%d)", h->max_cur, kSbpMaxCur);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipStreamSynchronize(h->stream));
  int cus = 0;
  GFS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
  const size_t SP = gfs::align_up((size_t)max_points_per_list, 64), SC = gfs::align_up((size_t)h->max_cur, 64);
  const Layout Y{SP * max_lists, (size_t)max_problems, SC, SP * max_problems, SP * max_problems * kListed};
  h->sim3.reset();
  std::unique_ptr<gfs_sim3_workspace> w(new gfs_sim3_workspace);
  if (int rc = w->alloc(Y.pts.bytes(), Y.kf.bytes(), Y.out.bytes(), max_lists, max_points_per_list, max_problems)) return rc;
  w->resident = 2 * std::max(cus, 1);
  h->sim3 = std::move(w);
  return GFS_OK;
}

int gfs_test_sim3_search_groups(gfs_sbp* h, int max_groups) {
  GFS_REQUIRE(h, GFS_ERR_INVALID_ARG, "gfs_test_sim3_search_groups: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_sim3_workspace* w = static_cast<gfs_sim3_workspace*>(h->sim3.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_test_sim3_search_groups: call gfs_sbp_reserve_sim3_search first");
  w->max_groups = max_groups;
  return GFS_OK;
}

int gfs_sim3_search(gfs_sbp* h, const gfs_fuse_points* lists, int n_lists, const gfs_sim3_search_problem* problems, int B,
                    gfs_sim3_search_result* results) {
  static const char who[] = "gfs_sim3_search", what[] = "problem";
  GFS_REQUIRE(h && lists && problems && results && n_lists > 0 && B > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_search: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_sim3_workspace* w = static_cast<gfs_sim3_workspace*>(h->sim3.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_sim3_search: call gfs_sbp_reserve_sim3_search first");
  GFS_REQUIRE(n_lists <= w->lists, GFS_ERR_CAPACITY, "gfs_sim3_search: %d lists exceed the reserve %d", n_lists, w->lists);
  GFS_REQUIRE(B <= w->kfs, GFS_ERR_CAPACITY, "gfs_sim3_search: %d problems exceed the reserve %d", B, w->kfs);
  GFS_HIP(hipSetDevice(h->device));
  // every refusal comes before anything is staged
  size_t T = 0, O = 0, OC = 0, SC = 64;
  int n_max = 0;
  std::vector<size_t> list_base;
  if (int rc = check_point_lists(who, lists, n_lists, w->points, list_base, &T)) return rc;
  for (int f = 0; f < B; f++) {
    const gfs_sim3_search_problem& k = problems[f];
    GFS_REQUIRE(k.mode == GFS_SIM3_FUSE || k.mode == GFS_SIM3_SBP || k.mode == GFS_SIM3_SBP_KFS, GFS_ERR_INVALID_ARG,
                "gfs_sim3_search: problem %d has the unknown mode %d", f, k.mode);
    if (int rc = check_search_kf_head(who, what, f, k, h->max_cur, k.scale_factors != nullptr, "scale factors", n_lists)) return rc;
    GFS_REQUIRE(k.n_kp == 0 || (k.kps_un && k.desc), GFS_ERR_INVALID_ARG, "gfs_sim3_search: problem %d has NULL key-point arrays", f);
    GFS_REQUIRE(k.mode != GFS_SIM3_FUSE || !k.kp_taken, GFS_ERR_INVALID_ARG, "gfs_sim3_search: problem %d gives kp_taken in GFS_SIM3_FUSE mode", f);
    GFS_REQUIRE(k.mode == GFS_SIM3_FUSE || gfs_sim3::ratio_ok(k.ratio_hamming), GFS_ERR_INVALID_ARG,
                "gfs_sim3_search: problem %d has ratio_hamming %g (needs 0 <= 50 ratio < 256)", f, (double)k.ratio_hamming);
    const int n = lists[k.list].n_mp;
    if (int rc = check_search_kf_tail(who, what, f, k, n, results[f])) return rc;
    SC = std::max(SC, gfs::align_up((size_t)k.n_kp, 64));
    O += gfs::align_up((size_t)n, 64);
    OC += gfs::align_up((size_t)n, 64) * listed_of(k.mode);
    n_max = std::max(n_max, n);
  }
  const Layout Y{T, (size_t)B, SC, O, OC};  // within the reserve: T <= lists x SP, O <= B x SP, OC <= kListed O, SC <= max_cur
  uint8_t* hk = w->kf.h.p;
  stage_point_lists(Y.p, w->pts.h.p, lists, n_lists, list_base);
  size_t o_at = 0, c_at = 0;
  for (int f = 0; f < B; f++) {
    const gfs_sim3_search_problem& k = problems[f];
    Sim3Problem& Q = Y.problems.at(hk)[f];
    memset(&Q, 0, sizeof(Q));
    fill_search_keyframe(Q.K, k);
    Q.n_mp = lists[k.list].n_mp;
    Q.list_base = (int)list_base[k.list];
    Q.out_base = (int)o_at;
    Q.cand_base = (int)c_at;
    Q.cand_stride = (int)gfs::align_up((size_t)Q.n_mp, 64);
    Q.mode = k.mode;
    o_at += (size_t)Q.cand_stride;
    c_at += (size_t)Q.cand_stride * listed_of(k.mode);
    uint8_t* oct = Y.oct.at(hk, (size_t)f * SC);
    stage_xy_oct(k.kps_un, k.n_kp, Y.xy.at(hk, (size_t)f * SC), oct);
    if (k.kp_taken)
      for (int i = 0; i < k.n_kp; i++)
        if (k.kp_taken[i]) oct[i] |= kTakenBit;
    Y.kdesc.put(hk, (size_t)f * SC, k.desc, (size_t)k.n_kp);
  }
  if (n_max > 0) {
    const uint8_t *dp = w->pts.d.p, *dk = w->kf.d.p;
    uint8_t* dq = w->out.d.p;
    // a workgroup a chunk while the device holds them all at once; beyond that a workgroup keeps its grid and walks several chunks
    const int chunks = (n_max + kThreads - 1) / kThreads;
    const int cap = w->max_groups < 0 ? chunks : std::max(1, (w->max_groups > 0 ? w->max_groups : w->resident) / B);
    const int rc = w->run(h->stream, Y.pts.bytes(), Y.kf.bytes(), Y.out.bytes(), [&]() -> int {
      GFS_LAUNCH("k_sim3_search", k_sim3_search, dim3(std::min(chunks, cap), B), dim3(kThreads), 0, h->stream, Y.problems.at(dk), Y.p.xw.at(dp),
                 Y.p.nrm.at(dp), Y.p.dmin.at(dp), Y.p.dmax.at(dp), Y.p.desc.at(dp), Y.xy.at(dk), Y.oct.at(dk), Y.kdesc.at(dk), (int)SC,
                 Y.exit.at(dq), Y.level.at(dq), Y.count.at(dq), Y.cidx.at(dq), Y.cdist.at(dq));
      return GFS_OK;
    });
    if (rc) return rc;
  }
  // ---- the replay, problem by problem in point order: the sequential loop's vpMatched, fed from the lists
  const uint8_t* ho = w->out.h.p;
  std::vector<uint8_t> taken;
  for (int f = 0; f < B; f++) {
    const gfs_sim3_search_problem& k = problems[f];
    const Sim3Problem& Q = Y.problems.at(hk)[f];
    const gfs_fuse_points& L = lists[k.list];
    gfs_sim3_search_result& r = results[f];
    const uint8_t* d_exit = Y.exit.at(ho, (size_t)Q.out_base);
    const int *d_level = Y.level.at(ho, (size_t)Q.out_base), *d_count = Y.count.at(ho, (size_t)Q.out_base);
    const int *d_cidx = Y.cidx.at(ho, (size_t)Q.cand_base), *d_cdist = Y.cdist.at(ho, (size_t)Q.cand_base);
    const bool dependent = k.mode != GFS_SIM3_FUSE;
    const int first = gfs_sim3::first_best_dist(k.mode), n_listed = listed_of(k.mode);
    if (dependent) {
      taken.assign((size_t)k.n_kp, 0);
      if (k.kp_taken)
        for (int j = 0; j < k.n_kp; j++) taken[j] = k.kp_taken[j] != 0;
    }
    int matched = 0;
    for (int i = 0; i < L.n_mp; i++) {
      int ex = d_exit[i], idx = -1, dist = first, level = d_level[i];
      if (k.mp_skip && k.mp_skip[i]) {
        ex = GFS_FUSE_SKIPPED;
        level = 0;
      } else if (ex == gfs_fuse::kNoCandidate) {  // the window was searched
        const int n = std::min(d_count[i], n_listed);
        int c = 0;
        while (c < n && dependent && taken[d_cidx[(size_t)c * Q.cand_stride + i]]) c++;
        if (c < n) {
          idx = d_cidx[(size_t)c * Q.cand_stride + i];
          dist = d_cdist[(size_t)c * Q.cand_stride + i];
        } else if (d_count[i] > n_listed) {  // every listed candidate went to an earlier point and more exist: this one search again
          const gfs_sim3::PointResult o = gfs_sim3::search_point(
              Q.K, k.mode, k.ratio_hamming, L.mp_xw + 3 * (size_t)i, L.mp_normal + 3 * (size_t)i, L.mp_min_dist[i], L.mp_max_dist[i],
              L.mp_desc + 32 * (size_t)i,
              [&](int j, float* x, float* y, int* oct) {
                *x = k.kps_un[j].x;
                *y = k.kps_un[j].y;
                *oct = k.kps_un[j].octave;
              },
              k.desc, taken.data());
          idx = o.best_idx;
          dist = o.best_dist;
        }
        if (gfs_sim3::accepted(k.mode, dist, k.ratio_hamming)) {
          ex = gfs_fuse::kMatched;
          if (dependent) taken[idx] = 1;  // vpMatched[bestIdx] = pMP
        }
      }
      r.exit[i] = (uint8_t)ex;
      r.best_idx[i] = idx;
      r.best_dist[i] = dist;
      r.level[i] = level;
      matched += ex == gfs_fuse::kMatched;
    }
    r.n_matched = matched;
  }
  return GFS_OK;
}

}  // extern "C"
