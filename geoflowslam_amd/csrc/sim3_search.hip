// gfs_sim3_search on the gfs_sbp handle (gfs_sbp_reserve_sim3_search allocates its workspace): the three Sim3 searches of loop
// closing -- ORBmatcher::Fuse(KeyFrame*, Sim3f&, ...) (reference src/ORBmatcher.cc:1550-1654) and the two
// SearchByProjection(KeyFrame*, Sim3f&, ...) (:432-529, :531-636) -- for every listed map point (the rule
// itself is sim3_search_rule.hpp, shared with the host).
// Grid (min(ceil(n / 256), groups), B), blockIdx.y = the (list, problem) pair.  k_sim3_search keeps k_fuse's structure: every
// workgroup builds its key frame's 64 x 48 grid in LDS (build_grid_lds, sbp_dev.hpp) with the positions and octaves of the
// key-points next to it -- bit 7 of the octave byte says that the key-point is taken at entry, which is the whole taken mask -- and
// then a lane owns one map point: projection, gates, PredictScale, the window walked as the runs of its grid columns, four items at a
// time with the descriptors of the survivors fetched together.  A workgroup that has its grid walks the chunks blockIdx.x,
// blockIdx.x + gridDim.x, ... of its list (no barrier inside that loop).
// What a lane delivers is not a match but a LIST: its first kListed candidates in (distance, visiting order) and the count of all of
// them.  A candidate lies in the window, passes the level filter, is not taken at entry, and has a distance below what bestDist starts
// at.  The dependency between the points of a projection search (a match takes its key-point from every later point) is resolved on
// the host after the download, in point order, from these lists (gfs_sim3_search below); so nothing is resolved across lanes on the
// device: no atomics on global memory, no waiting between workgroups, results independent of scheduling.
// LDS: 6 146 (cell starts) + 8 192 (items) + 2 x 16 384 (x, y) + 4 096 (octave | taken) + 12 288 (the cell counters of the build) +
// the header = 63 776 B, two workgroups a CU (160 KB).

#include <vector>

#include "sbp_handle.hpp"
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
  for (int i = tid; i < N; i += kThreads) {
    const float2 p = kf_xy[kf_at + i];
    s_kx[i] = p.x;
    s_ky[i] = p.y;
    s_oct[i] = kf_oct[kf_at + i];
  }
  auto cell_of = [&](int i) {  // Frame::PosInGrid
    const int px = (int)roundf((s_kx[i] - K.min_x) * K.grid_w_inv), py = (int)roundf((s_ky[i] - K.min_y) * K.grid_h_inv);
    return (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) ? px * kGridRows + py : -1;
  };
  build_grid_lds<kThreads>(N, cell_of, s_start, s_items, s_cnt, s_scan);
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
      const uint4* dl = reinterpret_cast<const uint4*>(mp_desc + 32 * at);
      const uint4 a0 = dl[0], a1 = dl[1];
      bool any = false, more = true;
      int ix = R.x0;
      int k = s_start[ix * kGridRows + R.y0], kend = s_start[ix * kGridRows + R.y1 + 1];
      auto next_item = [&]() {  // the next key-point index of the window in visiting order, or -1
        while (more && k >= kend) {
          if (++ix > R.x1) {
            more = false;
            break;
          }
          k = s_start[ix * kGridRows + R.y0];
          kend = s_start[ix * kGridRows + R.y1 + 1];
        }
        return more ? (int)s_items[k++] : -1;
      };
      while (more) {
        int j[4];
        bool pass[4];
        uint4 b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          j[u] = next_item();
          pass[u] = false;
          if (j[u] < 0) continue;
          if (!gfs_fuse::in_window(R, s_kx[j[u]], s_ky[j[u]])) continue;
          any = true;
          const int o = s_oct[j[u]];
          if (o & kTakenBit) continue;  // vpMatched[idx] (:506, :612), ahead of the level filter
          if (!gfs_sim3::level_ok(R, o)) continue;
          pass[u] = true;
          const uint4* dc = reinterpret_cast<const uint4*>(kd + 32 * (size_t)j[u]);
          b0[u] = dc[0];
          b1[u] = dc[1];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          if (!pass[u]) continue;
          const int d = hamming256(a0, a1, b0[u], b1[u]);
          if (d >= first) continue;  // 256 in the projection searches: `dist < bestDist` never holds
          count++;
          if (d < c_dist[kListed - 1]) {  // strict, and strict on the way up: the first visited of equal distances stays ahead
            c_dist[kListed - 1] = d;
            c_idx[kListed - 1] = j[u];
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
        }
      }
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

// The point lists, the problems (headers + key-point arrays) and the per-point lists, each one pinned block mirrored by one device block
struct gfs_sim3_workspace : gfs_sbp_workspace {
  int lists = 0, points = 0, problems = 0;
  int resident = 0;    // workgroups the device holds at once: two a CU
  int max_groups = 0;  // gfs_test_sim3_search_groups: 0 = resident, < 0 = a workgroup a chunk
  gfs::Mirror pts, kf, out;
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
  int rc = w->pts.alloc(Y.pts.bytes());
  if (!rc) rc = w->kf.alloc(Y.kf.bytes());
  if (!rc) rc = w->out.alloc(Y.out.bytes());
  if (rc) return rc;
  w->lists = max_lists;
  w->points = max_points_per_list;
  w->problems = max_problems;
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
  GFS_REQUIRE(h && lists && problems && results && n_lists > 0 && B > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_search: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_sim3_workspace* w = static_cast<gfs_sim3_workspace*>(h->sim3.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_sim3_search: call gfs_sbp_reserve_sim3_search first");
  GFS_REQUIRE(n_lists <= w->lists, GFS_ERR_CAPACITY, "gfs_sim3_search: %d lists exceed the reserve %d", n_lists, w->lists);
  GFS_REQUIRE(B <= w->problems, GFS_ERR_CAPACITY, "gfs_sim3_search: %d problems exceed the reserve %d", B, w->problems);
  GFS_HIP(hipSetDevice(h->device));
  // every refusal comes before anything is staged
  size_t T = 0, O = 0, OC = 0, SC = 64;
  int n_max = 0;
  std::vector<size_t> list_base((size_t)n_lists);
  for (int l = 0; l < n_lists; l++) {
    const gfs_fuse_points& L = lists[l];
    GFS_REQUIRE(L.n_mp >= 0 && L.n_mp <= w->points, GFS_ERR_CAPACITY, "gfs_sim3_search: list %d has %d map points (reserve %d)", l, L.n_mp,
                w->points);
    GFS_REQUIRE(L.n_mp == 0 || (L.mp_xw && L.mp_normal && L.mp_min_dist && L.mp_max_dist && L.mp_desc), GFS_ERR_INVALID_ARG,
                "gfs_sim3_search: list %d has NULL arrays", l);
    list_base[l] = T;
    T += gfs::align_up((size_t)L.n_mp, 64);
  }
  for (int f = 0; f < B; f++) {
    const gfs_sim3_search_problem& k = problems[f];
    GFS_REQUIRE(k.mode == GFS_SIM3_FUSE || k.mode == GFS_SIM3_SBP || k.mode == GFS_SIM3_SBP_KFS, GFS_ERR_INVALID_ARG,
                "gfs_sim3_search: problem %d has the unknown mode %d", f, k.mode);
    GFS_REQUIRE(k.n_kp >= 0 && k.n_kp <= h->max_cur, GFS_ERR_CAPACITY, "gfs_sim3_search: problem %d has %d key-points (capacity %d)", f, k.n_kp,
                h->max_cur);
    GFS_REQUIRE(k.n_levels > 0 && k.n_levels <= 16 && k.scale_factors, GFS_ERR_INVALID_ARG, "gfs_sim3_search: problem %d needs 1..16 scale factors", f);
    GFS_REQUIRE(k.list >= 0 && k.list < n_lists, GFS_ERR_INVALID_ARG, "gfs_sim3_search: problem %d names list %d of %d", f, k.list, n_lists);
    GFS_REQUIRE(k.n_kp == 0 || (k.kps_un && k.desc), GFS_ERR_INVALID_ARG, "gfs_sim3_search: problem %d has NULL key-point arrays", f);
    GFS_REQUIRE(k.mode != GFS_SIM3_FUSE || !k.kp_taken, GFS_ERR_INVALID_ARG, "gfs_sim3_search: problem %d gives kp_taken in GFS_SIM3_FUSE mode", f);
    GFS_REQUIRE(k.mode == GFS_SIM3_FUSE || gfs_sim3::ratio_ok(k.ratio_hamming), GFS_ERR_INVALID_ARG,
                "gfs_sim3_search: problem %d has ratio_hamming %g (needs 0 <= 50 ratio < 256)", f, (double)k.ratio_hamming);
    const int n = lists[k.list].n_mp;
    GFS_REQUIRE(n == 0 || (results[f].exit && results[f].best_idx && results[f].best_dist && results[f].level), GFS_ERR_INVALID_ARG,
                "gfs_sim3_search: problem %d has NULL result arrays", f);
    for (int i = 0; i < k.n_kp; i++)
      GFS_REQUIRE(k.kps_un[i].octave >= 0 && k.kps_un[i].octave < k.n_levels, GFS_ERR_INVALID_ARG,
                  "gfs_sim3_search: problem %d key-point %d has octave %d outside [0, %d)", f, i, k.kps_un[i].octave, k.n_levels);
    SC = std::max(SC, gfs::align_up((size_t)k.n_kp, 64));
    O += gfs::align_up((size_t)n, 64);
    OC += gfs::align_up((size_t)n, 64) * listed_of(k.mode);
    n_max = std::max(n_max, n);
  }
  const Layout Y{T, (size_t)B, SC, O, OC};  // within the reserve: T <= lists x SP, O <= B x SP, OC <= kListed O, SC <= max_cur
  uint8_t *hp = w->pts.h.p, *hk = w->kf.h.p;
  for (int l = 0; l < n_lists; l++) {
    const gfs_fuse_points& L = lists[l];
    const size_t at = list_base[l], n = (size_t)L.n_mp;
    Y.xw.put(hp, at, L.mp_xw, n);
    Y.nrm.put(hp, at, L.mp_normal, n);
    Y.dmin.put(hp, at, L.mp_min_dist, n);
    Y.dmax.put(hp, at, L.mp_max_dist, n);
    Y.desc.put(hp, at, L.mp_desc, n);
  }
  size_t o_at = 0, c_at = 0;
  for (int f = 0; f < B; f++) {
    const gfs_sim3_search_problem& k = problems[f];
    Sim3Problem& Q = Y.problems.at(hk)[f];
    memset(&Q, 0, sizeof(Q));
    for (int c = 0; c < 4; c++) Q.K.q[c] = k.Tcw_q[c];
    for (int c = 0; c < 3; c++) {
      Q.K.t[c] = k.Tcw_t[c];
      Q.K.Ow[c] = k.Ow[c];
    }
    Q.K.fx = k.fx;
    Q.K.fy = k.fy;
    Q.K.cx = k.cx;
    Q.K.cy = k.cy;
    Q.K.min_x = k.min_x;
    Q.K.max_x = k.max_x;
    Q.K.min_y = k.min_y;
    Q.K.max_y = k.max_y;
    Q.K.grid_w_inv = k.grid_w_inv;
    Q.K.grid_h_inv = k.grid_h_inv;
    Q.K.log_scale_factor = k.log_scale_factor;
    Q.K.th = k.th;
    Q.K.n_levels = k.n_levels;
    Q.K.n_kp = k.n_kp;
    for (int c = 0; c < k.n_levels; c++) Q.K.scale[c] = k.scale_factors[c];
    Q.n_mp = lists[k.list].n_mp;
    Q.list_base = (int)list_base[k.list];
    Q.out_base = (int)o_at;
    Q.cand_base = (int)c_at;
    Q.cand_stride = (int)gfs::align_up((size_t)Q.n_mp, 64);
    Q.mode = k.mode;
    o_at += (size_t)Q.cand_stride;
    c_at += (size_t)Q.cand_stride * listed_of(k.mode);
    float2* xy = Y.xy.at(hk, (size_t)f * SC);
    uint8_t* oct = Y.oct.at(hk, (size_t)f * SC);
    for (int i = 0; i < k.n_kp; i++) {
      xy[i] = make_float2(k.kps_un[i].x, k.kps_un[i].y);
      oct[i] = (uint8_t)(k.kps_un[i].octave | ((k.kp_taken && k.kp_taken[i]) ? kTakenBit : 0));
    }
    Y.kdesc.put(hk, (size_t)f * SC, k.desc, (size_t)k.n_kp);
  }
  if (n_max > 0) {
    hipStream_t s = h->stream;
    const uint8_t *dp = w->pts.d.p, *dk = w->kf.d.p;
    uint8_t* dq = w->out.d.p;
    if (int rc = w->pts.upload(s, 0, Y.pts.bytes())) return rc;
    if (int rc = w->kf.upload(s, 0, Y.kf.bytes())) return rc;
    // a workgroup a chunk while the device holds them all at once; beyond that a workgroup keeps its grid and walks several chunks
    const int chunks = (n_max + kThreads - 1) / kThreads;
    const int cap = w->max_groups < 0 ? chunks : std::max(1, (w->max_groups > 0 ? w->max_groups : w->resident) / B);
    GFS_LAUNCH("k_sim3_search", k_sim3_search, dim3(std::min(chunks, cap), B), dim3(kThreads), 0, s, Y.problems.at(dk), Y.xw.at(dp), Y.nrm.at(dp),
               Y.dmin.at(dp), Y.dmax.at(dp), Y.desc.at(dp), Y.xy.at(dk), Y.oct.at(dk), Y.kdesc.at(dk), (int)SC, Y.exit.at(dq), Y.level.at(dq),
               Y.count.at(dq), Y.cidx.at(dq), Y.cdist.at(dq));
    if (int rc = w->out.download(s, 0, Y.out.bytes())) return rc;
    GFS_HIP(hipStreamSynchronize(s));  // the call's one synchronisation
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
