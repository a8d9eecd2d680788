// gfs_fuse_search on the gfs_sbp handle (gfs_sbp_reserve_fuse allocates its workspace): ORBmatcher::Fuse(KeyFrame*,
// const vector<MapPoint*>&, th) (reference src/ORBmatcher.cc:1378-1548), the search of every listed map point (DESIGN.md section 13;
// the rule itself is fuse_rule.hpp, shared with the host).
// Grid (ceil(n / 256), B), blockIdx.y = the (list, key frame) problem.  Every workgroup builds its key frame's 64 x 48 grid in LDS
// (load_keyframe_grid_lds, sbp_dev.hpp: cell starts + the items sorted by cell, cells in index order), with position, mvuRight and
// octave of the key-points next to it and the level tables in the header; then a lane owns one map point: projection, gates,
// PredictScale and the walk of its window (walk_window, sbp_dev.hpp).  No point competes with another for a key-point, so nothing is
// resolved across lanes: no global atomics, no waiting between workgroups.
// LDS: 6 146 (cell starts) + 8 192 (items) + 3 x 16 384 (x, y, mvuRight) + 4 096 (octave) + the header = 67.8 KB, two workgroups a CU
// (160 KB).  The cell counters of the build (12 KB) live in the mvuRight table, which is filled after the grid is built; the cell
// of a key-point is recomputed from its position instead of kept.

#include "point_search.hpp"

using namespace gfs;

namespace {

constexpr int kFuseThreads = 256, kFuseWaves = kFuseThreads / 64;

struct FuseProblem {
  gfs_fuse::KeyFrame K;
  int n_mp, list_base, out_base, pad;  // the list's length and its first point in the point arrays; the problem's first output slot
};

static_assert(gfs_fuse::kNegDepth == GFS_FUSE_NEG_DEPTH && gfs_fuse::kNotInImage == GFS_FUSE_NOT_IN_IMAGE && gfs_fuse::kTooNear == GFS_FUSE_TOO_NEAR &&
                  gfs_fuse::kTooFar == GFS_FUSE_TOO_FAR && gfs_fuse::kViewAngle == GFS_FUSE_VIEW_ANGLE &&
                  gfs_fuse::kEmptyWindow == GFS_FUSE_EMPTY_WINDOW && gfs_fuse::kNoCandidate == GFS_FUSE_NO_CANDIDATE &&
                  gfs_fuse::kMatched == GFS_FUSE_MATCHED, "the rule's exits are the ABI's");
static_assert(gfs_fuse::kGridCols == kGridCols && gfs_fuse::kGridRows == kGridRows, "one grid");

__global__ __launch_bounds__(kFuseThreads) void k_fuse(const FuseProblem* __restrict__ problems, const float* __restrict__ mp_xw,
                                                       const float* __restrict__ mp_normal, const float* __restrict__ mp_min,
                                                       const float* __restrict__ mp_max, const uint8_t* __restrict__ mp_desc,
                                                       const float2* __restrict__ kf_xy, const float* __restrict__ kf_ur,
                                                       const uint8_t* __restrict__ kf_oct, const uint8_t* __restrict__ kf_desc, int SC,
                                                       uint8_t* __restrict__ o_exit, int* __restrict__ o_idx, int* __restrict__ o_dist,
                                                       int* __restrict__ o_level) {
  __shared__ unsigned short s_start[kCells + 1];
  __shared__ unsigned short s_items[kSbpMaxCur];
  __shared__ float s_kx[kSbpMaxCur], s_ky[kSbpMaxCur], s_ur[kSbpMaxCur];
  __shared__ uint8_t s_oct[kSbpMaxCur];
  __shared__ int s_scan[kFuseWaves];
  __shared__ FuseProblem s_P;
  static_assert(sizeof(float) * kSbpMaxCur >= sizeof(int) * kCells, "the mvuRight table must hold the cell counters");
  int* s_cnt = reinterpret_cast<int*>(s_ur);
  const int f = blockIdx.y, tid = threadIdx.x;
  if ((int)blockIdx.x * kFuseThreads >= problems[f].n_mp) return;  // (uniform: the grid is sized by the call's longest list)
  if (tid == 0) s_P = problems[f];
  __syncthreads();
  const gfs_fuse::KeyFrame& K = s_P.K;
  const int N = K.n_kp;
  const size_t kf_at = (size_t)f * SC;
  // ---- the key-points and the grid; the counters are done with when it stands: their table becomes mvuRight
  load_keyframe_grid_lds<kFuseThreads>(K, N, kf_xy + kf_at, kf_oct + kf_at, s_kx, s_ky, s_oct, s_start, s_items, s_cnt, s_scan);
  for (int i = tid; i < N; i += kFuseThreads) s_ur[i] = kf_ur[kf_at + i];
  __syncthreads();
  // ---- a lane per map point
  const int i = blockIdx.x * kFuseThreads + tid;
  if (i >= s_P.n_mp) return;
  const size_t at = (size_t)s_P.list_base + i, to = (size_t)s_P.out_base + i;
  const float P[3] = {mp_xw[3 * at], mp_xw[3 * at + 1], mp_xw[3 * at + 2]};
  const float Pn[3] = {mp_normal[3 * at], mp_normal[3 * at + 1], mp_normal[3 * at + 2]};
  const gfs_fuse::Proj R = gfs_fuse::project(K, P, Pn, mp_min[at], mp_max[at]);
  int best_dist = 256, best_idx = -1, ex = R.exit;
  if (R.exit < 0) {
    bool any = false;
    walk_window(
        R.x0, R.x1, R.y0, R.y1, s_start, s_items, mp_desc + 32 * at, kf_desc + 32 * kf_at,
        [&](int j) {
          const float kx = s_kx[j], ky = s_ky[j];
          if (!gfs_fuse::in_window(R, kx, ky)) return false;
          any = true;
          return gfs_fuse::candidate_ok(K, R, kx, ky, s_ur[j], (int)s_oct[j]);
        },
        [&](int j, int d) {
          if (d < best_dist) {  // strict: the first visited of equal distances wins
            best_dist = d;
            best_idx = j;
          }
        });
    ex = gfs_fuse::search_exit(any, best_dist);
  }
  o_exit[to] = (uint8_t)ex;
  o_idx[to] = best_idx;
  o_dist[to] = best_dist;
  o_level[to] = R.level;
}

using Layout = gfs::FuseLayout<FuseProblem>;

}  // namespace

struct gfs_fuse_workspace : gfs::PointSearchWorkspace {};

extern "C" {

int gfs_sbp_reserve_fuse(gfs_sbp* h, int max_lists, int max_points_per_list, int max_keyframes) {
  GFS_REQUIRE(h && max_lists > 0 && max_points_per_list > 0 && max_keyframes > 0, GFS_ERR_INVALID_ARG, "gfs_sbp_reserve_fuse: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipStreamSynchronize(h->stream));
  const size_t SP = gfs::align_up((size_t)max_points_per_list, 64), SC = gfs::align_up((size_t)h->max_cur, 64);
  const Layout Y{SP * max_lists, (size_t)max_keyframes, SC, SP * max_keyframes};
  h->fuse.reset();
  std::unique_ptr<gfs_fuse_workspace> w(new gfs_fuse_workspace);
  if (int rc = w->alloc(Y.pts.bytes(), Y.kf.bytes(), Y.out.bytes(), max_lists, max_points_per_list, max_keyframes)) return rc;
  h->fuse = std::move(w);
  return GFS_OK;
}

int gfs_fuse_search(gfs_sbp* h, const gfs_fuse_points* lists, int n_lists, const gfs_fuse_keyframe* kfs, int B, gfs_fuse_result* results) {
  static const char who[] = "gfs_fuse_search", what[] = "key frame";
  GFS_REQUIRE(h && lists && kfs && results && n_lists > 0 && B > 0, GFS_ERR_INVALID_ARG, "gfs_fuse_search: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_fuse_workspace* w = static_cast<gfs_fuse_workspace*>(h->fuse.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_fuse_search: call gfs_sbp_reserve_fuse first");
  GFS_REQUIRE(n_lists <= w->lists, GFS_ERR_CAPACITY, "gfs_fuse_search: %d lists exceed the reserve %d", n_lists, w->lists);
  GFS_REQUIRE(B <= w->kfs, GFS_ERR_CAPACITY, "gfs_fuse_search: %d key frames exceed the reserve %d", B, w->kfs);
  GFS_HIP(hipSetDevice(h->device));
  // every refusal comes before anything is staged
  size_t T = 0, O = 0, SC = 64;
  int n_max = 0;
  std::vector<size_t> list_base;
  if (int rc = check_point_lists(who, lists, n_lists, w->points, list_base, &T)) return rc;
  for (int f = 0; f < B; f++) {
    const gfs_fuse_keyframe& k = kfs[f];
    if (int rc = check_search_kf_head(who, what, f, k, h->max_cur, k.scale_factors && k.inv_level_sigma2, "scale factors and inverse level variances", n_lists))
      return rc;
    GFS_REQUIRE(k.n_kp == 0 || (k.kps_un && k.u_right && k.desc), GFS_ERR_INVALID_ARG, "gfs_fuse_search: key frame %d has NULL key-point arrays", f);
    const int n = lists[k.list].n_mp;
    if (int rc = check_search_kf_tail(who, what, f, k, n, results[f])) return rc;
    SC = std::max(SC, gfs::align_up((size_t)k.n_kp, 64));
    O += gfs::align_up((size_t)n, 64);
    n_max = std::max(n_max, n);
  }
  const Layout Y{T, (size_t)B, SC, O};  // within the reserve: T <= lists x SP, O <= B x SP, SC <= max_cur
  uint8_t* hk = w->kf.h.p;
  stage_point_lists(Y.p, w->pts.h.p, lists, n_lists, list_base);
  std::vector<size_t> out_base((size_t)B);
  size_t o_at = 0;
  for (int f = 0; f < B; f++) {
    const gfs_fuse_keyframe& k = kfs[f];
    FuseProblem& Q = Y.problems.at(hk)[f];
    memset(&Q, 0, sizeof(Q));
    fill_search_keyframe(Q.K, k);
    Q.K.bf = k.bf;
    for (int c = 0; c < k.n_levels; c++) Q.K.inv_sigma2[c] = k.inv_level_sigma2[c];
    Q.n_mp = lists[k.list].n_mp;
    Q.list_base = (int)list_base[k.list];
    Q.out_base = (int)o_at;
    out_base[f] = o_at;
    o_at += gfs::align_up((size_t)Q.n_mp, 64);
    stage_xy_oct(k.kps_un, k.n_kp, Y.xy.at(hk, (size_t)f * SC), Y.oct.at(hk, (size_t)f * SC));
    Y.ur.put(hk, (size_t)f * SC, k.u_right, (size_t)k.n_kp);
    Y.kdesc.put(hk, (size_t)f * SC, k.desc, (size_t)k.n_kp);
  }
  if (n_max > 0) {
    const uint8_t *dp = w->pts.d.p, *dk = w->kf.d.p;
    uint8_t* dq = w->out.d.p;
    const int rc = w->run(h->stream, Y.pts.bytes(), Y.kf.bytes(), Y.out.bytes(), [&]() -> int {
      GFS_LAUNCH("k_fuse", k_fuse, dim3((n_max + kFuseThreads - 1) / kFuseThreads, B), dim3(kFuseThreads), 0, h->stream, Y.problems.at(dk),
                 Y.p.xw.at(dp), Y.p.nrm.at(dp), Y.p.dmin.at(dp), Y.p.dmax.at(dp), Y.p.desc.at(dp), Y.xy.at(dk), Y.ur.at(dk), Y.oct.at(dk),
                 Y.kdesc.at(dk), (int)SC, Y.exit.at(dq), Y.idx.at(dq), Y.dist.at(dq), Y.level.at(dq));
      return GFS_OK;
    });
    if (rc) return rc;
  }
  const uint8_t* ho = w->out.h.p;
  for (int f = 0; f < B; f++) {
    const size_t n = (size_t)lists[kfs[f].list].n_mp, at = out_base[f];
    gfs_fuse_result& r = results[f];
    int matched = 0;
    Y.exit.get(r.exit, ho, at, n);
    Y.idx.get(r.best_idx, ho, at, n);
    Y.dist.get(r.best_dist, ho, at, n);
    Y.level.get(r.level, ho, at, n);
    for (size_t i = 0; i < n; i++) matched += r.exit[i] == GFS_FUSE_MATCHED;
    r.n_matched = matched;
  }
  return GFS_OK;
}

}  // extern "C"
