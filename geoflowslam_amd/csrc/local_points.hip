// gfs_search_local_points on the gfs_sbp handle (gfs_sbp_reserve_local allocates its workspace).
// Tracking::SearchLocalPoints, second loop onwards (reference src/Tracking.cc:4312-4358):
// Frame::isInFrustum (src/Frame.cc:876-931, Nleft == -1) + MapPoint::PredictScale (src/MapPoint.cc:565-579) for every listed
// local map point, the filter of ORBmatcher.cc:53-58, a stable compaction of the survivors into the arrays k_sbp mode 1 reads, then
// k_sbp itself -- all on one stream, no host step in between (DESIGN.md section 12 states the arithmetic).
//   k_lp_frustum: a thread per map point, blockIdx.y = frame.  Per-point outputs, the point's rank inside its block's part of the
//                 search set (wave ballots + the four wave totals through LDS), the block's counts to a small table.
//   k_lp_compact: position = counts of the preceding blocks + rank: list order is kept, no atomic decides a position and no workgroup
//                 waits for another (the kernel boundary is the only dependency).  Gathers projection / level / viewing cosine /
//                 descriptor / has_obs into k_sbp's arrays, writes the list index of every entry and patches n_last in the header.
// k_sbp writes cur_match / nmatches into the same result block as the per-point outputs and the index list: one copy out, after
// which the host maps cur_match (indices into the compacted set) to the caller's list indices.

#include "glibc_math.hpp"
#include "sbp_handle.hpp"

using namespace gfs;

namespace {

constexpr int kLpThreads = 256, kLpWaves = kLpThreads / 64;
constexpr float kLpMinDistFactor = 0.8f;  // MapPoint::GetMinDistanceInvariance (src/MapPoint.cc)
constexpr float kLpMaxDistFactor = 1.2f;  // MapPoint::GetMaxDistanceInvariance

struct LpFrame {
  int n_mp, n_levels, far_points, max_last;
  float R[9], t[3], Ow[3];
  float fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y;
  float log_scale_factor, view_cos_limit, th_far_points;
};
struct LpMeta {
  int n_to_match, n_searched, overflow, pad;
};

__global__ __launch_bounds__(kLpThreads) void k_lp_frustum(const LpFrame* __restrict__ frames, const float* __restrict__ xw,
                                                           const float* __restrict__ normal, const float* __restrict__ min_dist,
                                                           const float* __restrict__ max_dist, int SM, int NB,
                                                           uint8_t* __restrict__ in_view, float* __restrict__ proj,
                                                           float* __restrict__ depth, float* __restrict__ view_cos,
                                                           int* __restrict__ level, int* __restrict__ rank, int2* __restrict__ block_cnt) {
  __shared__ int s_search[kLpWaves], s_view[kLpWaves];
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * kLpThreads + tid;
  const LpFrame& F = frames[f];
  const size_t at = (size_t)f * SM + i;
  bool inview = false, search = false;
  if (i < F.n_mp) {
    const float P[3] = {xw[3 * at], xw[3 * at + 1], xw[3 * at + 2]};
    float pu = -1.0f, pv = -1.0f, pxr = 0.0f, vc = 0.0f;
    int lv = 0;
    float Pc[3];
    for (int r = 0; r < 3; r++) Pc[r] = ((F.R[3 * r] * P[0] + F.R[3 * r + 1] * P[1]) + F.R[3 * r + 2] * P[2]) + F.t[r];
    const float dep = sqrtf((Pc[0] * Pc[0] + Pc[1] * Pc[1]) + Pc[2] * Pc[2]);
    const float invz = 1.0f / Pc[2];
    do {
      if (Pc[2] < 0.0f) break;
      const float u = (F.fx * Pc[0]) / Pc[2] + F.cx, v = (F.fy * Pc[1]) / Pc[2] + F.cy;
      if (u < F.min_x || u > F.max_x) break;
      if (v < F.min_y || v > F.max_y) break;
      if (!(fabsf(u) <= 3.402823466e38f) || !(fabsf(v) <= 3.402823466e38f)) break;  // chosen rule: 0 / 0 -> out, (-1, -1) stays
      pu = u;
      pv = v;
      const float PO[3] = {P[0] - F.Ow[0], P[1] - F.Ow[1], P[2] - F.Ow[2]};
      const float dist = sqrtf((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
      const float mx = max_dist[at];
      if (dist < kLpMinDistFactor * min_dist[at] || dist > kLpMaxDistFactor * mx) break;
      const float Pn[3] = {normal[3 * at], normal[3 * at + 1], normal[3 * at + 2]};
      vc = ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]) / dist;
      if (vc < F.view_cos_limit) break;
      // PredictScale: (int)std::ceil(logf(ratio) / mfLogScaleFactor); a value no int holds converts to INT_MIN on x86-64 -> level 0
      const float c = ceilf(gfs_glibc::logf(mx / dist) / F.log_scale_factor);
      lv = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : 0;
      lv = lv < 0 ? 0 : (lv >= F.n_levels ? F.n_levels - 1 : lv);
      pxr = u - F.bf * invz;
      inview = true;
    } while (false);
    search = inview && !(F.far_points && dep > F.th_far_points);
    in_view[at] = inview ? 1 : 0;
    proj[3 * at] = pu;
    proj[3 * at + 1] = pv;
    proj[3 * at + 2] = pxr;
    depth[at] = dep;
    view_cos[at] = vc;
    level[at] = lv;
  }
  const unsigned long long ms = __ballot(search), mv = __ballot(inview);
  if (lane == 0) {
    s_search[wave] = __popcll(ms);
    s_view[wave] = __popcll(mv);
  }
  __syncthreads();
  if (i < F.n_mp) {
    int before = 0;
    for (int w = 0; w < wave; w++) before += s_search[w];
    rank[at] = search ? before + __popcll(ms & ((1ull << lane) - 1ull)) : -1;
  }
  if (tid == 0) {
    int a = 0, b = 0;
    for (int w = 0; w < kLpWaves; w++) {
      a += s_search[w];
      b += s_view[w];
    }
    block_cnt[(size_t)f * NB + blockIdx.x] = make_int2(a, b);
  }
}

__global__ __launch_bounds__(kLpThreads) void k_lp_compact(const LpFrame* __restrict__ frames, const int* __restrict__ rank,
                                                           const int2* __restrict__ block_cnt, int SM, int NB, int nb_used,
                                                           const float* __restrict__ proj, const float* __restrict__ view_cos,
                                                           const int* __restrict__ level, const uint8_t* __restrict__ desc,
                                                           const uint8_t* __restrict__ has_obs, SbpPair* __restrict__ pairs, int SL,
                                                           float* __restrict__ o_proj, uint8_t* __restrict__ o_desc, int* __restrict__ o_level,
                                                           float* __restrict__ o_cos, uint8_t* __restrict__ o_obs, int* __restrict__ o_index,
                                                           LpMeta* __restrict__ meta) {
  __shared__ int s_red[3][kLpWaves];
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LpFrame& F = frames[f];
  // the block's base (sum over the preceding blocks) and the frame's totals, from the count table
  int base = 0, total = 0, views = 0;
  for (int b = tid; b < nb_used; b += kLpThreads) {
    const int2 c = block_cnt[(size_t)f * NB + b];
    if (b < (int)blockIdx.x) base += c.x;
    total += c.x;
    views += c.y;
  }
  for (int ofs = 32; ofs > 0; ofs >>= 1) {
    base += __shfl_down(base, ofs, 64);
    total += __shfl_down(total, ofs, 64);
    views += __shfl_down(views, ofs, 64);
  }
  if (lane == 0) {
    s_red[0][wave] = base;
    s_red[1][wave] = total;
    s_red[2][wave] = views;
  }
  __syncthreads();
  base = total = views = 0;
  for (int w = 0; w < kLpWaves; w++) {
    base += s_red[0][w];
    total += s_red[1][w];
    views += s_red[2][w];
  }
  const bool overflow = total > F.max_last;  // k_sbp's tables end there: nothing is truncated, the search is skipped
  if (blockIdx.x == 0 && tid == 0) {
    pairs[f].n_last = overflow ? 0 : total;
    meta[f] = LpMeta{views, total, overflow ? 1 : 0, 0};
  }
  if (overflow) return;
  const int i = blockIdx.x * kLpThreads + tid;
  if (i >= F.n_mp) return;
  const size_t at = (size_t)f * SM + i;
  const int r = rank[at];
  if (r < 0) return;
  const size_t to = (size_t)f * SL + (base + r);  // base + r < total <= max_last <= SL
  o_proj[3 * to] = proj[3 * at];
  o_proj[3 * to + 1] = proj[3 * at + 1];
  o_proj[3 * to + 2] = proj[3 * at + 2];
  o_level[to] = level[at];
  o_cos[to] = view_cos[at];
  const uint4* d = reinterpret_cast<const uint4*>(desc + 32 * at);
  uint4* o = reinterpret_cast<uint4*>(o_desc + 32 * to);
  o[0] = d[0];
  o[1] = d[1];
  o_obs[to] = has_obs[at];
  o_index[to] = i;
}

using Layout = gfs::LocalLayout<LpFrame, LpMeta>;

}  // namespace

// The listed map points of a call, pinned and on the device; the results likewise (per-point outputs, the search set's list indices,
// k_sbp's cur_match / nmatches); ranks and block counts stay on the device.
struct gfs_local_workspace : gfs_sbp_workspace {
  int max_local = 0;
  gfs::Mirror in, out;
  gfs::DevBuf<int> d_rank;
  gfs::DevBuf<int2> d_block_cnt;
};

extern "C" {

int gfs_sbp_reserve_local(gfs_sbp* h, int max_local_points) {
  GFS_REQUIRE(h && max_local_points > 0, GFS_ERR_INVALID_ARG, "gfs_sbp_reserve_local: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipStreamSynchronize(h->stream));
  const int SM = (int)gfs::align_up((size_t)max_local_points, 64), SL = (int)gfs::align_up((size_t)h->max_last, 64);
  const int SC = (int)gfs::align_up((size_t)h->max_cur, 64);
  const Layout Z{(size_t)h->max_batch, SM, std::min(SM, SL), SC};
  h->local.reset();
  std::unique_ptr<gfs_local_workspace> w(new gfs_local_workspace);
  int rc = 0;
  if (!rc) rc = w->in.alloc(Z.in.bytes());
  if (!rc) rc = w->out.alloc(Z.out.bytes());
  if (!rc) rc = w->d_rank.alloc((size_t)SM * h->max_batch);
  if (!rc) rc = w->d_block_cnt.alloc((size_t)(SM / kLpThreads + 1) * h->max_batch);
  if (rc) return rc;
  w->max_local = max_local_points;
  h->local = std::move(w);
  return GFS_OK;
}

int gfs_search_local_points(gfs_sbp* h, const gfs_local_points_problem* problems, int B, gfs_local_points_result* results) {
  GFS_REQUIRE(h && problems && results && B > 0, GFS_ERR_INVALID_ARG, "gfs_search_local_points: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_search_local_points: batch %d exceeds capacity %d", B, h->max_batch);
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_local_workspace* w = static_cast<gfs_local_workspace*>(h->local.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_search_local_points: call gfs_sbp_reserve_local first");
  GFS_HIP(hipSetDevice(h->device));
  const int capM = w->max_local, capC = h->max_cur;
  for (int f = 0; f < B; f++) {
    const gfs_local_points_problem& p = problems[f];
    const gfs_local_points_result& r = results[f];
    GFS_REQUIRE(p.n_mp >= 0 && p.n_mp <= capM && p.n_cur >= 0 && p.n_cur <= capC, GFS_ERR_CAPACITY,
                "gfs_search_local_points: frame %d has %d map points / %d key-points (capacity %d / %d)", f, p.n_mp, p.n_cur, capM, capC);
    GFS_REQUIRE(p.n_levels > 0 && p.n_levels <= 16 && p.scale_factors, GFS_ERR_INVALID_ARG,
                "gfs_search_local_points: frame %d needs 1..16 scale factors", f);
    GFS_REQUIRE(p.n_mp == 0 || (p.mp_xw && p.mp_normal && p.mp_min_dist && p.mp_max_dist && p.mp_desc && p.mp_has_obs),
                GFS_ERR_INVALID_ARG, "gfs_search_local_points: frame %d has NULL map-point arrays", f);
    GFS_REQUIRE(p.n_mp == 0 || (r.in_view && r.proj && r.depth && r.view_cos && r.level), GFS_ERR_INVALID_ARG,
                "gfs_search_local_points: frame %d has NULL result arrays", f);
    GFS_REQUIRE(p.n_cur == 0 || (p.cur_kps_un && p.cur_u_right && p.cur_desc && p.cur_has_mp_obs && r.cur_match), GFS_ERR_INVALID_ARG,
                "gfs_search_local_points: frame %d has NULL key-point arrays", f);
  }
  const int SM = sbp_stride(B, capM, [&](int f) { return problems[f].n_mp; }), SC = sbp_stride(B, capC, [&](int f) { return problems[f].n_cur; });
  const int SL = std::min(SM, (int)gfs::align_up((size_t)h->max_last, 64));
  const SbpBlocks Y{(size_t)B, SL, SC};
  const Layout Z{(size_t)B, SM, SL, SC};
  uint8_t* li = w->in.h.p;
  for (int f = 0; f < B; f++) {
    const gfs_local_points_problem& p = problems[f];
    LpFrame& F = Z.frames.at(li)[f];
    F.n_mp = p.n_mp;
    F.n_levels = p.n_levels;
    F.far_points = p.far_points != 0;
    F.max_last = h->max_last;
    for (int k = 0; k < 9; k++) F.R[k] = p.Rcw[k];
    for (int k = 0; k < 3; k++) {
      F.t[k] = p.tcw[k];
      F.Ow[k] = p.Ow[k];
    }
    F.fx = p.fx;
    F.fy = p.fy;
    F.cx = p.cx;
    F.cy = p.cy;
    F.bf = p.bf;
    F.min_x = p.min_x;
    F.max_x = p.max_x;
    F.min_y = p.min_y;
    F.max_y = p.max_y;
    F.log_scale_factor = p.log_scale_factor;
    F.view_cos_limit = p.view_cos_limit;
    F.th_far_points = p.th_far_points;
    sbp_map_pair(Y.pairs.at(h->in.h.p)[f], p, 0);  // n_last: k_lp_compact writes the size of the search set
    const size_t at = (size_t)f * SM, n = (size_t)p.n_mp;
    Z.xw.put(li, at, p.mp_xw, n);
    Z.nrm.put(li, at, p.mp_normal, n);
    Z.dmin.put(li, at, p.mp_min_dist, n);
    Z.dmax.put(li, at, p.mp_max_dist, n);
    Z.desc.put(li, at, p.mp_desc, n);
    Z.obs.put(li, at, p.mp_has_obs, n);
    sbp_stage_cur(h, Y, f, p.n_cur, p.cur_kps_un, p.cur_u_right, p.cur_desc, p.cur_has_mp_obs);
  }
  hipStream_t s = h->stream;
  uint8_t *d = h->in.d.p, *dq = w->out.d.p;
  const uint8_t* dl = w->in.d.p;
  // three copies in: the listed map points, the pair headers, the key-point arrays (the map-point arrays of k_sbp are filled on the device)
  if (int rc = w->in.upload(s, 0, Z.in.bytes())) return rc;
  if (int rc = h->in.upload(s, 0, Y.pairs.bytes((size_t)B))) return rc;
  if (int rc = h->in.upload(s, Y.kp.off, Y.in.bytes())) return rc;
  const int nb = (SM + kLpThreads - 1) / kLpThreads, NB = SM / kLpThreads + 1;  // blocks of this call; rows of the count table
  GFS_LAUNCH("k_lp_frustum", k_lp_frustum, dim3(nb, B), dim3(kLpThreads), 0, s, Z.frames.at(dl), Z.xw.at(dl), Z.nrm.at(dl), Z.dmin.at(dl),
             Z.dmax.at(dl), SM, NB, Z.view.at(dq), Z.proj.at(dq), Z.depth.at(dq), Z.cos.at(dq), Z.level.at(dq), w->d_rank.p, w->d_block_cnt.p);
  GFS_LAUNCH("k_lp_compact", k_lp_compact, dim3(nb, B), dim3(kLpThreads), 0, s, Z.frames.at(dl), (const int*)w->d_rank.p,
             (const int2*)w->d_block_cnt.p, SM, NB, nb, Z.proj.at(dq), Z.cos.at(dq), Z.level.at(dq), Z.desc.at(dl), Z.obs.at(dl), Y.pairs.at(d), SL, Y.xw.at(d), Y.desc.at(d), Y.oct.at(d), Y.ang.at(d), Y.lobs.at(d), Z.index.at(dq),
             Z.meta.at(dq));
  if (int rc = sbp_launch(h, B, Y, Z.match.at(dq), Z.nm.at(dq))) return rc;
  if (int rc = w->out.download(s, 0, Z.out.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));  // the call's one synchronisation
  const uint8_t* lo = w->out.h.p;
  const LpMeta* meta = Z.meta.at(lo);
  int over = -1;
  for (int f = 0; f < B; f++) {
    const gfs_local_points_problem& p = problems[f];
    gfs_local_points_result& r = results[f];
    const size_t at = (size_t)f * SM, n = (size_t)p.n_mp;
    Z.view.get(r.in_view, lo, at, n);
    Z.proj.get(r.proj, lo, at, n);
    Z.depth.get(r.depth, lo, at, n);
    Z.cos.get(r.view_cos, lo, at, n);
    Z.level.get(r.level, lo, at, n);
    const int32_t *cm = Z.match.at(lo, (size_t)f * SC), *index = Z.index.at(lo, (size_t)f * SL);
    for (int i = 0; i < p.n_cur; i++) r.cur_match[i] = cm[i] >= 0 ? index[cm[i]] : cm[i];  // compacted set -> the caller's list
    r.n_to_match = meta[f].n_to_match;
    r.n_searched = meta[f].n_searched;
    r.nmatches = Z.nm.at(lo)[f];
    if (meta[f].overflow && over < 0) over = f;
  }
  GFS_REQUIRE(over < 0, GFS_ERR_CAPACITY, "gfs_search_local_points: frame %d has a search set of %d map points (capacity %d): not searched",
              over, meta[over].n_searched, h->max_last);
  return GFS_OK;
}

}  // extern "C"
