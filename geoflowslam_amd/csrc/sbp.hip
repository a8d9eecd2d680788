// ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (reference
// src/ORBmatcher.cc:1853-2063) on MI355X, single-camera frames (Nleft == -1), a batch of frame pairs per launch.
//
// One 256-thread workgroup per frame pair:
//   0. Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:734-761, 1073-1084): the 64 x 48 grid of the current frame as
//      a CSR table in LDS (cells keep ascending key-point order, like the reference's push_back);
//   A. in parallel over the last frame's map points: projection with Sophus::SE3f float arithmetic
//      (Thirdparty/Sophus/sophus/so3.hpp:358-367), Frame::GetFeaturesInArea (src/Frame.cc:1007-1071) and the Hamming
//      distances (ORBmatcher::DescriptorDistance :2536-2550) of the window's candidates, kept in visiting order;
//   B. the reference loop is order dependent (a key-point taken by an earlier map point with observations is skipped by
//      the later ones, :1914-1915), so the assignment itself runs in map-point order on one wave: the lanes check one
//      candidate each, a wave-wide arg-min (first minimum wins, as `dist < bestDist` does) picks the match;
//   C. rotation histogram + ComputeThreeMaxima (:2500-2532) and the final NULL-ing of inconsistent matches.
// Mode 1 is ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th, ...) (:43-206): the projections come
// with the map points (Frame::isInFrustum), the window depends on the viewing angle, and phase B keeps best and second best
// (two arg-min rounds) for the ratio test; no rotation histogram.
// Results are bit-exact integer work; the float decisions (image bounds, window membership, level ranges, histogram bins)
// use the reference's float expressions (the library is built with -ffp-contract=off).
#include <type_traits>

#include "fuse_rule.hpp"
#include "sbp_handle.hpp"

using namespace gfs;

namespace {

constexpr int kHisto = 30, kThHigh = 100;
constexpr int kSbpThreads = 1024;  // a thread per map point while their candidates are enumerated (dependent gathers: parallelism hides them)
constexpr int kSbpMaxLast = 8192;  // map points of the last frame
constexpr int kCand = 64;          // candidates kept per map point (more: the assignment pass re-enumerates them)
constexpr int kChunk = 32;         // map points per step of the assignment pass (their candidate lists are prefetched into LDS)

struct SbpView {
  const float* last_xw;
  const uint8_t* last_desc;
  const int* last_octave;
  const float* last_angle;
  const uint8_t* last_has_obs;
  const gfs_keypoint* cur_kp;
  const float* cur_ur;
  const uint8_t* cur_desc;
  const uint8_t* cur_has_obs;
};

using gfs_fuse::so3_act;  // SO3f * p (so3.hpp:358-367), shared with the host statement of the Fuse rule

struct Proj {
  float u, v, radius, ur, ur_gate;  // window centre / half size, predicted right-image x and its tolerance
  int minLevel, maxLevel, x0, x1, y0, y1;
  bool ok;
};

// projection of map point l + the cell range of its search window (everything before the candidate loop of :1878-1911)
__device__ __forceinline__ Proj sbp_project(const SbpPair& P, const SbpView& V, int l, bool bForward, bool bBackward) {
  Proj R;
  R.ok = false;
  if (P.mode == 1) {  // the projection was done by Frame::isInFrustum: (mTrackProjX, mTrackProjY, mTrackProjXR), level, viewCos
    R.u = V.last_xw[3 * l];
    R.v = V.last_xw[3 * l + 1];
    R.ur = V.last_xw[3 * l + 2];
    const int level = V.last_octave[l];
    float r = (double)V.last_angle[l] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos (:250-255)
    if ((double)P.th != 1.0) r *= P.th;
    R.radius = r * P.scale[level];
    R.ur_gate = R.radius;
    R.minLevel = level - 1;
    R.maxLevel = level;
  } else {
    float x3Dc[3];
    so3_act(P.Tcw_q, V.last_xw + 3 * l, x3Dc);
    for (int k = 0; k < 3; k++) x3Dc[k] += P.Tcw_t[k];
    const float invzc = (float)(1.0 / (double)x3Dc[2]);
    if (invzc < 0) return R;
    R.u = P.fx * x3Dc[0] / x3Dc[2] + P.cx;
    R.v = P.fy * x3Dc[1] / x3Dc[2] + P.cy;
    if (R.u < P.min_x || R.u > P.max_x) return R;
    if (R.v < P.min_y || R.v > P.max_y) return R;
    const int oct = V.last_octave[l];
    R.radius = P.th * P.scale[oct];
    R.ur = R.u - P.bf * invzc;
    R.ur_gate = R.radius;
    if (bForward) {
      R.minLevel = oct;
      R.maxLevel = -1;
    } else if (bBackward) {
      R.minLevel = 0;
      R.maxLevel = oct;
    } else {
      R.minLevel = oct - 1;
      R.maxLevel = oct + 1;
    }
  }
  R.x0 = max(0, (int)floorf((R.u - P.min_x - R.radius) * P.grid_w_inv));
  if (R.x0 >= kGridCols) return R;
  R.x1 = min(kGridCols - 1, (int)ceilf((R.u - P.min_x + R.radius) * P.grid_w_inv));
  if (R.x1 < 0) return R;
  R.y0 = max(0, (int)floorf((R.v - P.min_y - R.radius) * P.grid_h_inv));
  if (R.y0 >= kGridRows) return R;
  R.y1 = min(kGridRows - 1, (int)ceilf((R.v - P.min_y + R.radius) * P.grid_h_inv));
  if (R.y1 < 0) return R;
  R.ok = true;
  return R;
}

// The current frame's key-points as the candidate loop needs them, in LDS (filled with the grid): position, octave, mvuRight, and
// whether a map point with observations sits there on entry.
struct SbpCur {
  const float* x;
  const float* y;
  const uint8_t* oct;
  const float* ur;
  const uint8_t* has_obs;
};

// GetFeaturesInArea + the static filters of the candidate loop, in the reference's visiting order (walk_window, sbp_dev.hpp).
// f(i2, dist) is called for every candidate that survives them; returns whether vIndices2 was non-empty.
template <class F>
__device__ __forceinline__ bool sbp_candidates(const SbpPair& P, const SbpView& V, const SbpCur& C, const Proj& R, int l,
                                               const unsigned short* s_start, const unsigned short* s_items, F&& f) {
  const bool bCheckLevels = (R.minLevel > 0) || (R.maxLevel >= 0);
  bool any = false;
  walk_window(
      R.x0, R.x1, R.y0, R.y1, s_start, s_items, V.last_desc + 32 * (size_t)l, V.cur_desc,
      [&](int j) {
        if (bCheckLevels) {
          const int oct = C.oct[j];
          if (oct < R.minLevel) return false;
          if (R.maxLevel >= 0 && oct > R.maxLevel) return false;
        }
        const float distx = C.x[j] - R.u, disty = C.y[j] - R.v;
        if (!(fabsf(distx) < R.radius && fabsf(disty) < R.radius)) return false;
        any = true;
        if (C.has_obs[j]) return false;  // a map point with observations was there on entry: never replaced
        const float ur2 = C.ur[j];
        if (ur2 > 0) {
          const float er = fabsf(R.ur - ur2);
          if (er > R.ur_gate) return false;
        }
        return true;
      },
      f);
  return any;
}

// minimum of an unsigned value over the wave's 64 lanes, in every lane: quad permutes and row rotations (DPP) inside the rows of 16,
// the four row results through scalar registers
__device__ __forceinline__ unsigned wave_umin(unsigned v) {
  auto dpp = [](unsigned x, auto ctrl) { return (unsigned)__builtin_amdgcn_mov_dpp((int)x, decltype(ctrl)::value, 0xf, 0xf, true); };
  v = min(v, dpp(v, std::integral_constant<int, 0xB1>{}));   // lane ^ 1
  v = min(v, dpp(v, std::integral_constant<int, 0x4E>{}));   // lane ^ 2
  v = min(v, dpp(v, std::integral_constant<int, 0x124>{}));  // row_ror:4
  v = min(v, dpp(v, std::integral_constant<int, 0x128>{}));  // row_ror:8
  const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16),
                 r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(r0, r1), min(r2, r3));
}

#ifdef GFS_SBP_TIMING
#define SBP_T(k) { const long long _n = clock64(); if (threadIdx.x == 0) sbp_t[k] = _n; }
#else
#define SBP_T(k)
#endif
__global__ __launch_bounds__(kSbpThreads) void k_sbp(const SbpPair* __restrict__ pairs, const float* __restrict__ last_xw,
                                                     const uint8_t* __restrict__ last_desc, const int* __restrict__ last_octave,
                                                     const float* __restrict__ last_angle, const uint8_t* __restrict__ last_has_obs,
                                                     const gfs_keypoint* __restrict__ cur_kp, const float* __restrict__ cur_ur,
                                                     const uint8_t* __restrict__ cur_desc, const uint8_t* __restrict__ cur_has_obs,
                                                     int SL, int SC, unsigned* __restrict__ cand, int* __restrict__ cand_cnt,
                                                     int* __restrict__ lsel, int* __restrict__ cur_match, int* __restrict__ nmatches) {
  __shared__ unsigned short s_cell[kSbpMaxCur];
  __shared__ unsigned short s_start[kCells + 1];
  __shared__ unsigned short s_items[kSbpMaxCur];
  __shared__ short s_state[kSbpMaxCur];  // -1 untouched, -2 reset to NULL, >= 0 map point of last entry l
  // 16 KB used twice: the cell counters of the grid build, then the two candidate buffers of the assignment pass
  __shared__ unsigned s_pool[2 * kChunk * kCand];
  int* s_cnt = reinterpret_cast<int*>(s_pool);
  static_assert(2 * kChunk * kCand >= kCells, "the pool must hold the cell counters");
  __shared__ int s_hold[kSbpMaxCur];  // last taker of a key-point (assignment pass)
  __shared__ uint8_t s_hasobs[kSbpMaxLast];  // Observations() > 0 of the last frame's map points
  __shared__ uint8_t s_oct[kSbpMaxCur];      // octave of the current key-points (the ratio test of the map-point overload)
  __shared__ int s_scan[16];
  __shared__ float s_kx[kSbpMaxCur], s_ky[kSbpMaxCur], s_ur[kSbpMaxCur];  // key-point position, mvuRight
  __shared__ uint8_t s_ho[kSbpMaxCur];                                    // a map point with observations on entry
  __shared__ int s_hist[kHisto];
  __shared__ int s_ctl[4];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
#ifdef GFS_SBP_TIMING
  __shared__ long long sbp_t[8];
#endif
  SBP_T(0)
  // the pair's header lives in LDS: its scale table is indexed by the octave, and a private copy indexed at run time is a copy in
  // scratch memory -- every field access a round trip to the L1
  __shared__ SbpPair s_P;
  if (tid == 0) s_P = pairs[f];
  __syncthreads();
  const SbpPair& P = s_P;
  const SbpView V{last_xw + (size_t)f * SL * 3, last_desc + (size_t)f * SL * 32, last_octave + (size_t)f * SL,
                  last_angle + (size_t)f * SL, last_has_obs + (size_t)f * SL, cur_kp + (size_t)f * SC,
                  cur_ur + (size_t)f * SC, cur_desc + (size_t)f * SC * 32, cur_has_obs + (size_t)f * SC};
  unsigned* cnd = cand + (size_t)f * SL * kCand;
  int* ccnt = cand_cnt + (size_t)f * SL;
  int* sel = lsel + (size_t)f * SL;
  const int N = P.n_cur, NL = P.n_last;
  // ---- 0. grid (Frame::AssignFeaturesToGrid: the key-points of a cell in index order) + the key-point fields the windows look at
  for (int c = tid; c < kCells; c += kSbpThreads) s_cnt[c] = 0;
  if (tid < kHisto) s_hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += kSbpThreads) {  // (the cell count of build_grid_lds, fused with the loads)
    const gfs_keypoint kp = V.cur_kp[i];
    const int c = pos_in_grid(P, kp.x, kp.y);
    s_cell[i] = (unsigned short)c;  // 0xffff outside the grid
    s_state[i] = -1;
    s_oct[i] = (uint8_t)kp.octave;
    s_kx[i] = kp.x;
    s_ky[i] = kp.y;
    s_ur[i] = V.cur_ur[i];
    s_ho[i] = V.cur_has_obs[i];
    if (c >= 0) atomicAdd(&s_cnt[c], 1);
  }
  grid_from_counts_lds<kSbpThreads>(N, [&](int i) { return s_cell[i] == 0xffff ? -1 : (int)s_cell[i]; }, s_start, s_items, s_cnt, s_scan);
  const SbpCur Cur{s_kx, s_ky, s_oct, s_ur, s_ho};
  // twc = Tcw.inverse().translation(); tlc = Tlw * twc  (se3.hpp:208-211; the SO3 constructor re-normalises the conjugate)
  float qi[4] = {-P.Tcw_q[0], -P.Tcw_q[1], -P.Tcw_q[2], P.Tcw_q[3]};
  {
    const float nrm = sqrtf((qi[0] * qi[0] + qi[2] * qi[2]) + (qi[1] * qi[1] + qi[3] * qi[3]));
    for (int k = 0; k < 4; k++) qi[k] /= nrm;
  }
  const float mt[3] = {P.Tcw_t[0] * -1.0f, P.Tcw_t[1] * -1.0f, P.Tcw_t[2] * -1.0f};
  float twc[3], tlc[3];
  so3_act(qi, mt, twc);
  so3_act(P.Tlw_q, twc, tlc);
  for (int k = 0; k < 3; k++) tlc[k] += P.Tlw_t[k];
  const bool bForward = tlc[2] > P.b && !P.mono, bBackward = -tlc[2] > P.b && !P.mono;
  SBP_T(1)
  // ---- A. candidates of every map point (parallel)
  for (int l = tid; l < NL; l += kSbpThreads) {
    s_hasobs[l] = V.last_has_obs[l];
    const Proj R = sbp_project(P, V, l, bForward, bBackward);
    int n = 0;
    bool any = false;
    if (R.ok)
      any = sbp_candidates(P, V, Cur, R, l, s_start, s_items, [&](int i2, int dist) {
        if (n < kCand) cnd[(size_t)l * kCand + n] = (unsigned)i2 | ((unsigned)dist << 16);
        n++;
      });
    ccnt[l] = any ? n : -1;  // -1: vIndices2.empty() -> continue
  }
  __syncthreads();
  __syncthreads();
  SBP_T(2)
  // ---- B. assignment.  The reference walks the map points in index order; each takes its nearest candidate (first minimum in
  //         visiting order) among the key-points that do not hold a map point with observations yet (:1914-1915), i.e. that no
  //         EARLIER map point with Observations() > 0 has taken.  That is a serial dictatorship, and with one common priority order
  //         (the index) its outcome is the fixed point of deferred acceptance: every map point proposes to its best key-point
  //         that is not held by a lower-index blocker, every key-point keeps the lowest-index blocking proposer, the displaced
  //         ones propose again.  A key-point's holder index only ever decreases, so a map point's options only shrink and a
  //         handful of fully parallel rounds (the longest displacement chain) replace the walk over ~1000 map points on one wave.
  //         s_block[i2] = lowest index of a proposer with Observations() > 0 (a map point without observations takes a
  //         key-point without blocking it: later ones overwrite it, and every take counts -- :1929-1933).
  int* s_block = reinterpret_cast<int*>(s_pool);  // [kSbpMaxCur] (the cell counters are no longer needed)
  static_assert(2 * kChunk * kCand >= kSbpMaxCur, "the pool must hold the blocker table");
  for (int i = tid; i < N; i += kSbpThreads) {
    s_block[i] = 0x7fffffff;
    s_hold[i] = -1;
  }
  // best available candidate of map point l (everything the sequential code decides for it, given who blocks what): -1 = none
  auto decide = [&](int l) {
    const int n = ccnt[l];
    if (n < 0) return -1;
    unsigned key = 0xffffffffu, key2 = 0xffffffffu;  // dist << 16 | visiting order: the first minimum wins; the second best (mode 1)
    int idx = -1, idx2 = -1;
    auto offer = [&](int i2, int dist, int order) {
      if (s_block[i2] < l) return;  // mvpMapPoints[i2] && Observations() > 0 -> skip (:1914-1915)
      const unsigned kk = ((unsigned)dist << 16) | (unsigned)min(order, 0xffff);
      if (kk < key) {
        key2 = key;
        idx2 = idx;
        key = kk;
        idx = i2;
      } else if (kk < key2) {
        key2 = kk;
        idx2 = i2;
      }
    };
    if (n <= kCand) {
      for (int j = 0; j < n; j += 4) {  // (a row of the list is 256 bytes: four entries a load)
        const uint4 e4 = *reinterpret_cast<const uint4*>(cnd + (size_t)l * kCand + j);
        const unsigned e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int u = 0; u < 4; u++)
          if (j + u < n) offer((int)(e[u] & 0xffffu), (int)(e[u] >> 16), j + u);
      }
    } else {  // more candidates than the list holds: enumerate them again (rare)
      const Proj R = sbp_project(P, V, l, bForward, bBackward);
      int order = 0;
      sbp_candidates(P, V, Cur, R, l, s_start, s_items, [&](int i2, int dist) { offer(i2, dist, order++); });
    }
    const int bestDist = idx < 0 ? 256 : (int)(key >> 16);
    if (bestDist > kThHigh) return -1;
    if (P.mode == 1) {  // best / second-best ratio test when both sit on one pyramid level (:96-113)
      const int bestDist2 = idx2 < 0 ? 256 : (int)(key2 >> 16);
      const int bestLevel = s_oct[idx], bestLevel2 = idx2 < 0 ? -1 : (int)s_oct[idx2];
      if (bestLevel == bestLevel2 && (float)bestDist > P.nn_ratio * (float)bestDist2) return -1;
    }
    return idx;
  };
  __syncthreads();
  if (P.mode == 1) {
    // The ratio test makes a map point's choice depend on its SECOND best too, so a proposal can be withdrawn when a lower-index
    // blocker takes the second best away (or hands it back): the blocker table is not monotone and must not remember withdrawn
    // proposals.  Jacobi rounds: every map point decides from the blocker table of the previous round (read-only in this phase),
    // then the table is rebuilt from the current proposals.  sel[l] depends only on the proposals of map points below l, so after
    // round t the first t map points hold the sequential walk's choice for good: the fixed point is the reference's result, reached
    // in (longest dependency chain) rounds, and no thread reads the table while another writes it.
    for (int round = 0;; round++) {
      if (tid == 0) s_ctl[0] = 0;
      __syncthreads();
      bool changed = false;
      for (int l = tid; l < NL; l += kSbpThreads) {
        const int cur = round == 0 ? -3 : sel[l];
        const int now = decide(l);
        if (now != cur) {
          sel[l] = now;
          changed = true;
        }
      }
      if (changed) s_ctl[0] = 1;
      __syncthreads();
      const bool again = s_ctl[0] != 0;
      if (!again) break;  // (uniform: every thread read the same flag after the barrier)
      for (int i = tid; i < N; i += kSbpThreads) s_block[i] = 0x7fffffff;
      __syncthreads();
      for (int l = tid; l < NL; l += kSbpThreads) {
        const int now = sel[l];
        if (now >= 0 && s_hasobs[l]) atomicMin(&s_block[now], l);
      }
      __syncthreads();
    }
  } else {
    for (int round = 0;; round++) {
      if (tid == 0) s_ctl[0] = 0;
      __syncthreads();
      bool changed = false;
      for (int l = tid; l < NL; l += kSbpThreads) {
        const int cur = round == 0 ? -3 : sel[l];
        // a proposal stands until a lower-index blocker takes its key-point, "nothing" stands for good (options only shrink: a
        // key-point's blocker index only ever decreases, so the unique fixed point does not depend on the order of the updates)
        if (round > 0 && (cur < 0 || s_block[cur] >= l)) continue;
        const int now = decide(l);
        if (now != cur) {
          sel[l] = now;
          changed = true;
        }
        if (now >= 0 && s_hasobs[l] && atomicMin(&s_block[now], l) > l) changed = true;
      }
      if (changed) s_ctl[0] = 1;
      __syncthreads();
      const bool again = s_ctl[0] != 0;
      __syncthreads();
      if (!again) break;
    }
  }
  SBP_T(3)
  // takes: every map point with a proposal (an overwritten take counts like the reference counts it); the key-point ends up with the
  // LAST taker in index order = its blocker if it has one (nobody above a blocker can take it), else the highest-index taker
  int nm = 0;
  for (int l = tid; l < NL; l += kSbpThreads) {
    const int i2 = sel[l];
    if (i2 < 0) continue;
    nm++;
    atomicMax(&s_hold[i2], l);
    if (P.mode == 1) sel[l] = -1;  // (the rotation histogram below belongs to the frame-to-frame overload)
  }
  {
    for (int ofs = 32; ofs > 0; ofs >>= 1) nm += __shfl_down(nm, ofs, 64);
    if (tid == 0) s_ctl[0] = 0;
    __syncthreads();
    if (lane == 0 && nm) atomicAdd(&s_ctl[0], nm);
    __syncthreads();
  }
  for (int i = tid; i < N; i += kSbpThreads)
    if (s_hold[i] >= 0) s_state[i] = (short)s_hold[i];
  __syncthreads();
  if (P.mode == 0) {  // rotHist[bin].push_back(bestIdx2) of every assignment (:1935-1944), all map points at once
    for (int l = tid; l < NL; l += kSbpThreads) {
      const int best = sel[l];
      if (best < 0) continue;
      int bin = -1;
      if (P.check_orientation) {
        float rot = V.last_angle[l] - V.cur_kp[best].angle;
        if (rot < 0.0) rot += 360.0f;
        bin = (int)roundf(rot * (1.0f / kHisto));
        if (bin == kHisto) bin = 0;
        atomicAdd(&s_hist[bin], 1);
      }
      sel[l] = best | (bin << 16);
    }
  }
  __syncthreads();
  // ---- C. rotation consistency
  if (P.mode == 0 && P.check_orientation) {
    if (tid == 0) {  // ComputeThreeMaxima
      int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
      for (int i = 0; i < kHisto; i++) {
        const int s = s_hist[i];
        if (s > max1) {
          max3 = max2;
          max2 = max1;
          max1 = s;
          ind3 = ind2;
          ind2 = ind1;
          ind1 = i;
        } else if (s > max2) {
          max3 = max2;
          max2 = s;
          ind3 = ind2;
          ind2 = i;
        } else if (s > max3) {
          max3 = s;
          ind3 = i;
        }
      }
      if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
      } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
      }
      int nm = s_ctl[0];
      for (int i = 0; i < kHisto; i++)
        if (i != ind1 && i != ind2 && i != ind3) nm -= s_hist[i];
      s_ctl[0] = nm;
      s_ctl[1] = ind1;
      s_ctl[2] = ind2;
      s_ctl[3] = ind3;
    }
    __syncthreads();
    const int ind1 = s_ctl[1], ind2 = s_ctl[2], ind3 = s_ctl[3];
    for (int l = tid; l < NL; l += kSbpThreads) {
      const int e = sel[l];
      if (e < 0) continue;
      const int bin = e >> 16, i2 = e & 0xffff;
      if (bin != ind1 && bin != ind2 && bin != ind3) s_state[i2] = -2;  // CurrentFrame.mvpMapPoints[i2] = NULL
    }
    __syncthreads();
  }
  SBP_T(4)
#ifdef GFS_SBP_TIMING
  __syncthreads();
  if (tid == 0 && f == 0) printf("SBPT grid=%lld A=%lld B=%lld C=%lld N=%d NL=%d\n", sbp_t[1] - sbp_t[0], sbp_t[2] - sbp_t[1], sbp_t[3] - sbp_t[2], sbp_t[4] - sbp_t[3], N, NL);
#endif
  for (int i = tid; i < N; i += kSbpThreads) cur_match[(size_t)f * SC + i] = s_state[i];
  if (tid == 0) nmatches[f] = s_ctl[0];
}

}  // namespace

void gfs::sbp_stage_cur(gfs_sbp* h, const SbpBlocks& Y, int f, int n_cur, const gfs_keypoint* kps, const float* u_right, const uint8_t* desc,
                        const uint8_t* has_mp_obs) {
  uint8_t* b = h->in.h.p;
  const size_t at = (size_t)f * Y.SC, n = (size_t)n_cur;
  Y.kp.put(b, at, kps, n);
  Y.ur.put(b, at, u_right, n);
  Y.cdesc.put(b, at, desc, n);
  Y.cobs.put(b, at, has_mp_obs, n);
}

int gfs::sbp_launch(gfs_sbp* h, int B, const SbpBlocks& Y, int* cur_match, int* nmatches) {
  const uint8_t* d = h->in.d.p;
  GFS_LAUNCH("k_sbp", k_sbp, dim3(B), dim3(kSbpThreads), 0, h->stream, Y.pairs.at(d), Y.xw.at(d), Y.desc.at(d), Y.oct.at(d), Y.ang.at(d),
             Y.lobs.at(d), Y.kp.at(d), Y.ur.at(d), Y.cdesc.at(d), Y.cobs.at(d), Y.SL, Y.SC, h->d_cand.p, h->d_cand_cnt.p, h->d_lsel.p,
             cur_match, nmatches);
  return GFS_OK;
}

namespace {

// the last frame's (or the map's) per-point arrays of frame f into the pinned input block
void stage_last(gfs_sbp* h, const SbpBlocks& Y, int f, int n_last, const float* xw, const uint8_t* desc, const int32_t* octave,
                const float* angle, const uint8_t* has_obs) {
  uint8_t* b = h->in.h.p;
  const size_t at = (size_t)f * Y.SL, n = (size_t)n_last;
  Y.xw.put(b, at, xw, n);
  Y.desc.put(b, at, desc, n);
  Y.oct.put(b, at, octave, n);
  Y.ang.put(b, at, angle, n);
  Y.lobs.put(b, at, has_obs, n);
}

// uploads the staged batch, runs k_sbp, downloads cur_match / nmatches and hands them to the caller
template <class Problem>
int sbp_run(gfs_sbp* h, const Problem* problems, int B, const SbpBlocks& Y, int32_t* const* cur_match, int32_t* nmatches) {
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, Y.in.bytes())) return rc;
  if (int rc = sbp_launch(h, B, Y, Y.match.at(h->res.d.p), Y.nm.at(h->res.d.p))) return rc;
  if (int rc = h->res.download(s, 0, Y.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* r = h->res.h.p;
  for (int f = 0; f < B; f++) {
    Y.match.get(cur_match[f], r, (size_t)f * Y.SC, (size_t)problems[f].n_cur);
    nmatches[f] = Y.nm.at(r)[f];
  }
  return GFS_OK;
}

}  // namespace

extern "C" {

int gfs_sbp_create(int device, int max_last, int max_cur, int max_batch, gfs_sbp** out) {
  GFS_REQUIRE(out && max_last > 0 && max_cur > 0 && max_batch > 0, GFS_ERR_INVALID_ARG, "gfs_sbp_create: invalid argument");
  GFS_REQUIRE(max_cur <= kSbpMaxCur && max_last <= kSbpMaxLast, GFS_ERR_UNSUPPORTED,
              "gfs_sbp_create: at most %d current key-points and %d map points per frame", kSbpMaxCur, kSbpMaxLast);
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_sbp> h(new gfs_sbp);
  h->device = device;
  h->max_last = max_last;
  h->max_cur = max_cur;
  h->max_batch = max_batch;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const int SLmax = (int)gfs::align_up((size_t)max_last, 64), SCmax = (int)gfs::align_up((size_t)max_cur, 64);
  const size_t L = (size_t)SLmax * max_batch, B = max_batch;
  const SbpBlocks Y{B, SLmax, SCmax};
  int rc = 0;
  if (!rc) rc = h->in.alloc(Y.in.bytes());
  if (!rc) rc = h->res.alloc(Y.res.bytes());
  if (!rc) rc = h->d_cand.alloc(L * kCand);
  if (!rc) rc = h->d_cand_cnt.alloc(L);
  if (!rc) rc = h->d_lsel.alloc(L);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_sbp_destroy(gfs_sbp* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_search_by_projection(gfs_sbp* h, const gfs_sbp_problem* problems, int B, int32_t* const* cur_match, int32_t* nmatches) {
  GFS_REQUIRE(h && problems && cur_match && nmatches && B > 0, GFS_ERR_INVALID_ARG, "gfs_search_by_projection: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_search_by_projection: batch %d exceeds capacity %d", B, h->max_batch);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const int capL = h->max_last, capC = h->max_cur;
  const SbpBlocks Y{(size_t)B, sbp_stride(B, capL, [&](int f) { return problems[f].n_last; }),
                    sbp_stride(B, capC, [&](int f) { return problems[f].n_cur; })};
  for (int f = 0; f < B; f++) {
    const gfs_sbp_problem& p = problems[f];
    GFS_REQUIRE(p.n_last >= 0 && p.n_last <= capL && p.n_cur >= 0 && p.n_cur <= capC, GFS_ERR_CAPACITY,
                "gfs_search_by_projection: pair %d has %d map points / %d key-points (capacity %d / %d)", f, p.n_last, p.n_cur, capL, capC);
    GFS_REQUIRE(p.n_levels > 0 && p.n_levels <= 16 && p.scale_factors, GFS_ERR_INVALID_ARG,
                "gfs_search_by_projection: pair %d needs 1..16 scale factors", f);
    GFS_REQUIRE(p.n_cur == 0 || cur_match[f], GFS_ERR_INVALID_ARG, "gfs_search_by_projection: cur_match[%d] is NULL", f);
    GFS_REQUIRE(p.n_last == 0 || (p.last_xw && p.last_desc && p.last_octave && p.last_angle && p.last_mp_has_obs), GFS_ERR_INVALID_ARG,
                "gfs_search_by_projection: pair %d has NULL last-frame arrays", f);
    GFS_REQUIRE(p.n_cur == 0 || (p.cur_kps_un && p.cur_u_right && p.cur_desc && p.cur_has_mp_obs), GFS_ERR_INVALID_ARG,
                "gfs_search_by_projection: pair %d has NULL current-frame arrays", f);
    for (int l = 0; l < p.n_last; l++)
      GFS_REQUIRE(p.last_octave[l] >= 0 && p.last_octave[l] < p.n_levels, GFS_ERR_INVALID_ARG,
                  "gfs_search_by_projection: pair %d map point %d has octave %d outside [0, %d)", f, l, p.last_octave[l], p.n_levels);
    SbpPair& S = Y.pairs.at(h->in.h.p)[f];
    S.n_last = p.n_last;
    S.n_cur = p.n_cur;
    S.n_levels = p.n_levels;
    S.mono = p.mono;
    S.check_orientation = p.check_orientation;
    S.mode = 0;
    S.nn_ratio = 0.f;
    for (int k = 0; k < 4; k++) {
      S.Tcw_q[k] = p.Tcw_q[k];
      S.Tlw_q[k] = p.Tlw_q[k];
    }
    for (int k = 0; k < 3; k++) {
      S.Tcw_t[k] = p.Tcw_t[k];
      S.Tlw_t[k] = p.Tlw_t[k];
    }
    S.fx = p.fx;
    S.fy = p.fy;
    S.cx = p.cx;
    S.cy = p.cy;
    S.bf = p.bf;
    S.b = p.b;
    S.min_x = p.min_x;
    S.max_x = p.max_x;
    S.min_y = p.min_y;
    S.max_y = p.max_y;
    S.grid_w_inv = p.grid_w_inv;
    S.grid_h_inv = p.grid_h_inv;
    S.th = p.th;
    for (int k = 0; k < 16; k++) S.scale[k] = k < p.n_levels ? p.scale_factors[k] : 0.f;
    stage_last(h, Y, f, p.n_last, p.last_xw, p.last_desc, p.last_octave, p.last_angle, p.last_mp_has_obs);
    sbp_stage_cur(h, Y, f, p.n_cur, p.cur_kps_un, p.cur_u_right, p.cur_desc, p.cur_has_mp_obs);
  }
  return sbp_run(h, problems, B, Y, cur_match, nmatches);
}

int gfs_search_by_projection_map(gfs_sbp* h, const gfs_sbp_map_problem* problems, int B, int32_t* const* cur_match, int32_t* nmatches) {
  GFS_REQUIRE(h && problems && cur_match && nmatches && B > 0, GFS_ERR_INVALID_ARG, "gfs_search_by_projection_map: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_search_by_projection_map: batch %d exceeds capacity %d", B, h->max_batch);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const int capL = h->max_last, capC = h->max_cur;
  const SbpBlocks Y{(size_t)B, sbp_stride(B, capL, [&](int f) { return problems[f].n_mp; }),
                    sbp_stride(B, capC, [&](int f) { return problems[f].n_cur; })};
  for (int f = 0; f < B; f++) {
    const gfs_sbp_map_problem& p = problems[f];
    GFS_REQUIRE(p.n_mp >= 0 && p.n_mp <= capL && p.n_cur >= 0 && p.n_cur <= capC, GFS_ERR_CAPACITY,
                "gfs_search_by_projection_map: frame %d has %d map points / %d key-points (capacity %d / %d)", f, p.n_mp, p.n_cur, capL, capC);
    GFS_REQUIRE(p.n_levels > 0 && p.n_levels <= 16 && p.scale_factors, GFS_ERR_INVALID_ARG,
                "gfs_search_by_projection_map: frame %d needs 1..16 scale factors", f);
    GFS_REQUIRE(p.n_cur == 0 || cur_match[f], GFS_ERR_INVALID_ARG, "gfs_search_by_projection_map: cur_match[%d] is NULL", f);
    GFS_REQUIRE(p.n_mp == 0 || (p.mp_proj && p.mp_desc && p.mp_level && p.mp_view_cos && p.mp_has_obs), GFS_ERR_INVALID_ARG,
                "gfs_search_by_projection_map: frame %d has NULL map-point arrays", f);
    GFS_REQUIRE(p.n_cur == 0 || (p.cur_kps_un && p.cur_u_right && p.cur_desc && p.cur_has_mp_obs), GFS_ERR_INVALID_ARG,
                "gfs_search_by_projection_map: frame %d has NULL key-point arrays", f);
    for (int l = 0; l < p.n_mp; l++)
      GFS_REQUIRE(p.mp_level[l] >= 0 && p.mp_level[l] < p.n_levels, GFS_ERR_INVALID_ARG,
                  "gfs_search_by_projection_map: frame %d map point %d has level %d outside [0, %d)", f, l, p.mp_level[l], p.n_levels);
    sbp_map_pair(Y.pairs.at(h->in.h.p)[f], p, p.n_mp);
    stage_last(h, Y, f, p.n_mp, p.mp_proj, p.mp_desc, p.mp_level, p.mp_view_cos, p.mp_has_obs);
    sbp_stage_cur(h, Y, f, p.n_cur, p.cur_kps_un, p.cur_u_right, p.cur_desc, p.cur_has_mp_obs);
  }
  return sbp_run(h, problems, B, Y, cur_match, nmatches);
}

}  // extern "C"
