// Optimizer::PoseLidarVisualInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:6285-6760, 7173-7678) on
// MI355X: the pose step that ends Tracking::TrackLocalMap for IMU_RGBD with point-cloud observations, for a batch of problems with the
// two modes mixed freely (include/gfs_abi.h section 21).
//
// k_pose_inertial runs a whole problem in one launch.  That cannot stay: a round's association needs the whole device and depends on
// the previous round's pose.  A call queues, on the handle's stream, k_pli_init, then per round k_pli_assoc (one lane per cloud point
// over all problems: GenerateLidarEdge's body, lidar_assoc.hpp) and k_pli_round (one 256-thread workgroup per problem: the stable
// compaction of the surviving points in cloud-index order, the top-of-round scan, ten Gauss-Newton iterations, the re-classification,
// the next initPose), then k_pli_final (the recovery pass and the Hessian of the new prior); the problem's state (LState: the rule's
// Persist and what the rounds hand on) and the visual edges' state live in device memory between the launches, and the host waits
// once.  A problem that took the `edges < 10` break sets a flag: its later association and round launches return at once.
//
// The rule is pose_lidar_inertial_rule.hpp's and, through it, pose_inertial_rule.hpp's; every output has the bytes of the sequential
// restatement (tests/host/pose_lidar_inertial_restatement.cpp).  Inside a round the work is k_pose_inertial's: visual edges over the
// threads with the first two in registers, sums in edge order through an LDS slab (pose_lm_dev.hpp's ordered_sum), the small edges a
// lane each, the pivoted LDL' in LDS.  The lidar edges stay in global memory.  Twelve lanes build the iteration's perturbed poses
// into LDS; each thread computes J and the 27 terms of its lidar edges, and the ordered sums carry on from the entries the visual and
// the small edges left in the system matrix.  Those sums use the slab's rows in front of the work area (which holds the matrix by
// then): 170 edges a pass.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "gfs_common.hpp"
#include "lidar_assoc.hpp"
#include "pose_lidar_inertial_rule.hpp"
#include "pose_lm_dev.hpp"
#include "staging.hpp"
#include "wave_reduce.hpp"

using namespace gfs_pli;
using gfs_pose_lm::ordered_sum;
using gfs_red::block_sum256;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads;             // visual edges per pass of an ordered sum: one per thread
constexpr int kSlabStride = kChunk + 1;      // odd: the summing lanes read different banks
constexpr int kHessRows = 18;                // the 36 entries of a 6 x 6 Hessian block go in two halves
constexpr int kWorkAt = kHessRows * kSlabStride;  // Work lives behind the rows the Hessian sums use
constexpr int kWorkDoubles = (int)((sizeof(Work) + 7) / 8);
constexpr int kLdsDoubles = (kSys * kSlabStride > kWorkAt + kWorkDoubles) ? kSys * kSlabStride : kWorkAt + kWorkDoubles;
constexpr int kLidarChunk = 170;             // lidar edges per pass while Work is live: 27 rows in front of it
constexpr int kLidarStride = kLidarChunk + 1;
constexpr int kScanChunk = 4096;             // chi2 terms per pass of the top-of-round scan (Work is not live there)
static_assert(kSys * kLidarStride <= kWorkAt, "the lidar sums' rows end in front of the work area");
static_assert(kScanChunk <= kLdsDoubles, "the scan's terms fit the slab");
static_assert(kLdsDoubles * 8 + sizeof(Persist) + 13 * 7 * 8 + 256 <= 64 * 1024, "the slab, the work area, the state and the poses fit the static LDS limit");
static_assert(sizeof(Persist) % 8 == 0, "Persist is copied as 8-byte words");

// GenerateLidarEdge's literals (src/Optimizer.cc:8339-8421), the same as pose_lidar.hip hands to the shared association
struct Gates {
  static constexpr double kSqDisGate = 1.0, kPlaneGate = 0.2, kWeightSlope = 0.9, kMinWeight = 0.1;
};

struct LHead {  // one problem without its arrays
  Head h;
  float q[4], t[3], tcb_q[4], tcb_t[3];
  double kf_time_gap;
  int n_cloud, map_nb;
  const float4* map_pts;  // sorted by bucket; w = original index (bits)
  const int* map_start;   // [nb + 1]
};
struct LState {  // what a problem keeps between the launches of a call
  Persist P;
  double M[12];   // initPose of the next association
  double info_l;  // the information of the last entered round's lidar edges
  int robust, done, rounds_run, nBad, nInliers, n_lidar_inliers, last_it, last_nl;
  float avg, residual;
  int round_edges[4], round_valid[4];
  float round_chi2[4];
};
struct LOut {
  gfs_imu_estimate cur, other;
  int n_good, n_inliers, rounds_run;
  float avg;
  int n_lidar_inliers;
  float residual;
  int round_edges[4], round_valid[4];
  float round_chi2[4];
  double H[900];
};
struct VisView {  // the visual edges of the batch: inputs, and the state g2o keeps per edge plus mvbOutlier
  const double *xw, *obs;
  const float* w;
  const uint8_t *stereo, *close;
  double* err;
  uint8_t *level, *outlier;
  int stride;
};
struct LidarView {  // the association's per-point output and the per-round compacted edges
  const float* cloud;
  uint8_t* flag;
  float4* plane;
  float* s;
  int* eidx;       // [B][4][SC]
  float4* eplane;
  float* es;
  int stride;
};

// An edge as its thread keeps it
struct EdgeReg {
  double xw[3], obs[3], err[3], w;
  int stereo, close, level, outlier;
};

__device__ __forceinline__ void copy_words(void* dst, const void* src, int words, int tid) {
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
  const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
  for (int i = tid; i < words; i += kThreads) d[i] = s[i];
}

__global__ __launch_bounds__(kThreads) void k_pli_init(const LHead* __restrict__ heads, LState* __restrict__ states, VisView V) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const LHead& LH = heads[f];
  for (int e = tid; e < LH.h.n_obs; e += kThreads) {
    const size_t at = (size_t)f * V.stride + e;
    V.outlier[at] = 0;
    V.level[at] = 0;
    for (int k = 0; k < 3; k++) V.err[3 * at + k] = 0.0;
  }
  if (tid) return;
  LState& ST = states[f];
  persist_init(LH.h, ST.P);
  first_init_pose(LH.h.mode, LH.q, LH.t, ST.M);
  ST.info_l = kLidarInfo;
  ST.robust = 1;
  ST.done = ST.rounds_run = ST.nBad = ST.nInliers = ST.n_lidar_inliers = ST.last_nl = 0;
  ST.last_it = 0;
  ST.avg = ST.residual = 0.0f;
  for (int k = 0; k < 4; k++) {
    ST.round_edges[k] = ST.round_valid[k] = 0;
    ST.round_chi2[k] = 0.0f;
  }
}

__global__ __launch_bounds__(kThreads) void k_pli_assoc(const LHead* __restrict__ heads, const LState* __restrict__ states, LidarView Lv, int it) {
  const int f = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const LHead& LH = heads[f];
  const LState& ST = states[f];
  if (i >= LH.n_cloud || it >= LH.h.n_rounds || ST.done || LH.n_cloud < kMinCloud) return;
  const size_t at = (size_t)f * Lv.stride + i;
  Lv.flag[at] = 0;
  float d[5];
  int ind[5], slot[5];
  float4 pl;
  float s;
  if (!gfs_lidar::lidar_point_edge<Gates>(ST.M, Lv.cloud + 3 * at, LH.map_pts, LH.map_start, LH.map_nb, d, ind, slot, &pl, &s)) return;
  Lv.flag[at] = 1;
  Lv.plane[at] = pl;
  Lv.s[at] = s;
}

// What both k_pli_round and k_pli_final do with a problem's visual edges and small edges
struct Problem {
  const Head& h;
  const double *xw, *obs;
  const float* w;
  const uint8_t *stereo, *close;
  double* err;
  uint8_t *level, *outlier;
  __device__ Problem(const Head& h_, const VisView& V, int f)
      : h(h_), xw(V.xw + (size_t)f * V.stride * 3), obs(V.obs + (size_t)f * V.stride * 3), w(V.w + (size_t)f * V.stride),
        stereo(V.stereo + (size_t)f * V.stride), close(V.close + (size_t)f * V.stride), err(V.err + (size_t)f * V.stride * 3),
        level(V.level + (size_t)f * V.stride), outlier(V.outlier + (size_t)f * V.stride) {}
  __device__ EdgeReg load(int e) const {
    EdgeReg R;
    for (int k = 0; k < 3; k++) {
      R.xw[k] = xw[3 * e + k];
      R.obs[k] = obs[3 * e + k];
      R.err[k] = err[3 * e + k];
    }
    R.w = (double)w[e];
    R.stereo = stereo[e];
    R.close = close[e];
    R.level = level[e];
    R.outlier = outlier[e];
    return R;
  }
  __device__ void store(int e, const EdgeReg& R) const {
    for (int k = 0; k < 3; k++) err[3 * e + k] = R.err[k];
    level[e] = (uint8_t)R.level;
    outlier[e] = (uint8_t)R.outlier;
  }
};

// computeError + linearizeOplus of the small edges, a lane each in three waves; then the entries of their J' Omega over the threads
__device__ __forceinline__ void small_edges(const Head& h, Persist& P, Work& W, bool build, int tid) {
  if (tid == 0) small_edge_linearize(h, P, W, 0, build);
  if (tid == 64) {
    small_edge_linearize(h, P, W, 1, build);
    small_edge_linearize(h, P, W, 2, build);
  }
  if (tid == 128) small_edge_linearize(h, P, W, 3, build);
  __syncthreads();
  for (int idx = tid; idx < kAtOEntries; idx += kThreads) small_edge_AtO_entry(h.mode, W, idx);
  __syncthreads();
}

struct LidarEdges {  // the compacted edges of one round of one problem
  const float* cloud;
  const int* idx;
  const float4* plane;
  const float* s;
  __device__ void get(int l, float* p, float* pl, float* sc) const {
    const int i = idx[l];
    p[0] = cloud[3 * i], p[1] = cloud[3 * i + 1], p[2] = cloud[3 * i + 2];
    const float4 q = plane[l];
    pl[0] = q.x, pl[1] = q.y, pl[2] = q.z, pl[3] = q.w;
    *sc = s[l];
  }
};

__global__ __launch_bounds__(kThreads) void k_pli_round(const LHead* __restrict__ heads, LState* __restrict__ states, VisView V, LidarView Lv,
                                                       int it) {
  __shared__ double s_mem[kLdsDoubles];
  __shared__ Persist s_P;
  __shared__ double s_Wp[kPerturbed + 1][7];  // the twelve perturbed poses and the estimate itself, inverted
  __shared__ double s4[4];
  __shared__ int s_wcnt[4];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LHead& LH = heads[f];
  const Head& h = LH.h;
  LState& ST = states[f];
  if (it >= h.n_rounds || ST.done) return;  // uniform
  const int n = h.n_obs, mode = h.mode;
  const Calib& cam = h.cam;
  double* s_slab = s_mem;
  Work& W = *reinterpret_cast<Work*>(s_mem + kWorkAt);
  const Problem Pr(h, V, f);
  copy_words(&s_P, &ST.P, (int)(sizeof(Persist) / 8), tid);

  const int last = n > 0 ? n - 1 : 0;  // (a thread without an edge loads a valid one and never uses it; n == 0 loads nothing)
  EdgeReg R0, R1;
  if (n > 0) {
    R0 = Pr.load(min(tid, last));
    R1 = Pr.load(min(tid + kThreads, last));
  }
  auto with_edge = [&](int e, auto&& body) {  // e = tid + 256 k: k is the same in every thread of a pass
    const int k = (e - tid) / kThreads;
    if (k == 0) {
      body(R0);
    } else if (k == 1) {
      body(R1);
    } else {
      EdgeReg R = Pr.load(e);
      body(R);
      Pr.store(e, R);
    }
  };

  // ---- compaction of the surviving points in cloud-index order (GenerateLidarEdge's vector, nullptr entries skipped)
  const size_t cbase = (size_t)f * Lv.stride, rbase = ((size_t)f * 4 + it) * Lv.stride;
  int* eidx = Lv.eidx + rbase;
  float4* eplane = Lv.eplane + rbase;
  float* es = Lv.es + rbase;
  int nl = 0;
  if (LH.n_cloud >= kMinCloud)
    for (int base = 0; base < LH.n_cloud; base += kThreads) {
      const int i = base + tid;
      const bool keep = i < LH.n_cloud && Lv.flag[cbase + i];
      const unsigned long long m = __ballot(keep);
      const int below = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_wcnt[wave] = __popcll(m);
      __syncthreads();
      int off = nl;
      for (int w = 0; w < wave; w++) off += s_wcnt[w];
      if (keep) {
        const int pos = off + below;
        eidx[pos] = i;
        eplane[pos] = Lv.plane[cbase + i];
        es[pos] = Lv.s[cbase + i];
      }
      nl += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
      __syncthreads();
    }
  __syncthreads();  // the edges are read back by other threads below; s_P is complete
  const LidarEdges Le{Lv.cloud + 3 * cbase, eidx, eplane, es};
  const double info_l = lidar_information(mode, LH.kf_time_gap);

  // ---- the top of the round: chi2IMU, then chi2Lidar (a float, edge after edge) and valid_edge at the current estimate
  if (tid == 0) {
    inertial_before_round(s_P);
    s_P.ok = 1;
  }
  if (tid == 64) lidar_inverse_pose(s_P.s[0].Rcw, s_P.s[0].tcw, s_Wp[kPerturbed]);
  __syncthreads();
  float chiL = 0.0f;  // thread 0
  int n_valid = 0;
  {
    int valid = 0;
    for (int base = 0; base < nl; base += kScanChunk) {
      const int cnt = min(kScanChunk, nl - base);
      for (int l = base + tid; l < base + cnt; l += kThreads) {
        float p[3], pl[4], sc;
        Le.get(l, p, pl, &sc);
        const double c = lidar_chi2(lidar_error(s_Wp[kPerturbed], p, pl, sc), info_l);
        valid += c < kLidarValidChi2 ? 1 : 0;
        s_slab[l - base] = c;
      }
      __syncthreads();
      if (tid == 0) chiL = ordered_sum(s_slab, cnt, chiL);
      __syncthreads();
    }
    n_valid = (int)block_sum256((double)valid, s4);
    if (tid == 0 && nl > 0) chiL /= (float)nl;
  }
  const bool robust = ST.robust != 0;
  const int D = mode == kFrame ? 30 : 15;
  // the packed entry of the pose block, or the entry of b, that thread tid < 27 sums
  int sys_at = 0;
  if (tid < 21) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= tid) a++;
    sys_at = kLd * a + (tid - a * (a + 1) / 2);
  }

  for (int iteration = 0; iteration < kIterations; iteration++) {
    if (!s_P.ok) break;  // uniform: written before the last barrier of the previous iteration
    // ---- computeActiveErrors + buildSystem over the visual edges: 27 ordered sums
    {
      double Rcw[9], tcw[3];
      for (int k = 0; k < 9; k++) Rcw[k] = s_P.s[0].Rcw[k];
      for (int k = 0; k < 3; k++) tcw[k] = s_P.s[0].tcw[k];
      double run = 0;  // threads 0 .. 26: quantity tid
      for (int base = 0; base < n; base += kChunk) {
        const int e = base + tid;
        double acc[kSys];
#pragma unroll
        for (int k = 0; k < kSys; k++) acc[k] = 0;
        if (e < n) with_edge(e, [&](EdgeReg& R) {
          if (R.level) return;
          const bool st = R.stereo != 0;
          vis_error(cam, Rcw, tcw, R.xw, R.obs, st, R.err);
          double J[18], rho0, rho1 = 1.0;
          vis_jacobian(cam, Rcw, tcw, R.xw, st, J);
          if (robust) gfs_pi::huber(vis_chi2(R.err, R.w, st), huber_delta_visual(st), &rho0, &rho1);
          vis_quadratic_form(J, R.w, st, rho1, R.err, acc);
        });
#pragma unroll
        for (int k = 0; k < kSys; k++) s_slab[k * kSlabStride + tid] = acc[k];
        __syncthreads();
        if (tid < kSys) run = ordered_sum(s_slab + tid * kSlabStride, min(kChunk, n - base), run);
        __syncthreads();
      }
      if (tid < kSys) s_P.vis[tid] = run;
      __syncthreads();
    }
    // ---- the small edges, the system matrix and its right-hand side; the poses of the lidar edges' numeric Jacobian
    small_edges(h, s_P, W, true, tid);
    for (int idx = tid; idx < D * D; idx += kThreads) {
      const int R = idx / D, C = idx % D;
      if (C <= R) W.A[kLd * R + C] = system_entry(mode, s_P, W, R, C);
    }
    if (tid < D) W.b[tid] = system_rhs(mode, s_P, W, tid);
    if (tid == 0) W.sign = 0;
    if (nl > 0) {
      if (tid >= 64 && tid < 64 + kPerturbed) perturbed_inverse_pose(s_P.s[0], cam, tid - 64, s_Wp[tid - 64]);
      if (tid == 128) lidar_inverse_pose(s_P.s[0].Rcw, s_P.s[0].tcw, s_Wp[kPerturbed]);
    }
    __syncthreads();
    // ---- the lidar edges onto the pose block and b: the ordered sums carry on from what the other edges left there
    if (nl > 0) {
      double run = tid < 21 ? W.A[sys_at] : tid < kSys ? W.b[tid - 21] : 0.0;
      for (int base = 0; base < nl; base += kLidarChunk) {
        const int l = base + tid;
        if (tid < kLidarChunk) {
          double acc[kSys];
#pragma unroll
          for (int k = 0; k < kSys; k++) acc[k] = 0;
          if (l < nl) {
            float p[3], pl[4], sc;
            Le.get(l, p, pl, &sc);
            double J[6];
            lidar_jacobian(&s_Wp[0][0], p, pl, sc, J);
            lidar_quadratic_form(J, info_l, lidar_error(s_Wp[kPerturbed], p, pl, sc), acc);
          }
#pragma unroll
          for (int k = 0; k < kSys; k++) s_slab[k * kLidarStride + tid] = acc[k];
        }
        __syncthreads();
        if (tid < kSys) run = ordered_sum(s_slab + tid * kLidarStride, min(kLidarChunk, nl - base), run);
        __syncthreads();
      }
      if (tid < 21) W.A[sys_at] = run;
      else if (tid < kSys) W.b[tid - 21] = run;
      __syncthreads();
    }
    // ---- the dense solve
    for (int k = 0; k < D; k++) {
      if (tid == 0) ldlt_pivot(W.A, D, k, W.tr, W.temp);
      __syncthreads();
      if (tid >= k && tid < D) ldlt_row(W.A, k, tid, W.temp);
      __syncthreads();
      if (tid > k && tid < D) ldlt_scale(W.A, k, tid);
      if (tid == 0) ldlt_sign(W.A, k, &W.sign);
      __syncthreads();
    }
    if (tid == 0) {
      if (W.sign == 1) ldlt_substitute(W.A, D, W.tr, W.b, W.y, s_P.x);
      else s_P.ok = 0;  // x keeps what it held; the update below applies it and the round ends
    }
    __syncthreads();
    // ---- update: the vertices' oplus, disjoint state, a lane each in four waves
    if ((tid & 63) == 0) update_part(h, s_P, tid >> 6);
    __syncthreads();
  }
  // ---- nInliersLidar, residual, the next initPose
  if (tid == 0) {
    ST.n_lidar_inliers = n_valid;
    ST.residual = chiL;
    ST.round_edges[it] = nl;
    ST.round_valid[it] = n_valid;
    ST.round_chi2[it] = chiL;
    next_init_pose(s_P.s[0].Rwb, s_P.s[0].twb, LH.tcb_q, LH.tcb_t, ST.M);
  }
  // ---- the re-classification.  Outlier edges are re-evaluated at the current estimate (parallel); the float sum of the inliers'
  //      chi2 is added in the reference's order, the mono list then the stereo list, from terms parked in LDS
  float avg = 0.0f;  // thread 0
  int nBad, nInliers;
  {
    double Rcw[9], tcw[3];
    for (int k = 0; k < 9; k++) Rcw[k] = s_P.s[0].Rcw[k];
    for (int k = 0; k < 3; k++) tcw[k] = s_P.s[0].tcw[k];
    float* s_term = reinterpret_cast<float*>(s_slab);
    int bad_local = 0, good_local = 0;
    for (int pass = 0; pass < 2; pass++)
      for (int base = 0; base < n; base += kChunk) {
        const int e = base + tid;
        float term = 0.0f;
        if (e < n) with_edge(e, [&](EdgeReg& R) {
          const bool st = R.stereo != 0;
          if (st != (pass == 1)) return;
          if (R.outlier) vis_error(cam, Rcw, tcw, R.xw, R.obs, st, R.err);
          const float chi2 = (float)vis_chi2(R.err, R.w, st);
          const bool bad = st ? stereo_is_outlier(chi2, it) : mono_is_outlier(chi2, R.close != 0, vis_depth_positive(Rcw, tcw, R.xw), mode, it);
          R.outlier = R.level = bad ? 1 : 0;
          bad_local += bad ? 1 : 0;
          good_local += bad ? 0 : 1;
          term = bad ? 0.0f : chi2;
        });
        s_term[tid] = term;
        __syncthreads();
        if (tid == 0) avg = ordered_sum(s_term, min(kChunk, n - base), avg);
        __syncthreads();
      }
    nBad = (int)block_sum256((double)bad_local, s4);
    nInliers = (int)block_sum256((double)good_local, s4);
    if (tid == 0) avg /= (float)nInliers;
  }
  // ---- what the next launch of this problem reads
  if (tid < n) Pr.store(tid, R0);
  if (tid + kThreads < n) Pr.store(tid + kThreads, R1);
  __syncthreads();
  copy_words(&ST.P, &s_P, (int)(sizeof(Persist) / 8), tid);
  if (tid == 0) {
    ST.info_l = info_l;
    if (drops_visual_kernel(mode, it, h.n_rounds)) ST.robust = 0;
    ST.rounds_run = it + 1;
    ST.nBad = nBad;
    ST.nInliers = nInliers;
    ST.avg = avg;
    ST.last_it = it;
    ST.last_nl = nl;
    if (edge_count_with_lidar(mode, n, nl) < kMinEdges) ST.done = 1;  // break: before removeEdge
  }
}

__global__ __launch_bounds__(kThreads) void k_pli_final(const LHead* __restrict__ heads, const LState* __restrict__ states, VisView V,
                                                       LidarView Lv, uint8_t* __restrict__ outlier_out, LOut* __restrict__ outs) {
  __shared__ double s_mem[kLdsDoubles];
  __shared__ Persist s_P;
  __shared__ double s_Wp[kPerturbed][7];
  __shared__ double s4[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  const LHead& LH = heads[f];
  const Head& h = LH.h;
  const LState& ST = states[f];
  const int n = h.n_obs, mode = h.mode;
  const Calib& cam = h.cam;
  double* s_slab = s_mem;
  Work& W = *reinterpret_cast<Work*>(s_mem + kWorkAt);
  const Problem Pr(h, V, f);
  copy_words(&s_P, &ST.P, (int)(sizeof(Persist) / 8), tid);
  __syncthreads();
  const int D = mode == kFrame ? 30 : 15;
  int nBad = ST.nBad;
  double Rcw[9], tcw[3];
  for (int k = 0; k < 9; k++) Rcw[k] = s_P.s[0].Rcw[k];
  for (int k = 0; k < 3; k++) tcw[k] = s_P.s[0].tcw[k];
  // ---- recover not too bad points (:6677-6701): the verdicts go to the edges' state, which the Hessian below reads
  if (ST.nInliers < kFewInliers && !h.rec_init) {
    int bad_local = 0;
    for (int e = tid; e < n; e += kThreads) {
      EdgeReg R = Pr.load(e);
      const bool st = R.stereo != 0;
      vis_error(cam, Rcw, tcw, R.xw, R.obs, st, R.err);
      if (vis_chi2(R.err, R.w, st) < (st ? kChi2StereoOut : kChi2MonoOut)) R.outlier = 0;
      else bad_local++;
      Pr.store(e, R);
    }
    nBad = (int)block_sum256((double)bad_local, s4);
  }
  // ---- the Hessian of the new prior: the small edges re-linearised at the final state, then the inliers' 6 x 6 blocks in the
  //      order mono list, stereo list, then the lidar edges of the last entered round.  W.A holds it row-major with stride D
  small_edges(h, s_P, W, false, tid);
  for (int idx = tid; idx < D * D; idx += kThreads) W.A[idx] = hessian_entry(mode, W, idx / D, idx % D);
  if (tid < kPerturbed) perturbed_inverse_pose(s_P.s[0], cam, tid, s_Wp[tid]);
  __syncthreads();
  const int nl = ST.last_nl;
  const size_t cbase = (size_t)f * Lv.stride, rbase = ((size_t)f * 4 + ST.last_it) * Lv.stride;
  const LidarEdges Le{Lv.cloud + 3 * cbase, Lv.eidx + rbase, Lv.eplane + rbase, Lv.es + rbase};
  const double info_l = ST.info_l;
  const int off = hessian_visual_offset(mode);
#pragma unroll  // (`half` picks rows of J: a row index known at compile time keeps J in registers)
  for (int half = 0; half < 2; half++) {
    const int q = kHessRows * half + tid;  // threads 0 .. 17: entry (q / 6, q % 6)
    const int at = D * (off + q / 6) + off + q % 6;
    double run = tid < kHessRows ? W.A[at] : 0.0;
    for (int pass = 0; pass < 2; pass++)
      for (int base = 0; base < n; base += kChunk) {
        const int e = base + tid;
        double term[kHessRows];
#pragma unroll
        for (int k = 0; k < kHessRows; k++) term[k] = 0.0;
        if (e < n) {
          const bool st = Pr.stereo[e] != 0;
          if (st == (pass == 1) && !Pr.outlier[e]) {
            const double xw[3] = {Pr.xw[3 * e], Pr.xw[3 * e + 1], Pr.xw[3 * e + 2]};
            const double w = (double)Pr.w[e];
            double J[18];
            vis_jacobian(cam, Rcw, tcw, xw, st, J);
#pragma unroll
            for (int k = 0; k < kHessRows; k++) term[k] = vis_hessian_entry(J, w, st, half * 3 + k / 6, k % 6);  // rows 0-2, then 3-5
          }
        }
#pragma unroll
        for (int k = 0; k < kHessRows; k++) s_slab[k * kSlabStride + tid] = term[k];
        __syncthreads();
        if (tid < kHessRows) run = ordered_sum(s_slab + tid * kSlabStride, min(kChunk, n - base), run);
        __syncthreads();
      }
    for (int base = 0; base < nl; base += kChunk) {
      const int l = base + tid;
      double term[kHessRows];
#pragma unroll
      for (int k = 0; k < kHessRows; k++) term[k] = 0.0;
      if (l < nl) {
        float p[3], pl[4], sc;
        Le.get(l, p, pl, &sc);
        double J[6];
        lidar_jacobian(&s_Wp[0][0], p, pl, sc, J);
#pragma unroll
        for (int k = 0; k < kHessRows; k++) term[k] = lidar_hessian_entry(J, info_l, half * 3 + k / 6, k % 6);
      }
#pragma unroll
      for (int k = 0; k < kHessRows; k++) s_slab[k * kSlabStride + tid] = term[k];
      __syncthreads();
      if (tid < kHessRows) run = ordered_sum(s_slab + tid * kSlabStride, min(kChunk, nl - base), run);
      __syncthreads();
    }
    if (tid < kHessRows) W.A[at] = run;
    __syncthreads();
  }
  // ---- results
  LOut& O = outs[f];
  for (int idx = tid; idx < 900; idx += kThreads) O.H[idx] = idx < D * D ? W.A[idx] : 0.0;
  for (int e = tid; e < n; e += kThreads) outlier_out[(size_t)f * V.stride + e] = Pr.outlier[e];
  if (tid == 0) {
    for (int end = 0; end < 2; end++) {
      const State& s = s_P.s[end];
      gfs_imu_estimate& o = end == 0 ? O.cur : O.other;
      for (int k = 0; k < 9; k++) o.Rwb[k] = s.Rwb[k];
      for (int k = 0; k < 3; k++) o.twb[k] = s.twb[k], o.v[k] = s.v[k], o.bg[k] = s.bg[k], o.ba[k] = s.ba[k];
    }
    O.n_good = n - nBad;
    O.n_inliers = ST.nInliers;
    O.rounds_run = ST.rounds_run;
    O.avg = ST.avg;
    O.n_lidar_inliers = ST.n_lidar_inliers;
    O.residual = ST.residual;
    for (int k = 0; k < 4; k++) {
      O.round_edges[k] = ST.round_edges[k];
      O.round_valid[k] = ST.round_valid[k];
      O.round_chi2[k] = ST.round_chi2[k];
    }
  }
}

}  // namespace

struct gfs_pose_lidar_inertial {
  int device, max_obs, max_cloud, max_batch;
  hipStream_t stream;
  std::mutex mu;
  // one pinned block mirroring one device block for the inputs, one for the outputs: a call is one copy in, its kernels, one copy out
  struct Layout {  // S: visual edges per problem, SC: cloud points per problem
    gfs::Block<256> in, res;
    gfs::Field<LHead> heads;
    gfs::Field<double, 3> xw, obs;
    gfs::Field<float> w;
    gfs::Field<uint8_t> stereo, close;
    gfs::Field<float, 3> cloud;
    gfs::Field<LOut> out;
    gfs::Field<uint8_t> outlier;
    Layout(size_t B, size_t S, size_t SC)
        : heads(in, B), xw(in, B * S), obs(in, B * S), w(in, B * S), stereo(in, B * S), close(in, B * S), cloud(in, B * SC), out(res, B),
          outlier(res, B * S) {}
  };
  gfs::Mirror in, res;
  gfs::DevBuf<LState> d_state;
  gfs::DevBuf<double> d_err;
  gfs::DevBuf<uint8_t> d_level, d_outl, d_flag;
  gfs::DevBuf<float4> d_plane, d_eplane;
  gfs::DevBuf<float> d_s, d_es;
  gfs::DevBuf<int> d_eidx;
  // the last call's shape, for gfs_pose_lidar_inertial_fetch_edges
  int last_B = 0, last_SC = 0;
  std::vector<int> last_edges;  // [B][4]
};

extern "C" {

int gfs_pose_lidar_inertial_create(int device, int max_obs, int max_cloud, int max_batch, gfs_pose_lidar_inertial** out) {
  GFS_REQUIRE(out && max_obs > 0 && max_cloud > 0 && max_batch > 0, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_inertial_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_pose_lidar_inertial> h(new gfs_pose_lidar_inertial);
  h->device = device;
  h->max_obs = max_obs;
  h->max_cloud = max_cloud;
  h->max_batch = max_batch;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t S = gfs::align_up((size_t)max_obs, 64), SC = gfs::align_up((size_t)max_cloud, 64), B = max_batch;
  const gfs_pose_lidar_inertial::Layout L{B, S, SC};
  int rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->d_state.alloc(B);
  if (!rc) rc = h->d_err.alloc(B * S * 3);
  if (!rc) rc = h->d_level.alloc(B * S);
  if (!rc) rc = h->d_outl.alloc(B * S);
  if (!rc) rc = h->d_flag.alloc(B * SC);
  if (!rc) rc = h->d_plane.alloc(B * SC);
  if (!rc) rc = h->d_s.alloc(B * SC);
  if (!rc) rc = h->d_eidx.alloc(B * 4 * SC);
  if (!rc) rc = h->d_eplane.alloc(B * 4 * SC);
  if (!rc) rc = h->d_es.alloc(B * 4 * SC);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_pose_lidar_inertial_destroy(gfs_pose_lidar_inertial* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_pose_lidar_inertial_optimize(gfs_pose_lidar_inertial* h, const gfs_pose_lidar_inertial_problem* problems, int B,
                                     gfs_pose_lidar_inertial_solution* solutions) {
  GFS_REQUIRE(h && problems && solutions && B > 0, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_inertial_optimize: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_pose_lidar_inertial_optimize: batch %d exceeds capacity %d", B, h->max_batch);
  // every refusal before anything is staged.  (A map's n and device are read here without the map's owner being held to anything: a
  // map that is rebuilt while a call that uses it is being made is the caller's race, as with gfs_pose_lidar_optimize.)
  int S = 64, SC = 64, rounds = 0;  // strides of the per-problem arrays in this call
  for (int f = 0; f < B; f++) {
    const gfs_pose_lidar_inertial_problem& q = problems[f];
    const gfs_pose_inertial_problem& p = q.vi;
    GFS_REQUIRE(p.mode == GFS_POSE_INERTIAL_LAST_KEYFRAME || p.mode == GFS_POSE_INERTIAL_LAST_FRAME, GFS_ERR_INVALID_ARG,
                "gfs_pose_lidar_inertial_optimize: problem %d has mode %d", f, p.mode);
    GFS_REQUIRE(p.n_obs >= 0 && q.n_cloud >= 0, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_inertial_optimize: problem %d has n_obs = %d, n_cloud = %d", f,
                p.n_obs, q.n_cloud);
    GFS_REQUIRE(p.n_rounds >= 1 && p.n_rounds <= kMaxRounds, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_inertial_optimize: problem %d has n_rounds = %d",
                f, p.n_rounds);
    GFS_REQUIRE(p.n_obs <= h->max_obs, GFS_ERR_CAPACITY, "gfs_pose_lidar_inertial_optimize: problem %d has %d observations (capacity %d)", f,
                p.n_obs, h->max_obs);
    GFS_REQUIRE(q.n_cloud <= h->max_cloud, GFS_ERR_CAPACITY, "gfs_pose_lidar_inertial_optimize: problem %d has %d cloud points (capacity %d)", f,
                q.n_cloud, h->max_cloud);
    GFS_REQUIRE(p.n_obs == 0 || (p.xw && p.obs && p.inv_sigma2 && p.stereo && p.close && solutions[f].vi.outlier), GFS_ERR_INVALID_ARG,
                "gfs_pose_lidar_inertial_optimize: problem %d has NULL observation arrays", f);
    GFS_REQUIRE(q.n_cloud == 0 || q.cloud, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_inertial_optimize: problem %d has a NULL cloud", f);
    GFS_REQUIRE(q.n_cloud == 0 || (q.map && q.map->n >= 5), GFS_ERR_INVALID_ARG,
                "gfs_pose_lidar_inertial_optimize: problem %d: a cloud without a map, or a map of fewer than 5 points", f);
    GFS_REQUIRE(q.n_cloud == 0 || q.map->device == h->device, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_inertial_optimize: problem %d: map on another device", f);
    S = std::max(S, (int)gfs::align_up((size_t)p.n_obs, 64));
    SC = std::max(SC, (int)gfs::align_up((size_t)q.n_cloud, 64));
    rounds = std::max(rounds, (int)p.n_rounds);
  }
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_pose_lidar_inertial::Layout L{(size_t)B, (size_t)S, (size_t)SC};
  uint8_t* hi = h->in.h.p;
  for (int f = 0; f < B; f++) {
    const gfs_pose_lidar_inertial_problem& q = problems[f];
    const gfs_pose_inertial_problem& p = q.vi;
    LHead& LH = L.heads.at(hi)[f];
    fill_head(p, LH.h);
    memcpy(LH.q, q.q, sizeof(q.q)), memcpy(LH.t, q.t, sizeof(q.t));
    memcpy(LH.tcb_q, q.tcb_q, sizeof(q.tcb_q)), memcpy(LH.tcb_t, q.tcb_t, sizeof(q.tcb_t));
    LH.kf_time_gap = q.kf_time_gap;
    LH.n_cloud = q.n_cloud;
    LH.map_pts = q.n_cloud ? q.map->d_pts.p : nullptr;  // (a problem without a cloud is never associated)
    LH.map_start = q.n_cloud ? q.map->d_start.p : nullptr;
    LH.map_nb = q.n_cloud ? q.map->nb : 0;
    const size_t at = (size_t)f * S, n = (size_t)p.n_obs;
    L.xw.put(hi, at, p.xw, n);
    L.obs.put(hi, at, p.obs, n);
    L.w.put(hi, at, p.inv_sigma2, n);
    L.stereo.put(hi, at, p.stereo, n);
    L.close.put(hi, at, p.close, n);
    L.cloud.put(hi, (size_t)f * SC, q.cloud, (size_t)q.n_cloud);
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  uint8_t* dr = h->res.d.p;
  const LHead* d_heads = L.heads.at(di);
  const VisView V{L.xw.at(di), L.obs.at(di), L.w.at(di), L.stereo.at(di), L.close.at(di), h->d_err.p, h->d_level.p, h->d_outl.p, S};
  const LidarView Lv{L.cloud.at(di), h->d_flag.p, h->d_plane.p, h->d_s.p, h->d_eidx.p, h->d_eplane.p, h->d_es.p, SC};
  GFS_LAUNCH("k_pli_init", k_pli_init, dim3(B), dim3(kThreads), 0, s, d_heads, h->d_state.p, V);
  for (int it = 0; it < rounds; it++) {
    GFS_LAUNCH("k_pli_assoc", k_pli_assoc, dim3(gfs::div_up(SC, kThreads), B), dim3(kThreads), 0, s, d_heads, h->d_state.p, Lv, it);
    GFS_LAUNCH("k_pli_round", k_pli_round, dim3(B), dim3(kThreads), 0, s, d_heads, h->d_state.p, V, Lv, it);
  }
  GFS_LAUNCH("k_pli_final", k_pli_final, dim3(B), dim3(kThreads), 0, s, d_heads, h->d_state.p, V, Lv, L.outlier.at(dr), L.out.at(dr));
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  h->last_B = B;
  h->last_SC = SC;
  h->last_edges.assign((size_t)B * 4, 0);
  for (int f = 0; f < B; f++) {
    const LOut& O = L.out.at(hr)[f];
    gfs_pose_lidar_inertial_solution& r = solutions[f];
    r.vi.cur = O.cur;
    r.vi.other = O.other;
    r.vi.n_good = O.n_good;
    r.vi.n_inliers = O.n_inliers;
    r.vi.rounds_run = O.rounds_run;
    r.vi.avg_reproj = O.avg;
    memcpy(r.vi.H, O.H, sizeof(r.vi.H));
    L.outlier.get(r.vi.outlier, hr, (size_t)f * S, (size_t)problems[f].vi.n_obs);
    r.n_lidar_inliers = O.n_lidar_inliers;
    r.residual = O.residual;
    for (int k = 0; k < 4; k++) {
      r.round_edges[k] = O.round_edges[k];
      r.round_chi2[k] = O.round_chi2[k];
      r.round_valid[k] = O.round_valid[k];
      h->last_edges[(size_t)f * 4 + k] = O.round_edges[k];
    }
  }
  return GFS_OK;
}

int gfs_pose_lidar_inertial_fetch_edges(gfs_pose_lidar_inertial* h, int b, int round, int32_t* index, float* plane, float* s, int cap,
                                        int32_t* n) {
  GFS_REQUIRE(h && n && cap >= 0 && (cap == 0 || (index && plane && s)), GFS_ERR_INVALID_ARG,
              "gfs_pose_lidar_inertial_fetch_edges: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_REQUIRE(b >= 0 && b < h->last_B && round >= 0 && round < 4, GFS_ERR_INVALID_ARG,
              "gfs_pose_lidar_inertial_fetch_edges: problem %d / round %d outside the last call", b, round);
  GFS_HIP(hipSetDevice(h->device));
  const int cnt = h->last_edges[(size_t)b * 4 + round];
  *n = cnt;
  const int m = std::min(cnt, cap);
  if (m == 0) return GFS_OK;
  const size_t o = ((size_t)b * 4 + round) * h->last_SC;
  GFS_HIP(hipMemcpy(index, h->d_eidx.p + o, (size_t)m * 4, hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(plane, h->d_eplane.p + o, (size_t)m * 16, hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(s, h->d_es.p + o, (size_t)m * 4, hipMemcpyDeviceToHost));
  return GFS_OK;
}

}  // extern "C"
