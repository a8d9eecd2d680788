// Optimizer::PoseLidarVisualOptimization (reference src/Optimizer.cc:7698-8059) on MI355X: motion-only bundle adjustment of a batch
// of frames with the visual edges of PoseOptimization plus, per round, the point-to-plane edges GenerateLidarEdge (:8339-8421) builds
// from the frame's downsampled cloud and the local map (EdgeSE3LidarPoint2Plane, include/G2oTypes.h:574-600).
//
// A call runs k_pl_init, then per round k_pl_assoc (one thread per cloud point: pointAssociateToMap, exact 5-NN in the map's hash
// grid, the float ColPivHouseholderQR plane fit, the gates, the weight) and k_pl_round (one 256-thread workgroup per frame: compaction
// of the surviving edges in cloud-index order, chi2Lidar / valid_edge, the Levenberg-Marquardt loop over visual + lidar edges, the
// re-classification of the visual edges, the float pose of the next association).  The edges live in global memory: a few thousand
// lidar edges do not fit beside the LDS slab of the ordered sums.  Every sum over the edges is added in g2o's edge order (visual edges
// by key-point index, then lidar edges by cloud index) on one lane per quantity (GFS_POSE_SUMS_EDGE_ORDER, the bits of the sequential
// restatement tests/host/pose_lidar_restatement.cpp), or by a tree of fixed shape (GFS_POSE_SUMS_TREE).  The visual-edge bodies, the
// pivoted 6x6 solve (in both sum modes), the ordered sum and the LM bookkeeping are pose_lm_dev.hpp's, shared with pose.hip; the
// lidar edges, the loops and the edge storage are this file's.
//
// The numeric Jacobian of a lidar edge (core/base_unary_edge.hpp:82-123) evaluates the error at the estimate moved by +-1e-9 along
// each of the six axes.  Those twelve poses -- and their inverses, which computeError takes -- are the same for every edge: they are
// computed once per linearisation by twelve lanes and shared through LDS (g2o recomputes the same values edge by edge, so the bits do
// not change).  A step of 1e-9 takes SE3Quat::exp's small-angle branch: no sin / cos is evaluated for them.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "block_layouts.hpp"
#include "g2o_se3_dev.hpp"
#include "gfs_common.hpp"
#include "lidar_assoc.hpp"
#include "pose_lm_dev.hpp"
#include "wave_reduce.hpp"

using namespace gfs_se3;
using namespace gfs_lidar;
using namespace gfs_pose_lm;
using gfs_red::block_sum256;

namespace {

constexpr int kThreads = 256;
constexpr int kSlabStride = kThreads + 1;
constexpr int kSlabDoubles = kSys * kSlabStride;
// GenerateLidarEdge / PoseLidarVisualOptimization constants (tests/test_pose_lidar_constants.py reads them from here)
constexpr int kIts[4] = {10, 5, 5, 5};
constexpr int kMinCloud = 50;
constexpr double kSqDisGate = 1.0;
constexpr double kPlaneGate = 0.2;
constexpr double kWeightSlope = 0.9;
constexpr double kMinWeight = 0.1;
constexpr double kLidarInfo = 1e2;
constexpr double kLidarValidChi2 = 4.0;
constexpr double kThHuberLidar = 1.0;  // sqrt(1.0)
// handed to the shared association (lidar_assoc.hpp)
struct Gates {
  static constexpr double kSqDisGate = ::kSqDisGate, kPlaneGate = ::kPlaneGate, kWeightSlope = ::kWeightSlope, kMinWeight = ::kMinWeight;
};

struct LFrame {
  float q[4], t[3];
  float residual_in;
  double fx, fy, cx, cy, bf;
  int n_obs, n_cloud, n_iter, n_lidar_inliers_in;
  const float4* map_pts;  // sorted by bucket; w = original index (bits)
  const int* map_start;   // [nb + 1]
  int map_nb, map_n;
};
struct LState {
  double q[4], t[3];
  double M[12];
  float qf[4], tf[3];
  float avg, residual;
  int n_inliers, n_lidar_inliers, lidar_rounds, rounds_run, iterations_run, nBad, nGood, vis_robust, done;
  int round_edges[4], round_valid[4];
  float round_chi2[4];
};

// ------------------------------------------------------------------ Sophus::SE3f arithmetic (float): the rest in lidar_assoc.hpp
__device__ void se3f_of(const double* q, const double* t, float* qf, float* tf) {
  for (int i = 0; i < 4; i++) qf[i] = (float)q[i];
  for (int i = 0; i < 3; i++) tf[i] = (float)t[i];
  so3f_normalize(qf);
}

__global__ __launch_bounds__(kThreads) void k_pl_assoc(const LFrame* __restrict__ frames, const LState* __restrict__ states,
                                                      const float* __restrict__ cloud_all, int SC, int it, uint8_t* __restrict__ flag_all,
                                                      float4* __restrict__ plane_all, float* __restrict__ s_all) {
  const int f = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const LFrame& F = frames[f];
  const LState& S = states[f];
  if (i >= F.n_cloud || it >= F.n_iter || S.done || F.n_cloud < kMinCloud) return;
  uint8_t* flag = flag_all + (size_t)f * SC;
  flag[i] = 0;
  float d[5];
  int ind[5], slot[5];
  float4 pl;
  float s;
  if (!lidar_point_edge<Gates>(S.M, cloud_all + ((size_t)f * SC + i) * 3, F.map_pts, F.map_start, F.map_nb, d, ind, slot, &pl, &s)) return;
  flag[i] = 1;
  plane_all[(size_t)f * SC + i] = pl;
  s_all[(size_t)f * SC + i] = s;
}

// The association of LocalVisualLidarBA (src/Optimizer.cc:1327-1362): every lidar key-frame of the window at once (blockIdx.y), at
// its stored pose, against the one local map.  The same per-point body as k_pl_assoc.
__global__ __launch_bounds__(kThreads) void k_lba_lidar_assoc(const WindowKF* __restrict__ kfs, const float* __restrict__ cloud,
                                                             const float4* __restrict__ map_pts, const int* __restrict__ map_start,
                                                             int map_nb, uint8_t* __restrict__ flag, float4* __restrict__ plane,
                                                             float* __restrict__ s_all) {
  const WindowKF& K = kfs[blockIdx.y];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= K.n) return;
  const size_t g = (size_t)K.begin + i;
  flag[g] = 0;
  double M[12];
  init_pose_f(K.q, K.t, M);  // initPose = Converter::toMatrix4d(pKFi->GetPose().inverse()) (:1341)
  float d[5];
  int ind[5], slot[5];
  float4 pl;
  float s;
  if (!lidar_point_edge<Gates>(M, cloud + 3 * g, map_pts, map_start, map_nb, d, ind, slot, &pl, &s)) return;
  flag[g] = 1;
  plane[g] = pl;
  s_all[g] = s;
}

struct VisView {
  const double *xw, *obs;
  const float* w;
  const uint8_t* st;
  double *err, *chi2;
  uint8_t *level, *outl;
};

template <bool kTree>
__global__ __launch_bounds__(kThreads) void k_pl_round(const LFrame* __restrict__ frames, LState* __restrict__ states, VisView V, int S,
                                                      const float* __restrict__ cloud_all, const uint8_t* __restrict__ flag_all,
                                                      const float4* __restrict__ plane_all, const float* __restrict__ s_all, int SC,
                                                      int* __restrict__ eidx_all, float4* __restrict__ eplane_all,
                                                      float* __restrict__ es_all, double* __restrict__ lerr_all,
                                                      double* __restrict__ lchi2_all, int it) {
  __shared__ double s_slab[kSlabDoubles];
  __shared__ double s4[4];
  __shared__ double s_T[7], s_Tb[7], s_Wp[12][7], s_sys[kSys], s_x[6];
  __shared__ int s_flag[3], s_wcnt[4];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LFrame F = frames[f];
  LState& ST = states[f];
  if (it >= F.n_iter || ST.done) return;
  const int n = F.n_obs;
  const double* xw = V.xw + (size_t)f * S * 3;
  const double* obs = V.obs + (size_t)f * S * 3;
  const float* wv = V.w + (size_t)f * S;
  const uint8_t* st = V.st + (size_t)f * S;
  double* err = V.err + (size_t)f * S * 3;
  double* chi2 = V.chi2 + (size_t)f * S;
  uint8_t* level = V.level + (size_t)f * S;
  uint8_t* outl = V.outl + (size_t)f * S;
  const size_t rbase = ((size_t)f * 4 + it) * SC;
  int* eidx = eidx_all + rbase;
  float4* eplane = eplane_all + rbase;
  float* es = es_all + rbase;
  double* lerr = lerr_all + (size_t)f * SC;
  double* lchi2 = lchi2_all + (size_t)f * SC;
  const float* cloud = cloud_all + (size_t)f * SC * 3;

  // ---- compaction of the surviving points in cloud-index order (GenerateLidarEdge's vector, nullptr entries skipped)
  int nl = 0;
  if (F.n_cloud >= kMinCloud)
    for (int base = 0; base < F.n_cloud; base += kThreads) {
      const int i = base + tid;
      const bool keep = i < F.n_cloud && flag_all[(size_t)f * SC + i];
      const unsigned long long m = __ballot(keep);
      const int below = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_wcnt[wave] = __popcll(m);
      __syncthreads();
      int off = nl;
      for (int w = 0; w < wave; w++) off += s_wcnt[w];
      if (keep) {
        const int pos = off + below;
        eidx[pos] = i;
        eplane[pos] = plane_all[(size_t)f * SC + i];
        es[pos] = s_all[(size_t)f * SC + i];
      }
      nl += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
      __syncthreads();
    }
  __syncthreads();
  if (tid < 4) s_T[tid] = ST.q[tid];
  if (tid < 3) s_T[4 + tid] = ST.t[tid];
  __syncthreads();
  auto edge_p = [&](int l, double* p) {
    const int i = eidx[l];
    p[0] = (double)cloud[3 * i];
    p[1] = (double)cloud[3 * i + 1];
    p[2] = (double)cloud[3 * i + 2];
  };
  auto lidar_update = [&](int l, const double* W) {  // computeError of lidar edge l at the inverse pose W; returns its chi2
    double p[3];
    edge_p(l, p);
    const double e = lidar_err(W, p, eplane[l], es[l]);
    const double c = e * (kLidarInfo * e);
    lerr[l] = e;
    lchi2[l] = c;
    return c;
  };
  // ---- chi2Lidar (a float, edge after edge) and valid_edge at the current estimate
  {
    double W[7];
    se3_inverse(s_T, s_T + 4, W);
    float chiL = 0.0f;  // thread 0
    int valid = 0;
    for (int base = 0; base < nl; base += kSlabDoubles) {
      const int cnt = min(kSlabDoubles, nl - base);
      for (int l = base + tid; l < base + cnt; l += kThreads) {
        const double c = lidar_update(l, W);
        valid += c < kLidarValidChi2 ? 1 : 0;
        s_slab[l - base] = c;
      }
      __syncthreads();
      if (tid == 0) chiL = ordered_sum(s_slab, cnt, chiL);
      __syncthreads();
    }
    const int n_valid = (int)block_sum256((double)valid, s4);
    if (tid == 0) {
      ST.rounds_run = it + 1;
      ST.round_edges[it] = nl;
      ST.round_valid[it] = n_valid;
      if (nl > 0) {
        chiL /= (float)nl;
        ST.round_chi2[it] = chiL;
        ST.n_lidar_inliers = n_valid;
        ST.residual = chiL;
      }
    }
  }
  if (nl == 0) return;  // `continue`: no optimisation, no re-classification
  const bool vis_robust = ST.vis_robust != 0;
  const int E = n + nl;

  // errors + chi2 of the active edges at s_T; activeRobustChi2 (valid in thread 0)
  auto compute_active = [&]() {
    double T[7], W[7];
    for (int k = 0; k < 7; k++) T[k] = s_T[k];
    se3_inverse(T, T + 4, W);
    auto term_of = [&](int e) -> double {
      if (e < n) {
        if (level[e]) return 0.0;
        return vis_edge_update(F, xw + 3 * e, obs + 3 * e, st[e] != 0, (double)wv[e], T, vis_robust, err + 3 * e, chi2[e]);
      }
      double t, r1;
      huber(lidar_update(e - n, W), kThHuberLidar, &t, &r1);
      return t;
    };
    double chi = 0;
    if constexpr (kTree) {
      double mine = 0;
      for (int e = tid; e < E; e += kThreads) mine += term_of(e);
      return block_sum256(mine, s4);
    }
    for (int base = 0; base < E; base += kSlabDoubles) {
      const int cnt = min(kSlabDoubles, E - base);
      for (int e = base + tid; e < base + cnt; e += kThreads) s_slab[e - base] = term_of(e);
      __syncthreads();
      if (tid == 0) chi = ordered_sum(s_slab, cnt, chi);
      __syncthreads();
    }
    return chi;
  };

  int iterations = 0;
  LmState lm{-1, 2, 0};  // thread 0 only
  for (int iteration = 0; iteration < kIts[it]; iteration++) {
    double currentChi = compute_active();
    const double iniChi = currentChi;
    // ---- the twelve perturbed poses of the numeric Jacobian, inverted (shared by every lidar edge)
    if (tid < 12) {
      double u[6] = {0, 0, 0, 0, 0, 0}, qp[4], tp[3];
      u[tid >> 1] = (tid & 1) ? -1e-9 : 1e-9;
      pose_oplus(s_T, s_T + 4, u, qp, tp);
      se3_inverse(qp, tp, s_Wp[tid]);
    }
    __syncthreads();
    // ---- buildSystem
    {
      double T[7];
      for (int k = 0; k < 7; k++) T[k] = s_T[k];
      double run = 0, tsum[kSys];
#pragma unroll
      for (int k = 0; k < kSys; k++) tsum[k] = 0;
      for (int base = 0; base < E; base += kThreads) {
        const int e = base + tid;
        double acc[kSys];
#pragma unroll
        for (int k = 0; k < kSys; k++) acc[k] = 0;
        if (e < n && !level[e]) {
          vis_edge_quadratic_form(F, T, xw + 3 * e, st[e] != 0, (double)wv[e], vis_robust, chi2[e], err + 3 * e, acc);
        } else if (e >= n && e < E) {
          const int l = e - n;
          double p[3];
          edge_p(l, p);
          const float4 pl = eplane[l];
          const float sl = es[l];
          double J[6];
#pragma unroll
          for (int d = 0; d < 6; d++) J[d] = (1.0 / (2 * 1e-9)) * (lidar_err(s_Wp[2 * d], p, pl, sl) - lidar_err(s_Wp[2 * d + 1], p, pl, sl));
          double r0, rho1;
          huber(lchi2[l], kThHuberLidar, &r0, &rho1);
          const double ev = lerr[l];
          int o = 0;
#pragma unroll
          for (int a = 0; a < 6; a++) {
            acc[21 + a] = -(((rho1 * J[a]) * kLidarInfo) * ev);
#pragma unroll
            for (int c = 0; c <= a; c++) acc[o++] = (J[a] * (rho1 * kLidarInfo)) * J[c];
          }
        }
        if constexpr (kTree) {
#pragma unroll
          for (int k = 0; k < kSys; k++) tsum[k] += acc[k];
        } else {
#pragma unroll
          for (int k = 0; k < kSys; k++) s_slab[k * kSlabStride + tid] = acc[k];
          __syncthreads();
          if (tid < kSys) run = ordered_sum(s_slab + tid * kSlabStride, min(kThreads, E - base), run);
          __syncthreads();
        }
      }
      if constexpr (kTree) run = gfs_red::block_sum_many<kSys, kThreads / 64>(tsum, s_slab);
      if (tid < kSys) s_sys[tid] = run;
      __syncthreads();
    }
    if (tid == 0 && iteration == 0) lm_lambda_init(lm, s_sys);
    double rho = 0;
    int qmax = 0;
    bool again = true;
    while (again) {
      if (tid == 0) {
        for (int k = 0; k < 7; k++) s_Tb[k] = s_T[k];
        double x[6];
        const bool ok2 = ldlt6_solve_positive(s_sys, lm.currentLambda, s_sys + 21, x);  // in both sum modes
        if (ok2) {
          double qn[4], tn[3];
          pose_oplus(s_T, s_T + 4, x, qn, tn);
          for (int k = 0; k < 4; k++) s_T[k] = qn[k];
          for (int k = 0; k < 3; k++) s_T[4 + k] = tn[k];
        }
        for (int a = 0; a < 6; a++) s_x[a] = ok2 ? x[a] : 0.0;
        s_flag[0] = ok2 ? 1 : 0;
      }
      __syncthreads();
      double tempChi = compute_active();
      if (tid == 0) {
        const LmVerdict v = lm_judge_trial(lm, s_flag[0] != 0, tempChi, s_x, s_sys + 21, false, currentChi, rho, qmax);
        if (!v.accepted)
          for (int k = 0; k < 7; k++) s_T[k] = s_Tb[k];  // pop()
        s_flag[1] = v.again ? 1 : 0;
      }
      __syncthreads();
      again = s_flag[1] != 0;
      __syncthreads();
    }
    iterations++;
    if (tid == 0) s_flag[0] = lm_stop(lm, qmax, rho, iniChi, currentChi) ? 1 : 0;
    __syncthreads();
    const int stop = s_flag[0];
    __syncthreads();
    if (stop) break;
  }
  // ---- re-classification of the visual edges at the final estimate: mono list, then stereo list
  {
    double T[7];
    for (int k = 0; k < 7; k++) T[k] = s_T[k];
    for (int e = tid; e < n; e += kThreads)
      if (outl[e]) vis_edge_update(F, xw + 3 * e, obs + 3 * e, st[e] != 0, (double)wv[e], T, false, err + 3 * e, chi2[e]);
  }
  __syncthreads();
  float* s_term = reinterpret_cast<float*>(s_slab);
  constexpr int kTerms = 2 * kSlabDoubles;
  int bad_local = 0, good_local = 0;
  float avg = 0.0f;
  double mine_avg = 0.0;
  for (int pass = 0; pass < 2; pass++)
    for (int base = 0; base < n; base += kTerms) {
      const int cnt = min(kTerms, n - base);
      for (int e = base + tid; e < base + cnt; e += kThreads) {
        const float term = classify_edge(st[e] != 0, chi2[e], pass, outl[e], level[e], bad_local, good_local);
        if constexpr (kTree) mine_avg += (double)term;
        else s_term[e - base] = term;
      }
      if constexpr (!kTree) {
        __syncthreads();
        if (tid == 0) avg = ordered_sum(s_term, cnt, avg);
        __syncthreads();
      }
    }
  if constexpr (kTree) avg = (float)block_sum256(mine_avg, s4);
  const int nBad = (int)block_sum256((double)bad_local, s4);
  const int nGood = (int)block_sum256((double)good_local, s4);
  if (tid == 0) {
    ST.nBad = nBad;
    ST.nGood += nGood;  // never reset
    ST.avg = avg / (float)ST.nGood;
    ST.n_inliers = n - nBad;
    ST.iterations_run += iterations;
    ST.lidar_rounds++;
    for (int k = 0; k < 4; k++) ST.q[k] = s_T[k];
    for (int k = 0; k < 3; k++) ST.t[k] = s_T[4 + k];
    se3f_of(ST.q, ST.t, ST.qf, ST.tf);
    init_pose_f(ST.qf, ST.tf, ST.M);
    if (it == 2) ST.vis_robust = 0;
    if (n < 10) ST.done = 1;  // optimizer.edges().size() < 10
  }
}

__global__ void k_pl_init(const LFrame* __restrict__ frames, LState* __restrict__ states, VisView V, int S) {
  const int f = blockIdx.x;
  const LFrame& F = frames[f];
  for (int e = threadIdx.x; e < F.n_obs; e += blockDim.x) {
    V.outl[(size_t)f * S + e] = 0;
    V.level[(size_t)f * S + e] = 0;
    V.chi2[(size_t)f * S + e] = 0;
  }
  if (threadIdx.x) return;
  LState s;
  for (int k = 0; k < 4; k++) s.q[k] = (double)F.q[k];
  for (int k = 0; k < 3; k++) s.t[k] = (double)F.t[k];
  normalize_rotation(s.q);
  init_pose_f(F.q, F.t, s.M);
  s.done = F.n_obs < 3;  // return 0 before anything else, SetPose not called
  if (s.done) {
    for (int k = 0; k < 4; k++) s.qf[k] = F.q[k];
    for (int k = 0; k < 3; k++) s.tf[k] = F.t[k];
  } else {
    se3f_of(s.q, s.t, s.qf, s.tf);
  }
  s.avg = 0.f;
  s.residual = F.residual_in;
  s.n_lidar_inliers = F.n_lidar_inliers_in;
  s.lidar_rounds = s.rounds_run = s.iterations_run = s.nBad = s.nGood = 0;
  s.n_inliers = s.done ? 0 : F.n_obs;  // nInitialCorrespondences - nBad when no round re-classifies
  s.vis_robust = 1;
  for (int k = 0; k < 4; k++) {
    s.round_edges[k] = s.round_valid[k] = 0;
    s.round_chi2[k] = 0.f;
  }
  states[f] = s;
}

size_t next_pow2(size_t v) {
  size_t p = 64;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace

namespace gfs_lidar {
int min_cloud() { return kMinCloud; }
double edge_information() { return kLidarInfo; }
double edge_huber_delta() { return kThHuberLidar; }
int launch_window_assoc(const gfs_lidar_map* map, const WindowKF* d_kf, int n_kf, int max_n, const float* d_cloud, uint8_t* d_flag,
                        float4* d_plane, float* d_s, hipStream_t s) {
  if (n_kf <= 0 || max_n <= 0) return GFS_OK;
  GFS_LAUNCH("k_lba_lidar_assoc", k_lba_lidar_assoc, dim3(gfs::div_up(max_n, kThreads), n_kf), dim3(kThreads), 0, s, d_kf, d_cloud,
             map->d_pts.p, map->d_start.p, map->nb, d_flag, d_plane, d_s);
  return GFS_OK;
}
}  // namespace gfs_lidar

struct gfs_pose_lidar {
  int device, max_obs, max_cloud, max_batch;
  hipStream_t stream;
  std::mutex mu;
  int sum_order = GFS_POSE_SUMS_EDGE_ORDER;
  using Layout = gfs::PoseLidarLayout<LFrame>;
  gfs::Mirror in;
  gfs::DevBuf<LState> d_state;
  gfs::PinBuf<LState> h_state;
  gfs::DevBuf<double> d_err, d_chi2, d_lerr, d_lchi2;
  gfs::PinBuf<double> h_chi2;
  gfs::DevBuf<uint8_t> d_level, d_outl, d_flag;
  gfs::PinBuf<uint8_t> h_outl;
  gfs::DevBuf<float4> d_plane, d_eplane;
  gfs::DevBuf<float> d_s, d_es;
  gfs::DevBuf<int> d_eidx;
  // the last call's shape, for gfs_pose_lidar_fetch_edges
  int last_B = 0, last_SC = 0;
  std::vector<int> last_edges;  // [B][4]
};

extern "C" {

int gfs_lidar_map_create(int device, int max_points, gfs_lidar_map** out) {
  GFS_REQUIRE(out && max_points >= 5, GFS_ERR_INVALID_ARG, "gfs_lidar_map_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_lidar_map> m(new gfs_lidar_map);
  m->device = device;
  m->max_points = max_points;
  int rc = m->d_pts.alloc((size_t)max_points);
  if (!rc) rc = m->d_start.alloc(next_pow2(2 * (size_t)max_points) + 1);
  if (rc) return rc;
  *out = m.release();
  return GFS_OK;
}

void gfs_lidar_map_destroy(gfs_lidar_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

// The grid is a counting sort of the points by the hash of their 1.25 m cell, built on the host (the map changes at key-frame rate)
// and uploaded with the bucket offsets.  Points keep their original index for the distance ties.
int gfs_lidar_map_set(gfs_lidar_map* m, const float* xyz, int n) {
  GFS_REQUIRE(m && (xyz || n == 0), GFS_ERR_INVALID_ARG, "gfs_lidar_map_set: invalid argument");
  GFS_REQUIRE(n >= 5, GFS_ERR_INVALID_ARG, "gfs_lidar_map_set: %d map points (the reference reads the 5th neighbour)", n);
  GFS_REQUIRE(n <= m->max_points, GFS_ERR_CAPACITY, "gfs_lidar_map_set: %d points exceed capacity %d", n, m->max_points);
  for (int i = 0; i < 3 * n; i++)
    GFS_REQUIRE(std::isfinite(xyz[i]) && std::fabs(xyz[i]) < 1e6f, GFS_ERR_INVALID_ARG,
                "gfs_lidar_map_set: point %d is not finite or beyond 1e6 m", i / 3);
  const int nb = (int)next_pow2(2 * (size_t)n);
  std::vector<unsigned> key(n);
  std::vector<int> start(nb + 1, 0);
  for (int i = 0; i < n; i++) {
    key[i] = cell_hash(cell_of((double)xyz[3 * i]), cell_of((double)xyz[3 * i + 1]), cell_of((double)xyz[3 * i + 2]), nb);
    start[key[i] + 1]++;
  }
  for (int b = 0; b < nb; b++) start[b + 1] += start[b];
  std::vector<int> fill(start.begin(), start.end() - 1);
  std::vector<float4> pts(n);
  for (int i = 0; i < n; i++) {
    float4 P;
    P.x = xyz[3 * i];
    P.y = xyz[3 * i + 1];
    P.z = xyz[3 * i + 2];
    int bits = i;
    memcpy(&P.w, &bits, 4);
    pts[fill[key[i]]++] = P;
  }
  GFS_HIP(hipSetDevice(m->device));
  GFS_HIP(hipMemcpy(m->d_pts.p, pts.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
  GFS_HIP(hipMemcpy(m->d_start.p, start.data(), (size_t)(nb + 1) * sizeof(int), hipMemcpyHostToDevice));
  m->n = n;
  m->nb = nb;
  return GFS_OK;
}

int gfs_pose_lidar_create(int device, int max_obs, int max_cloud, int max_batch, gfs_pose_lidar** out) {
  GFS_REQUIRE(out && max_obs > 0 && max_cloud > 0 && max_batch > 0, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_pose_lidar> h(new gfs_pose_lidar);
  h->device = device;
  h->max_obs = max_obs;
  h->max_cloud = max_cloud;
  h->max_batch = max_batch;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t S = gfs::align_up((size_t)max_obs, 64), SC = gfs::align_up((size_t)max_cloud, 64), B = max_batch;
  const gfs_pose_lidar::Layout L{B, S, SC};
  int rc = 0;
  if (!rc) rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->d_state.alloc(B);
  if (!rc) rc = h->h_state.alloc(B);
  if (!rc) rc = h->d_err.alloc(B * S * 3);
  if (!rc) rc = h->d_chi2.alloc(B * S);
  if (!rc) rc = h->h_chi2.alloc(B * S);
  if (!rc) rc = h->d_level.alloc(B * S);
  if (!rc) rc = h->d_outl.alloc(B * S);
  if (!rc) rc = h->h_outl.alloc(B * S);
  if (!rc) rc = h->d_flag.alloc(B * SC);
  if (!rc) rc = h->d_plane.alloc(B * SC);
  if (!rc) rc = h->d_s.alloc(B * SC);
  if (!rc) rc = h->d_lerr.alloc(B * SC);
  if (!rc) rc = h->d_lchi2.alloc(B * SC);
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

void gfs_pose_lidar_destroy(gfs_pose_lidar* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_pose_lidar_set_sum_order(gfs_pose_lidar* h, int order) {
  GFS_REQUIRE(h && (order == GFS_POSE_SUMS_TREE || order == GFS_POSE_SUMS_EDGE_ORDER), GFS_ERR_INVALID_ARG,
              "gfs_pose_lidar_set_sum_order: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  h->sum_order = order;
  return GFS_OK;
}

int gfs_pose_lidar_optimize(gfs_pose_lidar* h, const gfs_pose_lidar_problem* problems, int B, gfs_pose_lidar_solution* solutions) {
  GFS_REQUIRE(h && problems && solutions && B > 0, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_optimize: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_pose_lidar_optimize: batch %d exceeds capacity %d", B, h->max_batch);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  int S = 64, SC = 64, rounds = 0;
  for (int f = 0; f < B; f++) {
    const gfs_pose_lidar_problem& p = problems[f];
    GFS_REQUIRE(!p.two_camera, GFS_ERR_UNSUPPORTED, "gfs_pose_lidar_optimize: frame %d: the two-camera branch is not implemented", f);
    GFS_REQUIRE(p.n_obs >= 0 && p.n_obs <= h->max_obs, GFS_ERR_CAPACITY, "gfs_pose_lidar_optimize: frame %d has %d observations (capacity %d)",
                f, p.n_obs, h->max_obs);
    GFS_REQUIRE(p.n_cloud >= 0 && p.n_cloud <= h->max_cloud, GFS_ERR_CAPACITY,
                "gfs_pose_lidar_optimize: frame %d has %d cloud points (capacity %d)", f, p.n_cloud, h->max_cloud);
    GFS_REQUIRE(p.n_iterations >= 0 && p.n_iterations <= 4, GFS_ERR_INVALID_ARG,
                "gfs_pose_lidar_optimize: frame %d: n_iterations %d (its[] has 4 entries)", f, p.n_iterations);
    GFS_REQUIRE(p.map && p.map->n >= 5, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_optimize: frame %d: no map, or a map of fewer than 5 points", f);
    GFS_REQUIRE(p.map->device == h->device, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_optimize: frame %d: map on another device", f);
    GFS_REQUIRE(p.n_obs == 0 || (p.xw && p.obs && p.inv_sigma2 && p.stereo && solutions[f].outlier && solutions[f].chi2),
                GFS_ERR_INVALID_ARG, "gfs_pose_lidar_optimize: frame %d has NULL observation arrays", f);
    GFS_REQUIRE(p.n_cloud == 0 || p.cloud, GFS_ERR_INVALID_ARG, "gfs_pose_lidar_optimize: frame %d has a NULL cloud", f);
    S = std::max(S, (int)gfs::align_up((size_t)p.n_obs, 64));
    SC = std::max(SC, (int)gfs::align_up((size_t)p.n_cloud, 64));
    rounds = std::max(rounds, (int)p.n_iterations);
  }
  const gfs_pose_lidar::Layout L{(size_t)B, (size_t)S, (size_t)SC};
  uint8_t* hi = h->in.h.p;
  for (int f = 0; f < B; f++) {
    const gfs_pose_lidar_problem& p = problems[f];
    LFrame& F = L.frames.at(hi)[f];
    for (int k = 0; k < 4; k++) F.q[k] = p.q[k];
    for (int k = 0; k < 3; k++) F.t[k] = p.t[k];
    F.residual_in = solutions[f].residual;
    F.n_lidar_inliers_in = solutions[f].n_lidar_inliers;
    F.fx = p.fx;
    F.fy = p.fy;
    F.cx = p.cx;
    F.cy = p.cy;
    F.bf = p.bf;
    F.n_obs = p.n_obs;
    F.n_cloud = p.n_cloud;
    F.n_iter = p.n_iterations;
    F.map_pts = p.map->d_pts.p;
    F.map_start = p.map->d_start.p;
    F.map_nb = p.map->nb;
    F.map_n = p.map->n;
    const size_t at = (size_t)f * S, n = (size_t)p.n_obs;
    L.xw.put(hi, at, p.xw, n);
    L.obs.put(hi, at, p.obs, n);
    L.w.put(hi, at, p.inv_sigma2, n);
    L.stereo.put(hi, at, p.stereo, n);
    L.cloud.put(hi, (size_t)f * SC, p.cloud, (size_t)p.n_cloud);
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  const LFrame* d_frames = L.frames.at(di);
  VisView V{L.xw.at(di), L.obs.at(di), L.w.at(di), L.stereo.at(di), h->d_err.p, h->d_chi2.p, h->d_level.p, h->d_outl.p};
  const float* d_cloud = L.cloud.at(di);
  GFS_LAUNCH("k_pl_init", k_pl_init, dim3(B), dim3(64), 0, s, d_frames, h->d_state.p, V, S);
  for (int it = 0; it < rounds; it++) {
    GFS_LAUNCH("k_pl_assoc", k_pl_assoc, dim3(SC / kThreads + (SC % kThreads ? 1 : 0), B), dim3(kThreads), 0, s, d_frames, h->d_state.p,
               d_cloud, SC, it, h->d_flag.p, h->d_plane.p, h->d_s.p);
    if (h->sum_order == GFS_POSE_SUMS_EDGE_ORDER)
      GFS_LAUNCH("k_pl_round", k_pl_round<false>, dim3(B), dim3(kThreads), 0, s, d_frames, h->d_state.p, V, S, d_cloud, h->d_flag.p,
                 h->d_plane.p, h->d_s.p, SC, h->d_eidx.p, h->d_eplane.p, h->d_es.p, h->d_lerr.p, h->d_lchi2.p, it);
    else
      GFS_LAUNCH("k_pl_round", k_pl_round<true>, dim3(B), dim3(kThreads), 0, s, d_frames, h->d_state.p, V, S, d_cloud, h->d_flag.p,
                 h->d_plane.p, h->d_s.p, SC, h->d_eidx.p, h->d_eplane.p, h->d_es.p, h->d_lerr.p, h->d_lchi2.p, it);
  }
  GFS_HIP(hipMemcpyAsync(h->h_state.p, h->d_state.p, (size_t)B * sizeof(LState), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipMemcpyAsync(h->h_outl.p, h->d_outl.p, (size_t)B * S, hipMemcpyDeviceToHost, s));
  GFS_HIP(hipMemcpyAsync(h->h_chi2.p, h->d_chi2.p, (size_t)B * S * 8, hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  h->last_B = B;
  h->last_SC = SC;
  h->last_edges.assign((size_t)B * 4, 0);
  for (int f = 0; f < B; f++) {
    const LState& O = h->h_state.p[f];
    gfs_pose_lidar_solution& r = solutions[f];
    const int n = problems[f].n_obs;
    if (n > 0) {
      memcpy(r.outlier, h->h_outl.p + (size_t)f * S, n);
      memcpy(r.chi2, h->h_chi2.p + (size_t)f * S, (size_t)n * 8);
    }
    for (int k = 0; k < 4; k++) r.q[k] = O.q[k];
    for (int k = 0; k < 3; k++) r.t[k] = O.t[k];
    for (int k = 0; k < 4; k++) r.qf[k] = O.qf[k];
    for (int k = 0; k < 3; k++) r.tf[k] = O.tf[k];
    r.avg_reproj_error = O.avg;
    r.n_inliers = O.n_inliers;
    r.n_lidar_inliers = O.n_lidar_inliers;
    r.residual = O.residual;
    r.lidar_rounds = O.lidar_rounds;
    r.rounds_run = O.rounds_run;
    r.iterations_run = O.iterations_run;
    for (int k = 0; k < 4; k++) {
      r.round_edges[k] = O.round_edges[k];
      r.round_chi2[k] = O.round_chi2[k];
      r.round_valid[k] = O.round_valid[k];
      h->last_edges[(size_t)f * 4 + k] = O.round_edges[k];
    }
  }
  return GFS_OK;
}

int gfs_pose_lidar_fetch_edges(gfs_pose_lidar* h, int b, int round, int32_t* index, float* plane, float* s, int cap, int32_t* n) {
  GFS_REQUIRE(h && n && cap >= 0 && (cap == 0 || (index && plane && s)), GFS_ERR_INVALID_ARG, "gfs_pose_lidar_fetch_edges: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_REQUIRE(b >= 0 && b < h->last_B && round >= 0 && round < 4, GFS_ERR_INVALID_ARG,
              "gfs_pose_lidar_fetch_edges: frame %d / round %d outside the last call", b, round);
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
