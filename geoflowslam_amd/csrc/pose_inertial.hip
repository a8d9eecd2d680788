// Optimizer::PoseInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:5899-6283, 6762-7171) on MI355X: the IMU
// pose step that ends Tracking::TrackLocalMap, for a batch of problems with the two modes mixed freely (include/gfs_abi.h section 19).
//
// One 256-thread workgroup owns one problem and runs its whole schedule in one launch, as k_pose_opt does: up to 4 x 10 Gauss-Newton
// iterations over the dense 15 x 15 / 30 x 30 system, the re-classifications, the recovery pass and the Hessian of the new prior, with
// no host round trip.  The rule -- every formula, the quirks kept and the written rules N / E / L / S -- is pose_inertial_rule.hpp's,
// shared with the sequential restatement (tests/host/pose_inertial_restatement.cpp), whose bytes every output has.  This file holds
// only who computes what:
//   * the visual edges are spread over the threads; a thread's first two edges live in registers for the whole solve, edges past 512
//     go through global memory.  Every sum over them -- the 21 + 6 entries of the pose block, the float avgReprojectionError, the 36
//     entries of the inliers' Hessian blocks -- is added in edge order: the threads park their terms in an LDS slab, one lane per
//     quantity adds its row (pose_lm_dev.hpp's ordered_sum).
//   * the inertial, random-walk and prior edges are linearised by one lane each, in different waves; the entries of their J' Omega, of
//     the system matrix and of the returned Hessian are spread over the threads, each entry computed by the rule's function for it.
//   * the pivoted LDL' lives in LDS: the pivot search and the transposition on one lane, the rows of an elimination step on a lane
//     each, the substitution on one lane (its dependent chain cannot be reordered without changing the bits).
#include <memory>
#include <mutex>

#include "gfs_common.hpp"
#include "pose_inertial_rule.hpp"
#include "pose_lm_dev.hpp"
#include "staging.hpp"
#include "wave_reduce.hpp"

using namespace gfs_pi;
using gfs_pose_lm::ordered_sum;
using gfs_red::block_sum256;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads;             // edges per pass of an ordered sum: one per thread
constexpr int kSlabStride = kChunk + 1;      // odd: the summing lanes read different banks
constexpr int kHessRows = 18;                // the 36 entries of the inliers' blocks go in two halves
constexpr int kWorkAt = kHessRows * kSlabStride;  // Work lives behind the rows the Hessian sums use
constexpr int kWorkDoubles = (int)((sizeof(Work) + 7) / 8);
constexpr int kLdsDoubles = (kSys * kSlabStride > kWorkAt + kWorkDoubles) ? kSys * kSlabStride : kWorkAt + kWorkDoubles;
static_assert(kLdsDoubles * 8 + sizeof(Persist) + 256 <= 64 * 1024, "the slab, the work area and the state fit the static LDS limit");

struct PiOut {
  gfs_imu_estimate cur, other;
  int n_good, n_inliers, rounds_run;
  float avg;
  double H[900];
};

// An edge as its thread keeps it: the inputs (read once) and what g2o keeps per edge (error vector, level) plus mvbOutlier
struct EdgeReg {
  double xw[3], obs[3], err[3], w;
  int stereo, close, level, outlier;
};

__global__ __launch_bounds__(kThreads) void k_pose_inertial(const Head* __restrict__ heads, const double* __restrict__ xw_all,
                                                            const double* __restrict__ obs_all, const float* __restrict__ w_all,
                                                            const uint8_t* __restrict__ stereo_all, const uint8_t* __restrict__ close_all, int stride,
                                                            uint8_t* __restrict__ outlier_all, double* __restrict__ err_all,
                                                            uint8_t* __restrict__ level_all, PiOut* __restrict__ outs) {
  __shared__ double s_mem[kLdsDoubles];
  __shared__ Persist s_P;
  __shared__ double s4[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  const Head& h = heads[f];
  const int n = h.n_obs, mode = h.mode;
  const Calib& cam = h.cam;
  double* s_slab = s_mem;
  Work& W = *reinterpret_cast<Work*>(s_mem + kWorkAt);
  const double* xw_f = xw_all + (size_t)f * stride * 3;
  const double* obs_f = obs_all + (size_t)f * stride * 3;
  const float* w_f = w_all + (size_t)f * stride;
  const uint8_t* stereo_f = stereo_all + (size_t)f * stride;
  const uint8_t* close_f = close_all + (size_t)f * stride;
  uint8_t* outlier = outlier_all + (size_t)f * stride;
  double* err = err_all + (size_t)f * stride * 3;
  uint8_t* level = level_all + (size_t)f * stride;

  auto load_edge = [&](int e, bool with_state) {
    EdgeReg R;
    for (int k = 0; k < 3; k++) {
      R.xw[k] = xw_f[3 * e + k];
      R.obs[k] = obs_f[3 * e + k];
      R.err[k] = with_state ? err[3 * e + k] : 0.0;
    }
    R.w = (double)w_f[e];
    R.stereo = stereo_f[e];
    R.close = close_f[e];
    R.level = with_state ? level[e] : 0;
    R.outlier = with_state ? outlier[e] : 0;
    return R;
  };
  auto store_edge = [&](int e, const EdgeReg& R) {
    for (int k = 0; k < 3; k++) err[3 * e + k] = R.err[k];
    level[e] = (uint8_t)R.level;
    outlier[e] = (uint8_t)R.outlier;
  };
  const int last = n > 0 ? n - 1 : 0;  // (a thread without an edge loads a valid one and never uses it; n == 0 loads nothing)
  EdgeReg R0, R1;
  if (n > 0) {
    R0 = load_edge(min(tid, last), false);
    R1 = load_edge(min(tid + kThreads, last), false);
  }
  auto with_edge = [&](int e, auto&& body) {  // e = tid + 256 k: k is the same in every thread of a pass
    const int k = (e - tid) / kThreads;
    if (k == 0) {
      body(R0);
    } else if (k == 1) {
      body(R1);
    } else {
      EdgeReg R = load_edge(e, true);
      body(R);
      store_edge(e, R);
    }
  };
  for (int e = tid + 2 * kThreads; e < n; e += kThreads) {
    outlier[e] = 0;
    level[e] = 0;
    for (int k = 0; k < 3; k++) err[3 * e + k] = 0.0;
  }
  if (tid == 0) persist_init(h, s_P);
  __syncthreads();
  const int D = mode == kFrame ? 30 : 15;

  // computeError + linearizeOplus of the small edges, a lane each in three waves; then the entries of their J' Omega over the threads
  auto small_edges = [&](bool build) {
    if (tid == 0) small_edge_linearize(h, s_P, W, 0, build);
    if (tid == 64) {
      small_edge_linearize(h, s_P, W, 1, build);
      small_edge_linearize(h, s_P, W, 2, build);
    }
    if (tid == 128) small_edge_linearize(h, s_P, W, 3, build);
    __syncthreads();
    for (int idx = tid; idx < kAtOEntries; idx += kThreads) small_edge_AtO_entry(mode, W, idx);
    __syncthreads();
  };

  bool robust = true;  // the visual edges' kernels: dropped after round 2
  int nBad = 0, nInliers = 0, rounds_run = 0;
  float avg = 0.0f;  // thread 0
  for (int it = 0; it < h.n_rounds; it++) {
    if (tid == 0) s_P.ok = 1;
    __syncthreads();
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
            if (robust) huber(vis_chi2(R.err, R.w, st), huber_delta_visual(st), &rho0, &rho1);
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
      // ---- the small edges, the system matrix and its right-hand side
      small_edges(true);
      for (int idx = tid; idx < D * D; idx += kThreads) {
        const int R = idx / D, C = idx % D;
        if (C <= R) W.A[kLd * R + C] = system_entry(mode, s_P, W, R, C);
      }
      if (tid < D) W.b[tid] = system_rhs(mode, s_P, W, tid);
      if (tid == 0) W.sign = 0;
      __syncthreads();
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
    if (tid == 0) inertial_after_round(h, s_P);
    // ---- the re-classification.  Outlier edges are re-evaluated at the current estimate (parallel); the float sum of the inliers'
    //      chi2 is added in the reference's order, the mono list then the stereo list, from terms parked in LDS
    {
      double Rcw[9], tcw[3];
      for (int k = 0; k < 9; k++) Rcw[k] = s_P.s[0].Rcw[k];
      for (int k = 0; k < 3; k++) tcw[k] = s_P.s[0].tcw[k];
      float* s_term = reinterpret_cast<float*>(s_slab);
      int bad_local = 0, good_local = 0;
      avg = 0.0f;
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
    if (it == 2) robust = false;
    rounds_run = it + 1;
    __syncthreads();
    if (edge_count(mode, n) < kMinEdges) break;
  }
  // ---- recover not too bad points (:6210-6234)
  if (nInliers < kFewInliers && !h.rec_init) {
    double Rcw[9], tcw[3];
    for (int k = 0; k < 9; k++) Rcw[k] = s_P.s[0].Rcw[k];
    for (int k = 0; k < 3; k++) tcw[k] = s_P.s[0].tcw[k];
    int bad_local = 0;
    for (int e = tid; e < n; e += kThreads)
      with_edge(e, [&](EdgeReg& R) {
        const bool st = R.stereo != 0;
        vis_error(cam, Rcw, tcw, R.xw, R.obs, st, R.err);
        if (vis_chi2(R.err, R.w, st) < (st ? kChi2StereoOut : kChi2MonoOut)) R.outlier = 0;
        else bad_local++;
      });
    nBad = (int)block_sum256((double)bad_local, s4);
  }
  // ---- the Hessian of the new prior: the small edges re-linearised at the final state, then the inliers' 6 x 6 blocks in the
  //      order mono list, stereo list.  W.A holds it row-major with stride D
  small_edges(false);
  for (int idx = tid; idx < D * D; idx += kThreads) W.A[idx] = hessian_entry(mode, W, idx / D, idx % D);
  __syncthreads();
  {
    double Rcw[9], tcw[3];
    for (int k = 0; k < 9; k++) Rcw[k] = s_P.s[0].Rcw[k];
    for (int k = 0; k < 3; k++) tcw[k] = s_P.s[0].tcw[k];
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
          if (e < n) with_edge(e, [&](EdgeReg& R) {
            const bool st = R.stereo != 0;
            if (st != (pass == 1) || R.outlier) return;
            double J[18];
            vis_jacobian(cam, Rcw, tcw, R.xw, st, J);
#pragma unroll
            for (int k = 0; k < kHessRows; k++) {
              const int a = half * 3 + k / 6, c = k % 6;  // rows 0-2 in the first half, 3-5 in the second
              term[k] = vis_hessian_entry(J, R.w, st, a, c);
            }
          });
#pragma unroll
          for (int k = 0; k < kHessRows; k++) s_slab[k * kSlabStride + tid] = term[k];
          __syncthreads();
          if (tid < kHessRows) run = ordered_sum(s_slab + tid * kSlabStride, min(kChunk, n - base), run);
          __syncthreads();
        }
      if (tid < kHessRows) W.A[at] = run;
      __syncthreads();
    }
  }
  // ---- results
  PiOut& O = outs[f];
  for (int idx = tid; idx < 900; idx += kThreads) O.H[idx] = idx < D * D ? W.A[idx] : 0.0;
  if (tid < n) outlier[tid] = (uint8_t)R0.outlier;
  if (tid + kThreads < n) outlier[tid + kThreads] = (uint8_t)R1.outlier;
  if (tid == 0) {
    for (int end = 0; end < 2; end++) {
      const State& s = s_P.s[end];
      gfs_imu_estimate& o = end == 0 ? O.cur : O.other;
      for (int k = 0; k < 9; k++) o.Rwb[k] = s.Rwb[k];
      for (int k = 0; k < 3; k++) o.twb[k] = s.twb[k], o.v[k] = s.v[k], o.bg[k] = s.bg[k], o.ba[k] = s.ba[k];
    }
    O.n_good = n - nBad;
    O.n_inliers = nInliers;
    O.rounds_run = rounds_run;
    O.avg = avg;
  }
}

}  // namespace

struct gfs_pose_inertial {
  int device, max_obs, max_batch;
  hipStream_t stream;
  std::mutex mu;
  // one pinned block mirroring one device block for the inputs, one for the outputs: a call is one copy in, the kernel, one copy out
  struct Layout {  // S: visual edges per problem
    gfs::Block<256> in, res;
    gfs::Field<Head> heads;
    gfs::Field<double, 3> xw, obs;
    gfs::Field<float> w;
    gfs::Field<uint8_t> stereo, close;
    gfs::Field<PiOut> out;
    gfs::Field<uint8_t> outlier;
    Layout(size_t B, size_t S)
        : heads(in, B), xw(in, B * S), obs(in, B * S), w(in, B * S), stereo(in, B * S), close(in, B * S), out(res, B), outlier(res, B * S) {}
  };
  gfs::Mirror in, res;
  gfs::DevBuf<double> d_err;
  gfs::DevBuf<uint8_t> d_level;
};

extern "C" {

int gfs_pose_inertial_create(int device, int max_obs, int max_batch, gfs_pose_inertial** out) {
  GFS_REQUIRE(out && max_obs > 0 && max_batch > 0, GFS_ERR_INVALID_ARG, "gfs_pose_inertial_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_pose_inertial> h(new gfs_pose_inertial);
  h->device = device;
  h->max_obs = max_obs;
  h->max_batch = max_batch;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t Smax = gfs::align_up((size_t)max_obs, 64);
  const gfs_pose_inertial::Layout L{(size_t)max_batch, Smax};
  int rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->d_err.alloc(Smax * max_batch * 3);
  if (!rc) rc = h->d_level.alloc(Smax * max_batch);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_pose_inertial_destroy(gfs_pose_inertial* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_pose_inertial_optimize(gfs_pose_inertial* h, const gfs_pose_inertial_problem* problems, int B, gfs_pose_inertial_solution* solutions) {
  GFS_REQUIRE(h && problems && solutions && B > 0, GFS_ERR_INVALID_ARG, "gfs_pose_inertial_optimize: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_pose_inertial_optimize: batch %d exceeds capacity %d", B, h->max_batch);
  // every refusal before anything is staged
  int S = 64;  // stride of the per-problem arrays in this call
  for (int f = 0; f < B; f++) {
    const gfs_pose_inertial_problem& p = problems[f];
    GFS_REQUIRE(p.mode == GFS_POSE_INERTIAL_LAST_KEYFRAME || p.mode == GFS_POSE_INERTIAL_LAST_FRAME, GFS_ERR_INVALID_ARG,
                "gfs_pose_inertial_optimize: problem %d has mode %d", f, p.mode);
    GFS_REQUIRE(p.n_obs >= 0, GFS_ERR_INVALID_ARG, "gfs_pose_inertial_optimize: problem %d has n_obs = %d", f, p.n_obs);
    GFS_REQUIRE(p.n_rounds >= 1 && p.n_rounds <= kMaxRounds, GFS_ERR_INVALID_ARG, "gfs_pose_inertial_optimize: problem %d has n_rounds = %d", f,
                p.n_rounds);
    GFS_REQUIRE(p.n_obs <= h->max_obs, GFS_ERR_CAPACITY, "gfs_pose_inertial_optimize: problem %d has %d observations (capacity %d)", f, p.n_obs,
                h->max_obs);
    GFS_REQUIRE(p.n_obs == 0 || (p.xw && p.obs && p.inv_sigma2 && p.stereo && p.close && solutions[f].outlier), GFS_ERR_INVALID_ARG,
                "gfs_pose_inertial_optimize: problem %d has NULL observation arrays", f);
    S = std::max(S, (int)gfs::align_up((size_t)p.n_obs, 64));
  }
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_pose_inertial::Layout L{(size_t)B, (size_t)S};
  uint8_t* hi = h->in.h.p;
  for (int f = 0; f < B; f++) {
    const gfs_pose_inertial_problem& p = problems[f];
    fill_head(p, L.heads.at(hi)[f]);
    const size_t at = (size_t)f * S, n = (size_t)p.n_obs;
    L.xw.put(hi, at, p.xw, n);
    L.obs.put(hi, at, p.obs, n);
    L.w.put(hi, at, p.inv_sigma2, n);
    L.stereo.put(hi, at, p.stereo, n);
    L.close.put(hi, at, p.close, n);
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  uint8_t* dr = h->res.d.p;
  GFS_LAUNCH("k_pose_inertial", k_pose_inertial, dim3(B), dim3(kThreads), 0, s, L.heads.at(di), L.xw.at(di), L.obs.at(di), L.w.at(di),
             L.stereo.at(di), L.close.at(di), S, L.outlier.at(dr), h->d_err.p, h->d_level.p, L.out.at(dr));
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  for (int f = 0; f < B; f++) {
    const PiOut& O = L.out.at(hr)[f];
    gfs_pose_inertial_solution& r = solutions[f];
    r.cur = O.cur;
    r.other = O.other;
    r.n_good = O.n_good;
    r.n_inliers = O.n_inliers;
    r.rounds_run = O.rounds_run;
    r.avg_reproj = O.avg;
    memcpy(r.H, O.H, sizeof(r.H));
    L.outlier.get(r.outlier, hr, (size_t)f * S, (size_t)problems[f].n_obs);
  }
  return GFS_OK;
}

}  // extern "C"
