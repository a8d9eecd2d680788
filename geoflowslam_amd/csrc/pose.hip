// Optimizer::PoseOptimization (reference src/Optimizer.cc:763-1098) on MI355X: motion-only bundle adjustment of a
// batch of frames, conventional-SLAM branch (pFrame->mpCamera2 == nullptr).
//
// One 256-thread workgroup owns one frame and runs its whole schedule on the device: 4 rounds x optimize(10) of the g2o
// Levenberg-Marquardt loop over one VertexSE3Expmap with unary mono / stereo edges and Huber kernels, and the outlier
// re-classification between rounds (:972-1073).  This file holds the kernel's loops, the edges kept in registers and the fast oplus of
// the tree mode; the bodies the loops call -- edge error and quadratic form, the 6x6 solves, the ordered sum, the LM bookkeeping, the
// classification step -- are pose_lm_dev.hpp's, shared with pose_lidar.hip.
// Edges are spread over the threads, but every sum over the edges -- activeRobustChi2 (core/sparse_optimizer.cpp:104-122) and
// the 21 + 6 entries of the normal equations (core/base_unary_edge.hpp:43-72, one edge after the other into the vertex's
// block) -- is added in g2o's order, the edge order: the threads park their terms in an LDS slab and one lane per quantity
// adds them up sequentially.  Together with glibc's sin / cos / pow (glibc_math.hpp) every double of the solve has the bits
// the sequential CPU restatement (oracle/pose_oracle.cpp) produces; the sign of a gain ratio at a converged state (one more LM
// iteration or not) depends on exactly that.  No Eigen / g2o build exists in this image to pin the association of an edge's products
// against: "bit-identical" is a statement about the restatement, the bar against the reference is 1e-5.  The scalar LM bookkeeping
// runs on thread 0 and is broadcast through LDS.
// Quirks kept: every round restarts from the frame's pose, nGood is never reset, and the optimised pose is returned but meant to
// be discarded.
#include <memory>
#include <mutex>

#include "block_layouts.hpp"
#include "g2o_se3_dev.hpp"
#include "gfs_common.hpp"
#include "pose_lm_dev.hpp"
#include "wave_reduce.hpp"

using namespace gfs_se3;
using namespace gfs_pose_lm;
using gfs_red::block_sum256;

namespace {

constexpr int kPoseThreads = 256;

struct PoseFrame {
  double q[4], t[3];
  double fx, fy, cx, cy, bf;
  int n_obs, n_rounds, its, pad;
};
struct PoseOut {
  double q[4], t[3];
  float avg;
  int n_inliers, rounds_run, iterations_run;
};

struct EdgeView {
  const double* xw;
  const double* obs;
  const float* w;
  const uint8_t* stereo;
};

// An edge as its thread keeps it: the inputs (read once) and the state g2o keeps per edge (error vector, chi2, level) plus mvbOutlier.
struct EdgeReg {
  double xw[3], obs[3], err[3], chi2, w;
  int stereo, level, outlier;
};

// Ordered sums: kChunk edges per pass (one per thread) park their 27 terms in an LDS slab, row q = quantity q with an odd
// row stride (the 27 summing lanes then read different banks); lane q adds its row to its running value in index order.
constexpr int kChunk = kPoseThreads;
constexpr int kSlabStride = kChunk + 1;
constexpr int kSlabDoubles = kSys * kSlabStride;  // also the capacity of one pass of the chi2 sum

// kTree = false: every sum over the edges in edge order on one lane (the bits of the sequential restatement; a chain of n dependent
//   additions, 21 cycles each, three times an LM iteration).
// kTree = true (the default of the handle): the same terms added by a tree of FIXED shape -- a thread adds its own edges (e = tid,
//   tid + 256, ...) in index order, then the 256 partial sums are folded by the wave shuffle tree and the four waves in order.  The
//   shape depends on nothing but the number of edges, so a frame gives the same bits alone or inside any batch; against the
//   restatement the sums differ in their last bits (relative 1e-16), the bar on the pose is 1e-5, and an outlier flag can only
//   differ where an edge's chi2 sits within rounding of its threshold (tests/test_gpu_pose.py proves that for every flip).

// VertexSE3Expmap::oplusImpl as pose_oplus (g2o_se3_dev.hpp), for the tree-sum default: the device library's sin / cos and a plain
// cube instead of the bit-for-bit restatement of glibc's (a few hundred instructions on the one lane everybody waits for), fused
// multiply-adds.  Same formulas, results within rounding.
__device__ __forceinline__ void pose_oplus_fast(const double* q_in, const double* t_in, const double* u, double* q_out, double* t_out) {
#pragma clang fp contract(fast)
  const double om[3] = {u[0], u[1], u[2]}, ups[3] = {u[3], u[4], u[5]};
  const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
  const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
  double O2[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
  double R[9], V[9];
  if (theta < 0.00001) {
    for (int i = 0; i < 9; i++) {
      R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i];
      V[i] = R[i];
    }
  } else {
    double sn, cn;
    sincos(theta, &sn, &cn);
    const double a = sn / theta, b = (1 - cn) / (theta * theta), c = (theta - sn) / (theta * theta * theta);
    for (int i = 0; i < 9; i++) {
      R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * O[i] + b * O2[i];
      V[i] = (i % 4 == 0 ? 1.0 : 0.0) + b * O[i] + c * O2[i];
    }
  }
  double eq[4], et[3];
  R_to_quat(R, eq);
  for (int r = 0; r < 3; r++) et[r] = V[3 * r] * ups[0] + V[3 * r + 1] * ups[1] + V[3 * r + 2] * ups[2];
  normalize_rotation(eq);
  double rt[3];
  quat_rotate(eq, t_in, rt);
  const double* a = eq;
  const double* b = q_in;
  double q[4];
  q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  normalize_rotation(q);
  for (int i = 0; i < 3; i++) t_out[i] = et[i] + rt[i];
  for (int i = 0; i < 4; i++) q_out[i] = q[i];
}

#ifdef GFS_POSE_TIMING
#define PT_INIT long long pt_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt_last = clock64();
#define PT(k) { const long long _n = clock64(); pt_acc[k] += _n - pt_last; pt_last = _n; }
#define PT_END if (tid == 0 && f == 0) printf("POSET setup=%lld active=%lld build=%lld solve=%lld trial=%lld decide=%lld classify=%lld its=%d\n", pt_acc[0], pt_acc[1], pt_acc[2], pt_acc[3], pt_acc[4], pt_acc[5], pt_acc[6], O.iterations_run);
#else
#define PT_INIT
#define PT(k)
#define PT_END
#endif
template <bool kTree>
__global__ __launch_bounds__(kPoseThreads) void k_pose_opt(const PoseFrame* __restrict__ frames, const double* __restrict__ xw_all,
                                                           const double* __restrict__ obs_all, const float* __restrict__ w_all,
                                                           const uint8_t* __restrict__ stereo_all, int stride,
                                                           uint8_t* __restrict__ outlier_all, double* __restrict__ chi2_all,
                                                           double* __restrict__ err_all, uint8_t* __restrict__ level_all,
                                                           PoseOut* __restrict__ outs) {
  __shared__ double s4[4];
  __shared__ double s_slab[kSlabDoubles];
  __shared__ double s_T[7], s_Tb[7];  // current estimate, backup (push / pop)
  __shared__ double s_sys[kSys];
  __shared__ double s_x[6];
  __shared__ int s_flag[3];
  const int f = blockIdx.x, tid = threadIdx.x;
  PT_INIT
  const PoseFrame F = frames[f];
  const int n = F.n_obs;
  EdgeView E{xw_all + (size_t)f * stride * 3, obs_all + (size_t)f * stride * 3, w_all + (size_t)f * stride,
             stereo_all + (size_t)f * stride};
  uint8_t* outlier = outlier_all + (size_t)f * stride;
  double* chi2 = chi2_all + (size_t)f * stride;
  double* err = err_all + (size_t)f * stride * 3;
  uint8_t* level = level_all + (size_t)f * stride;
  double q0[4] = {F.q[0], F.q[1], F.q[2], F.q[3]};
  normalize_rotation(q0);  // SE3Quat(q, t) constructor
  // Edge e belongs to thread e % 256 in every pass of the kernel.  The thread's first two edges (frames of up to 512 observations:
  // the usual case) live in registers for the whole solve -- inputs, error vector, chi2, level, outlier flag; without that every one
  // of the ~50 passes over the edges starts with a round trip to memory for 56 bytes an edge and ends with another for the state.
  // Edges beyond them go through global memory (load, pass body, store).
  auto load_edge = [&](int e, bool with_state) {
    EdgeReg R;
    for (int k = 0; k < 3; k++) {
      R.xw[k] = E.xw[3 * e + k];
      R.obs[k] = E.obs[3 * e + k];
      R.err[k] = with_state ? err[3 * e + k] : 0.0;
    }
    R.w = (double)E.w[e];
    R.stereo = E.stereo[e];
    R.chi2 = with_state ? chi2[e] : 0.0;
    R.level = with_state ? level[e] : 0;
    R.outlier = with_state ? outlier[e] : 0;
    return R;
  };
  auto store_edge = [&](int e, const EdgeReg& R) {
    for (int k = 0; k < 3; k++) err[3 * e + k] = R.err[k];
    chi2[e] = R.chi2;
    level[e] = (uint8_t)R.level;
    outlier[e] = (uint8_t)R.outlier;
  };
  EdgeReg R0 = load_edge(min(tid, n - 1 < 0 ? 0 : n - 1), false), R1 = load_edge(min(tid + kPoseThreads, n - 1 < 0 ? 0 : n - 1), false);
  auto with_edge = [&](int e, auto&& body) {  // e = tid + 256 k: k is the same in every thread of a pass
    const int k = (e - tid) / kPoseThreads;
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
  for (int e = tid + 2 * kPoseThreads; e < n; e += kPoseThreads) {
    outlier[e] = 0;
    level[e] = 0;
    chi2[e] = 0;
  }
  if (tid < 4) s_T[tid] = q0[tid];
  if (tid < 3) s_T[4 + tid] = F.t[tid];
  __syncthreads();
  PoseOut O;
  for (int k = 0; k < 4; k++) O.q[k] = q0[k];
  for (int k = 0; k < 3; k++) O.t[k] = F.t[k];
  O.avg = 0.f;
  O.n_inliers = 0;
  O.rounds_run = 0;
  O.iterations_run = 0;
  if (n < 3) {  // nInitialCorrespondences < 3 -> return 0 (:958)
    if (tid < n) {
      outlier[tid] = 0;
      chi2[tid] = 0;
    }
    if (tid == 0) outs[f] = O;
    return;
  }
  // errors + chi2 of the active edges at the current estimate; returns activeRobustChi2, summed in edge order (thread 0 only)
  auto compute_active = [&](bool robust) {
    double T[7];
    for (int k = 0; k < 7; k++) T[k] = s_T[k];
    double chi = 0;
    if constexpr (kTree) {
      double mine = 0;
      for (int e = tid; e < n; e += kPoseThreads)
        with_edge(e, [&](EdgeReg& R) {
          if (!R.level) mine += vis_edge_update(F, R.xw, R.obs, R.stereo != 0, R.w, T, robust, R.err, R.chi2);
        });
      return block_sum256(mine, s4);
    }
    for (int base = 0; base < n; base += kSlabDoubles) {
      const int cnt = min(kSlabDoubles, n - base);
      for (int e = base + tid; e < base + cnt; e += kPoseThreads) {
        double term = 0;  // an edge that is not active adds nothing (x + 0 = x)
        with_edge(e, [&](EdgeReg& R) {
          if (!R.level) term = vis_edge_update(F, R.xw, R.obs, R.stereo != 0, R.w, T, robust, R.err, R.chi2);
        });
        s_slab[e - base] = term;
      }
      __syncthreads();
      if (tid == 0) chi = ordered_sum(s_slab, cnt, chi);
      __syncthreads();
    }
    return chi;
  };
  int nBad = 0, nGood = 0;
  PT(0)
  for (int it = 0; it < F.n_rounds; it++) {
    const bool robust = it <= 2;  // setRobustKernel(0) at the end of round 2
    if (tid < 4) s_T[tid] = q0[tid];  // setEstimate(pFrame->GetPose()): the frame pose never changes
    if (tid < 3) s_T[4 + tid] = F.t[tid];
    int local_active = 0;
    for (int e = tid; e < n; e += kPoseThreads) with_edge(e, [&](EdgeReg& R) { local_active += R.level == 0; });
    __syncthreads();
    const int n_active = (int)block_sum256((double)local_active, s4);
    LmState lm{-1, 2, 0};  // thread 0 only
    // g2o computes the active errors at the top of every iteration; after an ACCEPTED trial they are what that trial has just left
    // in the edges, at the same estimate -- same values, same sum -- so the pass is run only after a rejected one (pop(): estimate
    // restored, the edges keep the trial's errors), after an accepted one whose solve had failed, and at the start of a round
    bool fresh = false;       // uniform
    double currentChi = 0;    // thread 0
    for (int iteration = 0; iteration < F.its && n_active > 0; iteration++) {
      PT(5)
      if (!fresh) currentChi = compute_active(robust);
      const double iniChi = currentChi;
      PT(1)
      // ---- buildSystem: linearizeOplus + constructQuadraticForm, summed over the threads' edges
      {
        double T[7];
        for (int k = 0; k < 7; k++) T[k] = s_T[k];
        double run = 0;  // threads 0 .. 26: quantity tid, added up edge by edge
        double tsum[kSys];  // kTree: the thread's own sums over its edges
#pragma unroll
        for (int k = 0; k < kSys; k++) tsum[k] = 0;
        for (int base = 0; base < n; base += kChunk) {
          const int e = base + tid;
          double acc[kSys];
#pragma unroll
          for (int k = 0; k < kSys; k++) acc[k] = 0;
          if (e < n) with_edge(e, [&](EdgeReg& R) {
            if (R.level) return;
            vis_edge_quadratic_form(F, T, R.xw, R.stereo != 0, R.w, robust, R.chi2, R.err, acc);
          });
          if constexpr (kTree) {
#pragma unroll
            for (int k = 0; k < kSys; k++) tsum[k] += acc[k];
          } else {
#pragma unroll
            for (int k = 0; k < kSys; k++) s_slab[k * kSlabStride + tid] = acc[k];
            __syncthreads();
            if (tid < kSys) run = ordered_sum(s_slab + tid * kSlabStride, min(kChunk, n - base), run);
            __syncthreads();
          }
        }
        if constexpr (kTree) run = gfs_red::block_sum_many<kSys, kPoseThreads / 64>(tsum, s_slab);  // valid in threads 0 .. 26
        if (tid < kSys) s_sys[tid] = run;
        __syncthreads();
      }
      PT(2)
      if (tid == 0 && iteration == 0) lm_lambda_init(lm, s_sys);
      double rho = 0;
      int qmax = 0;
      bool again = true;
      while (again) {
        if (tid == 0) {
          for (int k = 0; k < 7; k++) s_Tb[k] = s_T[k];  // push()
          double x[6];
          const bool ok2 = kTree ? ldlt6_solve_spd_fast(s_sys, lm.currentLambda, s_sys + 21, x) : ldlt6_solve_positive(s_sys, lm.currentLambda, s_sys + 21, x);
          if (ok2) {
            double qn[4], tn[3];
            if constexpr (kTree) pose_oplus_fast(s_T, s_T + 4, x, qn, tn);
            else pose_oplus(s_T, s_T + 4, x, qn, tn);
            for (int k = 0; k < 4; k++) s_T[k] = qn[k];
            for (int k = 0; k < 3; k++) s_T[4 + k] = tn[k];
          }
          for (int a = 0; a < 6; a++) s_x[a] = ok2 ? x[a] : 0.0;
          s_flag[0] = ok2 ? 1 : 0;
        }
        __syncthreads();
        PT(3)
        double tempChi = compute_active(robust);
        PT(4)
        if (tid == 0) {
          const LmVerdict v = lm_judge_trial(lm, s_flag[0] != 0, tempChi, s_x, s_sys + 21, kTree, currentChi, rho, qmax);
          if (!v.accepted)
            for (int k = 0; k < 7; k++) s_T[k] = s_Tb[k];  // pop(): estimate restored, edge errors stay those of the trial
          s_flag[1] = v.again ? 1 : 0;
          // (an unsolved trial can be "accepted" too -- currentChi = inf from an edge at z = 0 beats the DBL_MAX an unsolved trial
          //  counts as -- and then currentChi is that DBL_MAX, not the sum the edges hold: the next iteration computes it afresh)
          s_flag[2] = v.accepted && s_flag[0] != 0 ? 1 : 0;
        }
        __syncthreads();
        again = s_flag[1] != 0;
        fresh = s_flag[2] != 0;
        __syncthreads();
      }
      if (tid == 0) {
        O.iterations_run++;
        s_flag[0] = lm_stop(lm, qmax, rho, iniChi, currentChi) ? 1 : 0;
      }
      __syncthreads();
      const int stop = s_flag[0];
      __syncthreads();
      if (stop) break;
    }
    PT(5)
    // ---- classification (:972-1060).  Outlier edges of the previous round are re-evaluated at the final estimate
    //      (parallel); the float accumulation runs on thread 0 in the reference's order (mono list, then stereo list).
    {
      double T[7];
      for (int k = 0; k < 7; k++) T[k] = s_T[k];
      for (int e = tid; e < n; e += kPoseThreads)
        with_edge(e, [&](EdgeReg& R) {
          if (R.outlier) vis_edge_update(F, R.xw, R.obs, R.stereo != 0, R.w, T, false, R.err, R.chi2);
        });
    }
    __syncthreads();
    {
      // every edge is classified by its own thread; what is order dependent -- the float sum of the inliers' chi2, mono list first,
      // then the stereo list, each in creation order (:972-1060) -- is added up by one lane from terms parked in LDS (an edge that
      // is not an inlier of the list at hand parks +0, which changes nothing)
      float* s_term = reinterpret_cast<float*>(s_slab);
      constexpr int kTerms = 2 * kSlabDoubles;
      int bad_local = 0, good_local = 0;
      float avg = 0.0f;  // thread 0
      double mine_avg = 0.0;  // kTree: the thread's inlier terms (floats, added exactly in double), mono list first, then the stereo list
      for (int pass = 0; pass < 2; pass++)
        for (int base = 0; base < n; base += kTerms) {
          const int cnt = min(kTerms, n - base);
          for (int e = base + tid; e < base + cnt; e += kPoseThreads) {
            float term = 0.0f;
            with_edge(e, [&](EdgeReg& R) { term = classify_edge(R.stereo != 0, R.chi2, pass, R.outlier, R.level, bad_local, good_local); });
            if constexpr (kTree) mine_avg += (double)term;
            else s_term[e - base] = term;
          }
          if constexpr (!kTree) {
            __syncthreads();
            if (tid == 0) avg = ordered_sum(s_term, cnt, avg);
            __syncthreads();
          }
        }
      if constexpr (kTree) {  // (float terms, exactly representable in double: every partial sum in double, rounded once)
        avg = (float)block_sum256(mine_avg, s4);
      }
      nBad = (int)block_sum256((double)bad_local, s4);
      nGood += (int)block_sum256((double)good_local, s4);  // nGood is never reset between the rounds
      if (tid == 0) {
        avg /= (float)nGood;
        O.avg = avg;
        O.rounds_run = it + 1;
      }
    }
    __syncthreads();
    PT(6)
    if (n < 10) break;  // optimizer.edges().size() < 10 (:1073)
  }
  if (tid < n) store_edge(tid, R0);  // what the host reads back: mvbOutlier and the per-edge chi2
  if (tid + kPoseThreads < n) store_edge(tid + kPoseThreads, R1);
  if (tid == 0) {
    for (int k = 0; k < 4; k++) O.q[k] = s_T[k];
    for (int k = 0; k < 3; k++) O.t[k] = s_T[4 + k];
    O.n_inliers = n - nBad;
    outs[f] = O;
  }
  PT_END
}

}  // namespace

struct gfs_pose {
  int device, max_obs, max_batch;
  hipStream_t stream;
  std::mutex mu;
  // One pinned arena that mirrors one device block for the inputs (frames | xw | obs | w | stereo) and one for the outputs
  // (out | chi2 | outlier): a call is ONE copy in, the kernel, ONE copy out (five + three copies before: ~10 us of host time and a
  // copy-engine round trip each, more than the kernel's share of a single frame).
  // The layout is that of a call with B frames, arrays strided by the call's largest observation count, rounded up, per frame.
  using Layout = gfs::PoseLayout<PoseFrame, PoseOut>;
  gfs::Mirror in, res;
  gfs::DevBuf<double> d_err;
  gfs::DevBuf<uint8_t> d_level;
  int sum_order = GFS_POSE_SUMS_EDGE_ORDER;  // the ABI default reproduces g2o's integer outputs; the tree is opt-in (gfs_abi.h)
};

extern "C" {

int gfs_pose_create(int device, int max_obs, int max_batch, gfs_pose** out) {
  GFS_REQUIRE(out && max_obs > 0 && max_batch > 0, GFS_ERR_INVALID_ARG, "gfs_pose_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_pose> h(new gfs_pose);
  h->device = device;
  h->max_obs = max_obs;
  h->max_batch = max_batch;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t Smax = gfs::align_up((size_t)max_obs, 64), E = Smax * max_batch, B = max_batch;
  int rc = 0;
  const gfs_pose::Layout L{B, Smax};
  if (!rc) rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->d_err.alloc(E * 3);
  if (!rc) rc = h->d_level.alloc(E);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_pose_destroy(gfs_pose* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_pose_set_sum_order(gfs_pose* h, int order) {
  GFS_REQUIRE(h && (order == GFS_POSE_SUMS_TREE || order == GFS_POSE_SUMS_EDGE_ORDER), GFS_ERR_INVALID_ARG,
              "gfs_pose_set_sum_order: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  h->sum_order = order;
  return GFS_OK;
}

int gfs_pose_optimize(gfs_pose* h, const gfs_pose_problem* problems, int B, gfs_pose_solution* solutions) {
  GFS_REQUIRE(h && problems && solutions && B > 0, GFS_ERR_INVALID_ARG, "gfs_pose_optimize: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_pose_optimize: batch %d exceeds capacity %d", B, h->max_batch);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  int S = 64;  // stride of the per-frame arrays in this call
  for (int f = 0; f < B; f++) {
    GFS_REQUIRE(problems[f].n_obs >= 0 && problems[f].n_obs <= h->max_obs, GFS_ERR_CAPACITY,
                "gfs_pose_optimize: frame %d has %d observations (capacity %d)", f, problems[f].n_obs, h->max_obs);
    S = std::max(S, (int)gfs::align_up((size_t)problems[f].n_obs, 64));
  }
  S = std::min(S, (int)gfs::align_up((size_t)h->max_obs, 64));
  const gfs_pose::Layout L{(size_t)B, (size_t)S};
  uint8_t* hi = h->in.h.p;
  for (int f = 0; f < B; f++) {
    const gfs_pose_problem& p = problems[f];
    GFS_REQUIRE(p.n_obs == 0 || (p.xw && p.obs && p.inv_sigma2 && p.stereo), GFS_ERR_INVALID_ARG,
                "gfs_pose_optimize: frame %d has NULL observation arrays", f);
    GFS_REQUIRE(p.n_obs == 0 || (solutions[f].outlier && solutions[f].chi2), GFS_ERR_INVALID_ARG,
                "gfs_pose_optimize: frame %d has NULL output arrays", f);
    PoseFrame& F = L.frames.at(hi)[f];
    for (int k = 0; k < 4; k++) F.q[k] = p.q[k];
    for (int k = 0; k < 3; k++) F.t[k] = p.t[k];
    F.fx = p.fx;
    F.fy = p.fy;
    F.cx = p.cx;
    F.cy = p.cy;
    F.bf = p.bf;
    F.n_obs = p.n_obs;
    F.n_rounds = p.n_rounds;
    F.its = p.its;
    F.pad = 0;
    const size_t at = (size_t)f * S, n = (size_t)p.n_obs;
    L.xw.put(hi, at, p.xw, n);
    L.obs.put(hi, at, p.obs, n);
    L.w.put(hi, at, p.inv_sigma2, n);
    L.stereo.put(hi, at, p.stereo, n);
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  uint8_t* dr = h->res.d.p;
  auto launch = [&](auto kernel) -> int {
    GFS_LAUNCH("k_pose_opt", kernel, dim3(B), dim3(kPoseThreads), 0, s, L.frames.at(di), L.xw.at(di), L.obs.at(di), L.w.at(di),
               L.stereo.at(di), S, L.outlier.at(dr), L.chi2.at(dr), h->d_err.p, h->d_level.p, L.out.at(dr));
    return GFS_OK;
  };
  const int rc_launch = h->sum_order == GFS_POSE_SUMS_EDGE_ORDER ? launch(k_pose_opt<false>) : launch(k_pose_opt<true>);
  if (rc_launch) return rc_launch;
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  for (int f = 0; f < B; f++) {
    const PoseOut& O = L.out.at(hr)[f];
    gfs_pose_solution& r = solutions[f];
    const int n = problems[f].n_obs;
    L.outlier.get(r.outlier, hr, (size_t)f * S, n);
    L.chi2.get(r.chi2, hr, (size_t)f * S, n);
    for (int k = 0; k < 4; k++) r.q[k] = O.q[k];
    for (int k = 0; k < 3; k++) r.t[k] = O.t[k];
    r.avg_reproj_error = O.avg;
    r.n_inliers = O.n_inliers;
    r.rounds_run = O.rounds_run;
    r.iterations_run = O.iterations_run;
  }
  return GFS_OK;
}

}  // extern "C"
