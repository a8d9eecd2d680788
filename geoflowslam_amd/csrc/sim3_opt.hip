// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2797-3054) on MI355X: the Sim3 refinement of loop verification, between the two
// Sim3 projection searches of LoopClosing (sim3_search.hip).
//
// One 256-thread workgroup owns one problem and runs its whole schedule on the device: optimize(5) of the g2o Levenberg-Marquardt
// loop over ONE free VertexSim3Expmap with two binary edges per pair against fixed points (EdgeSim3ProjectXYZ, then
// EdgeInverseSim3ProjectXYZ, include/OptimizableTypes.h:189-232) and Huber kernels; the first inlier check (:2993-3016), which reads the
// chi2 the solve's last computeActiveErrors left in the edges; the early return (:3024); optimize(10 or 5) on the survivors without
// kernels; the final check (:3032-3046), which does recompute.  An edge lives in its thread's registers, the two edges of a pair in
// neighbouring lanes (the first four edges of a thread; pairs beyond 512 go through global memory).  The Jacobians are g2o's numeric
// ones (core/base_binary_edge.hpp:131-205: central differences through the vertex's oplus, delta 1e-9, only the Sim3 column block
// because every point is fixed); the 14 perturbed
// estimates exp(+-delta e_d) S12 and their inverses are the same for every edge of a linearisation and are computed once, by 14 lanes.
// Every sum over the edges -- activeRobustChi2 and the 28 + 7 entries of the normal equations (base_binary_edge.hpp:55-120, the `to`
// half) -- is added in edge order e12(0), e21(0), e12(1), ...: the threads park their terms in an LDS slab and one lane per quantity
// adds them sequentially, as in k_pose_opt.  With sim3_dev.hpp's arithmetic every double of a fixed-scale solve has the bits of the
// sequential restatement (tests/host/sim3_opt_restatement.cpp), with a free scale too: the exp of the scale update is glibc's, restated
// (glibc_math.hpp).
// The scalar LM bookkeeping runs on thread 0; the 7 x 7 is factored with Eigen::LDLT's pivoting also when the scale is fixed (its
// entry (6, 6) is then 0 + lambda).
// Kept as g2o does it: the solver's x survives a failed solve and both optimize() calls (core/solver.cpp:48-66), is applied also after
// a failed solve, and its scale entry is zeroed in place by the fixed-scale oplus (OptimizableTypes.h:175-182).
#include <cmath>
#include <memory>
#include <mutex>

#include "gfs_common.hpp"
#include "pose_lm_dev.hpp"
#include "sim3_dev.hpp"
#include "staging.hpp"
#include "wave_reduce.hpp"

using namespace gfs_pose_lm;
using gfs_red::block_sum256;

namespace {

constexpr int kThreads = 256;
constexpr int kDim = 7;
constexpr int kH = kDim * (kDim + 1) / 2;  // 28: the lower triangle of H
constexpr int kSys7 = kH + kDim;           // + b
constexpr int kFirstIterations = 5, kMoreIterationsAfterRemoval = 10, kMoreIterations = 5;  // :2988, :3019-3022
constexpr int kMinCorrespondences = 10;                                                     // :3024

struct Sim3Head {
  double s12[8], cam[2][4];  // cam[0]: camera 1 (the e12 edges), cam[1]: camera 2 (the e21 edges)
  double th2, huber_delta;   // (double)th2; (double)(float)sqrt(th2)
  int fix_scale, n;          // n: pairs; edge 2 i = e12(i), 2 i + 1 = e21(i)
};
struct Sim3Out {
  double s12[8];
  int n_in, n_bad, status, its[2];
  int pad;
};

// Ordered sums: 128 edges park their 35 terms in an LDS slab, row q = quantity q with an odd row stride; lane q adds its row to its
// running value in index order.  35 x 129 doubles = 36 KB of LDS
constexpr int kChunk = 128;
constexpr int kSlabStride = kChunk + 1;
constexpr int kSlabDoubles = kSys7 * kSlabStride;
constexpr int kChiEdges = 4096;  // edges per pass of the chi2 sum
static_assert(kChiEdges <= kSlabDoubles && kThreads % kChunk == 0 && kChunk % 64 == 0, "slab passes");

// An edge as its thread keeps it: the inputs (read once) and what g2o keeps per edge (error vector, chi2), and its pair's state.
// Edge e belongs to thread e % 256: an even thread only ever holds e12 edges, an odd one e21 edges, and the two edges of a pair sit in
// neighbouring lanes
struct EdgeReg {
  double X[3], obs[2], w, err[2], chi2;
  int state;
};

// obs - cam.project(S.map(X)): Pinhole::project(Vector3d), src/CameraModels/Pinhole.cpp:35-41
__device__ __forceinline__ void project_error(const double* S, const double* X, const double* cam, const double* obs, double* r) {
  double m[3];
  gfs_sim3::sim3_map(S, X, m);
  r[0] = obs[0] - (cam[0] * m[0] / m[2] + cam[2]);
  r[1] = obs[1] - (cam[1] * m[1] / m[2] + cam[3]);
}

// computeError of an edge at S (the estimate for an e12 edge, its inverse for an e21 edge); returns its term of activeRobustChi2
__device__ __forceinline__ double edge_update(const double* S, const double* cam, bool robust, double huber_delta, EdgeReg& R) {
  project_error(S, R.X, cam, R.obs, R.err);
  R.chi2 = R.err[0] * R.w * R.err[0] + R.err[1] * R.w * R.err[1];
  double term = R.chi2, r1;
  if (robust) gfs_se3::huber(R.chi2, huber_delta, &term, &r1);
  return term;
}

// linearizeOplus (numeric) + constructQuadraticForm of one edge: its 28 + 7 terms.  P: the 14 perturbed estimates (their inverses for
// an e21 edge), [2 d] = +delta, [2 d + 1] = -delta
__device__ __forceinline__ void edge_quadratic_form(const double* P, const double* cam, const EdgeReg& R, bool robust, double huber_delta,
                                                    double (&acc)[kSys7]) {
  const double scalar = 1.0 / (2 * gfs_sim3::kNumericDelta);
  double J[2][kDim];
#pragma unroll
  for (int d = 0; d < kDim; d++) {
    double ep[2], em[2];
    project_error(P + 8 * (2 * d), R.X, cam, R.obs, ep);
    project_error(P + 8 * (2 * d + 1), R.X, cam, R.obs, em);
    J[0][d] = scalar * (ep[0] - em[0]);
    J[1][d] = scalar * (ep[1] - em[1]);
  }
  double rho1 = 1.0;
  double omega_r[2] = {-(R.w * R.err[0]), -(R.w * R.err[1])};
  if (robust) {
    double r0;
    gfs_se3::huber(R.chi2, huber_delta, &r0, &rho1);
    omega_r[0] *= rho1;
    omega_r[1] *= rho1;
  }
  const double ww = robust ? rho1 * R.w : R.w;
  int o = 0;
#pragma unroll
  for (int a = 0; a < kDim; a++) {
    acc[kH + a] = J[0][a] * omega_r[0] + J[1][a] * omega_r[1];  // b += B' omega_r
#pragma unroll
    for (int c = 0; c <= a; c++) acc[o++] = (J[0][a] * ww) * J[0][c] + (J[1][a] * ww) * J[1][c];  // A += (B' Omega) B, lower triangle
  }
}

// Phase clock of workgroup 0 (-DGFS_SIM3_OPT_TIMING; tools/bench_sim3_opt.py --loop under such a build): cycles of thread 0 between marks
#ifdef GFS_SIM3_OPT_TIMING
#define ST_INIT long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_last = clock64();
#define ST(k) { const long long _n = clock64(); st_acc[k] += _n - st_last; st_last = _n; }
#define ST_END if (tid == 0 && f == 0) printf("SIM3T setup=%lld errors=%lld chi_sum=%lld perturbed=%lld forms=%lld system_sums=%lld solve_judge=%lld checks=%lld its=%d+%d n=%d\n", st_acc[0], st_acc[1], st_acc[2], st_acc[3], st_acc[4], st_acc[5], st_acc[6], st_acc[7], O.its[0], O.its[1], n);
#else
#define ST_INIT
#define ST(k)
#define ST_END
#endif

// X [2 n][3], obs [2 n][2], w [2 n]: the edges' point, observation and information in edge order; stride: edges per problem
__global__ __launch_bounds__(kThreads) void k_sim3_opt(const Sim3Head* __restrict__ heads, const double* __restrict__ X_all,
                                                       const double* __restrict__ obs_all, const float* __restrict__ w_all, int stride,
                                                       uint8_t* __restrict__ state_all, double* __restrict__ chi2_all,
                                                       double* __restrict__ err_all, Sim3Out* __restrict__ outs) {
  __shared__ double s4[4];
  __shared__ double s_slab[kSlabDoubles];
  __shared__ double s_S[2][8], s_Sb[8];  // [0] the current estimate, [1] its inverse; the backup (push / pop)
  __shared__ double s_P[2][14 * 8];      // [0] exp(+-delta e_d) S12, [1] their inverses
  __shared__ double s_sys[kSys7];
  __shared__ double s_x[kDim];  // the solver's x: survives failed solves and both phases
  __shared__ double s_cam[2][4];
  __shared__ int s_flag[3];
  const int f = blockIdx.x, tid = threadIdx.x;
  ST_INIT
  const Sim3Head& F = heads[f];
  const int n = F.n, ne = 2 * n;
  const int fix_scale = F.fix_scale;
  const double th2 = F.th2, huber_delta = F.huber_delta;
  const int kind = tid & 1;  // 0: this thread's edges are e12 edges, 1: e21 edges
  const size_t at = (size_t)f * stride;
  const double* X = X_all + at * 3;
  const double* obs = obs_all + at * 2;
  const float* w = w_all + at;
  uint8_t* state = state_all + at;  // per edge here; the host reads the even ones
  double* chi2 = chi2_all + at;
  double* err = err_all + at * 2;
  auto load_edge = [&](int e, bool with_state) {
    EdgeReg R;
    for (int k = 0; k < 3; k++) R.X[k] = X[3 * e + k];
    for (int k = 0; k < 2; k++) {
      R.obs[k] = obs[2 * e + k];
      R.err[k] = with_state ? err[2 * e + k] : 0.0;
    }
    R.w = (double)w[e];
    R.chi2 = with_state ? chi2[e] : 0.0;
    R.state = with_state ? state[e] : GFS_SIM3_PAIR_INLIER;
    return R;
  };
  auto store_edge = [&](int e, const EdgeReg& R) {
    for (int k = 0; k < 2; k++) err[2 * e + k] = R.err[k];
    chi2[e] = R.chi2;
    state[e] = (uint8_t)R.state;
  };
  // The thread's first four edges (problems of up to 512 pairs: the usual case) live in registers for the whole solve; edges beyond
  // them go through global memory (load, pass body, store).  (clamped loads: nothing is read when there is no edge)
  const int last = ne > 0 ? ne - 1 : 0;
  EdgeReg R0{}, R1{}, R2{}, R3{};
  if (ne > 0) {
    R0 = load_edge(min(tid, last), false);
    R1 = load_edge(min(tid + kThreads, last), false);
    R2 = load_edge(min(tid + 2 * kThreads, last), false);
    R3 = load_edge(min(tid + 3 * kThreads, last), false);
  }
  auto with_edge = [&](int e, auto&& body) {  // e = tid + 256 k: k is the same in every thread of a pass
    const int k = (e - tid) / kThreads;
    if (k == 0) {
      body(R0);
    } else if (k == 1) {
      body(R1);
    } else if (k == 2) {
      body(R2);
    } else if (k == 3) {
      body(R3);
    } else {
      EdgeReg R = load_edge(e, true);
      body(R);
      store_edge(e, R);
    }
  };
  for (int e = tid + 4 * kThreads; e < ne; e += kThreads) {
    state[e] = GFS_SIM3_PAIR_INLIER;
    chi2[e] = 0;
    err[2 * e] = err[2 * e + 1] = 0;
  }
  if (tid < 8) s_S[0][tid] = F.s12[tid];
  if (tid < 8) s_cam[tid >> 2][tid & 3] = F.cam[tid >> 2][tid & 3];
  if (tid < kDim) s_x[tid] = 0.0;
  __syncthreads();
  double cam[4];
  for (int k = 0; k < 4; k++) cam[k] = s_cam[kind][k];
  Sim3Out O;
  for (int k = 0; k < 8; k++) O.s12[k] = F.s12[k];
  O.n_in = 0;
  O.n_bad = 0;
  O.status = GFS_SIM3_OPT_EARLY_RETURN;
  O.its[0] = O.its[1] = 0;
  O.pad = 0;

  // errors + chi2 of the edges still in the graph at the current estimate; returns activeRobustChi2, summed in edge order (thread 0)
  auto compute_active = [&](bool robust) {
    if (tid == 0) {  // g2o inverts the estimate inside every e21 edge: the same eight doubles each time
      double Si[8];
      gfs_sim3::sim3_inverse(s_S[0], Si);
      for (int k = 0; k < 8; k++) s_S[1][k] = Si[k];
    }
    __syncthreads();
    double S[8];
    for (int k = 0; k < 8; k++) S[k] = s_S[kind][k];
    double chi = 0;
    for (int base = 0; base < ne; base += kChiEdges) {
      const int cnt = min(kChiEdges, ne - base);
      for (int e = base + tid; e < base + cnt; e += kThreads) {
        double term = 0;  // an edge that left the graph adds nothing (x + 0 = x)
        with_edge(e, [&](EdgeReg& R) {
          if (R.state == GFS_SIM3_PAIR_INLIER) term = edge_update(S, cam, robust, huber_delta, R);
        });
        s_slab[e - base] = term;
      }
      __syncthreads();
      ST(1)
      if (tid == 0) chi = ordered_sum(s_slab, cnt, chi);
      __syncthreads();
      ST(2)
    }
    return chi;
  };

  ST(0)
  // the two optimize() calls (core/sparse_optimizer.cpp:354-419 around optimization_algorithm_levenberg.cpp:61-169), each followed by
  // its check
  int nBad = 0;
  for (int phase = 0; phase < 2; phase++) {
    const bool robust = phase == 0;  // setRobustKernel(0) on the pairs that stay (:3014-3015)
    const int its = phase == 0 ? kFirstIterations : nBad > 0 ? kMoreIterationsAfterRemoval : kMoreIterations;
    int iterations_run = 0;  // thread 0
    LmState lm{-1, 2, 0};    // thread 0 only: lambda and _ni start anew in each call
    bool fresh = false;      // uniform: the edges hold the errors at the current estimate and currentChi is their sum (see k_pose_opt)
    double currentChi = 0;   // thread 0
    // (no edge: initializeOptimization finds no vertex and optimize() returns at once)
    for (int iteration = 0; iteration < its && n > 0; iteration++) {
      if (!fresh) currentChi = compute_active(robust);
      const double iniChi = currentChi;
      // ---- buildSystem: the perturbed estimates once, then linearizeOplus + constructQuadraticForm of every edge
      if (tid < 14) {
        double add[kDim], Pp[8], Ppi[8];
#pragma unroll
        for (int d = 0; d < kDim; d++) add[d] = d != tid / 2 ? 0.0 : (tid & 1) ? -gfs_sim3::kNumericDelta : gfs_sim3::kNumericDelta;
        gfs_sim3::sim3_oplus_glibc_exp(s_S[0], add, fix_scale != 0, Pp);
        gfs_sim3::sim3_inverse(Pp, Ppi);
        for (int k = 0; k < 8; k++) {
          s_P[0][8 * tid + k] = Pp[k];
          s_P[1][8 * tid + k] = Ppi[k];
        }
      }
      __syncthreads();
      ST(3)
      {
        double run = 0;  // threads 0 .. 34: quantity tid, added up edge by edge
        for (int base = 0; base < ne; base += kThreads) {
          const int e = base + tid;
          double acc[kSys7];
#pragma unroll
          for (int k = 0; k < kSys7; k++) acc[k] = 0;
          if (e < ne) with_edge(e, [&](EdgeReg& R) {
            if (R.state == GFS_SIM3_PAIR_INLIER) edge_quadratic_form(s_P[kind], cam, R, robust, huber_delta, acc);
          });
          for (int sub = 0; sub < kThreads / kChunk && base + sub * kChunk < ne; sub++) {
            if (tid / kChunk == sub) {
#pragma unroll
              for (int k = 0; k < kSys7; k++) s_slab[k * kSlabStride + tid % kChunk] = acc[k];
            }
            __syncthreads();
            ST(4)
            if (tid < kSys7) run = ordered_sum(s_slab + tid * kSlabStride, min(kChunk, ne - base - sub * kChunk), run);
            __syncthreads();
            ST(5)
          }
        }
        if (tid < kSys7) s_sys[tid] = run;
        __syncthreads();
      }
      if (tid == 0 && iteration == 0) {  // computeLambdaInit
        lm.currentLambda = 1e-5 * max_abs_diagonal<kDim>(s_sys);
        lm.ni = 2;
        lm.nBadLm = 0;
      }
      double rho = 0;
      int qmax = 0;
      bool again = true;
      while (again) {
        if (tid == 0) {
          for (int k = 0; k < 8; k++) s_Sb[k] = s_S[0][k];  // push()
          double x[kDim], Sn[8];
          const bool ok2 = ldlt_solve_positive<kDim>(s_sys, lm.currentLambda, s_sys + kH, x);
          if (ok2)
            for (int a = 0; a < kDim; a++) s_x[a] = x[a];
          if (fix_scale) s_x[6] = 0;  // oplusImpl writes through its argument
          gfs_sim3::sim3_oplus_glibc_exp(s_Sb, s_x, fix_scale != 0, Sn);
          for (int k = 0; k < 8; k++) s_S[0][k] = Sn[k];
          s_flag[0] = ok2 ? 1 : 0;
        }
        __syncthreads();
        ST(6)
        double tempChi = compute_active(robust);
        if (tid == 0) {
          const bool ok2 = s_flag[0] != 0;
          if (!ok2) tempChi = 1.79769313486231570e308;
          rho = currentChi - tempChi;
          double scale = 0;
          for (int a = 0; a < kDim; a++) scale += s_x[a] * (lm.currentLambda * s_x[a] + s_sys[kH + a]);
          scale += 1e-3;
          rho /= scale;
          const bool accepted = rho > 0 && isfinite(tempChi);
          if (accepted) {
            double alpha = 1. - gfs_glibc::pow3(2 * rho - 1);
            alpha = fmin(alpha, 2. / 3.);
            lm.currentLambda *= fmax(1. / 3., alpha);
            lm.ni = 2;
            currentChi = tempChi;
          } else {
            lm.currentLambda *= lm.ni;
            lm.ni *= 2;
            for (int k = 0; k < 8; k++) s_S[0][k] = s_Sb[k];  // pop(): estimate restored, the edges keep the trial's errors
          }
          qmax++;
          s_flag[1] = rho < 0 && qmax < 10 ? 1 : 0;
          s_flag[2] = accepted && ok2 ? 1 : 0;
        }
        __syncthreads();
        again = s_flag[1] != 0;
        fresh = s_flag[2] != 0;
        __syncthreads();
        ST(6)
      }
      if (tid == 0) {
        iterations_run++;
        s_flag[0] = lm_stop(lm, qmax, rho, iniChi, currentChi) ? 1 : 0;
      }
      __syncthreads();
      const int stop = s_flag[0];
      __syncthreads();
      if (stop) break;
    }
    O.its[phase] = iterations_run;
    ST(6)
    if (phase == 0) {
      // ---- the first check (:2993-3016): chi2() as the solve left it, no computeError().  The pair's other edge is the neighbouring lane's
      int bad_local = 0;
      for (int base = 0; base < ne; base += kThreads) {
        const int e = base + tid;
        double mine = 0;
        if (e < ne) with_edge(e, [&](EdgeReg& R) { mine = R.chi2; });
        const double other = __shfl_xor(mine, 1, 64);
        if (e < ne) with_edge(e, [&](EdgeReg& R) {
          if (mine > th2 || other > th2) {
            R.state = GFS_SIM3_PAIR_REMOVED_FIRST;
            bad_local += kind == 0;
          }
        });
      }
      nBad = (int)block_sum256((double)bad_local, s4);
      O.n_bad = nBad;
      if (n - nBad < kMinCorrespondences) break;  // return 0, g2oS12 untouched (:3024)
    } else {
      // ---- the final check (:3032-3046): computeError() first
      if (tid == 0) {
        double Si[8];
        gfs_sim3::sim3_inverse(s_S[0], Si);
        for (int k = 0; k < 8; k++) s_S[1][k] = Si[k];
      }
      __syncthreads();
      double S[8];
      for (int k = 0; k < 8; k++) S[k] = s_S[kind][k];
      int in_local = 0;
      for (int base = 0; base < ne; base += kThreads) {
        const int e = base + tid;
        double mine = 0;
        int alive = 0;
        if (e < ne) with_edge(e, [&](EdgeReg& R) {
          alive = R.state == GFS_SIM3_PAIR_INLIER;
          if (alive) edge_update(S, cam, false, huber_delta, R);
          mine = R.chi2;
        });
        const double other = __shfl_xor(mine, 1, 64);
        if (e < ne && alive) with_edge(e, [&](EdgeReg& R) {
          if (mine > th2 || other > th2) R.state = GFS_SIM3_PAIR_REMOVED_FINAL;
          else in_local += kind == 0;
        });
      }
      O.n_in = (int)block_sum256((double)in_local, s4);
      O.status = GFS_SIM3_OPT_BOTH_PHASES;
      for (int k = 0; k < 8; k++) O.s12[k] = s_S[0][k];
    }
  }
  ST(7)
  if (tid < ne) store_edge(tid, R0);
  if (tid + kThreads < ne) store_edge(tid + kThreads, R1);
  if (tid + 2 * kThreads < ne) store_edge(tid + 2 * kThreads, R2);
  if (tid + 3 * kThreads < ne) store_edge(tid + 3 * kThreads, R3);
  if (tid == 0) outs[f] = O;
  ST_END
}

}  // namespace

struct gfs_sim3_opt {
  int device, max_batch, max_pairs;
  hipStream_t stream;
  std::mutex mu;
  // one pinned block mirroring one device block for the inputs, one for the outputs: a call is one copy in, the kernel, one copy out
  struct Layout {  // S: edges per problem
    gfs::Block<256> in, res;
    gfs::Field<Sim3Head> heads;
    gfs::Field<double, 3> X;
    gfs::Field<double, 2> obs;
    gfs::Field<float> w;
    gfs::Field<Sim3Out> out;
    gfs::Field<double> chi2;
    gfs::Field<uint8_t> state;
    Layout(size_t B, size_t S) : heads(in, B), X(in, B * S), obs(in, B * S), w(in, B * S), out(res, B), chi2(res, B * S), state(res, B * S) {}
  };
  gfs::Mirror in, res;
  gfs::DevBuf<double> d_err;
};

extern "C" {

int gfs_sim3_opt_create(int device, int max_batch, int max_pairs, gfs_sim3_opt** out) {
  GFS_REQUIRE(out && max_batch > 0 && max_pairs > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_opt_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_sim3_opt> h(new gfs_sim3_opt);
  h->device = device;
  h->max_batch = max_batch;
  h->max_pairs = max_pairs;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t Smax = gfs::align_up(2 * (size_t)max_pairs, 64);  // edges
  const gfs_sim3_opt::Layout L{(size_t)max_batch, Smax};
  int rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->d_err.alloc(Smax * max_batch * 2);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_sim3_opt_destroy(gfs_sim3_opt* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_sim3_optimize(gfs_sim3_opt* h, const gfs_sim3_opt_problem* problems, int B, gfs_sim3_opt_solution* solutions) {
  GFS_REQUIRE(h && problems && solutions && B > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_optimize: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_sim3_optimize: batch %d exceeds capacity %d", B, h->max_batch);
  // every refusal before anything is staged
  int S = 64;  // stride of the per-problem arrays in this call, in edges
  for (int f = 0; f < B; f++) {
    const gfs_sim3_opt_problem& p = problems[f];
    GFS_REQUIRE(p.n_pairs >= 0, GFS_ERR_INVALID_ARG, "gfs_sim3_optimize: problem %d has n_pairs = %d", f, p.n_pairs);
    GFS_REQUIRE(p.n_pairs <= h->max_pairs, GFS_ERR_CAPACITY, "gfs_sim3_optimize: problem %d has %d pairs (capacity %d)", f, p.n_pairs,
                h->max_pairs);
    GFS_REQUIRE(std::isfinite(p.th2) && p.th2 > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_optimize: problem %d: th2 must be finite and > 0", f);
    GFS_REQUIRE(p.n_pairs == 0 || (p.x1c && p.x2c && p.obs1 && p.obs2 && p.inv_sigma2_1 && p.inv_sigma2_2), GFS_ERR_INVALID_ARG,
                "gfs_sim3_optimize: problem %d has NULL pair arrays", f);
    GFS_REQUIRE(p.n_pairs == 0 || solutions[f].pair_state, GFS_ERR_INVALID_ARG, "gfs_sim3_optimize: problem %d has a NULL pair_state", f);
    S = std::max(S, (int)gfs::align_up(2 * (size_t)p.n_pairs, 64));
  }
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_sim3_opt::Layout L{(size_t)B, (size_t)S};
  uint8_t* hi = h->in.h.p;
  for (int f = 0; f < B; f++) {
    const gfs_sim3_opt_problem& p = problems[f];
    Sim3Head& F = L.heads.at(hi)[f];
    for (int k = 0; k < 8; k++) F.s12[k] = p.s12[k];
    for (int k = 0; k < 4; k++) {
      F.cam[0][k] = p.cam1[k];
      F.cam[1][k] = p.cam2[k];
    }
    F.th2 = (double)p.th2;
    F.huber_delta = (double)sqrtf(p.th2);  // const float deltaHuber = sqrt(th2) (:2843)
    F.fix_scale = p.fix_scale != 0;
    F.n = p.n_pairs;
    // the edges in the order the reference adds them: e12(i) against x2c, obs1; e21(i) against x1c, obs2
    double* X = L.X.at(hi, (size_t)f * S);
    double* ob = L.obs.at(hi, (size_t)f * S);
    float* w = L.w.at(hi, (size_t)f * S);
    for (int i = 0; i < p.n_pairs; i++) {
      for (int k = 0; k < 3; k++) {
        X[6 * i + k] = p.x2c[3 * i + k];
        X[6 * i + 3 + k] = p.x1c[3 * i + k];
      }
      for (int k = 0; k < 2; k++) {
        ob[4 * i + k] = p.obs1[2 * i + k];
        ob[4 * i + 2 + k] = p.obs2[2 * i + k];
      }
      w[2 * i] = p.inv_sigma2_1[i];
      w[2 * i + 1] = p.inv_sigma2_2[i];
    }
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  uint8_t* dr = h->res.d.p;
  GFS_LAUNCH("k_sim3_opt", k_sim3_opt, dim3(B), dim3(kThreads), 0, s, L.heads.at(di), L.X.at(di), L.obs.at(di), L.w.at(di), S,
             L.state.at(dr), L.chi2.at(dr), h->d_err.p, L.out.at(dr));
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  for (int f = 0; f < B; f++) {
    const Sim3Out& O = L.out.at(hr)[f];
    gfs_sim3_opt_solution& r = solutions[f];
    const size_t n = (size_t)problems[f].n_pairs;
    const uint8_t* st = L.state.at(hr, (size_t)f * S);  // per edge, the same for both edges of a pair
    for (size_t i = 0; i < n; i++) r.pair_state[i] = st[2 * i];
    if (r.chi2) L.chi2.get(r.chi2, hr, (size_t)f * S, 2 * n);
    for (int k = 0; k < 8; k++) r.s12[k] = O.s12[k];
    r.n_in = O.n_in;
    r.n_bad = O.n_bad;
    r.status = O.status;
    r.iterations_run[0] = O.its[0];
    r.iterations_run[1] = O.its[1];
  }
  return GFS_OK;
}

}  // extern "C"
