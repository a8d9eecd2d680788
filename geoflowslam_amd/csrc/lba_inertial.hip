// Optimizer::LocalInertialBA's numeric core (reference src/Optimizer.cc:3589-3626) on MI355X: one Levenberg optimize() over the N
// window key frames (15 unknowns each), the marginalised map points and the chain of inertial edges (include/gfs_abi.h section 20).
//
// The rule -- every formula, every sum's order, the Levenberg state machine, the quirks kept and the written rules -- is
// lba_inertial_rule.hpp's, shared with the sequential restatement (tests/host/lba_inertial_restatement.cpp), whose bytes every output
// has.  This file holds only who computes what.  The whole schedule is queued at once: `iterations` build groups and ten trial groups
// after each; the state machine (Ctl) lives in device memory, k_li_decide makes the trial's decision there, and every kernel of a
// group that has nothing to do (the iteration was closed by an accepted trial, the solve has terminated) returns at once.  The host
// waits once, for the results.
//   build group   k_li_small<false>  the 3 N small edges, a workgroup a set: linearisation on a lane each, J' Omega over the threads
//                 k_li_vis           a lane a landmark: its edges in order -> Hll, bl, per edge Hpl and the 27 pose-block terms, chi2
//                 k_li_posesum       a wave a key frame: the 27 pose-block sums, the small edges' share first, then its edges in order
//                 k_li_begin         one lane: the robust chi2 total, lm_begin_iteration
//   trial group   k_li_inv           a lane a landmark: (Hll + lambda I)^-1, per edge Hpl Inv and its share of the right-hand side
//                 k_li_assemble      a lane an entry of the reduced system: the base value, then its Schur terms in list order
//                 k_li_solve         one workgroup: the dense LDL' (rule D) in LDS up to kLdsRows rows, in HBM / L2 above
//                 k_li_update        a lane a key frame: the trial state; one lane: the poses' share of computeScale
//                 k_li_small<true>   the small edges' errors at the trial state
//                 k_li_back          a lane a landmark: its step, the trial point, its share of computeScale, its edges' chi2
//                 k_li_decide        one workgroup: the totals, lm_trial, the accepted state copied over the current one
//   k_li_final    a lane a landmark: isDepthPositive and the erase verdict of its edges, the points; one workgroup: the key frames
// Sums over landmarks go through the fixed pairwise tree of kChunk = 256 partials (chunk_tree), one workgroup a chunk.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "gfs_common.hpp"
#include "lba_inertial_rule.hpp"
#include "staging.hpp"

using namespace gfs_li;

namespace {

constexpr int kThreads = kChunk;     // landmark kernels: one workgroup is one chunk of the chi2 / scale sums
constexpr int kSolveThreads = 512;   // a lane a row of the reduced system
constexpr int kMaxOpt = kSolveThreads / 15;
constexpr int kInFlight = 8;         // terms of an ordered sum fetched together; they are still added one by one, in order

struct OutScalars {
  float err, err_end;
  int iterations_run, trials_run;
  double final_lambda;
};

struct Dev {
  int N, F, P, E, D, K, n_chunks, pad;
  Calib cam;
  const Set* sets;
  State *st_cur, *st_trial;        // [N + 1]: index N is the fixed key frame in front of the window
  double *cam_cur, *cam_trial;     // [K][12] Rcw, tcw by key-frame index
  double *pts_cur, *pts_trial;     // [P][3]
  const int32_t *pt_begin, *edge_kf;
  const double* obs;
  const float* w;
  const uint8_t *stereo, *close;
  const int32_t *pose_begin, *pose_edges;  // a key frame's edges, ascending
  const int32_t *blk_begin, *contrib;      // per block tri(i, j) of the reduced system: its (e1, e2) in landmark-then-edge order
  SetEdges *se, *se_trial;
  double *echi2, *Hll, *bl, *Hpl, *T, *vis, *Y, *inv, *bfull, *M, *bs, *x;
  double *chi_chunk, *chi_chunk_trial, *scale_chunk;
  Ctl* ctl;
  gfs_imu_state* out_window;
  double *out_points, *out_chi2;
  uint8_t *out_dp, *out_erase;
  OutScalars* out;
};

__device__ __forceinline__ double tree256(double v, double* s) {  // chunk_tree over the workgroup's 256 partials
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int h = kChunk / 2; h >= 1; h >>= 1) {
    if (tid < h) s[tid] += s[tid + h];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreads) void k_li_init(Dev D, double lambda_init) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    lm_init(*D.ctl, lambda_init);
    D.st_trial[D.N] = D.st_cur[D.N];
  }
  for (int k = tid; k < 12 * D.K; k += kThreads) D.cam_trial[k] = D.cam_cur[k];
}

template <bool TRIAL>
__global__ __launch_bounds__(kThreads) void k_li_small(Dev D) {
  const Ctl& c = *D.ctl;
  if (TRIAL ? !c.iter_open : c.done) return;
  const int s = blockIdx.x, tid = threadIdx.x;
  const State* st = TRIAL ? D.st_trial : D.st_cur;
  SetEdges& E = (TRIAL ? D.se_trial : D.se)[s];
  if (tid == 0) set_inertial(D.sets[s], st[s + 1], st[s], E, !TRIAL);
  if (tid == 64) set_walks(D.sets[s], st[s + 1], st[s], E, !TRIAL);
  if (TRIAL) return;
  __syncthreads();
  for (int idx = tid; idx < kSetAtO; idx += kThreads) set_AtO_entry(E, idx);
}

__global__ __launch_bounds__(kThreads) void k_li_vis(Dev D) {
  __shared__ double s_tree[kChunk];
  if (D.ctl->done) return;
  const int l = blockIdx.x * kThreads + threadIdx.x;
  double part = 0.0;
  if (l < D.P) {
    double hl[9];
#pragma unroll
    for (int k = 0; k < 9; k++) hl[k] = 0.0;
    double xw[3];
    for (int k = 0; k < 3; k++) xw[k] = D.pts_cur[3 * (size_t)l + k];
    for (int e = D.pt_begin[l]; e < D.pt_begin[l + 1]; e++) {
      const int kf = D.edge_kf[e];
      const bool stv = D.stereo[e] != 0;
      const double w = (double)D.w[e];
      double Rcw[9], tcw[3], ob[3];
      for (int k = 0; k < 9; k++) Rcw[k] = D.cam_cur[12 * (size_t)kf + k];
      for (int k = 0; k < 3; k++) tcw[k] = D.cam_cur[12 * (size_t)kf + 9 + k], ob[k] = D.obs[3 * (size_t)e + k];
      double er[3], rho0, rho1;
      vis_error(D.cam, Rcw, tcw, xw, ob, stv, er);
      const double c2 = vis_chi2(er, w, stv);
      huber(c2, huber_delta_visual(stv), &rho0, &rho1);
      D.echi2[e] = c2;
      part += rho0;
      double Jl[9], t9[9];
      vis_point_jacobian(D.cam, Rcw, tcw, xw, stv, Jl);
      vis_point_form(Jl, w, stv, rho1, er, t9);
#pragma unroll
      for (int k = 0; k < 9; k++) hl[k] += t9[k];
      if (kf < D.N) {
        double Jp[18], acc[kSys], H18[18];
        vis_jacobian(D.cam, Rcw, tcw, xw, stv, Jp);
        vis_quadratic_form(Jp, w, stv, rho1, er, acc);
        vis_hpl(Jp, Jl, w, stv, rho1, H18);
#pragma unroll
        for (int k = 0; k < kSys; k++) D.T[27 * (size_t)e + k] = acc[k];
#pragma unroll
        for (int k = 0; k < 18; k++) D.Hpl[18 * (size_t)e + k] = H18[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) D.Hll[6 * (size_t)l + k] = hl[k];
#pragma unroll
    for (int k = 0; k < 3; k++) D.bl[3 * (size_t)l + k] = hl[6 + k];
  }
  const double sum = tree256(part, s_tree);
  if (threadIdx.x == 0) D.chi_chunk[blockIdx.x] = sum;
}

__global__ __launch_bounds__(64) void k_li_posesum(Dev D) {
  if (D.ctl->done) return;
  const int i = blockIdx.x, q = threadIdx.x;
  if (q >= kSys) return;
  double run = pose_block_start(D.N, D.se, i, q);
  const int end = D.pose_begin[i + 1];
  int k = D.pose_begin[i];
  for (; k + kInFlight <= end; k += kInFlight) {  // (as a plain loop every term waits for two dependent loads)
    double t[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; u++) t[u] = D.T[27 * (size_t)D.pose_edges[k + u] + q];
#pragma unroll
    for (int u = 0; u < kInFlight; u++) run += t[u];
  }
  for (; k < end; k++) run += D.T[27 * (size_t)D.pose_edges[k] + q];
  D.vis[27 * i + q] = run;
}

__global__ __launch_bounds__(64) void k_li_begin(Dev D, int open) {
  Ctl& c = *D.ctl;
  if (c.done || threadIdx.x != 0) return;
  double total = 0.0;
  for (int s = 0; s < D.N; s++)
    for (int k = 0; k < 3; k++) total += D.se[s].chi[k];
  for (int b = 0; b < D.n_chunks; b++) total += D.chi_chunk[b];
  lm_begin_iteration(c, total, open != 0);
}

__global__ __launch_bounds__(kThreads) void k_li_inv(Dev D) {
  const Ctl& c = *D.ctl;
  if (!c.iter_open) return;
  const int l = blockIdx.x * kThreads + threadIdx.x;
  if (l >= D.P) return;
  double h[6], inv[9], b3[3];
  for (int k = 0; k < 6; k++) h[k] = D.Hll[6 * (size_t)l + k];
  for (int k = 0; k < 3; k++) b3[k] = D.bl[3 * (size_t)l + k];
  inverse3(h, c.lambda, inv);
  for (int k = 0; k < 9; k++) D.inv[9 * (size_t)l + k] = inv[k];
  for (int e = D.pt_begin[l]; e < D.pt_begin[l + 1]; e++)
    if (D.edge_kf[e] < D.N) vis_y(D.Hpl + 18 * (size_t)e, inv, b3, D.Y + 24 * (size_t)e);
}

__global__ __launch_bounds__(kThreads) void k_li_assemble(Dev D) {
  const Ctl& c = *D.ctl;
  if (!c.iter_open) return;
  const int idx = blockIdx.x * kThreads + threadIdx.x, n = D.D;
  if (idx >= n * (n + 1)) return;
  const int R = idx / (n + 1), C = idx % (n + 1);
  const int iR = R / 15, r = R % 15;
  if (C == n) {  // the right-hand side
    double v = rhs_base(D.N, D.se, D.vis, R);
    D.bfull[R] = v;
    if (r < 6) {
      const int end = D.pose_begin[iR + 1];
      int k = D.pose_begin[iR];
      for (; k + kInFlight <= end; k += kInFlight) {
        double t[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; u++) t[u] = D.Y[24 * (size_t)D.pose_edges[k + u] + 18 + r];
#pragma unroll
        for (int u = 0; u < kInFlight; u++) v -= t[u];
      }
      for (; k < end; k++) v -= D.Y[24 * (size_t)D.pose_edges[k] + 18 + r];
    }
    D.bs[R] = v;
    return;
  }
  if (C > R) return;
  const int iC = C / 15, cc = C % 15;
  double v = system_base(D.N, D.se, D.vis, R, C);
  if (R == C) v += c.lambda;
  if (r < 6 && cc < 6) {
    const int blk = (int)tri(iR, iC), end = D.blk_begin[blk + 1];
    auto term = [&](int k) { return schur_term(D.Y + 24 * (size_t)D.contrib[2 * (size_t)k], D.Hpl + 18 * (size_t)D.contrib[2 * (size_t)k + 1], r, cc); };
    int k = D.blk_begin[blk];
    for (; k + kInFlight <= end; k += kInFlight) {
      double t[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; u++) t[u] = term(k + u);
#pragma unroll
      for (int u = 0; u < kInFlight; u++) v -= t[u];
    }
    for (; k < end; k++) v -= term(k);
  }
  D.M[tri(R, C)] = v;
}

// rule D by one workgroup, a lane a row.  LDS: the packed triangle is copied into LDS and factored there; else in place in HBM / L2
template <bool LDS>
__global__ __launch_bounds__(kSolveThreads) void k_li_solve(Dev D) {
  extern __shared__ __align__(16) double lds[];
  __shared__ double s_temp[kSolveThreads], s_y[kSolveThreads];
  __shared__ int s_ok;
  Ctl& c = *D.ctl;
  if (!c.iter_open) return;
  const int tid = threadIdx.x, n = D.D;
  double* A = LDS ? lds : D.M;
  if (LDS)
    for (int k = tid; k < (int)tri(n, 0); k += kSolveThreads) lds[k] = D.M[k];
  if (tid == 0) s_ok = 1;
  __syncthreads();
  for (int k = 0; k < n; k++) {
    if (tid < k) ldlt_temp(A, k, tid, s_temp);
    __syncthreads();
    if (tid >= k && tid < n) ldlt_row_packed(A, k, tid, s_temp);
    __syncthreads();
    const double d = A[tri(k, k)];
    if (!pivot_ok(d)) {  // uniform: every lane reads the same pivot
      if (tid == 0) s_ok = 0;
      break;
    }
    if (tid > k && tid < n) A[tri(tid, k)] /= d;
    __syncthreads();
  }
  __syncthreads();
  const bool ok = s_ok != 0;
  if (ok) {
    if (tid < n) s_y[tid] = D.bs[tid];
    for (int j = 0; j < n; j++) {
      __syncthreads();
      if (tid > j && tid < n) ldlt_forward(A, j, tid, s_y);
    }
    __syncthreads();
    if (tid < n) s_y[tid] /= A[tri(tid, tid)];
    for (int j = n - 1; j >= 0; j--) {
      __syncthreads();
      if (tid < j) ldlt_backward(A, j, tid, s_y);
    }
    __syncthreads();
  }
  if (tid < n) D.x[tid] = ok ? s_y[tid] : 0.0;  // rule F
  if (tid == 0) c.ok2 = ok ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_li_update(Dev D) {
  Ctl& c = *D.ctl;
  if (!c.iter_open) return;
  const int tid = threadIdx.x;
  if (tid < D.N) {
    State s = D.st_cur[tid];
    keyframe_update(s, D.cam, D.x + 15 * tid);
    D.st_trial[tid] = s;
    for (int k = 0; k < 9; k++) D.cam_trial[12 * tid + k] = s.Rcw[k];
    for (int k = 0; k < 3; k++) D.cam_trial[12 * tid + 9 + k] = s.tcw[k];
  }
  if (tid == 63) {  // the poses' share of computeScale
    double sc = 0.0;
    for (int j = 0; j < D.D; j++) sc += D.x[j] * (c.lambda * D.x[j] + D.bfull[j]);
    c.scale_pose = sc;
  }
}

__global__ __launch_bounds__(kThreads) void k_li_back(Dev D) {
  __shared__ double s_tree[kChunk];
  const Ctl& c = *D.ctl;
  if (!c.iter_open) return;
  const int l = blockIdx.x * kThreads + threadIdx.x;
  double part_scale = 0.0, part_chi = 0.0;
  if (l < D.P) {
    double b3[3], c3[3], d3[3] = {0.0, 0.0, 0.0}, xw[3];
    for (int k = 0; k < 3; k++) b3[k] = c3[k] = D.bl[3 * (size_t)l + k];
    if (c.ok2) {
      double inv[9];
      for (int k = 0; k < 9; k++) inv[k] = D.inv[9 * (size_t)l + k];
      for (int e = D.pt_begin[l]; e < D.pt_begin[l + 1]; e++)
        if (D.edge_kf[e] < D.N) back_edge(D.Hpl + 18 * (size_t)e, D.x + 15 * (size_t)D.edge_kf[e], c3);
      mv3(inv, c3, d3);
    }
    for (int k = 0; k < 3; k++) {
      xw[k] = D.pts_cur[3 * (size_t)l + k] + d3[k];
      D.pts_trial[3 * (size_t)l + k] = xw[k];
      part_scale += d3[k] * (c.lambda * d3[k] + b3[k]);
    }
    for (int e = D.pt_begin[l]; e < D.pt_begin[l + 1]; e++) {
      const int kf = D.edge_kf[e];
      const bool stv = D.stereo[e] != 0;
      double Rcw[9], tcw[3], ob[3], er[3], rho0, rho1;
      for (int k = 0; k < 9; k++) Rcw[k] = D.cam_trial[12 * (size_t)kf + k];
      for (int k = 0; k < 3; k++) tcw[k] = D.cam_trial[12 * (size_t)kf + 9 + k], ob[k] = D.obs[3 * (size_t)e + k];
      vis_error(D.cam, Rcw, tcw, xw, ob, stv, er);
      const double c2 = vis_chi2(er, (double)D.w[e], stv);
      huber(c2, huber_delta_visual(stv), &rho0, &rho1);
      D.echi2[e] = c2;
      part_chi += rho0;
    }
  }
  const double ss = tree256(part_scale, s_tree), sc = tree256(part_chi, s_tree);
  if (threadIdx.x == 0) D.scale_chunk[blockIdx.x] = ss, D.chi_chunk_trial[blockIdx.x] = sc;
}

__global__ __launch_bounds__(kThreads) void k_li_decide(Dev D) {
  __shared__ int s_acc;
  Ctl& c = *D.ctl;
  if (!c.iter_open) return;
  __syncthreads();  // (every lane has read iter_open before lane 0 may clear it)
  const int tid = threadIdx.x;
  if (tid == 0) {
    double temp = 0.0, scale = c.scale_pose;
    for (int s = 0; s < D.N; s++)
      for (int k = 0; k < 3; k++) temp += D.se_trial[s].chi[k];
    for (int b = 0; b < D.n_chunks; b++) temp += D.chi_chunk_trial[b], scale += D.scale_chunk[b];
    s_acc = lm_trial(c, temp, scale) ? 1 : 0;
  }
  __syncthreads();
  if (!s_acc) return;
  for (int k = tid; k < 3 * D.P; k += kThreads) D.pts_cur[k] = D.pts_trial[k];
  for (int k = tid; k < 12 * D.N; k += kThreads) D.cam_cur[k] = D.cam_trial[k];
  if (tid < D.N) D.st_cur[tid] = D.st_trial[tid];
}

__global__ __launch_bounds__(kThreads) void k_li_final(Dev D) {
  const int tid = threadIdx.x, l = blockIdx.x * kThreads + tid;
  if (blockIdx.x == 0) {
    if (tid < D.N) {
      const State& s = D.st_cur[tid];
      gfs_imu_state& o = D.out_window[tid];
      for (int k = 0; k < 9; k++) o.Rwb[k] = s.Rwb[k], o.Rcw[k] = s.Rcw[k];
      for (int k = 0; k < 3; k++) o.twb[k] = s.twb[k], o.tcw[k] = s.tcw[k], o.v[k] = s.v[k], o.bg[k] = s.bg[k], o.ba[k] = s.ba[k];
    }
    if (tid == 64) {
      const Ctl& c = *D.ctl;
      D.out->err = (float)c.first_total, D.out->err_end = (float)c.last_total;
      D.out->iterations_run = c.iterations_run, D.out->trials_run = c.trials_run, D.out->final_lambda = c.lambda;
    }
  }
  if (l >= D.P) return;
  double xw[3];
  for (int k = 0; k < 3; k++) xw[k] = D.out_points[3 * (size_t)l + k] = D.pts_cur[3 * (size_t)l + k];
  for (int e = D.pt_begin[l]; e < D.pt_begin[l + 1]; e++) {
    const double* cm = D.cam_cur + 12 * (size_t)D.edge_kf[e];
    const bool dp = vis_depth_positive(cm, cm + 9, xw);
    const double c2 = D.echi2[e];
    D.out_chi2[e] = c2;
    D.out_dp[e] = dp ? 1 : 0;
    D.out_erase[e] = (D.stereo[e] ? erase_stereo(c2) : erase_mono(c2, D.close[e] != 0, dp)) ? 1 : 0;
  }
}

// The dynamic-LDS ceiling of a kernel is one global setting per function: set once per device to what kLdsRows rows need
int raise_lds_limit(int device) {
  static std::mutex mu;
  static bool done[64] = {};
  std::lock_guard<std::mutex> lk(mu);
  if (device >= 0 && device < 64 && done[device]) return GFS_OK;
  GFS_HIP(hipFuncSetAttribute((const void*)k_li_solve<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(tri(kLdsRows, 0) * sizeof(double))));
  if (device >= 0 && device < 64) done[device] = true;
  return GFS_OK;
}

}  // namespace

struct gfs_lba_inertial {
  int device, max_opt, max_fixed, max_points, max_edges;
  size_t max_pairs;
  hipStream_t stream;
  std::mutex mu;
  // what a call uploads (the states and points are the solve's current state: it works on them in place), what it works in, and
  // what it downloads
  struct Layout {
    gfs::Block<256> in, work, res;
    gfs::Field<Set> sets;
    gfs::Field<State> st_cur;
    gfs::Field<double, 12> cam_cur;
    gfs::Field<double, 3> pts_cur, obs;
    gfs::Field<int32_t> pt_begin, edge_kf, pose_begin, pose_edges, blk_begin;
    gfs::Field<int32_t, 2> contrib;
    gfs::Field<float> w;
    gfs::Field<uint8_t> stereo, close;
    gfs::Field<State> st_trial;
    gfs::Field<double, 12> cam_trial;
    gfs::Field<double, 3> pts_trial;
    gfs::Field<SetEdges> se, se_trial;
    gfs::Field<double> echi2, Hll, bl, Hpl, T, vis, Y, inv, bfull, M, bs, x, chi_chunk, chi_chunk_trial, scale_chunk;
    gfs::Field<Ctl> ctl;
    gfs::Field<gfs_imu_state> out_window;
    gfs::Field<double, 3> out_points;
    gfs::Field<double> out_chi2;
    gfs::Field<uint8_t> out_dp, out_erase;
    gfs::Field<OutScalars> out;
    Layout(size_t N, size_t F, size_t P, size_t E, size_t pairs)
        : sets(in, N), st_cur(in, N + 1), cam_cur(in, N + 1 + F), pts_cur(in, P), obs(in, E), pt_begin(in, P + 1), edge_kf(in, E),
          pose_begin(in, N + 1), pose_edges(in, E), blk_begin(in, (size_t)tri(N, 0) + 1), contrib(in, pairs), w(in, E), stereo(in, E),
          close(in, E), st_trial(work, N + 1), cam_trial(work, N + 1 + F), pts_trial(work, P), se(work, N), se_trial(work, N),
          echi2(work, E), Hll(work, 6 * P), bl(work, 3 * P), Hpl(work, 18 * E), T(work, 27 * E), vis(work, 27 * N), Y(work, 24 * E),
          inv(work, 9 * P), bfull(work, 15 * N), M(work, (size_t)tri(15 * N, 0)), bs(work, 15 * N), x(work, 15 * N),
          chi_chunk(work, P / kChunk + 1), chi_chunk_trial(work, P / kChunk + 1), scale_chunk(work, P / kChunk + 1), ctl(work, 1),
          out_window(res, N), out_points(res, P), out_chi2(res, E), out_dp(res, E), out_erase(res, E), out(res, 1) {}
  };
  gfs::Mirror in, res;
  gfs::DevBuf<uint8_t> work;
};

extern "C" {

int gfs_lba_inertial_create(int device, int max_opt, int max_fixed, int max_points, int max_edges, gfs_lba_inertial** out) {
  GFS_REQUIRE(out && max_opt > 0 && max_opt <= kMaxOpt && max_fixed >= 0 && max_points > 0 && max_edges > 0, GFS_ERR_INVALID_ARG,
              "gfs_lba_inertial_create: invalid argument (max_opt 1..%d)", kMaxOpt);
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  if (int rc = raise_lds_limit(device)) return rc;
  std::unique_ptr<gfs_lba_inertial> h(new gfs_lba_inertial);
  h->device = device, h->max_opt = max_opt, h->max_fixed = max_fixed, h->max_points = max_points, h->max_edges = max_edges;
  h->max_pairs = (size_t)max_edges * (size_t)max_opt;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const gfs_lba_inertial::Layout L{(size_t)max_opt, (size_t)max_fixed, (size_t)max_points, (size_t)max_edges, h->max_pairs};
  int rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->work.alloc(L.work.bytes());
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_lba_inertial_destroy(gfs_lba_inertial* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_lba_inertial_solve(gfs_lba_inertial* h, const gfs_lba_inertial_problem* pp, gfs_lba_inertial_solution* sol) {
  GFS_REQUIRE(h && pp && sol, GFS_ERR_INVALID_ARG, "gfs_lba_inertial_solve: invalid argument");
  const gfs_lba_inertial_problem& p = *pp;
  const int N = p.n_opt, F = p.n_fixed, P = p.n_points, E = p.n_edges;
  // every refusal before anything is staged
  GFS_REQUIRE(N >= 1 && F >= 0 && P >= 0 && E >= 0 && p.iterations >= 0, GFS_ERR_INVALID_ARG,
              "gfs_lba_inertial_solve: n_opt = %d, n_fixed = %d, n_points = %d, n_edges = %d, iterations = %d", N, F, P, E, p.iterations);
  GFS_REQUIRE(N <= h->max_opt && F <= h->max_fixed && P <= h->max_points && E <= h->max_edges, GFS_ERR_CAPACITY,
              "gfs_lba_inertial_solve: window %d + %d key frames, %d points, %d edges exceeds capacity %d + %d, %d, %d", N, F, P, E, h->max_opt,
              h->max_fixed, h->max_points, h->max_edges);
  GFS_REQUIRE(p.window && p.window_imu && p.inertial && p.point_edge_begin && (F == 0 || (p.fixed_Rcw && p.fixed_tcw)) && (P == 0 || p.points) &&
                  (E == 0 || (p.edge_kf && p.obs && p.inv_sigma2 && p.stereo && p.close)),
              GFS_ERR_INVALID_ARG, "gfs_lba_inertial_solve: a required array of the problem is NULL");
  GFS_REQUIRE(sol->window && (P == 0 || sol->points) && (E == 0 || (sol->edge_chi2 && sol->edge_depth_positive && sol->edge_erase)),
              GFS_ERR_INVALID_ARG, "gfs_lba_inertial_solve: a required array of the solution is NULL");
  GFS_REQUIRE(p.point_edge_begin[0] == 0 && p.point_edge_begin[P] == E, GFS_ERR_INVALID_ARG,
              "gfs_lba_inertial_solve: point_edge_begin runs from %d to %d, not from 0 to n_edges = %d", p.point_edge_begin[0], p.point_edge_begin[P], E);
  for (int l = 0; l < P; l++)
    GFS_REQUIRE(p.point_edge_begin[l] <= p.point_edge_begin[l + 1], GFS_ERR_INVALID_ARG, "gfs_lba_inertial_solve: point_edge_begin descends at %d", l);
  const int K = N + 1 + F;
  for (int e = 0; e < E; e++)
    GFS_REQUIRE(p.edge_kf[e] >= 0 && p.edge_kf[e] < K, GFS_ERR_INVALID_ARG, "gfs_lba_inertial_solve: edge %d names key frame %d of %d", e, p.edge_kf[e], K);
  GFS_REQUIRE(p.n_cameras == 1, GFS_ERR_UNSUPPORTED, "gfs_lba_inertial_solve: %d cameras (only one is implemented)", p.n_cameras);
  for (int i = 0; i < N; i++)
    GFS_REQUIRE(p.window_imu[i] != 0, GFS_ERR_UNSUPPORTED, "gfs_lba_inertial_solve: window key frame %d has no IMU (bImu false)", i);
  // the lists of the reduced system (gba_lists.hpp's order): per block its (e1, e2), per key frame its edges
  std::vector<int64_t> blk_count((size_t)tri(N, 0) + 1, 0);
  std::vector<int32_t> pose_count((size_t)N + 1, 0);
  auto for_each_pair = [&](auto&& f) {
    for (int l = 0; l < P; l++)
      for (int e1 = p.point_edge_begin[l]; e1 < p.point_edge_begin[l + 1]; e1++) {
        const int i = p.edge_kf[e1];
        if (i >= N) continue;
        for (int e2 = p.point_edge_begin[l]; e2 < p.point_edge_begin[l + 1]; e2++) {
          const int j = p.edge_kf[e2];
          if (j <= i) f((size_t)tri(i, j), e1, e2);
        }
      }
  };
  for_each_pair([&](size_t b, int, int) { blk_count[b + 1]++; });
  for (size_t b = 0; b + 1 < blk_count.size(); b++) blk_count[b + 1] += blk_count[b];
  const int64_t pairs = blk_count.back();
  GFS_REQUIRE((uint64_t)pairs <= h->max_pairs, GFS_ERR_CAPACITY, "gfs_lba_inertial_solve: %lld Schur pairs exceed capacity %zu", (long long)pairs,
              h->max_pairs);

  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_lba_inertial::Layout L{(size_t)N, (size_t)F, (size_t)P, (size_t)E, (size_t)pairs};
  uint8_t* hi = h->in.h.p;
  Dev D;
  memset(&D, 0, sizeof(D));
  D.N = N, D.F = F, D.P = P, D.E = E, D.D = 15 * N, D.K = K, D.n_chunks = gfs::div_up(P, kChunk);
  fill_calib(p, D.cam);
  for (int i = 0; i < N; i++) {
    fill_set(p.inertial[i], i == N - 1, L.sets.at(hi)[i]);
    fill_state(p.window[i], L.st_cur.at(hi)[i]);
  }
  fill_state(p.prev, L.st_cur.at(hi)[N]);
  for (int k = 0; k < K; k++) {
    double* cm = L.cam_cur.at(hi, k);
    const double* Rcw = k <= N ? L.st_cur.at(hi)[k].Rcw : p.fixed_Rcw + 9 * (size_t)(k - N - 1);
    const double* tcw = k <= N ? L.st_cur.at(hi)[k].tcw : p.fixed_tcw + 3 * (size_t)(k - N - 1);
    memcpy(cm, Rcw, 9 * sizeof(double)), memcpy(cm + 9, tcw, 3 * sizeof(double));
  }
  L.pts_cur.put(hi, 0, p.points, P);
  L.obs.put(hi, 0, p.obs, E);
  L.pt_begin.put(hi, 0, p.point_edge_begin, (size_t)P + 1);
  L.edge_kf.put(hi, 0, p.edge_kf, E);
  L.w.put(hi, 0, p.inv_sigma2, E);
  L.stereo.put(hi, 0, p.stereo, E);
  L.close.put(hi, 0, p.close, E);
  {
    int32_t* bb = L.blk_begin.at(hi);
    for (size_t b = 0; b < blk_count.size(); b++) bb[b] = (int32_t)blk_count[b];
    std::vector<int64_t> at(blk_count.begin(), blk_count.end() - 1);
    int32_t* cb = L.contrib.at(hi);
    for_each_pair([&](size_t b, int e1, int e2) {
      const int64_t k = at[b]++;
      cb[2 * k] = e1, cb[2 * k + 1] = e2;
    });
    for (int e = 0; e < E; e++)
      if (p.edge_kf[e] < N) pose_count[(size_t)p.edge_kf[e] + 1]++;
    for (int i = 0; i < N; i++) pose_count[(size_t)i + 1] += pose_count[(size_t)i];
    L.pose_begin.put(hi, 0, pose_count.data(), (size_t)N + 1);
    std::vector<int32_t> pos(pose_count.begin(), pose_count.end() - 1);
    int32_t* pe = L.pose_edges.at(hi);
    for (int e = 0; e < E; e++)
      if (p.edge_kf[e] < N) pe[pos[(size_t)p.edge_kf[e]]++] = e;
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  uint8_t *di = h->in.d.p, *dw = h->work.p, *dr = h->res.d.p;
  D.sets = L.sets.at(di), D.st_cur = L.st_cur.at(di), D.cam_cur = L.cam_cur.at(di), D.pts_cur = L.pts_cur.at(di), D.obs = L.obs.at(di);
  D.pt_begin = L.pt_begin.at(di), D.edge_kf = L.edge_kf.at(di), D.pose_begin = L.pose_begin.at(di), D.pose_edges = L.pose_edges.at(di);
  D.blk_begin = L.blk_begin.at(di), D.contrib = L.contrib.at(di), D.w = L.w.at(di), D.stereo = L.stereo.at(di), D.close = L.close.at(di);
  D.st_trial = L.st_trial.at(dw), D.cam_trial = L.cam_trial.at(dw), D.pts_trial = L.pts_trial.at(dw), D.se = L.se.at(dw), D.se_trial = L.se_trial.at(dw);
  D.echi2 = L.echi2.at(dw), D.Hll = L.Hll.at(dw), D.bl = L.bl.at(dw), D.Hpl = L.Hpl.at(dw), D.T = L.T.at(dw), D.vis = L.vis.at(dw), D.Y = L.Y.at(dw);
  D.inv = L.inv.at(dw), D.bfull = L.bfull.at(dw), D.M = L.M.at(dw), D.bs = L.bs.at(dw), D.x = L.x.at(dw), D.chi_chunk = L.chi_chunk.at(dw);
  D.chi_chunk_trial = L.chi_chunk_trial.at(dw), D.scale_chunk = L.scale_chunk.at(dw), D.ctl = L.ctl.at(dw);
  D.out_window = L.out_window.at(dr), D.out_points = L.out_points.at(dr), D.out_chi2 = L.out_chi2.at(dr), D.out_dp = L.out_dp.at(dr);
  D.out_erase = L.out_erase.at(dr), D.out = L.out.at(dr);

  const dim3 lm_grid(std::max(D.n_chunks, 1)), lm_block(kThreads);
  const int n = D.D;
  const bool in_lds = n <= kLdsRows;
  const size_t lds_bytes = in_lds ? (size_t)tri(n, 0) * sizeof(double) : 0;
  GFS_LAUNCH("k_li_init", k_li_init, dim3(1), lm_block, 0, s, D, p.lambda_init);
  for (int it = 0; it < p.iterations || it == 0; it++) {
    GFS_LAUNCH("k_li_small", k_li_small<false>, dim3(N), lm_block, 0, s, D);
    GFS_LAUNCH("k_li_vis", k_li_vis, lm_grid, lm_block, 0, s, D);
    GFS_LAUNCH("k_li_posesum", k_li_posesum, dim3(N), dim3(64), 0, s, D);
    GFS_LAUNCH("k_li_begin", k_li_begin, dim3(1), dim3(64), 0, s, D, it < p.iterations ? 1 : 0);
    if (it >= p.iterations) break;
    for (int q = 0; q < kMaxTrials; q++) {
      GFS_LAUNCH("k_li_inv", k_li_inv, lm_grid, lm_block, 0, s, D);
      GFS_LAUNCH("k_li_assemble", k_li_assemble, dim3(gfs::div_up(n * (n + 1), kThreads)), lm_block, 0, s, D);
      if (in_lds) GFS_LAUNCH("k_li_solve_lds", k_li_solve<true>, dim3(1), dim3(kSolveThreads), lds_bytes, s, D);
      else GFS_LAUNCH("k_li_solve_hbm", k_li_solve<false>, dim3(1), dim3(kSolveThreads), 0, s, D);
      GFS_LAUNCH("k_li_update", k_li_update, dim3(1), dim3(64), 0, s, D);
      GFS_LAUNCH("k_li_small_trial", k_li_small<true>, dim3(N), lm_block, 0, s, D);
      GFS_LAUNCH("k_li_back", k_li_back, lm_grid, lm_block, 0, s, D);
      GFS_LAUNCH("k_li_decide", k_li_decide, dim3(1), lm_block, 0, s, D);
    }
  }
  GFS_LAUNCH("k_li_final", k_li_final, lm_grid, lm_block, 0, s, D);
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  L.out_window.get(sol->window, hr, 0, N);
  L.out_points.get(sol->points, hr, 0, P);
  L.out_chi2.get(sol->edge_chi2, hr, 0, E);
  L.out_dp.get(sol->edge_depth_positive, hr, 0, E);
  L.out_erase.get(sol->edge_erase, hr, 0, E);
  const OutScalars& O = *L.out.at(hr);
  sol->err = O.err, sol->err_end = O.err_end, sol->iterations_run = O.iterations_run, sol->trials_run = O.trials_run;
  sol->final_lambda = O.final_lambda;
  return GFS_OK;
}

}  // extern "C"
