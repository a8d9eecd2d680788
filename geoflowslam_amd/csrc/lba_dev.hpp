// Device code of the bundle adjustments (lba.hip): the LM state and the window descriptor, the edge arithmetic, the body of every
// phase (b_*), the phase kernels of one window (k_lba_*) and of a batch of windows (kb_lba_*).  gba_dev.hpp adds the global bundle
// adjustment's reduced system behind it; both handles (lba_host.hpp, gba_host.hpp) launch these kernels.
#pragma once
#include "g2o_se3_dev.hpp"
#include "gfs_common.hpp"
#include "lidar_assoc.hpp"
#include "wave_reduce.hpp"

namespace {

constexpr int kThreads = 1024;
constexpr int kFlagInts = 8;  // one slot of gfs_lba::h_flags: 4 ints + 2 doubles
constexpr int kMaxFreeLds = 30;  // up to this many free poses the reduced system (180 x 180 packed) is factored in LDS

// LM bookkeeping of the multi-kernel path, resident in HBM (the scalar logic of OptimizationAlgorithmLevenberg::solve)
struct LbaState {
  double lambda, ni, current_chi, ini_chi, temp_chi, rho, last_chi;
  int cur;                       // which of the two estimate buffers holds the accepted state
  int qmax, n_bad, iters;
  int solve_ok;                  // LinearSolver succeeded in the current trial
  int again, terminate;          // outputs of k_lba_decide for the host loop
  int err_at_cur;                // chi2 / err / part_chi already hold the accepted estimate's values (the accepted trial computed them)
  int phase, it;                 // batched entry: 0 = build next, 1 = trial next, 2 = done; index of the running LM iteration
  int spec_ok, pad_;             // k_lba_decide: the trial was accepted and the loop goes on -- the build group of the NEXT iteration, queued
                                 // behind it speculatively by gfs_lba_solve's host loop (gate = 1), may run (round 6)
};

// The descriptor's pointers carry the GLOBAL address space in device code: the batched kernels read their descriptor from an array
// in memory, and pointers that come out of memory are otherwise GENERIC — every access through them a FLAT instruction (64-bit
// VGPR addresses, both wait counters).  Host code (and the host functions as the device pass parses them) sees plain pointers and
// assigns through a cast to the member's type.
#if defined(__HIP_DEVICE_COMPILE__)
#define GFS_GLOBAL __attribute__((address_space(1)))
#else
#define GFS_GLOBAL
#endif
struct LbaDev {
  // problem (edges landmark-major)
  int n_poses, n_points, n_edges, n_free;
  const GFS_GLOBAL double* pose_q0;  // [n_poses][4]
  const GFS_GLOBAL double* pose_t0;  // [n_poses][3]
  const GFS_GLOBAL int* free_index;  // [n_poses] -> free slot or -1
  const GFS_GLOBAL int* free_pose;   // [n_free]  -> pose
  const GFS_GLOBAL double* points0;  // [n_points][3]
  const GFS_GLOBAL int* e_pose;
  const GFS_GLOBAL int* e_point;
  const GFS_GLOBAL double* e_obs;  // [n_edges][3]
  const GFS_GLOBAL double* e_w;    // inv_sigma2
  const GFS_GLOBAL unsigned char* e_stereo;
  const GFS_GLOBAL int* pt_begin;     // [n_points+1]
  const GFS_GLOBAL int* pose_begin;   // [n_free+1]
  const GFS_GLOBAL int* pose_edges;   // edge ids (landmark-major numbering), ascending, per free pose
  const GFS_GLOBAL int* edge_of;      // [n_free][n_points] edge id or -1 (the FIRST edge of a (pose, landmark) pair)
  const GFS_GLOBAL int* lm_wg;        // [n_lm_wg + 1] landmark ranges of the workgroups of b_build_landmarks (<= kMk edges each, or one landmark)
  int n_lm_wg;
  const GFS_GLOBAL int* e_dup;        // [n_edges] first edge of the same (pose, landmark) pair, -1 for a first edge; NULL: no duplicates
  double fx, fy, cx, cy, bf, huber_mono, huber_stereo;
  int iterations;
  // state / workspace
  GFS_GLOBAL double* q;    // [n_poses][4] current
  GFS_GLOBAL double* t;    // [n_poses][3]
  GFS_GLOBAL double* X;    // [n_points][3]
  GFS_GLOBAL double* q_try;
  GFS_GLOBAL double* t_try;
  GFS_GLOBAL double* X_try;
  GFS_GLOBAL double* chi2;   // [n_edges] last computeActiveErrors
  GFS_GLOBAL double* err;    // [n_edges][3]
  GFS_GLOBAL double* Hpl;    // [n_edges][18] row-major (6 pose rows x 3 point cols)
  GFS_GLOBAL double* Hll;    // [n_points][6] symmetric (xx,xy,xz,yy,yz,zz)
  GFS_GLOBAL double* bl;     // [n_points][3]
  GFS_GLOBAL double* Dinv;   // [n_points][6]
  GFS_GLOBAL double* Hpp;    // [n_free][21] upper triangle row-major
  GFS_GLOBAL double* bp;     // [n_free][6]
  GFS_GLOBAL double* xl;     // [n_points][3]
  GFS_GLOBAL double* xp;     // [n_free*6]
  GFS_GLOBAL int* out_info;       // [0]=iterations_run [1]=failed flag
  GFS_GLOBAL double* out_stats;   // [0]=final chi2 [1]=final lambda
  int mode;            // 0 = full solve, 1 = linearise only
  // multi-kernel path (one launch per phase, all CUs): LM state, per-block partial sums, the reduced system in HBM
  GFS_GLOBAL struct LbaState* S;
  GFS_GLOBAL double* part_chi;    // [n_err_blocks] robust chi2 partial sums of the last k_lba_errors
  GFS_GLOBAL double* part_scale;  // [n_upd_blocks] computeScale partial sums of the last k_lba_update
  GFS_GLOBAL double* Hs;          // packed lower triangle of the Schur complement (6 n_free)^2 / 2
  GFS_GLOBAL double* bs;          // [6 n_free]
  int n_err_blocks, n_upd_blocks;
  GFS_GLOBAL double* out_pack;  // results in one block: chi2 [n_edges], q [n_poses][4], t [n_poses][3], X [n_points][3], chi2 / lambda, iterations / buffer
  // Schur products by landmark chunks: partial blocks [chunk][pose pair][36] and right-hand sides [chunk][free pose][6]
  GFS_GLOBAL double* schur_part;
  GFS_GLOBAL double* schur_part_b;
  int n_schur_chunks, n_pair_tiles, schur_sub;  // chunks of kSchurPts landmarks; tiles of kMk pose pairs; landmarks staged at a time
  int schur_mfma;  // 1: b_schur_mfma (n_schur_chunks chunks of kSchurMPts landmarks, n_pair_tiles = 128 x 128 blocks of the lower triangle)
  // LocalVisualLidarBA (gfs_lba_solve_lidar): the point-to-plane edges of the window's lidar key-frames, compacted per key-frame in
  // cloud order at the key-frame's offset in the concatenated cloud.  n_lidar_kf = 0 (every other entry): no lidar edges.
  int n_lidar_kf;    // lidar key-frames: the first n_lidar_kf workgroups of k_lba_errors, ahead of the reprojection edges' (g2o's order)
  int n_lidar_free;  // ... of which free: the workgroups of k_lba_lidar_build
  const GFS_GLOBAL gfs_lidar::WindowKF* lkf;  // [n_lidar_kf]
  const GFS_GLOBAL int* lkf_free;             // [n_lidar_free] -> lidar key-frame
  const GFS_GLOBAL float* lcloud;             // [3 x concatenated cloud]
  const GFS_GLOBAL int* l_cnt;                // [n_lidar_kf] edges of each lidar key-frame
  const GFS_GLOBAL int* l_idx;                // edge -> cloud index in its key-frame's cloud
  const GFS_GLOBAL float4* l_plane;           // edge -> (pa, pb, pc, pd)
  const GFS_GLOBAL float* l_s;                // edge -> s
  GFS_GLOBAL double* l_chi2;                  // edge -> chi2 of the last k_lba_errors
  double l_info, l_huber;                     // the edges' information and Huber delta
};

using namespace gfs_se3;

// residual of one edge (computeError): types_six_dof_expmap.h:157-162 / .cpp:190-197 (float invz) and
// include/OptimizableTypes.h:108-115 + src/CameraModels/Pinhole.cpp:35-41
__device__ __forceinline__ void edge_residual(const LbaDev& D, int e, const double* q, const double* t, const double* X,
                                              double* xc, double* r) {
  const int pi = D.e_pose[e], li = D.e_point[e];
  quat_rotate(q + 4 * pi, X + 3 * li, xc);
  xc[0] += t[3 * pi];
  xc[1] += t[3 * pi + 1];
  xc[2] += t[3 * pi + 2];
  const double* obs = D.e_obs + 3 * e;
  if (D.e_stereo[e]) {
    const float invz = (float)(1.0 / xc[2]);
    const double u = xc[0] * (double)invz * D.fx + D.cx, v = xc[1] * (double)invz * D.fy + D.cy;
    const float bf = (float)D.bf;
    const double ur = u - (double)(bf * invz);
    r[0] = obs[0] - u;
    r[1] = obs[1] - v;
    r[2] = obs[2] - ur;
  } else {
    r[0] = obs[0] - (D.fx * xc[0] / xc[2] + D.cx);
    r[1] = obs[1] - (D.fy * xc[1] / xc[2] + D.cy);
    r[2] = 0;
  }
}

// linearizeOplus (types_six_dof_expmap.cpp:228-275; src/OptimizableTypes.cpp:134-154): Ji (3x3), Jj (3x6) row-major
__device__ __forceinline__ void edge_jacobians(const LbaDev& D, int e, const double* q, const double* xc, double* Ji, double* Jj) {
  double R[9];
  quat_to_R(q + 4 * D.e_pose[e], R);
  const double x = xc[0], y = xc[1], z = xc[2], fx = D.fx, fy = D.fy, bf = D.bf;
  if (D.e_stereo[e]) {
    const double z_2 = z * z;
    for (int c = 0; c < 3; c++) {
      Ji[c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
      Ji[3 + c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
      Ji[6 + c] = Ji[c] - bf * R[6 + c] / z_2;
    }
    Jj[0] = x * y / z_2 * fx;
    Jj[1] = -(1 + (x * x / z_2)) * fx;
    Jj[2] = y / z * fx;
    Jj[3] = -1. / z * fx;
    Jj[4] = 0;
    Jj[5] = x / z_2 * fx;
    Jj[6] = (1 + y * y / z_2) * fy;
    Jj[7] = -x * y / z_2 * fy;
    Jj[8] = -x / z * fy;
    Jj[9] = 0;
    Jj[10] = -1. / z * fy;
    Jj[11] = y / z_2 * fy;
    Jj[12] = Jj[0] - bf * y / z_2;
    Jj[13] = Jj[1] + bf * x / z_2;
    Jj[14] = Jj[2];
    Jj[15] = Jj[3];
    Jj[16] = 0;
    Jj[17] = Jj[5] - bf / z_2;
  } else {
    const double pj[6] = {-(fx / z), -0.0, -(-fx * x / (z * z)), -0.0, -(fy / z), -(-fy * y / (z * z))};
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < 3; c++) Ji[r * 3 + c] = pj[r * 3] * R[c] + pj[r * 3 + 1] * R[3 + c] + pj[r * 3 + 2] * R[6 + c];
    const double sd[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < 6; c++) Jj[r * 6 + c] = pj[r * 3] * sd[c] + pj[r * 3 + 1] * sd[6 + c] + pj[r * 3 + 2] * sd[12 + c];
    for (int c = 0; c < 3; c++) Ji[6 + c] = 0;
    for (int c = 0; c < 6; c++) Jj[12 + c] = 0;
  }
}

// deterministic block reduction (1024 threads): wave shuffle tree, then the 16 wave results in order
__device__ double block_max(double v, double* s16) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int ofs = 32; ofs > 0; ofs >>= 1) v = fmax(v, __shfl_down(v, ofs, 64));
  __syncthreads();
  if (lane == 0) s16[wave] = v;
  __syncthreads();
  double r = 0;
  for (int w = 0; w < 16; w++) r = fmax(r, s16[w]);
  return r;
}

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // packed lower, i >= j

__device__ __forceinline__ void inv3_sym(const double* h /*xx,xy,xz,yy,yz,zz*/, double lambda, double* o) {
  const double a = h[0] + lambda, b = h[1], c = h[2], d = h[3] + lambda, e = h[4], f = h[5] + lambda;
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  const double id = 1.0 / det;
  o[0] = c00 * id;
  o[1] = c01 * id;
  o[2] = c02 * id;
  o[3] = (a * f - c * c) * id;
  o[4] = (b * c - a * e) * id;
  o[5] = (a * d - b * b) * id;
}

// ================================================================================================
// The phase kernels: one launch per phase so that every phase uses the whole chip instead of one CU (the whole LM loop in a
// single workgroup, the first implementation, was latency-bound: 61 ms for the C5 window).  The scalar LM logic lives in
// LbaState (HBM) and runs in k_lba_begin / k_lba_decide; the host only enqueues the phases and reads two flags per trial.
// The two estimate buffers (q/t/X and q_try/t_try/X_try) swap roles when a step is accepted (S->cur).
// ================================================================================================
constexpr int kMk = 256;  // threads per workgroup of the wide kernels

__device__ __forceinline__ double* sel(double* a, double* b, int which) { return which ? b : a; }

__device__ __forceinline__ void b_init(const LbaDev& D, const int bx, const int gdx) {
  const int g = bx * kMk + threadIdx.x, G = gdx * kMk;
  for (int i = g; i < D.n_poses; i += G) {
    double q[4] = {D.pose_q0[4 * i], D.pose_q0[4 * i + 1], D.pose_q0[4 * i + 2], D.pose_q0[4 * i + 3]};
    normalize_rotation(q);
    for (int k = 0; k < 4; k++) D.q[4 * i + k] = D.q_try[4 * i + k] = q[k];
    for (int k = 0; k < 3; k++) D.t[3 * i + k] = D.t_try[3 * i + k] = D.pose_t0[3 * i + k];
  }
  for (int i = g; i < 3 * D.n_points; i += G) D.X[i] = D.X_try[i] = D.points0[i];
  for (size_t i = g; i < (size_t)D.n_edges * 18; i += G) D.Hpl[i] = 0;  // the blocks of fixed-pose edges stay zero
  if (g == 0) {
    LbaState& S = *D.S;
    S.lambda = -1;
    S.ni = 2;
    S.current_chi = S.ini_chi = S.temp_chi = S.rho = S.last_chi = 0;
    S.cur = 0;
    S.qmax = S.n_bad = S.iters = 0;
    S.solve_ok = 1;
    S.again = S.terminate = 0;
    S.phase = S.it = 0;
    S.err_at_cur = 0;
    S.spec_ok = S.pad_ = 0;
  }
}
__global__ __launch_bounds__(kMk) void k_lba_init(LbaDev D) { b_init(D, blockIdx.x, gridDim.x); }


// ---- LocalVisualLidarBA's point-to-plane edges (EdgeSE3LidarPoint2Plane, src/Optimizer.cc:1327-1362): information 1e2 (:1348) and
// Huber delta thHuberLidar = (float) sqrt(1.0) (:1328) come in LbaDev::l_info / l_huber from pose_lidar.hip's definitions
// (gfs_lidar::edge_information / edge_huber_delta)

// the robust chi2 of lidar key-frame k's edges at the estimate (q, t), its edges over the threads, fixed-shape reduction: part_chi[k]
__device__ __forceinline__ void b_lidar_errors(const LbaDev& D, const int k, const double* q, const double* t, double* s4) {
  const gfs_lidar::WindowKF& K = D.lkf[k];
  const int p = K.pose, n = D.l_cnt[k], base = K.begin;
  double W[7];
  gfs_lidar::se3_inverse(q + 4 * p, t + 3 * p, W);
  double local = 0;
  for (int l = threadIdx.x; l < n; l += kMk) {
    const float* po = D.lcloud + 3 * ((size_t)base + D.l_idx[base + l]);
    const double pt[3] = {(double)po[0], (double)po[1], (double)po[2]};
    const double ev = gfs_lidar::lidar_err(W, pt, D.l_plane[base + l], D.l_s[base + l]);
    const double c = ev * (D.l_info * ev);
    D.l_chi2[base + l] = c;
    double r0, r1;
    huber(c, D.l_huber, &r0, &r1);
    local += r0;
  }
  const double tot = gfs_red::block_sum256(local, s4);
  if (threadIdx.x == 0) D.part_chi[k] = tot;
}

// computeActiveErrors on the accepted (trial = 0) or the trial estimate (trial = 1; falls back to the accepted one when the
// linear solve failed, like the reference which restores the estimate before recomputing the errors)
__device__ __forceinline__ void b_errors(const LbaDev& D, const int bx, const int gdx, int trial) {
  __shared__ double s4[4];
  const LbaState& S = *D.S;
  // computeActiveErrors at the top of an iteration that follows an accepted trial would recompute, at the same estimate, what that
  // trial's own evaluation left in chi2 / err / part_chi
  if (!trial && S.err_at_cur) return;
  const int which = (trial && S.solve_ok) ? (S.cur ^ 1) : S.cur;
  const double *q = sel(D.q, D.q_try, which), *t = sel(D.t, D.t_try, which), *X = sel(D.X, D.X_try, which);
  if (bx < D.n_lidar_kf) {  // (uniform per workgroup)
    b_lidar_errors(D, bx, q, t, s4);
    return;
  }
  double local = 0;
  const int e = (bx - D.n_lidar_kf) * kMk + threadIdx.x;
  if (e < D.n_edges) {
    double xc[3], r[3];
    edge_residual(D, e, q, t, X, xc, r);
    const double c = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * D.e_w[e];
    D.chi2[e] = c;
    D.err[3 * e] = r[0];
    D.err[3 * e + 1] = r[1];
    D.err[3 * e + 2] = r[2];
    double r0, r1;
    huber(c, D.e_stereo[e] ? D.huber_stereo : D.huber_mono, &r0, &r1);
    local = r0;
  }
  const double tot = gfs_red::block_sum256(local, s4);
  if (threadIdx.x == 0) D.part_chi[bx] = tot;
}
// gate = 1 (k_lba_errors / build_landmarks / build_poses / begin): a launch queued speculatively behind k_lba_decide -- it runs only if that
// trial was accepted and the loop goes on (LbaState::spec_ok); uniform per launch, in front of every barrier
__global__ __launch_bounds__(kMk) void k_lba_errors(LbaDev D, int trial, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_errors(D, blockIdx.x, gridDim.x, trial);
}


// buildSystem, landmark side: Hll, bl and the per-edge pose-landmark blocks.  16 lanes per landmark (its edges over the
// lanes, the 9 sums folded by xor-shuffles inside the group in a fixed order), 8 landmarks per 128-thread workgroup.
__device__ __forceinline__ void b_build_landmarks(const LbaDev& D, const int bx, const int gdx) {
  // One thread per EDGE: a workgroup takes a run of whole landmarks holding at most kMk edges (lm_wg, packed by the host; a
  // landmark with more than kMk edges gets a workgroup to itself and the threads stride over its edges).  The nine landmark
  // sums (Hll, bl) of an edge go through LDS and thread <-> (landmark, component) adds its landmark's edges in edge order.
  // (16 lanes per landmark, the round-1 mapping, left half the lanes idle: a landmark of this window has 16.5 edges on
  // average, so nearly every group ran a second, almost empty pass.)
  __shared__ double s_c[kMk][9];
  const LbaState& S = *D.S;
  const double *q = sel(D.q, D.q_try, S.cur), *t = sel(D.t, D.t_try, S.cur), *X = sel(D.X, D.X_try, S.cur);
  const int l0 = D.lm_wg[bx], l1 = D.lm_wg[bx + 1];
  const int e0 = D.pt_begin[l0], e1 = D.pt_begin[l1];
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // H (xx,xy,xz,yy,yz,zz), b
  for (int e = e0 + threadIdx.x; e < e1; e += kMk) {
    double xc[3], r[3], Ji[9], Jj[18];
    edge_residual(D, e, q, t, X, xc, r);
    edge_jacobians(D, e, q, xc, Ji, Jj);
    double r0, r1;
    huber(D.chi2[e], D.e_stereo[e] ? D.huber_stereo : D.huber_mono, &r0, &r1);
    const double w = r1 * D.e_w[e];
    double omr[3];
    for (int k = 0; k < 3; k++) omr[k] = -(D.e_w[e] * D.err[3 * e + k]) * r1;
    int o = 0;
    for (int a = 0; a < 3; a++) {
      acc[6 + a] += Ji[a] * omr[0] + Ji[3 + a] * omr[1] + Ji[6 + a] * omr[2];
      for (int c = a; c < 3; c++) acc[o++] += Ji[a] * w * Ji[c] + Ji[3 + a] * w * Ji[3 + c] + Ji[6 + a] * w * Ji[6 + c];
    }
    if (D.free_index[D.e_pose[e]] >= 0) {
      double* B = D.Hpl + 18 * (size_t)e;
      for (int a = 0; a < 6; a++)
        for (int c = 0; c < 3; c++) B[3 * a + c] = Jj[a] * w * Ji[c] + Jj[6 + a] * w * Ji[3 + c] + Jj[12 + a] * w * Ji[6 + c];
    }
  }
#pragma unroll
  for (int k = 0; k < 9; k++) s_c[threadIdx.x][k] = acc[k];
  __syncthreads();
  const int nl = l1 - l0;
  for (int u = threadIdx.x; u < nl * 9; u += kMk) {
    const int l = l0 + u / 9, k = u - (u / 9) * 9;
    int s0 = D.pt_begin[l] - e0, s1 = D.pt_begin[l + 1] - e0;
    if (e1 - e0 > kMk) {  // one landmark with more edges than threads: every thread holds a partial sum of it
      s0 = 0;
      s1 = kMk;
    }
    double v = 0;
    for (int sl = s0; sl < s1; sl++) v += s_c[sl][k];
    if (k < 6)
      D.Hll[6 * (size_t)l + k] = v;
    else
      D.bl[3 * (size_t)l + (k - 6)] = v;
  }
  // several edges between one pose and one landmark (a rig seeing the point with two cameras): g2o adds their J_pose^T Omega J_point
  // into the one Hpl block of that vertex pair (core/block_solver.hpp:143-295 allocates it once).  The first edge's block takes
  // the sum, in edge order, and the later ones are cleared: everything downstream (Schur products, back-substitution) sums over
  // edges.  gfs_lba_linearize (mode 1) reports the per-edge blocks instead.
  if (D.e_dup && D.mode == 0) {
    __threadfence_block();
    __syncthreads();
    for (int l = l0 + threadIdx.x; l < l1; l += kMk) {
      for (int e = D.pt_begin[l]; e < D.pt_begin[l + 1]; e++) {
        const int first = D.e_dup[e];
        if (first < 0 || D.free_index[D.e_pose[e]] < 0) continue;
        double* B = D.Hpl + 18 * (size_t)e;
        double* A = D.Hpl + 18 * (size_t)first;
        for (int k = 0; k < 18; k++) {
          A[k] += B[k];
          B[k] = 0;
        }
      }
    }
  }
}
__global__ __launch_bounds__(kMk) void k_lba_build_landmarks(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_build_landmarks(D, blockIdx.x, gridDim.x);
}


// buildSystem, pose side: one workgroup per free pose, threads over its edges, fixed-order reduction
// (kPoseWg threads a pose: a free pose of the configs[4] window has ~2 500 edges, and an edge is a chain of dependent loads --
// index, then its data -- so the kernel's time is edges per THREAD: 10 at 256 threads, 27 us a launch; 2.5 at 1 024, round 5)
constexpr int kPoseWg = 1024;
__device__ __forceinline__ void b_build_poses(const LbaDev& D, const int bx, const int gdx) {
  __shared__ double s_buf[(kPoseWg / 64) * 32];
  const LbaState& S = *D.S;
  const double *q = sel(D.q, D.q_try, S.cur), *t = sel(D.t, D.t_try, S.cur), *X = sel(D.X, D.X_try, S.cur);
  const int f = bx;
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = 0;
  for (int i = D.pose_begin[f] + threadIdx.x; i < D.pose_begin[f + 1]; i += kPoseWg) {
    const int e = D.pose_edges[i];
    double xc[3], r[3], Ji[9], Jj[18];
    edge_residual(D, e, q, t, X, xc, r);
    edge_jacobians(D, e, q, xc, Ji, Jj);
    double r0, r1;
    huber(D.chi2[e], D.e_stereo[e] ? D.huber_stereo : D.huber_mono, &r0, &r1);
    const double w = r1 * D.e_w[e];
    double omr[3];
    for (int k = 0; k < 3; k++) omr[k] = -(D.e_w[e] * D.err[3 * e + k]) * r1;
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = a; c < 6; c++) acc[o++] += Jj[a] * w * Jj[c] + Jj[6 + a] * w * Jj[6 + c] + Jj[12 + a] * w * Jj[12 + c];
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] += Jj[a] * omr[0] + Jj[6 + a] * omr[1] + Jj[12 + a] * omr[2];
  }
  const double v = gfs_red::block_sum_many<27, kPoseWg / 64>(acc, s_buf);
  if (threadIdx.x < 21)
    D.Hpp[21 * f + threadIdx.x] = v;
  else if (threadIdx.x < 27)
    D.bp[6 * f + (threadIdx.x - 21)] = v;
}
__global__ __launch_bounds__(kPoseWg) void k_lba_build_poses(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_build_poses(D, blockIdx.x, gridDim.x);
}


// buildSystem, lidar side: BaseUnaryEdge::linearizeOplus (core/base_unary_edge.hpp:82-123: central differences, delta 1e-9) and
// constructQuadraticForm of the edges of one free lidar key-frame, one workgroup each.  The twelve perturbed poses (and their inverses,
// which computeError takes) are the same for every edge: twelve lanes compute them once.  The 6 x 6 block and 6-vector are reduced
// in a fixed shape and added to the key-frame's Hpp / bp after the reprojection edges' sum (k_lba_build_poses), before the initial
// lambda and the Schur products.  A key-frame whose association left no edge is not touched.
__global__ __launch_bounds__(kMk) void k_lba_lidar_build(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  __shared__ double s_Wp[12][7];
  __shared__ double s_buf[(kMk / 64) * 32];
  const int k = D.lkf_free[blockIdx.x];
  const gfs_lidar::WindowKF& K = D.lkf[k];
  const int n = D.l_cnt[k], base = K.begin, tid = threadIdx.x;
  const double info = D.l_info;
  if (n == 0) return;
  const LbaState& S = *D.S;
  const double *q = sel(D.q, D.q_try, S.cur) + 4 * K.pose, *t = sel(D.t, D.t_try, S.cur) + 3 * K.pose;
  if (tid < 12) {
    double u[6] = {0, 0, 0, 0, 0, 0}, qp[4], tp[3];
    u[tid >> 1] = (tid & 1) ? -1e-9 : 1e-9;
    pose_oplus(q, t, u, qp, tp);
    gfs_lidar::se3_inverse(qp, tp, s_Wp[tid]);
  }
  double W[7];
  gfs_lidar::se3_inverse(q, t, W);
  __syncthreads();
  double acc[27];
#pragma unroll
  for (int j = 0; j < 27; j++) acc[j] = 0;
  for (int l = tid; l < n; l += kMk) {
    const float* po = D.lcloud + 3 * ((size_t)base + D.l_idx[base + l]);
    const double pt[3] = {(double)po[0], (double)po[1], (double)po[2]};
    const float4 pl = D.l_plane[base + l];
    const float sl = D.l_s[base + l];
    double J[6];
#pragma unroll
    for (int d = 0; d < 6; d++)
      J[d] = (1.0 / (2 * 1e-9)) * (gfs_lidar::lidar_err(s_Wp[2 * d], pt, pl, sl) - gfs_lidar::lidar_err(s_Wp[2 * d + 1], pt, pl, sl));
    const double ev = gfs_lidar::lidar_err(W, pt, pl, sl);
    double r0, rho1;
    huber(ev * (info * ev), D.l_huber, &r0, &rho1);
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = a; c < 6; c++) acc[o++] += (J[a] * (rho1 * info)) * J[c];
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] += -(((rho1 * J[a]) * info) * ev);
  }
  const double v = gfs_red::block_sum_many<27, kMk / 64>(acc, s_buf);
  const int f = D.free_index[K.pose];
  if (tid < 21)
    D.Hpp[21 * f + tid] += v;
  else if (tid < 27)
    D.bp[6 * f + (tid - 21)] += v;
}

// GenerateLidarEdge's vector, nullptr entries skipped: the points of lidar key-frame blockIdx.x that k_lba_lidar_assoc kept, compacted
// in cloud-index order (ballot per wave, the waves in order) at the key-frame's offset; l_cnt = their number
__global__ __launch_bounds__(kMk) void k_lba_lidar_compact(const gfs_lidar::WindowKF* __restrict__ kfs, const uint8_t* __restrict__ flag,
                                                           const float4* __restrict__ plane, const float* __restrict__ s_in,
                                                           int* __restrict__ cnt, int* __restrict__ idx, float4* __restrict__ eplane,
                                                           float* __restrict__ es) {
  __shared__ int s_wcnt[kMk / 64];
  const gfs_lidar::WindowKF K = kfs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nl = 0;
  for (int b0 = 0; b0 < K.n; b0 += kMk) {
    const int i = b0 + tid;
    const bool keep = i < K.n && flag[(size_t)K.begin + i];
    const unsigned long long m = __ballot(keep);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = nl;
    for (int w = 0; w < wave; w++) off += s_wcnt[w];
    if (keep) {
      const size_t pos = (size_t)K.begin + off + below;
      idx[pos] = i;
      eplane[pos] = plane[(size_t)K.begin + i];
      es[pos] = s_in[(size_t)K.begin + i];
    }
    for (int w = 0; w < kMk / 64; w++) nl += s_wcnt[w];
    __syncthreads();
  }
  if (tid == 0) cnt[blockIdx.x] = nl;
}


// start of an LM iteration: currentChi, and at iteration 0 computeLambdaInit (tau * max |diag H|)
__device__ __forceinline__ void b_begin(const LbaDev& D, const int bx, const int gdx, int iteration) {
  __shared__ double s16[16];
  LbaState& S = *D.S;
  double chi = 0;
  if (threadIdx.x == 0)
    for (int b = 0; b < D.n_err_blocks; b++) chi += D.part_chi[b];
  if (iteration == 0) {
    double mx = 0;
    for (int i = threadIdx.x; i < D.n_free * 6; i += kThreads) {
      const int f = i / 6, a = i % 6;
      mx = fmax(mx, fabs(D.Hpp[21 * f + (a * 6 - a * (a - 1) / 2)]));
    }
    for (int i = threadIdx.x; i < D.n_points * 3; i += kThreads) {
      const int l = i / 3, a = i % 3;
      mx = fmax(mx, fabs(D.Hll[6 * (size_t)l + (a == 0 ? 0 : a == 1 ? 3 : 5)]));
    }
    mx = block_max(mx, s16);
    if (threadIdx.x == 0) {
      S.lambda = 1e-5 * mx;
      S.ni = 2;
      S.n_bad = 0;
    }
  }
  if (threadIdx.x == 0) {
    S.current_chi = S.ini_chi = chi;
    S.rho = 0;
    S.qmax = 0;
    S.again = 0;
  }
}
__global__ __launch_bounds__(kThreads) void k_lba_begin(LbaDev D, int iteration, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_begin(D, blockIdx.x, gridDim.x, iteration);
}


__device__ __forceinline__ void b_dinv(const LbaDev& D, const int bx, const int gdx) {
  const int l = bx * kMk + threadIdx.x;
  if (l < D.n_points) inv3_sym(D.Hll + 6 * (size_t)l, D.S->lambda, D.Dinv + 6 * (size_t)l);
}
__global__ __launch_bounds__(kMk) void k_lba_dinv(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_dinv(D, blockIdx.x, gridDim.x);
}


// Schur complement, one workgroup per pose pair (i1 >= i2): Hs(i1,i2) = [i1==i2](Hpp + lambda I) - sum_l B_i1 Dinv_l B_i2^T
__device__ __forceinline__ void b_schur(const LbaDev& D, const int bx, const int gdx) {
  __shared__ double s_buf[(kMk / 64) * 32];
  const double lambda = D.S->lambda;
  const int pr = bx;
  int i1 = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
  while (i1 * (i1 + 1) / 2 > pr) i1--;
  while ((i1 + 1) * (i1 + 2) / 2 <= pr) i1++;
  const int i2 = pr - i1 * (i1 + 1) / 2;
  double acc[36], accb[6];
#pragma unroll
  for (int k = 0; k < 36; k++) acc[k] = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) accb[k] = 0;
  const int* eo = D.edge_of + (size_t)i2 * D.n_points;
  for (int i = D.pose_begin[i1] + threadIdx.x; i < D.pose_begin[i1 + 1]; i += kMk) {
    const int e1 = D.pose_edges[i];
    const int l = D.e_point[e1];
    const int e2 = eo[l];
    if (e2 < 0) continue;
    const double* Bi = D.Hpl + 18 * (size_t)e1;
    const double* Bj = D.Hpl + 18 * (size_t)e2;
    const double* Di = D.Dinv + 6 * (size_t)l;
    const double d9[9] = {Di[0], Di[1], Di[2], Di[1], Di[3], Di[4], Di[2], Di[4], Di[5]};
    double BD[18];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c < 3; c++) BD[3 * a + c] = Bi[3 * a] * d9[c] + Bi[3 * a + 1] * d9[3 + c] + Bi[3 * a + 2] * d9[6 + c];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c < 6; c++) acc[6 * a + c] += BD[3 * a] * Bj[3 * c] + BD[3 * a + 1] * Bj[3 * c + 1] + BD[3 * a + 2] * Bj[3 * c + 2];
    if (i1 == i2) {
      const double* bl = D.bl + 3 * (size_t)l;
#pragma unroll
      for (int a = 0; a < 6; a++) accb[a] += BD[3 * a] * bl[0] + BD[3 * a + 1] * bl[1] + BD[3 * a + 2] * bl[2];
    }
  }
  // 36 + 6 sums over the workgroup: two many-value reductions (32, then the remaining 4 + 6)
  double head[32], tail[10];
#pragma unroll
  for (int k = 0; k < 32; k++) head[k] = acc[k];
#pragma unroll
  for (int k = 0; k < 4; k++) tail[k] = acc[32 + k];
#pragma unroll
  for (int k = 0; k < 6; k++) tail[4 + k] = accb[k];
  const double v0 = gfs_red::block_sum_many<32, kMk / 64>(head, s_buf);
  const double v1 = gfs_red::block_sum_many<10, kMk / 64>(tail, s_buf);
  const int tk = threadIdx.x;
  // threads 0..31 own acc[0..31] (v0); threads 0..3 own acc[32..35] and threads 4..9 own accb[0..5] (v1)
  auto store_h = [&](int k, double val) {
    const int a = k / 6, c = k % 6;
    if (i1 != i2) {
      D.Hs[tri(6 * i1 + a, 6 * i2 + c)] = -val;
    } else if (a >= c) {
      const int ua = c, uc = a;  // Hpp upper-triangle index of (c, a)
      const double hpp = D.Hpp[21 * i1 + (ua * 6 - ua * (ua - 1) / 2 + (uc - ua))];
      D.Hs[tri(6 * i1 + a, 6 * i1 + c)] = hpp + (a == c ? lambda : 0.0) - val;
    }
  };
  if (tk < 32) store_h(tk, v0);
  if (tk < 4) store_h(32 + tk, v1);
  if (i1 == i2 && tk >= 4 && tk < 10) D.bs[6 * i1 + (tk - 4)] = D.bp[6 * i1 + (tk - 4)] - v1;
}
__global__ __launch_bounds__(kMk) void k_lba_schur(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_schur(D, blockIdx.x, gridDim.x);
}

// The same products taken landmark by landmark.  b_schur gives a workgroup to a pose pair, and every pair re-reads the 6x3
// blocks of its two poses for each common landmark: Hpl is read ~n_free times (L2 traffic, 0.8 MB per pair).  Here a workgroup
// takes a chunk of kSchurPts landmarks: the blocks B_f (6x3) of every free pose seeing a landmark, and B_f Dinv_l, are staged
// in LDS once (schur_sub landmarks at a time), and thread <-> pose pair (i1 >= i2) accumulates its 6x6 block (and, on the
// diagonal, B Dinv b_l) over the chunk's landmarks in index order.  Per-chunk partial blocks go to HBM; b_schur_reduce adds
// them in chunk order: the sums have a fixed order that does not depend on the launch (a window solved alone or in a batch
// gives the same bits).  Pose pairs beyond kMk: blockIdx.x = chunk * n_pair_tiles + tile.
constexpr int kSchurPts = 64;
constexpr int kSchurSlot = 38;  // doubles per staged (landmark, pose): B (18), B Dinv (18), + 2: 16 lanes' 16-byte reads of consecutive poses hit distinct banks

__device__ __forceinline__ void b_schur_chunks(const LbaDev& D, const int bx) {
  extern __shared__ __align__(16) double lds[];
  const int F = D.n_free, NP = D.n_points, SB = D.schur_sub;
  const int chunk = bx / D.n_pair_tiles, tile = bx - chunk * D.n_pair_tiles;
  double* s_blk = lds;                                   // [SB][F][kSchurSlot]
  double* s_bl = s_blk + (size_t)SB * F * kSchurSlot;    // [SB][4]
  int* s_edge = (int*)(s_bl + 4 * SB);                   // [SB][F] edge id or -1
  const int npairs = F * (F + 1) / 2;
  const int pr = tile * kMk + threadIdx.x;
  int i1 = 0, i2 = 0;
  if (pr < npairs) {
    i1 = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
    while (i1 * (i1 + 1) / 2 > pr) i1--;
    while ((i1 + 1) * (i1 + 2) / 2 <= pr) i1++;
    i2 = pr - i1 * (i1 + 1) / 2;
  }
  double acc[36], accb[6];
#pragma unroll
  for (int k = 0; k < 36; k++) acc[k] = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) accb[k] = 0;
  const int l_begin = chunk * kSchurPts, l_end = min(l_begin + kSchurPts, NP);
  for (int l0 = l_begin; l0 < l_end; l0 += SB) {
    const int nl = min(SB, l_end - l0);
    __syncthreads();  // the previous sub-batch has been consumed
    for (int u = threadIdx.x; u < nl * F; u += kMk) {
      const int p = u / F, f = u - p * F, l = l0 + p;
      const int e = D.edge_of[(size_t)f * NP + l];
      s_edge[p * F + f] = e;
      if (e >= 0) {
        const double* B = D.Hpl + 18 * (size_t)e;
        const double* Di = D.Dinv + 6 * (size_t)l;
        const double d9[9] = {Di[0], Di[1], Di[2], Di[1], Di[3], Di[4], Di[2], Di[4], Di[5]};
        double* o = s_blk + (size_t)(p * F + f) * kSchurSlot;
#pragma unroll
        for (int a = 0; a < 6; a++) {
          const double b0 = B[3 * a], b1 = B[3 * a + 1], b2 = B[3 * a + 2];
          o[3 * a] = b0;
          o[3 * a + 1] = b1;
          o[3 * a + 2] = b2;
#pragma unroll
          for (int c = 0; c < 3; c++) o[18 + 3 * a + c] = b0 * d9[c] + b1 * d9[3 + c] + b2 * d9[6 + c];
        }
      }
    }
    if (threadIdx.x < nl * 3) s_bl[4 * (threadIdx.x / 3) + threadIdx.x % 3] = D.bl[3 * (size_t)l0 + threadIdx.x];
    __syncthreads();
    if (pr < npairs) {
      for (int p = 0; p < nl; p++) {
        if (s_edge[p * F + i1] < 0 || s_edge[p * F + i2] < 0) continue;
        const double* BD = s_blk + (size_t)(p * F + i1) * kSchurSlot + 18;
        const double* Bj = s_blk + (size_t)(p * F + i2) * kSchurSlot;
        double bd[18], bj[18];
#pragma unroll
        for (int k = 0; k < 18; k++) {
          bd[k] = BD[k];
          bj[k] = Bj[k];
        }
        // fused multiply-adds: this loop is the kernel's VALU time, and the order of the sums already differs from g2o's
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int c = 0; c < 6; c++)
            acc[6 * a + c] = fma(bd[3 * a + 2], bj[3 * c + 2], fma(bd[3 * a + 1], bj[3 * c + 1], fma(bd[3 * a], bj[3 * c], acc[6 * a + c])));
        if (i1 == i2) {
          const double* bl = s_bl + 4 * p;
#pragma unroll
          for (int a = 0; a < 6; a++) accb[a] = fma(bd[3 * a + 2], bl[2], fma(bd[3 * a + 1], bl[1], fma(bd[3 * a], bl[0], accb[a])));
        }
      }
    }
  }
  if (pr < npairs) {
    double* o = D.schur_part + ((size_t)chunk * npairs + pr) * 36;
#pragma unroll
    for (int k = 0; k < 36; k++) o[k] = acc[k];
    if (i1 == i2) {
      double* ob = D.schur_part_b + ((size_t)chunk * F + i1) * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) ob[k] = accb[k];
    }
  }
}
__global__ __launch_bounds__(kMk) void k_lba_schur_chunks(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_schur_chunks(D, blockIdx.x);
}

// ---- the same sum on the matrix cores.  With W_l (6F x 3: the blocks B_f of landmark l stacked, zero where pose f does not see
// it) the Schur sum over landmarks is  S = sum_l (W_l Dinv_l) W_l^T = [WD_1 WD_2 ...] [W_1 W_2 ...]^T : one (6F x 3L)(3L x 6F)
// product, double precision, v_mfma_f64_16x16x4_f64.  The right-hand side rides along as one more row: row n = 6F of WD holds
// Dinv_l b_l, so that S[n][c] = sum_l B_c Dinv_l b_l.  A workgroup takes a chunk of kSchurMPts landmarks and one 128 x 128 block
// (bi >= bj) of S: kSchurSub landmarks (24 columns = 6 k-steps, nothing padded) are staged at a time in LDS, column-major with a
// row stride of 144 doubles (the four k-groups of a fragment read land in disjoint bank halves), each of the 4 waves owns a share
// of the block's 16 x 16 tiles and keeps them in registers across the chunk (diagonal block: tile rows w and 7 - w of the lower
// triangle, 9 tiles a wave; off-diagonal: rows 2w, 2w + 1, 16 tiles).  The edges of a run of landmarks are contiguous
// (landmark-major order), so the staging threads read e_pose / e_point / Hpl of edge e0 + tid directly, one sub-batch ahead of the
// products.  Per-chunk partial blocks go to HBM ([chunk][row][col], leading dimension 128 NB) and b_schur_reduce adds them in
// chunk order.  Operands are products of single roundings (fused multiply-add inside the matrix core), like b_schur_chunks.
// (round 6: 64 landmarks a workgroup instead of 128 -- a configs[4] window of 3 000 landmarks is 47 workgroups instead of 24 on the 256 CUs,
//  one window 2.13 - 2.16 -> 2.00 ms; 32: 2.02 ms; the batched path, whose launches fill the chip either way, is unchanged.  The partial
//  blocks are added in chunk order by the reduce kernel: the chunk size is part of the arithmetic, the same for one window and a batch)
#ifndef GFS_SCHUR_MPTS
#define GFS_SCHUR_MPTS 64
#endif
constexpr int kSchurMPts = GFS_SCHUR_MPTS;  // landmarks per workgroup
constexpr int kSchurSub = 8;     // landmarks staged at a time
constexpr int kSchurLd = 144;    // row stride (doubles) of a staged column
typedef double d4_t __attribute__((ext_vector_type(4)));

template <bool DIAG, int W>
__device__ __forceinline__ void schur_mfma_ksteps(const double* __restrict__ s_a, const double* __restrict__ s_b, d4_t (&acc0)[8],
                                                  d4_t (&acc1)[8]) {
  constexpr int r0 = DIAG ? W : 2 * W, r1 = DIAG ? 7 - W : 2 * W + 1;
  constexpr int nc0 = DIAG ? r0 + 1 : 8, nc1 = DIAG ? r1 + 1 : 8;
  const int lane = threadIdx.x & 63, row = lane & 15, kk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < 3 * kSchurSub / 4; ks++) {
    const double* ca = s_a + (4 * ks + kk) * kSchurLd + row;
    const double* cb = s_b + (4 * ks + kk) * kSchurLd + row;
    const double a0 = ca[16 * r0], a1 = ca[16 * r1];
    double b[8];
#pragma unroll
    for (int c = 0; c < 8; c++)
      if (c < nc1 || c < nc0) b[c] = cb[16 * c];
#pragma unroll
    for (int c = 0; c < 8; c++) {
      if (c < nc0) acc0[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[c], acc0[c], 0, 0, 0);
      if (c < nc1) acc1[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[c], acc1[c], 0, 0, 0);
    }
  }
}

template <bool DIAG, int W>
__device__ __forceinline__ void schur_mfma_store(double* __restrict__ out, int ld, const d4_t (&acc0)[8], const d4_t (&acc1)[8]) {
  constexpr int r0 = DIAG ? W : 2 * W, r1 = DIAG ? 7 - W : 2 * W + 1;
  constexpr int nc0 = DIAG ? r0 + 1 : 8, nc1 = DIAG ? r1 + 1 : 8;
  const int lane = threadIdx.x & 63, col = lane & 15, rq = lane >> 4;
#pragma unroll
  for (int c = 0; c < 8; c++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (c < nc0) out[(size_t)(16 * r0 + rq + 4 * i) * ld + 16 * c + col] = acc0[c][i];
      if (c < nc1) out[(size_t)(16 * r1 + rq + 4 * i) * ld + 16 * c + col] = acc1[c][i];
    }
}

// workgroup barrier that waits for this wave's LDS traffic only: __syncthreads() also drains the vector-memory counter, i.e. it
// would wait for the global loads of the NEXT sub-batch that are meant to stay in flight across the products
#define GFS_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
template <bool kOneBlock>
__device__ __forceinline__ void b_schur_mfma(const LbaDev& D, const int bx) {
  extern __shared__ __align__(16) double lds[];
  const int F = D.n_free, NP = D.n_points, n = 6 * F;
  const int NB = (n + 1 + 127) / 128, nbp = NB * (NB + 1) / 2, ld = 128 * NB;
  const int chunk = bx / nbp, bp = bx - chunk * nbp;
  int bi = (int)((sqrt(8.0 * bp + 1.0) - 1.0) * 0.5);
  while (bi * (bi + 1) / 2 > bp) bi--;
  while ((bi + 1) * (bi + 2) / 2 <= bp) bi++;
  const int bj = bp - bi * (bi + 1) / 2;
  double* s_a = lds;                                  // [24][kSchurLd]  rows of block bi of [WD; Dinv b]
  double* s_b = s_a + 3 * kSchurSub * kSchurLd;       // [24][kSchurLd]  rows of block bj of W
  double* s_dinv = s_b + 3 * kSchurSub * kSchurLd;    // [kSchurMPts][6]
  double* s_v = s_dinv + 6 * kSchurMPts;              // [kSchurMPts][3]  Dinv_l b_l
  int* s_ptb = (int*)(s_v + 3 * kSchurMPts);          // [kSchurMPts + 1]
  int* s_free = s_ptb + kSchurMPts + 1;               // [n_poses]
  const int tid = threadIdx.x, wave = tid >> 6;
  const int l_begin = chunk * kSchurMPts, l_end = min(l_begin + kSchurMPts, NP), nlm = l_end - l_begin;
  for (int i = tid; i < 6 * nlm; i += kMk) s_dinv[i] = D.Dinv[6 * (size_t)l_begin + i];
  for (int i = tid; i <= nlm; i += kMk) s_ptb[i] = D.pt_begin[l_begin + i];
  for (int i = tid; i < D.n_poses; i += kMk) s_free[i] = D.free_index[i];
  __syncthreads();
  for (int p = tid; p < nlm; p += kMk) {
    const double* Di = s_dinv + 6 * p;
    const double* bl = D.bl + 3 * (size_t)(l_begin + p);
    const double b0 = bl[0], b1 = bl[1], b2 = bl[2];
    s_v[3 * p] = fma(Di[2], b2, fma(Di[1], b1, Di[0] * b0));
    s_v[3 * p + 1] = fma(Di[4], b2, fma(Di[3], b1, Di[1] * b0));
    s_v[3 * p + 2] = fma(Di[5], b2, fma(Di[4], b1, Di[2] * b0));
  }
  d4_t acc0[8], acc1[8];
#pragma unroll
  for (int c = 0; c < 8; c++) acc0[c] = acc1[c] = d4_t{0, 0, 0, 0};
  // edge prefetch registers (one edge per thread and pass; a sub-batch has at most kSchurSub * n_poses edges)
  double Bn[18];
  int pose_n = -1, lm_n = 0;
  auto fetch = [&](int sb_l0, int pass) {
    pose_n = -1;
    if (sb_l0 >= l_end) return;
    const int e0 = s_ptb[sb_l0 - l_begin], e1 = s_ptb[min(sb_l0 + kSchurSub, l_end) - l_begin];
    const int e = e0 + pass * kMk + tid;
    if (e < e1 && !(D.e_dup && D.e_dup[e] >= 0)) {  // (a duplicate's block has been added to its first edge's)
      pose_n = D.e_pose[e];
      lm_n = D.e_point[e];
      const double* B = D.Hpl + 18 * (size_t)e;
#pragma unroll
      for (int k = 0; k < 18; k++) Bn[k] = B[k];
    }
  };
  const int a_lo = 128 * bi, b_lo = 128 * bj;
  fetch(l_begin, 0);
  for (int l0 = l_begin; l0 < l_end; l0 += kSchurSub) {
    GFS_LDS_BARRIER();  // the previous sub-batch has been consumed (and s_v is complete the first time round)
    for (int i = tid; i < 2 * 3 * kSchurSub * kSchurLd / 2; i += kMk) ((double2*)s_a)[i] = double2{0.0, 0.0};  // s_a and s_b are adjacent
    GFS_LDS_BARRIER();
    const int e0 = s_ptb[l0 - l_begin], e1 = s_ptb[min(l0 + kSchurSub, l_end) - l_begin];
    const int npass = (e1 - e0 + kMk - 1) / kMk;
    for (int pass = 0; pass < npass; pass++) {
      if (pass > 0) fetch(l0, pass);
      if (pose_n >= 0) {
        const int f = s_free[pose_n], p = lm_n - l0;
        if (f >= 0) {
          const double* Di = s_dinv + 6 * (lm_n - l_begin);
          const double d9[9] = {Di[0], Di[1], Di[2], Di[1], Di[3], Di[4], Di[2], Di[4], Di[5]};
#pragma unroll
          for (int a = 0; a < 6; a++) {
            const int rg = 6 * f + a;  // global row
            const double b0 = Bn[3 * a], b1 = Bn[3 * a + 1], b2 = Bn[3 * a + 2];
            if ((unsigned)(rg - b_lo) < 128u) {
#pragma unroll
              for (int k = 0; k < 3; k++) s_b[(3 * p + k) * kSchurLd + rg - b_lo] = Bn[3 * a + k];
            }
            if ((unsigned)(rg - a_lo) < 128u) {
#pragma unroll
              for (int k = 0; k < 3; k++) s_a[(3 * p + k) * kSchurLd + rg - a_lo] = fma(b2, d9[6 + k], fma(b1, d9[3 + k], b0 * d9[k]));
            }
          }
        }
      }
    }
    // the extra row: Dinv_l b_l at global row n
    if ((unsigned)(n - a_lo) < 128u && tid < 3 * kSchurSub && l0 + tid / 3 < l_end)
      s_a[tid * kSchurLd + n - a_lo] = s_v[3 * (l0 - l_begin) + tid];
    fetch(l0 + kSchurSub, 0);  // the next sub-batch's edges travel while the products run
    GFS_LDS_BARRIER();
    if (kOneBlock || bi == bj) {
      switch (wave) {
        case 0: schur_mfma_ksteps<true, 0>(s_a, s_b, acc0, acc1); break;
        case 1: schur_mfma_ksteps<true, 1>(s_a, s_b, acc0, acc1); break;
        case 2: schur_mfma_ksteps<true, 2>(s_a, s_b, acc0, acc1); break;
        default: schur_mfma_ksteps<true, 3>(s_a, s_b, acc0, acc1); break;
      }
    } else {
      switch (wave) {
        case 0: schur_mfma_ksteps<false, 0>(s_a, s_b, acc0, acc1); break;
        case 1: schur_mfma_ksteps<false, 1>(s_a, s_b, acc0, acc1); break;
        case 2: schur_mfma_ksteps<false, 2>(s_a, s_b, acc0, acc1); break;
        default: schur_mfma_ksteps<false, 3>(s_a, s_b, acc0, acc1); break;
      }
    }
  }
  double* out = D.schur_part + (size_t)chunk * ld * ld + (size_t)a_lo * ld + b_lo;
  if (kOneBlock || bi == bj) {
    switch (wave) {
      case 0: schur_mfma_store<true, 0>(out, ld, acc0, acc1); break;
      case 1: schur_mfma_store<true, 1>(out, ld, acc0, acc1); break;
      case 2: schur_mfma_store<true, 2>(out, ld, acc0, acc1); break;
      default: schur_mfma_store<true, 3>(out, ld, acc0, acc1); break;
    }
  } else {
    switch (wave) {
      case 0: schur_mfma_store<false, 0>(out, ld, acc0, acc1); break;
      case 1: schur_mfma_store<false, 1>(out, ld, acc0, acc1); break;
      case 2: schur_mfma_store<false, 2>(out, ld, acc0, acc1); break;
      default: schur_mfma_store<false, 3>(out, ld, acc0, acc1); break;
    }
  }
}
template <bool kOneBlock>
__global__ __launch_bounds__(kMk, kOneBlock ? 2 : 1) void k_lba_schur_mfma(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_schur_mfma<kOneBlock>(D, blockIdx.x);
}

// the reduction for b_schur_mfma's partial blocks: Hs entry (r, c), r >= c, and bs[c] = bp[c] - S[n][c]
__device__ __forceinline__ void b_schur_reduce_mfma(const LbaDev& D, const int bx) {
  const int F = D.n_free, n = 6 * F, ntri = n * (n + 1) / 2;
  const int NB = (n + 1 + 127) / 128, ld = 128 * NB;
  const int k = bx * kMk + threadIdx.x;
  if (k >= ntri + n) return;
  int r, c;
  if (k < ntri) {
    r = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > k) r--;
    while ((r + 1) * (r + 2) / 2 <= k) r++;
    c = k - r * (r + 1) / 2;
  } else {
    r = n;
    c = k - ntri;
  }
  const double* part = D.schur_part + (size_t)r * ld + c;
  double sum = 0;
  for (int ch = 0; ch < D.n_schur_chunks; ch++) sum += part[(size_t)ch * ld * ld];
  if (k >= ntri) {
    D.bs[c] = D.bp[c] - sum;
  } else {
    const int i1 = r / 6, a = r - 6 * i1, i2 = c / 6, cc = c - 6 * i2;
    if (i1 != i2) {
      D.Hs[k] = -sum;
    } else {
      const double hpp = D.Hpp[21 * i1 + (cc * 6 - cc * (cc - 1) / 2 + (a - cc))];
      D.Hs[k] = hpp + (a == cc ? D.S->lambda : 0.0) - sum;
    }
  }
}
__global__ __launch_bounds__(kMk) void k_lba_schur_reduce_mfma(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_schur_reduce_mfma(D, blockIdx.x);
}

// Hs = [diagonal block](Hpp + lambda I) - sum over chunks (in chunk order), bs = bp - sum: one thread per entry of the packed
// lower triangle, then one per entry of the right-hand side
__device__ __forceinline__ void b_schur_reduce(const LbaDev& D, const int bx) {
  const int F = D.n_free, n = 6 * F, ntri = n * (n + 1) / 2, npairs = F * (F + 1) / 2;
  const int k = bx * kMk + threadIdx.x;
  if (k < ntri) {
    int r = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > k) r--;
    while ((r + 1) * (r + 2) / 2 <= k) r++;
    const int c = k - r * (r + 1) / 2;
    const int i1 = r / 6, a = r - 6 * i1, i2 = c / 6, cc = c - 6 * i2;
    const double* part = D.schur_part + ((size_t)(i1 * (i1 + 1) / 2 + i2)) * 36 + 6 * a + cc;
    double sum = 0;
    for (int ch = 0; ch < D.n_schur_chunks; ch++) sum += part[(size_t)ch * npairs * 36];
    if (i1 != i2) {
      D.Hs[k] = -sum;
    } else {  // a >= cc: Hpp's upper-triangle entry (cc, a)
      const double hpp = D.Hpp[21 * i1 + (cc * 6 - cc * (cc - 1) / 2 + (a - cc))];
      D.Hs[k] = hpp + (a == cc ? D.S->lambda : 0.0) - sum;
    }
  } else if (k < ntri + n) {
    const int j = k - ntri;
    double sum = 0;
    for (int ch = 0; ch < D.n_schur_chunks; ch++) sum += D.schur_part_b[(size_t)ch * n + j];
    D.bs[j] = D.bp[j] - sum;
  }
}
__global__ __launch_bounds__(kMk) void k_lba_schur_reduce(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_schur_reduce(D, blockIdx.x);
}



// LDL^T + triangular solves of the reduced pose system by a single workgroup, 6-wide block columns (n = 6 n_free).  Two solvers
// with two arithmetics; a window takes the one its size selects (kMaxFreeLds), alone or in a batch, so its result does not depend
// on its company:
//  - b_solve_lds: the packed triangle fits the 160 KB of LDS (n <= 180, i.e. up to 30 free poses) and is factored there, with
//    reciprocal pivots and fused multiply-adds;
//  - b_solve_hbm (larger windows): factored in place in HBM / L2 with divisions and separately rounded products, the subtraction
//    sequence of the column-by-column form.
// The reference solves this system with a sparse Cholesky (g2o LinearSolverEigen): there is no operation order to follow in
// either, only a fixed one to keep.
//
// The reduced system in LDS (n <= 180): LDL^T by 6-wide block columns with the pivots' reciprocals and the scaled panel
// P = L D kept beside L, so that a panel row costs 15 fused multiply-adds + 6 products instead of 6 dependent divisions and the
// trailing update 6 fused multiply-adds an entry; the forward substitution rides along with the factorisation (the right-hand
// side is one more row of every panel), and the backward substitution is done by a single wave (n values, no workgroup
// barriers).
__device__ __forceinline__ void b_solve_lds(const LbaDev& D) {
  extern __shared__ __align__(16) double lds[];
  __shared__ int s_flag;
  __shared__ double s_w[6][6], s_y[6];
  const int n = 6 * D.n_free;
  double* Hs = lds;                               // packed lower triangle, L in place
  double* bs = Hs + (size_t)n * (n + 1) / 2;      // [n]
  double* invd = bs + n;                          // [n] 1 / d
  double* pan = invd + n;                         // [n][6] P = L D of the current block column
  // (eight loads in flight: as a plain loop the 7 trips of a 120-row system are 7 dependent round trips)
  gfs::strided_batch<8>(D.Hs, (int)threadIdx.x, kThreads, n * (n + 1) / 2, [&](int k, double v) { Hs[k] = v; });
  for (int k = threadIdx.x; k < n; k += kThreads) bs[k] = D.bs[k];
  if (threadIdx.x == 0) s_flag = 0;
  __syncthreads();
  bool ok = true;
  for (int jb = 0; jb < n; jb += 6) {
    if (threadIdx.x == 0) {  // (a) the 6x6 diagonal block and the block's share of the forward substitution, on one lane
      double a[6][6], y[6];
#pragma unroll
      for (int i = 0; i < 6; i++) {
        y[i] = bs[jb + i];
#pragma unroll
        for (int k = 0; k <= i; k++) a[i][k] = Hs[tri(jb + i, jb + k)];
      }
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const double d = a[c][c];
        if (d == 0.0 || !isfinite(d)) bad = true;
        const double r = bad ? 0.0 : 1.0 / d;
        invd[jb + c] = r;
#pragma unroll
        for (int i = c + 1; i < 6; i++) {
          const double p = a[i][c];  // = L(i,c) d
          s_w[i][c] = p;
          a[i][c] = p * r;
        }
#pragma unroll
        for (int k = c + 1; k < 6; k++)
#pragma unroll
          for (int i = k; i < 6; i++) a[i][k] = fma(-a[i][c], s_w[k][c], a[i][k]);
      }
      if (bad) s_flag = 1;
#pragma unroll
      for (int c = 0; c < 6; c++)
#pragma unroll
        for (int c2 = 0; c2 < c; c2++) y[c] = fma(-a[c][c2], y[c2], y[c]);
#pragma unroll
      for (int i = 0; i < 6; i++) {
        bs[jb + i] = y[i];
        s_y[i] = y[i];
#pragma unroll
        for (int k = 0; k <= i; k++) Hs[tri(jb + i, jb + k)] = a[i][k];
      }
    }
    __syncthreads();
    if (s_flag) {
      ok = false;
      break;
    }
    for (int i = jb + 6 + threadIdx.x; i < n; i += kThreads) {  // (b) panel rows: P(i,c) and L(i,c) = P(i,c) / d_c, and bs[i]
      double l[6], acc = bs[i];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double v = Hs[tri(i, jb + c)];
#pragma unroll
        for (int c2 = 0; c2 < c; c2++) v = fma(-l[c2], s_w[c][c2], v);
        pan[6 * (i - jb - 6) + c] = v;
        l[c] = v * invd[jb + c];
        Hs[tri(i, jb + c)] = l[c];
        acc = fma(-l[c], s_y[c], acc);
      }
      bs[i] = acc;
    }
    __syncthreads();
    const int m = n - jb - 6;  // (c) trailing size
    for (int k = threadIdx.x; k < m * (m + 1) / 2; k += kThreads) {
      int r = (int)((sqrtf(8.0f * (float)k + 1.0f) - 1.0f) * 0.5f);  // (a guess: the two loops settle it)
      while (r * (r + 1) / 2 > k) r--;
      while ((r + 1) * (r + 2) / 2 <= k) r++;
      const int c = k - r * (r + 1) / 2;
      const int ii = jb + 6 + r, kk = jb + 6 + c;
      double v = Hs[tri(ii, kk)];
#pragma unroll
      for (int c2 = 0; c2 < 6; c2++) v = fma(-pan[6 * r + c2], Hs[tri(kk, jb + c2)], v);
      Hs[tri(ii, kk)] = v;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) D.S->solve_ok = ok ? 1 : 0;
  if (!ok || threadIdx.x >= 64) return;
  // one wave from here on: z = D^-1 y, then L^T x = z from the last block up (LDS accesses of one wave keep their order)
  const int lane = threadIdx.x;
  for (int i = lane; i < n; i += 64) bs[i] *= invd[i];
  for (int jb = n - 6; jb >= 0; jb -= 6) {
    if (lane == 0) {
      double y[6], l[6][6];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        y[c] = bs[jb + c];
#pragma unroll
        for (int c2 = c + 1; c2 < 6; c2++) l[c2][c] = Hs[tri(jb + c2, jb + c)];
      }
#pragma unroll
      for (int c = 5; c >= 0; c--)
#pragma unroll
        for (int c2 = 5; c2 > c; c2--) y[c] = fma(-l[c2][c], y[c2], y[c]);
#pragma unroll
      for (int c = 0; c < 6; c++) bs[jb + c] = y[c];
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < jb; i += 64) {
      double v = bs[i];
#pragma unroll
      for (int c = 5; c >= 0; c--) v = fma(-Hs[tri(jb + c, i)], bs[jb + c], v);
      bs[i] = v;
    }
    __builtin_amdgcn_wave_barrier();
  }
  for (int i = lane; i < n; i += 64) D.xp[i] = bs[i];
}

// The reduced system in HBM / L2 (n > 180), factored in place: only the right-hand side and the current 6-column panel are held
// in LDS, so the trailing update reads and writes each element once.
__device__ __forceinline__ void b_solve_hbm(const LbaDev& D) {
  extern __shared__ __align__(16) double lds[];
  __shared__ int s_flag;
  const int n = 6 * D.n_free;
  double* Hs = D.Hs;
  double* bs = lds;       // [n]
  double* pan = lds + n;  // panel rows [n][6] followed by the 6 pivots
  for (int k = threadIdx.x; k < n; k += kThreads) bs[k] = D.bs[k];
  if (threadIdx.x == 0) s_flag = 0;
  __syncthreads();
  // LDL^T by 6-wide block columns (n = 6 n_free): every entry sees the same subtraction sequence as in the column-by-column
  // form, but a block step costs 3 barriers instead of 18:
  //   (a) the 6x6 diagonal block is factored by one lane, (b) every row below solves its 6 entries against it (rows are
  //   independent), (c) the trailing triangle takes the rank-6 update.
  bool ok = true;
  for (int jb = 0; jb < n && ok; jb += 6) {
    if (threadIdx.x == 0) {  // the 21 entries are pulled into registers first: one memory latency instead of ~100 dependent ones
      double a[6][6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k <= i; k++) a[i][k] = Hs[tri(jb + i, jb + k)];
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const double d = a[c][c];
        if (d == 0.0 || !isfinite(d)) bad = true;
        if (!bad) {
#pragma unroll
          for (int i = c + 1; i < 6; i++) a[i][c] /= d;
#pragma unroll
          for (int k = c + 1; k < 6; k++)
#pragma unroll
            for (int i = k; i < 6; i++) a[i][k] -= a[i][c] * a[k][c] * d;
        }
      }
      if (bad) s_flag = 1;
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k <= i; k++) Hs[tri(jb + i, jb + k)] = a[i][k];
    }
    __syncthreads();
    if (s_flag) {
      ok = false;
      break;
    }
    for (int i = jb + 6 + threadIdx.x; i < n; i += kThreads) {  // (b) panel rows
      for (int c = 0; c < 6; c++) {
        double v = Hs[tri(i, jb + c)];
        for (int c2 = 0; c2 < c; c2++) v -= Hs[tri(i, jb + c2)] * Hs[tri(jb + c, jb + c2)] * Hs[tri(jb + c2, jb + c2)];
        Hs[tri(i, jb + c)] = v / Hs[tri(jb + c, jb + c)];
      }
    }
    __syncthreads();
    const int m = n - jb - 6;  // (c) trailing size; panel and pivots into LDS: the update then touches HBM once per element
    for (int k = threadIdx.x; k < 6 * m; k += kThreads) pan[k] = Hs[tri(jb + 6 + k / 6, jb + k % 6)];
    if (threadIdx.x < 6) pan[6 * m + threadIdx.x] = Hs[tri(jb + threadIdx.x, jb + threadIdx.x)];
    __syncthreads();
    for (int k = threadIdx.x; k < m * (m + 1) / 2; k += kThreads) {
      int r = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
      while (r * (r + 1) / 2 > k) r--;
      while ((r + 1) * (r + 2) / 2 <= k) r++;
      const int c = k - r * (r + 1) / 2;
      const int ii = jb + 6 + r, kk = jb + 6 + c;
      double v = Hs[tri(ii, kk)];
      for (int c2 = 0; c2 < 6; c2++) v -= pan[6 * r + c2] * pan[6 * c + c2] * pan[6 * m + c2];
      Hs[tri(ii, kk)] = v;
    }
    __syncthreads();
  }
  if (ok) {
    // forward substitution (unit lower), block by block: the 6 unknowns of a block on one lane, then all rows below
    for (int jb = 0; jb < n; jb += 6) {
      if (threadIdx.x == 0) {
        double y[6], l[6][6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
          y[c] = bs[jb + c];
#pragma unroll
          for (int c2 = 0; c2 < c; c2++) l[c][c2] = Hs[tri(jb + c, jb + c2)];
        }
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
          for (int c2 = 0; c2 < c; c2++) y[c] -= l[c][c2] * y[c2];
#pragma unroll
        for (int c = 0; c < 6; c++) bs[jb + c] = y[c];
      }
      __syncthreads();
      for (int i = jb + 6 + threadIdx.x; i < n; i += kThreads) {
        double v = bs[i];
        for (int c = 0; c < 6; c++) v -= Hs[tri(i, jb + c)] * bs[jb + c];
        bs[i] = v;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += kThreads) bs[i] /= Hs[tri(i, i)];
    __syncthreads();
    // backward substitution with L^T, from the last block up
    for (int jb = n - 6; jb >= 0; jb -= 6) {
      if (threadIdx.x == 0) {
        double y[6], l[6][6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
          y[c] = bs[jb + c];
#pragma unroll
          for (int c2 = c + 1; c2 < 6; c2++) l[c2][c] = Hs[tri(jb + c2, jb + c)];
        }
#pragma unroll
        for (int c = 5; c >= 0; c--)
#pragma unroll
          for (int c2 = 5; c2 > c; c2--) y[c] -= l[c2][c] * y[c2];
#pragma unroll
        for (int c = 0; c < 6; c++) bs[jb + c] = y[c];
      }
      __syncthreads();
      for (int i = threadIdx.x; i < jb; i += kThreads) {
        double v = bs[i];
        for (int c = 5; c >= 0; c--) v -= Hs[tri(jb + c, i)] * bs[jb + c];
        bs[i] = v;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += kThreads) D.xp[i] = bs[i];
  }
  if (threadIdx.x == 0) D.S->solve_ok = ok ? 1 : 0;
}
template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_lba_solve(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  if (kLds)
    b_solve_lds(D);
  else
    b_solve_hbm(D);
}


// landmark back-substitution, update of the trial estimate, computeScale partial sums
__device__ __forceinline__ void b_update(const LbaDev& D, const int bx, const int gdx) {
  __shared__ double s4[4];
  const LbaState& S = *D.S;
  double loc = 0;
  if (S.solve_ok) {
    const int cur = S.cur;
    const double *q = sel(D.q, D.q_try, cur), *t = sel(D.t, D.t_try, cur), *X = sel(D.X, D.X_try, cur);
    double *qn = sel(D.q, D.q_try, cur ^ 1), *tn = sel(D.t, D.t_try, cur ^ 1), *Xn = sel(D.X, D.X_try, cur ^ 1);
    const double lambda = S.lambda;
    const int l = bx * kMk + threadIdx.x;
    if (l < D.n_points) {
      double cl[3] = {D.bl[3 * (size_t)l], D.bl[3 * (size_t)l + 1], D.bl[3 * (size_t)l + 2]};
      // (edges in order, the same subtractions as a plain loop; but a plain loop is one chain of three dependent round trips an
      //  edge -- pose index, free index, block -- for ~16 edges a landmark: four edges' indices and two edges' blocks are asked for
      //  together, round 5)
      const int e_end = D.pt_begin[l + 1];
      for (int eb = D.pt_begin[l]; eb < e_end; eb += 4) {
        int ep[4], f[4];
#pragma unroll
        for (int u = 0; u < 4; u++) ep[u] = D.e_pose[min(eb + u, e_end - 1)];
#pragma unroll
        for (int u = 0; u < 4; u++) f[u] = eb + u < e_end ? D.free_index[ep[u]] : -1;
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
          double Bv[2][18], xv[2][6];
#pragma unroll
          for (int u = 0; u < 2; u++) {
            const int e = min(eb + 2 * h2 + u, e_end - 1), ff = max(f[2 * h2 + u], 0);
#pragma unroll
            for (int k = 0; k < 18; k++) Bv[u][k] = D.Hpl[18 * (size_t)e + k];
#pragma unroll
            for (int a = 0; a < 6; a++) xv[u][a] = D.xp[6 * ff + a];
          }
#pragma unroll
          for (int u = 0; u < 2; u++) {
            if (f[2 * h2 + u] < 0) continue;
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
              for (int a = 0; a < 6; a++) cl[c] -= Bv[u][3 * a + c] * xv[u][a];
          }
        }
      }
      const double* Di = D.Dinv + 6 * (size_t)l;
      const double xl[3] = {Di[0] * cl[0] + Di[1] * cl[1] + Di[2] * cl[2], Di[1] * cl[0] + Di[3] * cl[1] + Di[4] * cl[2],
                            Di[2] * cl[0] + Di[4] * cl[1] + Di[5] * cl[2]};
      for (int c = 0; c < 3; c++) {
        D.xl[3 * (size_t)l + c] = xl[c];
        Xn[3 * (size_t)l + c] = X[3 * (size_t)l + c] + xl[c];
        loc += xl[c] * (lambda * xl[c] + D.bl[3 * (size_t)l + c]);
      }
    }
    if (bx == 0) {
      for (int f = threadIdx.x; f < D.n_free; f += kMk) {
        const int p = D.free_pose[f];
        pose_oplus(q + 4 * p, t + 3 * p, D.xp + 6 * f, qn + 4 * p, tn + 3 * p);
        for (int a = 0; a < 6; a++) loc += D.xp[6 * f + a] * (lambda * D.xp[6 * f + a] + D.bp[6 * f + a]);
      }
    }
  }
  const double tot = gfs_red::block_sum256(loc, s4);
  if (threadIdx.x == 0) D.part_scale[bx] = tot;
}
__global__ __launch_bounds__(kMk) void k_lba_update(LbaDev D, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_update(D, blockIdx.x, gridDim.x);
}


// end of an LM trial (and, when the trial loop ends, of the iteration): rho test, lambda update, termination tests
__device__ __forceinline__ void b_decide(const LbaDev& D, const int bx, int force_end, int* __restrict__ host_flags,
                                         double* __restrict__ snap = nullptr) {
  if (threadIdx.x != 0 || bx != 0) return;
  LbaState& S = *D.S;
  if (!force_end) {
    double temp_chi = 0, scale = 0;
    for (int b = 0; b < D.n_err_blocks; b++) temp_chi += D.part_chi[b];
    for (int b = 0; b < D.n_upd_blocks; b++) scale += D.part_scale[b];
    if (!S.solve_ok) {
      temp_chi = 1.79769313486231570e308;
      scale = 0;
    }
    S.temp_chi = temp_chi;
    S.rho = (S.current_chi - temp_chi) / (scale + 1e-3);
    if (S.rho > 0 && isfinite(temp_chi)) {
      double alpha = 1. - gfs_glibc::pow3(2 * S.rho - 1);
      alpha = fmin(alpha, 2. / 3.);
      S.lambda *= fmax(1. / 3., alpha);
      S.ni = 2;
      S.current_chi = temp_chi;
      S.cur ^= 1;  // discardTop: the trial becomes the estimate
      S.err_at_cur = 1;
    } else {
      S.lambda *= S.ni;
      S.ni *= 2;
      S.err_at_cur = 0;  // (the arrays hold the rejected trial's values)
    }
    S.qmax++;
    S.again = (S.rho < 0 && S.qmax < 10) ? 1 : 0;
  } else {
    S.again = 0;  // the stop flag ended the trial loop
    S.err_at_cur = 0;
  }
  S.terminate = 0;
  if (!S.again) {
    S.iters++;
    S.last_chi = S.current_chi;
    if (S.qmax == 10 || S.rho == 0) {
      S.terminate = 1;
    } else {
      if ((S.ini_chi - S.current_chi) * 1e3 < S.ini_chi)
        S.n_bad++;
      else
        S.n_bad = 0;
      if (S.n_bad >= 3) S.terminate = 1;
    }
  }
  S.spec_ok = (!S.again && !S.terminate && !force_end) ? 1 : 0;
  host_flags[0] = S.again;
  host_flags[1] = S.terminate;
  host_flags[2] = S.cur;
  host_flags[3] = S.iters;
  if (snap) {  // what k_lba_finish reports if the loop ends HERE (gfs_lba_solve: an iteration running ahead of a stop flag is discarded)
    snap[0] = S.lambda;
    snap[1] = S.last_chi;
  }
}
// host_out: one slot of gfs_lba::h_flags -- {again, terminate, cur, iters} and, 16 bytes on, {lambda, last_chi}
__global__ void k_lba_decide(LbaDev D, int force_end, int* __restrict__ host_out, int gate) {
  if (gate && !D.S->spec_ok) return;
  b_decide(D, blockIdx.x, force_end, host_out, reinterpret_cast<double*>(host_out + 4));
}
// the state k_lba_decide left behind an earlier iteration, put back (an iteration that ran ahead of the caller's stop flag is discarded:
// its trial only wrote the OTHER estimate buffer); the errors are evaluated again at that estimate by the caller
__global__ void k_lba_restore(LbaDev D, int cur, int iters, double lambda, double last_chi) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  LbaState& S = *D.S;
  S.cur = cur;
  S.iters = iters;
  S.lambda = lambda;
  S.last_chi = last_chi;
  S.err_at_cur = 0;
  S.spec_ok = 0;
}


__device__ __forceinline__ void b_finish(const LbaDev& D, const int bx) {
  if (threadIdx.x != 0 || bx != 0) return;
  const LbaState& S = *D.S;
  D.out_info[0] = S.iters;
  D.out_info[1] = S.cur;
  D.out_stats[0] = D.mode == 1 ? S.current_chi : S.last_chi;
  D.out_stats[1] = D.mode == 1 ? 0.0 : S.lambda;
}
__global__ void k_lba_finish(LbaDev D) { b_finish(D, blockIdx.x); }

// the results of a window gathered into one block (one copy to the host instead of six): layout of LbaDev::out_pack
__device__ __forceinline__ void b_pack(const LbaDev& D, const int bx, const int gdx) {
  const int cur = D.out_info[1];  // which estimate buffer holds the accepted state (b_finish)
  const double *q = sel(D.q, D.q_try, cur), *t = sel(D.t, D.t_try, cur), *X = sel(D.X, D.X_try, cur);
  const int E = D.n_edges, NQ = D.n_poses, NP = D.n_points;
  double* o = D.out_pack;
  const int g = bx * kMk + threadIdx.x, G = gdx * kMk;
  for (int i = g; i < E; i += G) o[i] = D.chi2[i];
  o += E;
  for (int i = g; i < 4 * NQ; i += G) o[i] = q[i];
  o += 4 * NQ;
  for (int i = g; i < 3 * NQ; i += G) o[i] = t[i];
  o += 3 * NQ;
  for (int i = g; i < 3 * NP; i += G) o[i] = X[i];
  o += 3 * NP;
  if (g == 0) {
    o[0] = D.out_stats[0];
    o[1] = D.out_stats[1];
    o[2] = (double)D.out_info[0];
    o[3] = (double)cur;
  }
}
__global__ __launch_bounds__(kMk) void k_lba_pack(LbaDev D) { b_pack(D, blockIdx.x, gridDim.x); }


// ------------------------------------------------------------------------------------------------
// Batched windows (gfs_lba_solve_batch): the same phase kernels with the window index in blockIdx.y.  Every window carries its
// own LM state machine (LbaState::phase: 0 = build the system next, 1 = a trial step next, 2 = done); the host launches
// "rounds" of [build group][trial group] over all windows, a kernel leaves at once when its window is in another phase or its
// block index is beyond that window's size.  Same bodies, same arithmetic: a window's result does not depend on the batch.
// ------------------------------------------------------------------------------------------------
#define GFS_LBAB_PROLOGUE(PHASE, NEED)                         \
  const LbaDev D = DD[blockIdx.y];                             \
  if (D.S->phase != (PHASE)) return;                           \
  const int need = (NEED);                                     \
  if ((int)blockIdx.x >= need) return;

__global__ __launch_bounds__(kMk) void kb_lba_init(const LbaDev* __restrict__ DD) {
  const LbaDev D = DD[blockIdx.y];
  b_init(D, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(kMk) void kb_lba_errors(const LbaDev* __restrict__ DD, int trial) {
  GFS_LBAB_PROLOGUE(trial ? 1 : 0, D.n_err_blocks)
  b_errors(D, blockIdx.x, need, trial);
}
__global__ __launch_bounds__(kMk) void kb_lba_build_landmarks(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(0, D.n_lm_wg)
  b_build_landmarks(D, blockIdx.x, need);
}
__global__ __launch_bounds__(kPoseWg) void kb_lba_build_poses(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(0, D.n_free)
  b_build_poses(D, blockIdx.x, need);
}
__global__ __launch_bounds__(kThreads) void kb_lba_begin(const LbaDev* __restrict__ DD, int* __restrict__ n_done) {
  GFS_LBAB_PROLOGUE(0, 1)
  b_begin(D, blockIdx.x, need, D.S->it);
  __syncthreads();
  if (threadIdx.x == 0) {
    LbaState& S = *D.S;
    if (D.iterations <= 0) {
      // optimize(0): the errors have been evaluated, nothing else happens to this window (what gfs_lba_solve reports for it:
      // the chi2 of the initial estimate, lambda 0, no iteration)
      S.last_chi = S.current_chi;
      S.lambda = 0;
      S.phase = 2;
      atomicAdd(n_done, 1);
    } else {
      S.phase = 1;  // the build group is complete for this window: trials follow
    }
  }
}
__global__ __launch_bounds__(kMk) void kb_lba_dinv(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(1, D.n_upd_blocks)
  b_dinv(D, blockIdx.x, need);
}
__global__ __launch_bounds__(kMk) void kb_lba_schur(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(1, (D.schur_sub || D.schur_mfma) ? 0 : D.n_free * (D.n_free + 1) / 2)
  b_schur(D, blockIdx.x, need);
}
__global__ __launch_bounds__(kMk) void kb_lba_schur_chunks(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(1, D.schur_sub ? D.n_schur_chunks * D.n_pair_tiles : 0)
  b_schur_chunks(D, blockIdx.x);
}
__global__ __launch_bounds__(kMk) void kb_lba_schur_reduce(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(1, D.schur_sub ? (6 * D.n_free * (6 * D.n_free + 1) / 2 + 6 * D.n_free + kMk - 1) / kMk : 0)
  b_schur_reduce(D, blockIdx.x);
}
template <bool kOneBlock>
__global__ __launch_bounds__(kMk, kOneBlock ? 2 : 1) void kb_lba_schur_mfma(const LbaDev* __restrict__ DD) {
  // every window takes the instance gfs_lba_solve would launch for it (one 128 x 128 block of pose pairs or several), whatever
  // else is in the batch: the host launches both instances when the batch mixes the two kinds
  GFS_LBAB_PROLOGUE(1, D.schur_mfma && (D.n_pair_tiles == 1) == kOneBlock ? D.n_schur_chunks * D.n_pair_tiles : 0)
  b_schur_mfma<kOneBlock>(D, blockIdx.x);
}
__global__ __launch_bounds__(kMk) void kb_lba_schur_reduce_mfma(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(1, D.schur_mfma ? (6 * D.n_free * (6 * D.n_free + 1) / 2 + 6 * D.n_free + kMk - 1) / kMk : 0)
  b_schur_reduce_mfma(D, blockIdx.x);
}
template <bool kLds>
__global__ __launch_bounds__(kThreads) void kb_lba_solve(const LbaDev* __restrict__ DD) {
  // every window takes the variant gfs_lba_solve would give it (the two differ in arithmetic), whatever else is in the batch
  GFS_LBAB_PROLOGUE(1, (D.n_free <= kMaxFreeLds) == kLds ? 1 : 0)
  if (kLds)
    b_solve_lds(D);
  else
    b_solve_hbm(D);
}
__global__ __launch_bounds__(kMk) void kb_lba_update(const LbaDev* __restrict__ DD) {
  GFS_LBAB_PROLOGUE(1, D.n_upd_blocks)
  b_update(D, blockIdx.x, need);
}
// end of a trial: the scalar LM logic of k_lba_decide, then the window's next phase (another trial, the next iteration's build,
// or done: optimize(iterations) ran out or the algorithm terminated)
__global__ void kb_lba_decide(const LbaDev* __restrict__ DD, int force_end, int* __restrict__ flags_all, int* __restrict__ n_done) {
  const LbaDev D = DD[blockIdx.x];
  if (threadIdx.x != 0 || D.S->phase != 1) return;
  b_decide(D, 0, force_end, flags_all + 4 * blockIdx.x);
  LbaState& S = *D.S;
  if (S.again) return;  // phase stays 1
  S.it++;
  if (S.terminate || S.it >= D.iterations || force_end) {
    S.phase = 2;
    atomicAdd(n_done, 1);
  } else {
    S.phase = 0;
  }
}
__global__ void kb_lba_finish(const LbaDev* __restrict__ DD) {
  const LbaDev D = DD[blockIdx.x];
  b_finish(D, 0);
}
__global__ __launch_bounds__(kMk) void kb_lba_pack(const LbaDev* __restrict__ DD) {
  const LbaDev D = DD[blockIdx.y];
  b_pack(D, blockIdx.x, gridDim.x);
}
#undef GFS_LBAB_PROLOGUE

}  // namespace
