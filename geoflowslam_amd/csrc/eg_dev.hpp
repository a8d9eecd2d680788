// Essential-graph optimisation (gfs_essential_graph_optimize; Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:2042-2413): the
// kernels in front of and behind the tiled factorisation of gba_dev.hpp.  Included by lba.hip behind gba_dev.hpp; eg_host.hpp queues
// them.  VertexSim3Expmap vertices, EdgeSim3 edges with information w I_7, no robust kernel, g2o's numeric Jacobians
// (core/base_binary_edge.hpp:147-200) through sim3_dev.hpp.  With _fix_scale column 6 of every Jacobian is exactly zero (both
// perturbations are the same estimate), so a free vertex then has 6 dimensions and the system none for the scale.
//
// Per iteration:  k_eg_linearize   one edge a lane: residual, chi2, the Jacobian columns of its free vertices (through a workspace in
//                                  HBM: 98 doubles a lane would not stay in registers), then the edge's blocks
//                 k_eg_begin       g2o's bookkeeping at the top of solve(); the first lambda is the caller's (setUserLambdaInit)
// Per trial:      memset + k_eg_assemble   one wave per listed block of the lower triangle (eg_lists.hpp): the edge blocks summed in
//                                  list order = edge order, lambda on the diagonal, the right-hand side
//                 k_gba_diag ... k_gba_back   gba_dev.hpp, unchanged: they read D.S, D.xp and the GbaDev's n, T, tiles, W, rhs
//                 k_eg_update      one free vertex a lane: oplus into the other estimate buffer, its terms of computeScale
//                 k_eg_errors      chi2 of every edge at the trial estimate
//                 k_lba_decide     lba_dev.hpp, unchanged: D.part_chi is the per-edge chi2 and D.part_scale the per-vertex terms, so its
//                                  two sums run in edge order and in vertex order
// No atomics; every sum's order is fixed by the problem.
#pragma once
#include "sim3_dev.hpp"

namespace {

constexpr int kEgEdgeDoubles = 3 * 49 + 14;  // per edge: Hii, Hij, Hjj (row-major, row stride 7), bi, bj
constexpr int kEgWg = 64;                    // lanes of the one-edge-a-lane kernels: edges are few, one wave a workgroup spreads them

struct EgDev {
  int n_vert, n_edges, n_free, dim, fix_scale;
  double lambda_init;
  const GFS_GLOBAL int* free_index;  // [n_vert] -> free slot or -1
  const GFS_GLOBAL int* free_vert;   // [n_free] -> vertex
  const GFS_GLOBAL int* e_i;         // vertex 0 of the edge
  const GFS_GLOBAL int* e_j;         // vertex 1
  const GFS_GLOBAL double* e_meas;   // [n_edges][8]
  const GFS_GLOBAL double* e_w;
  GFS_GLOBAL double* est;            // [2][n_vert][8]: the estimate (LbaState::cur) and the trial
  GFS_GLOBAL double* chi2;           // [n_edges] of the last k_eg_linearize / k_eg_errors
  GFS_GLOBAL double* J;              // [n_edges][2][49] Jacobian workspace, row-major 7 x 7
  GFS_GLOBAL double* blocks;         // [n_edges][kEgEdgeDoubles]
  GFS_GLOBAL double* b;              // [dim n_free] the right-hand side as assembled (the solve works in place on GbaDev::rhs)
  GFS_GLOBAL double* scale;          // [n_free] computeScale terms of the last k_eg_update
  long long n_blocks;
  const GFS_GLOBAL int* blk_i;            // [n_blocks] free slots, blk_i >= blk_j
  const GFS_GLOBAL int* blk_j;
  const GFS_GLOBAL long long* blk_begin;  // [n_blocks + 1]
  const GFS_GLOBAL int* contrib;          // 4 edge + kind (eg_lists.hpp)
};

__device__ __forceinline__ void eg_load8(const GFS_GLOBAL double* p, double* o) {
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = p[k];
}

// the estimates (both buffers) from the caller's, as they came: g2o's setEstimate does not touch them
__global__ __launch_bounds__(kMk) void k_eg_init(EgDev E, const double* __restrict__ v0) {
  const size_t n = 8 * (size_t)E.n_vert;
  for (size_t k = (size_t)blockIdx.x * kMk + threadIdx.x; k < n; k += (size_t)gridDim.x * kMk) E.est[k] = E.est[n + k] = v0[k];
}

__global__ __launch_bounds__(kEgWg) void k_eg_errors(LbaDev D, EgDev E, int trial) {
  const LbaState& S = *D.S;
  if (trial && !S.solve_ok) return;
  const int e = blockIdx.x * kEgWg + threadIdx.x;
  if (e >= E.n_edges) return;
  const GFS_GLOBAL double* est = E.est + (size_t)(S.cur ^ trial) * 8 * E.n_vert;
  double C[8], v0[8], v1[8], err[7];
  eg_load8(E.e_meas + 8 * (size_t)e, C);
  eg_load8(est + 8 * (size_t)E.e_i[e], v0);
  eg_load8(est + 8 * (size_t)E.e_j[e], v1);
  gfs_sim3::sim3_edge_residual(C, v0, v1, err);
  const double w = E.e_w[e];
  double chi = 0;
  for (int k = 0; k < 7; k++) chi += err[k] * (w * err[k]);
  E.chi2[e] = chi;
}

__global__ __launch_bounds__(kEgWg) void k_eg_linearize(LbaDev D, EgDev E) {
  const int e = blockIdx.x * kEgWg + threadIdx.x;
  if (e >= E.n_edges) return;
  const GFS_GLOBAL double* est = E.est + (size_t)D.S->cur * 8 * E.n_vert;
  const int vi = E.e_i[e], vj = E.e_j[e];
  const bool free_i = E.free_index[vi] >= 0, free_j = E.free_index[vj] >= 0;
  double C[8], v0[8], v1[8], err[7];
  eg_load8(E.e_meas + 8 * (size_t)e, C);
  eg_load8(est + 8 * (size_t)vi, v0);
  eg_load8(est + 8 * (size_t)vj, v1);
  gfs_sim3::sim3_edge_residual(C, v0, v1, err);
  const double w = E.e_w[e];
  double chi = 0;
  for (int k = 0; k < 7; k++) chi += err[k] * (w * err[k]);
  E.chi2[e] = chi;
  if (!free_i && !free_j) return;
  // linearizeOplus: per free vertex and dimension the error at oplus(+delta e_d) minus the error at oplus(-delta e_d), times 1 / (2 delta)
  const double delta = gfs_sim3::kNumericDelta, scalar = 1.0 / (2 * delta);
  const int dim = E.dim;
  GFS_GLOBAL double* J = E.J + 98 * (size_t)e;
#pragma unroll 1
  for (int side = 0; side < 2; side++) {
    if (!(side ? free_j : free_i)) continue;
#pragma unroll 1
    for (int d = 0; d < dim; d++) {
      // (the moved vertex picked element by element: a pointer chosen at run time would put the estimates into scratch memory)
      double base[8], add[7], moved[8], a0[8], a1[8], ep[7], em[7];
#pragma unroll
      for (int k = 0; k < 8; k++) base[k] = side ? v1[k] : v0[k];
#pragma unroll 1
      for (int sign = 0; sign < 2; sign++) {
#pragma unroll
        for (int k = 0; k < 7; k++) add[k] = k == d ? (sign ? -delta : delta) : 0.0;
        gfs_sim3::sim3_oplus(base, add, E.fix_scale != 0, moved);
#pragma unroll
        for (int k = 0; k < 8; k++) a0[k] = side ? v0[k] : moved[k], a1[k] = side ? moved[k] : v1[k];
        gfs_sim3::sim3_edge_residual(C, a0, a1, em);
        if (sign == 0) {
#pragma unroll
          for (int k = 0; k < 7; k++) ep[k] = em[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 7; k++) J[49 * side + 7 * k + d] = scalar * (ep[k] - em[k]);
    }
  }
  // constructQuadraticForm (:55-90) with omega = w I: omega_r = -(w e); AtO = A^T omega; Hii += AtO A, Hij += AtO B, Hjj += (B^T omega) B,
  // b += J^T omega_r.  The blocks of a fixed vertex are never read.
  double omega_r[7];
  for (int k = 0; k < 7; k++) omega_r[k] = -(w * err[k]);
  GFS_GLOBAL double* out = E.blocks + (size_t)kEgEdgeDoubles * e;
  const GFS_GLOBAL double *A = J, *B = J + 49;
#pragma unroll 1
  for (int a = 0; a < dim; a++) {
    double At[7], Bt[7];
    for (int k = 0; k < 7; k++) {
      At[k] = free_i ? A[7 * k + a] * w : 0.0;
      Bt[k] = free_j ? B[7 * k + a] * w : 0.0;
    }
#pragma unroll 1
    for (int c = 0; c < dim; c++) {
      double hii = 0, hij = 0, hjj = 0;
      for (int k = 0; k < 7; k++) {
        const double ac = free_i ? A[7 * k + c] : 0.0, bc = free_j ? B[7 * k + c] : 0.0;
        hii += At[k] * ac;
        hij += At[k] * bc;
        hjj += Bt[k] * bc;
      }
      out[7 * a + c] = hii;
      out[49 + 7 * a + c] = hij;
      out[98 + 7 * a + c] = hjj;
    }
    double bi = 0, bj = 0;
    for (int k = 0; k < 7; k++) {
      bi += (free_i ? A[7 * k + a] : 0.0) * omega_r[k];
      bj += (free_j ? B[7 * k + a] : 0.0) * omega_r[k];
    }
    out[147 + a] = bi;
    out[154 + a] = bj;
  }
}

// top of OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-86): currentChi, and at iteration 0 the
// lambda computeLambdaInit returns when the user's is positive (:170-173)
__global__ void k_eg_begin(LbaDev D, EgDev E, int iteration) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  LbaState& S = *D.S;
  double chi = 0;
  for (int e = 0; e < E.n_edges; e++) chi += E.chi2[e];
  if (iteration == 0) {
    S.lambda = E.lambda_init;
    S.ni = 2;
    S.n_bad = 0;
  }
  S.current_chi = S.ini_chi = chi;
  S.rho = 0;
  S.qmax = 0;
  S.again = 0;
}

// One wave per listed block (bi, bj), bi >= bj: lane a * dim + c sums entry (a, c) over the block's list.  kind 0 / 1: the edge's Hii /
// Hjj on a diagonal block; 2: Hij as stored (free(i) > free(j)); 3: Hij transposed (free(i) < free(j)).  On a diagonal block the
// lanes behind the entries sum the right-hand side over the same list.  A block of dimension 7 may straddle tiles: every entry is
// addressed on its own.
__global__ __launch_bounds__(kMk) void k_eg_assemble(LbaDev D, EgDev E, GbaDev G) {
  if (blockIdx.x == 0) {  // the padded rows of the last tile: identity, zero right-hand side; and the trial's solve starts out fine
    const int last = G.T - 1;
    for (int r = G.n + (int)threadIdx.x; r < G.T * kP; r += kMk) {
      G.tiles[gba_sys::tile_offset(last, last) + (size_t)(r - last * kP) * (kP + 1)] = 1.0;
      G.rhs[r] = 0.0;
    }
    if (threadIdx.x == 0) D.S->solve_ok = 1;
  }
  const long long blk = (long long)blockIdx.x * (kMk / 64) + (threadIdx.x >> 6);
  if (blk >= E.n_blocks) return;
  const int lane = threadIdx.x & 63, dim = E.dim;
  const int bi = E.blk_i[blk], bj = E.blk_j[blk];
  const long long k0 = E.blk_begin[blk], k1 = E.blk_begin[blk + 1];
  if (lane < dim * dim) {
    const int a = lane / dim, c = lane - dim * a;
    if (bi == bj && a < c) return;  // only the lower triangle of a diagonal tile is meaningful
    double acc = 0;
    for (long long k = k0; k < k1; k++) {
      const int ck = E.contrib[k], kind = ck & 3;
      const GFS_GLOBAL double* blkp = E.blocks + (size_t)kEgEdgeDoubles * (ck >> 2);
      acc += kind == 0 ? blkp[7 * a + c] : kind == 1 ? blkp[98 + 7 * a + c] : kind == 2 ? blkp[49 + 7 * a + c] : blkp[49 + 7 * c + a];
    }
    if (bi == bj && a == c) acc += D.S->lambda;
    G.tiles[gba_sys::elem_offset((size_t)dim * bi + a, (size_t)dim * bj + c)] = acc;
  } else if (bi == bj && lane < dim * dim + dim) {
    const int a = lane - dim * dim;
    double acc = 0;
    for (long long k = k0; k < k1; k++) {
      const int ck = E.contrib[k];
      acc += E.blocks[(size_t)kEgEdgeDoubles * (ck >> 2) + ((ck & 3) == 0 ? 147 : 154) + a];
    }
    G.rhs[(size_t)dim * bi + a] = acc;
    E.b[(size_t)dim * bi + a] = acc;
  }
}

// the step applied: every free vertex's oplus into the other buffer and its terms of computeScale, sum x (lambda x + b)
__global__ __launch_bounds__(kEgWg) void k_eg_update(LbaDev D, EgDev E) {
  const LbaState& S = *D.S;
  const int f = blockIdx.x * kEgWg + threadIdx.x;
  if (f >= E.n_free) return;
  if (!S.solve_ok) {
    E.scale[f] = 0;
    return;
  }
  const int v = E.free_vert[f], dim = E.dim;
  const size_t n8 = 8 * (size_t)E.n_vert;
  double est[8], u[7], out[8], loc = 0;
  eg_load8(E.est + (size_t)S.cur * n8 + 8 * (size_t)v, est);
#pragma unroll
  for (int a = 0; a < 7; a++) {
    u[a] = 0;
    if (a < dim) {
      const double x = D.xp[(size_t)dim * f + a];
      u[a] = x;
      loc += x * (S.lambda * x + E.b[(size_t)dim * f + a]);
    }
  }
  gfs_sim3::sim3_oplus(est, u, E.fix_scale != 0, out);
  GFS_GLOBAL double* o = E.est + (size_t)(S.cur ^ 1) * n8 + 8 * (size_t)v;
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = out[k];
  E.scale[f] = loc;
}

// The map points behind the poses (src/Optimizer.cc:2387-2409): correctedSwr.map(Srw.map(P)) in double, cast to float.  before: the
// reference key-frame's Sim3 before the optimisation (Srw); after: its estimate after, inverted here (correctedSwr).  ref < 0: as is.
__global__ __launch_bounds__(kMk) void k_eg_correct_points(int m, const float* __restrict__ xyz, const int* __restrict__ ref,
                                                           const double* __restrict__ before, const double* __restrict__ after,
                                                           float* __restrict__ out) {
  const int i = blockIdx.x * kMk + threadIdx.x;
  if (i >= m) return;
  const int r = ref[i];
  const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  if (r < 0) {
    out[3 * (size_t)i] = x, out[3 * (size_t)i + 1] = y, out[3 * (size_t)i + 2] = z;
    return;
  }
  double Srw[8], Siw[8], Swr[8];
  for (int k = 0; k < 8; k++) Srw[k] = before[8 * (size_t)r + k], Siw[k] = after[8 * (size_t)r + k];
  gfs_sim3::sim3_inverse(Siw, Swr);
  const double P[3] = {(double)x, (double)y, (double)z};
  double Pr[3], Pw[3];
  gfs_sim3::sim3_map(Srw, P, Pr);
  gfs_sim3::sim3_map(Swr, Pr, Pw);
  for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = (float)Pw[k];
}

// the tiled system as the packed lower triangle is k_gba_pack_lower's (the test tap)

}  // namespace
