// Global bundle adjustment (gfs_gba_solve): the reduced pose system of a whole map, assembled from structure lists and factored
// tile by tile over the whole chip.  Included by lba.hip behind lba_dev.hpp, the kernels of the local bundle adjustment, whose
// descriptor (LbaDev), LM state and every other phase kernel (errors, build, begin, dinv, update, decide, finish) this path shares;
// gba_host.hpp queues them.
//
// Storage: gba_tiles.hpp (lower-triangle tiles of kP = 96 rows in HBM).  One launch per dependent step, no waiting between
// workgroups.  Per trial:
//   memset            the tiles to +0.0 (the factorisation works in place: every trial starts from zeros)
//   k_gba_assemble    one wave per listed block (gba_lists.hpp): Hs_ij = [i = j](Hpp_i + lambda I) - sum B_e1 Dinv_l B_e2^T over the
//                     block's list in list order, and on a diagonal block bs_i = bp_i - sum B_e Dinv_l bl_l over the pose's edges
//   per panel p:
//     k_gba_diag      (a) tile (p, p) factored L D L^T in LDS by one workgroup, column by column; the panel's share of the forward
//                         substitution y_p = L_pp^-1 b_p rides along
//     k_gba_panel     (b) one workgroup per tile (i, p), i > p: W = A_ip L_pp^-T row by row, L_ip = W D^-1 in place, W kept in the
//                         panel workspace; b_i -= L_ip y_p
//     k_gba_trail     (c) one workgroup per tile (i, j), i >= j > p: A_ij -= W_i L_jp^T on v_mfma_f64_16x16x4_f64, k ascending
//   k_gba_scale       z = D^-1 y
//   k_gba_back        per panel from the last: z_j -= L_qj^T x_q for every j < q (one workgroup a tile), and the workgroup of
//                     j = q - 1 goes on to solve L^T x = z on its diagonal tile
// Every sum has an order fixed by the problem and kP alone: no atomics, nothing depends on the grid or on timing.  A zero or
// non-finite pivot clears LbaState::solve_ok (the semantics of b_solve_lds / b_solve_hbm) and every later kernel of the trial
// leaves at once.
#pragma once
#include "gba_tiles.hpp"

namespace {

using gba_sys::kP;
constexpr int kGbaLd = kP + 1;  // LDS row stride of a staged tile: a column walk touches every bank once
constexpr size_t kGbaTileLds = (size_t)kP * kGbaLd * sizeof(double);

struct GbaDev {
  int n, T;               // rows of the reduced system (6 n_free), panels
  long long n_blocks;
  const GFS_GLOBAL int* blk_i;            // [n_blocks]
  const GFS_GLOBAL int* blk_j;
  const GFS_GLOBAL long long* blk_begin;  // [n_blocks + 1]
  const GFS_GLOBAL int* contrib;          // [.][2] edge pairs
  const GFS_GLOBAL long long* pose_begin; // [n_free + 1]
  const GFS_GLOBAL int* pose_edges;
  GFS_GLOBAL double* tiles;               // gba_tiles.hpp
  GFS_GLOBAL double* W;                   // [T][kP][kP] panel workspace: W_i = L_ip D of the current panel
  GFS_GLOBAL double* rhs;                 // [T kP] right-hand side, then y, z, x in place
};

// ---- Schur assembly ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMk) void k_gba_assemble(LbaDev D, GbaDev G) {
  if (blockIdx.x == 0) {  // the padded rows of the last tile: identity, zero right-hand side; and the trial's solve starts out fine
    const int last = G.T - 1;
    for (int r = G.n + (int)threadIdx.x; r < G.T * kP; r += kMk) {
      G.tiles[gba_sys::tile_offset(last, last) + (size_t)(r - last * kP) * (kP + 1)] = 1.0;
      G.rhs[r] = 0.0;
    }
    if (threadIdx.x == 0) D.S->solve_ok = 1;
  }
  const long long b = (long long)blockIdx.x * (kMk / 64) + (threadIdx.x >> 6);
  if (b >= G.n_blocks) return;
  const int lane = threadIdx.x & 63;
  const int i = G.blk_i[b], j = G.blk_j[b];
  const double lambda = D.S->lambda;
  if (lane < 36) {
    const int a = lane / 6, c = lane - 6 * a;
    double acc = 0;
    for (long long k = G.blk_begin[b]; k < G.blk_begin[b + 1]; k++) {
      const int e1 = G.contrib[2 * k], e2 = G.contrib[2 * k + 1];
      const GFS_GLOBAL double* Bi = D.Hpl + 18 * (size_t)e1 + 3 * a;
      const GFS_GLOBAL double* Bj = D.Hpl + 18 * (size_t)e2 + 3 * c;
      const GFS_GLOBAL double* Di = D.Dinv + 6 * (size_t)D.e_point[e1];
      const double b0 = Bi[0], b1 = Bi[1], b2 = Bi[2];
      const double bd0 = b0 * Di[0] + b1 * Di[1] + b2 * Di[2];
      const double bd1 = b0 * Di[1] + b1 * Di[3] + b2 * Di[4];
      const double bd2 = b0 * Di[2] + b1 * Di[4] + b2 * Di[5];
      acc += bd0 * Bj[0] + bd1 * Bj[1] + bd2 * Bj[2];
    }
    const size_t at = gba_sys::elem_offset(6 * (size_t)i + a, 6 * (size_t)j + c);
    if (i != j) {
      G.tiles[at] = -acc;
    } else if (a >= c) {  // Hpp's upper-triangle entry (c, a)
      const double hpp = D.Hpp[21 * (size_t)i + (c * 6 - c * (c - 1) / 2 + (a - c))];
      G.tiles[at] = hpp + (a == c ? lambda : 0.0) - acc;
    }
  } else if (lane < 42 && i == j) {
    const int a = lane - 36;
    double acc = 0;
    for (long long k = G.pose_begin[i]; k < G.pose_begin[i + 1]; k++) {
      const int e = G.pose_edges[k];
      const size_t l = (size_t)D.e_point[e];
      const GFS_GLOBAL double* B = D.Hpl + 18 * (size_t)e + 3 * a;
      const GFS_GLOBAL double* Di = D.Dinv + 6 * l;
      const GFS_GLOBAL double* bl = D.bl + 3 * l;
      const double b0 = B[0], b1 = B[1], b2 = B[2];
      const double bd0 = b0 * Di[0] + b1 * Di[1] + b2 * Di[2];
      const double bd1 = b0 * Di[1] + b1 * Di[3] + b2 * Di[4];
      const double bd2 = b0 * Di[2] + b1 * Di[4] + b2 * Di[5];
      acc += bd0 * bl[0] + bd1 * bl[1] + bd2 * bl[2];
    }
    G.rhs[6 * (size_t)i + a] = D.bp[6 * (size_t)i + a] - acc;
  }
}

// the tiled system as the packed lower triangle, row by row (the test tap; stream-ordered ahead of the factorisation)
__global__ __launch_bounds__(kMk) void k_gba_pack_lower(GbaDev G, double* __restrict__ out, double* __restrict__ out_b) {
  const size_t n = (size_t)G.n, total = n * (n + 1) / 2;
  for (size_t k = (size_t)blockIdx.x * kMk + threadIdx.x; k < total; k += (size_t)gridDim.x * kMk) {
    size_t r = (size_t)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > k) r--;
    while ((r + 1) * (r + 2) / 2 <= k) r++;
    out[k] = G.tiles[gba_sys::elem_offset(r, k - r * (r + 1) / 2)];
  }
  for (size_t k = (size_t)blockIdx.x * kMk + threadIdx.x; k < n; k += (size_t)gridDim.x * kMk) out_b[k] = G.rhs[k];
}

// ---- (a) the diagonal tile ------------------------------------------------------------------------------------------------------
// L D L^T of tile (p, p) in LDS: column c divides by the pivot and takes the rank-one update of what is to its right; the unit
// lower factor stays below the diagonal, D on it.  The right-hand side's rows follow each column (y = L^-1 b).
__global__ __launch_bounds__(kMk) void k_gba_diag(LbaDev D, GbaDev G, int p) {
  extern __shared__ __align__(16) double lds[];
  __shared__ double s_w[kP], s_l[kP], s_y[kP];
  if (!D.S->solve_ok) return;
  double* s_A = lds;  // [kP][kGbaLd]
  GFS_GLOBAL double* A = G.tiles + gba_sys::tile_offset(p, p);
  const int tid = threadIdx.x;
  for (int k = tid; k < kP * kP; k += kMk) s_A[(k / kP) * kGbaLd + k % kP] = A[k];
  if (tid < kP) s_y[tid] = G.rhs[(size_t)p * kP + tid];
  __syncthreads();
  bool ok = true;
  for (int c = 0; c < kP; c++) {
    const double d = s_A[c * kGbaLd + c];  // (every thread reads the same pivot: the branch is uniform)
    if (d == 0.0 || !isfinite(d)) {
      ok = false;
      break;
    }
    const int i = c + 1 + tid;
    if (i < kP) {
      const double w = s_A[i * kGbaLd + c], l = w / d;
      s_w[i] = w;
      s_l[i] = l;
      s_A[i * kGbaLd + c] = l;
      s_y[i] -= l * s_y[c];
    }
    __syncthreads();
    const int m = kP - 1 - c;
    for (int k = tid; k < m * m; k += kMk) {
      const int ii = c + 1 + k / m, kk = c + 1 + k % m;
      if (ii >= kk) s_A[ii * kGbaLd + kk] -= s_l[ii] * s_w[kk];
    }
    __syncthreads();
  }
  if (!ok) {
    if (tid == 0) D.S->solve_ok = 0;
    return;
  }
  for (int k = tid; k < kP * kP; k += kMk) A[k] = s_A[(k / kP) * kGbaLd + k % kP];
  if (tid < kP) G.rhs[(size_t)p * kP + tid] = s_y[tid];
}

// ---- (b) the tile column below it ---------------------------------------------------------------------------------------------
// A_ip = L_ip D L_pp^T = W L_pp^T: row r of W by forward substitution against the unit factor (k ascending), one thread a row.
__global__ __launch_bounds__(kMk) void k_gba_panel(LbaDev D, GbaDev G, int p) {
  extern __shared__ __align__(16) double lds[];
  if (!D.S->solve_ok) return;
  double* s_L = lds;                  // [kP][kGbaLd]  L_pp, D on its diagonal
  double* s_W = lds + kP * kGbaLd;    // [kP][kGbaLd]  A_ip, then W
  const int i = p + 1 + blockIdx.x, tid = threadIdx.x;
  const GFS_GLOBAL double* Lpp = G.tiles + gba_sys::tile_offset(p, p);
  GFS_GLOBAL double* A = G.tiles + gba_sys::tile_offset(i, p);
  GFS_GLOBAL double* Wo = G.W + (size_t)i * kP * kP;
  for (int k = tid; k < kP * kP; k += kMk) {
    s_L[(k / kP) * kGbaLd + k % kP] = Lpp[k];
    s_W[(k / kP) * kGbaLd + k % kP] = A[k];
  }
  __syncthreads();
  if (tid < kP) {
    double* w = s_W + tid * kGbaLd;
    for (int c = 1; c < kP; c++) {
      double v = w[c];
      const double* lc = s_L + c * kGbaLd;
      for (int k = 0; k < c; k++) v -= w[k] * lc[k];
      w[c] = v;
    }
    double b = G.rhs[(size_t)i * kP + tid];
    for (int c = 0; c < kP; c++) b -= (w[c] / s_L[c * kGbaLd + c]) * G.rhs[(size_t)p * kP + c];
    G.rhs[(size_t)i * kP + tid] = b;
  }
  __syncthreads();
  for (int k = tid; k < kP * kP; k += kMk) {
    const int r = k / kP, c = k % kP;
    const double w = s_W[r * kGbaLd + c];
    Wo[k] = w;
    A[k] = w / s_L[c * kGbaLd + c];
  }
}

// ---- (c) the trailing update --------------------------------------------------------------------------------------------------
// A_ij -= W_i L_jp^T for one tile: the K = kP products in slabs of kGbaSlab columns staged in LDS (k-major, so that the 16 lanes of a
// fragment read consecutive doubles), 36 tiles of 16 x 16 over the 4 waves (9 each), accumulators in registers, k ascending.
// f64 fragments: A operand lane -> (row = lane & 15, k = lane >> 4), B operand lane -> (k = lane >> 4, col = lane & 15), C / D lane ->
// (col = lane & 15, row = (lane >> 4) + 4 reg).
constexpr int kGbaSlab = 32;
__global__ __launch_bounds__(kMk) void k_gba_trail(LbaDev D, GbaDev G, int p) {
  __shared__ double s_a[kGbaSlab * kGbaLd], s_b[kGbaSlab * kGbaLd];
  if (!D.S->solve_ok) return;
  const int pr = blockIdx.x;
  int a = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
  while (a * (a + 1) / 2 > pr) a--;
  while ((a + 1) * (a + 2) / 2 <= pr) a++;
  const int i = p + 1 + a, j = p + 1 + (pr - a * (a + 1) / 2);
  const GFS_GLOBAL double* Wi = G.W + (size_t)i * kP * kP;
  const GFS_GLOBAL double* Lj = G.tiles + gba_sys::tile_offset(j, p);
  GFS_GLOBAL double* C = G.tiles + gba_sys::tile_offset(i, j);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  constexpr int kT = kP / 16, kPer = kT * kT / 4;  // 6 x 6 tiles, 9 a wave
  static_assert(kT * kT % 4 == 0, "the 16 x 16 tiles divide over the four waves");
  d4_t acc[kPer];
#pragma unroll
  for (int u = 0; u < kPer; u++) acc[u] = d4_t{0, 0, 0, 0};
  for (int k0 = 0; k0 < kP; k0 += kGbaSlab) {
    __syncthreads();  // the previous slab has been consumed
    for (int k = tid; k < kP * kGbaSlab; k += kMk) {
      const int r = k / kGbaSlab, kc = k - r * kGbaSlab;
      s_a[kc * kGbaLd + r] = Wi[r * kP + k0 + kc];
      s_b[kc * kGbaLd + r] = Lj[r * kP + k0 + kc];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kGbaSlab / 4; ks++) {
      const double* ca = s_a + (4 * ks + kq) * kGbaLd + l16;
      const double* cb = s_b + (4 * ks + kq) * kGbaLd + l16;
#pragma unroll
      for (int u = 0; u < kPer; u++) {
        const int t = wave * kPer + u, tr = t / kT, tc = t - tr * kT;
        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[16 * tr], cb[16 * tc], acc[u], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kPer; u++) {
    const int t = wave * kPer + u, tr = t / kT, tc = t - tr * kT;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int at = (16 * tr + kq + 4 * q) * kP + 16 * tc + l16;
      C[at] -= acc[u][q];
    }
  }
}

// ---- substitutions ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMk) void k_gba_scale(LbaDev D, GbaDev G) {
  if (!D.S->solve_ok) return;
  const int r = blockIdx.x * kMk + threadIdx.x;
  if (r < G.T * kP) G.rhs[r] /= G.tiles[gba_sys::tile_offset(r / kP, r / kP) + (size_t)(r % kP) * (kP + 1)];
}

// step q = T ... 1: workgroup b takes tile row j = q - 1 - b.  For q < T it subtracts L_qj^T x_q from z_j (rows of L_qj ascending);
// workgroup 0 then holds the final z_{q-1} and solves L^T x = z on its diagonal tile from the last row up.
__global__ __launch_bounds__(kMk) void k_gba_back(LbaDev D, GbaDev G, int q) {
  extern __shared__ __align__(16) double lds[];
  __shared__ double s_z[kP];
  if (!D.S->solve_ok) return;
  const int j = q - 1 - blockIdx.x, tid = threadIdx.x;
  double z = 0;
  if (tid < kP) {
    z = G.rhs[(size_t)j * kP + tid];
    if (q < G.T) {
      const GFS_GLOBAL double* L = G.tiles + gba_sys::tile_offset(q, j);
      const GFS_GLOBAL double* x = G.rhs + (size_t)q * kP;
      for (int r = 0; r < kP; r++) z -= L[r * kP + tid] * x[r];
    }
  }
  if (blockIdx.x != 0) {
    if (tid < kP) G.rhs[(size_t)j * kP + tid] = z;
    return;
  }
  double* s_L = lds;  // [kP][kGbaLd]
  const GFS_GLOBAL double* Ljj = G.tiles + gba_sys::tile_offset(j, j);
  for (int k = tid; k < kP * kP; k += kMk) s_L[(k / kP) * kGbaLd + k % kP] = Ljj[k];
  if (tid < kP) s_z[tid] = z;
  __syncthreads();
  for (int r = kP - 1; r >= 1; r--) {  // x_r is final: every row above takes its term
    if (tid < r) s_z[tid] -= s_L[r * kGbaLd + tid] * s_z[r];
    __syncthreads();
  }
  if (tid < kP) {
    const size_t g = (size_t)j * kP + tid;
    G.rhs[g] = s_z[tid];
    if (g < (size_t)G.n) D.xp[g] = s_z[tid];
  }
}

}  // namespace
