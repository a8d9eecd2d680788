// Device pieces the matcher kernels of sbp.hip, local_points.hip and fuse.hip share: the frame grid, the LDS capacity of a frame's
// key-points, the pair header k_sbp reads (k_lp_compact patches its n_last) and the descriptor distance.
#pragma once
#include "gfs_common.hpp"

namespace gfs {

constexpr int kGridCols = 64, kGridRows = 48, kCells = kGridCols * kGridRows;  // include/Frame.h FRAME_GRID_COLS / ROWS
constexpr int kSbpMaxCur = 4096;                                               // key-points of the current frame (LDS tables)

struct SbpPair {
  int n_last, n_cur, n_levels, mono, check_orientation;
  int mode;  // 0 = frame to frame (:1853-2063), 1 = map points with Frame::isInFrustum projections (:43-206)
  float nn_ratio;
  float Tcw_q[4], Tcw_t[3], Tlw_q[4], Tlw_t[3];
  float fx, fy, cx, cy, bf, b, min_x, max_x, min_y, max_y, grid_w_inv, grid_h_inv, th;
  float scale[16];
};

// A key frame's grid in LDS as k_fuse and k_sim3_search walk it (Frame::AssignFeaturesToGrid: the key-points of a cell in index
// order): s_start [kCells + 1] = the first item of every cell (a cell is ix * kGridRows + iy, so the cells iy = y0 .. y1 of one
// column are one contiguous run), s_items = the key-point indices sorted by cell.  cell_of(i) = the cell of key-point i or -1, read
// from tables the caller's threads filled before the call (the first barrier here orders them); s_cnt [kCells] and s_scan [Threads / 64] are scratch, free again on return.  All
// Threads threads of the workgroup call it; it ends with a barrier.
template <int Threads, class CellOf>
__device__ __forceinline__ void build_grid_lds(int N, CellOf&& cell_of, unsigned short* s_start, unsigned short* s_items, int* s_cnt, int* s_scan) {
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = tid; c < kCells; c += Threads) s_cnt[c] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += Threads) {
    const int c = cell_of(i);
    if (c >= 0) atomicAdd(&s_cnt[c], 1);
  }
  __syncthreads();
  {
    constexpr int per = kCells / Threads;  // 12 (3072 cells over 256 threads)
    static_assert(per * Threads == kCells, "the cells divide over the threads");
    int cnt[per], local = 0;
#pragma unroll
    for (int k = 0; k < per; k++) {
      cnt[k] = s_cnt[tid * per + k];
      local += cnt[k];
    }
    int incl = local;  // exclusive scan over the threads: shuffles inside the wave, the wave totals through LDS
#pragma unroll
    for (int ofs = 1; ofs < 64; ofs <<= 1) {
      const int v = __shfl_up(incl, ofs, 64);
      if (lane >= ofs) incl += v;
    }
    if (lane == 63) s_scan[tid >> 6] = incl;
    __syncthreads();
    int run = incl - local;
    for (int w = 0; w < (tid >> 6); w++) run += s_scan[w];
#pragma unroll
    for (int k = 0; k < per; k++) {
      s_start[tid * per + k] = (unsigned short)run;
      s_cnt[tid * per + k] = 0;  // now the fill counter of the cell
      run += cnt[k];
    }
    if (tid == Threads - 1) s_start[kCells] = (unsigned short)run;
  }
  __syncthreads();
  for (int i = tid; i < N; i += Threads) {  // into the cell in arrival order ...
    const int c = cell_of(i);
    if (c < 0) continue;
    s_items[s_start[c] + atomicAdd(&s_cnt[c], 1)] = (unsigned short)i;
  }
  __syncthreads();
  for (int c = tid; c < kCells; c += Threads) {  // ... then every cell in index order (a handful of items: insertion sort)
    const int b = s_start[c], e = s_start[c + 1];
    for (int a = b + 1; a < e; a++) {
      const unsigned short v = s_items[a];
      int q = a;
      while (q > b && s_items[q - 1] > v) {
        s_items[q] = s_items[q - 1];
        q--;
      }
      s_items[q] = v;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

}  // namespace gfs
