// Device pieces the matcher kernels of sbp.hip, local_points.hip, fuse.hip and sim3_search.hip share: the frame grid and its build in
// LDS, the walk of a search window over it, the LDS capacity of a frame's key-points, the pair header k_sbp reads (k_lp_compact patches
// its n_last), the descriptor distance, and the node search of the feature-vector matchers (triangulate.hip, bow_search.hip).
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

// Frame::PosInGrid (src/Frame.cc:1073-1084): the cell ix * kGridRows + iy of a key-point at (x, y), or -1 outside the grid.  K is any
// header with the grid's origin and inverse cell sizes.
template <class Frame>
__device__ __forceinline__ int pos_in_grid(const Frame& K, float x, float y) {
  const int px = (int)roundf((x - K.min_x) * K.grid_w_inv), py = (int)roundf((y - K.min_y) * K.grid_h_inv);
  return (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) ? px * kGridRows + py : -1;
}

// A frame's grid in LDS as the matcher kernels walk it (Frame::AssignFeaturesToGrid: the key-points of a cell in index order):
// s_start [kCells + 1] = the first item of every cell (a cell is ix * kGridRows + iy, so the cells iy = y0 .. y1 of one column are one
// contiguous run), s_items = the key-point indices sorted by cell.  cell_of(i) = the cell of key-point i or -1, read from tables the
// caller's threads filled before the call; s_cnt [kCells] and s_scan [Threads / 64] are scratch, free again on return.  All Threads
// threads of the workgroup call it; it begins with a barrier (which orders those tables) and ends with one.
// grid_from_counts_lds is the part behind the count, for a caller that counts while it loads its key-points (k_sbp): s_cnt holds the
// number of key-points of every cell.
template <int Threads, class CellOf>
__device__ __forceinline__ void grid_from_counts_lds(int N, CellOf&& cell_of, unsigned short* s_start, unsigned short* s_items, int* s_cnt,
                                                     int* s_scan) {
  const int tid = threadIdx.x, lane = tid & 63;
  __syncthreads();
  {
    constexpr int per = kCells / Threads;  // 12 (3072 cells over 256 threads), 3 over 1024
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

template <int Threads, class CellOf>
__device__ __forceinline__ void build_grid_lds(int N, CellOf&& cell_of, unsigned short* s_start, unsigned short* s_items, int* s_cnt, int* s_scan) {
  const int tid = threadIdx.x;
  for (int c = tid; c < kCells; c += Threads) s_cnt[c] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += Threads) {
    const int c = cell_of(i);
    if (c >= 0) atomicAdd(&s_cnt[c], 1);
  }
  grid_from_counts_lds<Threads>(N, cell_of, s_start, s_items, s_cnt, s_scan);
}

// The start of k_fuse and k_sim3_search: key frame K's N key-points (position xy, octave byte oct) into s_kx, s_ky, s_oct and its grid
// into s_start / s_items.  s_cnt and s_scan are build_grid_lds's scratch: a caller may alias them onto a table it fills afterwards.
template <int Threads, class Frame>
__device__ __forceinline__ void load_keyframe_grid_lds(const Frame& K, int N, const float2* __restrict__ xy, const uint8_t* __restrict__ oct,
                                                       float* s_kx, float* s_ky, uint8_t* s_oct, unsigned short* s_start,
                                                       unsigned short* s_items, int* s_cnt, int* s_scan) {
  for (int i = threadIdx.x; i < N; i += Threads) {
    const float2 p = xy[i];
    s_kx[i] = p.x;
    s_ky[i] = p.y;
    s_oct[i] = oct[i];
  }
  build_grid_lds<Threads>(N, [&](int i) { return pos_in_grid(K, s_kx[i], s_ky[i]); }, s_start, s_items, s_cnt, s_scan);
}

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Frame::GetFeaturesInArea's visit of the window of cells [x0, x1] x [y0, y1] (src/Frame.cc:1007-1071) and the distance of what it
// keeps, in the reference's order (ix, iy, cell order).  The items are stored by cell, so the cells iy = y0 .. y1 of one grid column are
// ONE contiguous run of s_items: a window is x1 - x0 + 1 runs (<= 13 for the largest radius), not (x1 - x0 + 1) (y1 - y0 + 1) cells of
// which two thirds are empty.  The items are walked four at a time: gate(j) says from the caller's LDS tables whether key-point j
// counts, the descriptors of the survivors (32 bytes each from desc) are fetched together -- one round trip to memory per four items,
// for the survivors only -- and offer(j, dist) gets each survivor's distance to the 32 bytes at query, in visiting order.
template <class Gate, class Offer>
__device__ __forceinline__ void walk_window(int x0, int x1, int y0, int y1, const unsigned short* s_start, const unsigned short* s_items,
                                            const uint8_t* __restrict__ query, const uint8_t* __restrict__ desc, Gate&& gate, Offer&& offer) {
  const uint4* dq = reinterpret_cast<const uint4*>(query);
  const uint4 a0 = dq[0], a1 = dq[1];
  int ix = x0;
  int k = s_start[ix * kGridRows + y0], kend = s_start[ix * kGridRows + y1 + 1];
  bool more = true;
  auto next_item = [&]() {  // the next key-point index of the window in visiting order, or -1
    while (more && k >= kend) {
      if (++ix > x1) {
        more = false;
        break;
      }
      k = s_start[ix * kGridRows + y0];
      kend = s_start[ix * kGridRows + y1 + 1];
    }
    return more ? (int)s_items[k++] : -1;
  };
  while (more) {
    int j[4];
    bool pass[4];
    uint4 b0[4], b1[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      j[u] = next_item();
      pass[u] = j[u] >= 0 && gate(j[u]);
      if (!pass[u]) continue;
      const uint4* dc = reinterpret_cast<const uint4*>(desc + 32 * (size_t)j[u]);
      b0[u] = dc[0];
      b1[u] = dc[1];
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (pass[u]) offer(j[u], hamming256(a0, a1, b0[u], b1[u]));
  }
}

// the position of id in the ascending ids [n] (a key frame's feature-vector nodes), or -1
__device__ __forceinline__ int find_node(const int* __restrict__ ids, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < n && ids[lo] == id) ? lo : -1;
}

}  // namespace gfs
