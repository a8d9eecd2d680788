// The pieces of the pcl::VoxelGrid pipeline that more than one translation unit runs: the order-preserving
// float encoding of the bounding-box atomics, the block scan, the grid dimensions with PCL's overflow checks, the stable 8-bit LSD
// radix sort of (key, value) pairs whose element count may live on the device, and the in-order sum of one voxel's points.
// Users: lidar_map.hip (the local map) and frame_cloud.hip (the frame cloud's three filters and its radius-search grid).
#pragma once
#include <hip/hip_runtime.h>

namespace gfs_voxel {

constexpr int kThreads = 256;
constexpr int kItems = 8;
constexpr int kTile = kThreads * kItems;
constexpr int kBins = 256;
constexpr float kBound = 1e6f;  // gfs_lidar_map_set's bound; lidar_point_edge's grid walk relies on it
constexpr float kTwo31 = 2147483648.0f;
enum { kFlagBad = 1, kFlagUnsupported = 2, kFlagPassthrough = 4 };

// float <-> unsigned whose unsigned order is the float order
__device__ __forceinline__ unsigned f_enc(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// exclusive scan of one int per thread over a block of T threads (sh: T ints); *total = the block's sum
template <int T>
__device__ __forceinline__ int block_scan(int v, int* sh, int* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < T; o <<= 1) {
    const int a = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += a;
    __syncthreads();
  }
  const int incl = sh[tid];
  *total = sh[T - 1];
  __syncthreads();
  return incl - v;
}

// pcl::VoxelGrid::applyFilter's grid from the bounding box: 0 = filter, else kFlagPassthrough / kFlagUnsupported
struct VoxelGridDims {
  float inv;
  int min_b[3], div[3];
};
__device__ __forceinline__ int voxel_grid_dims(const float* mn, const float* mx, float leaf, VoxelGridDims* g) {
  g->inv = 1.0f / leaf;
  long long prod = 1;
  for (int a = 0; a < 3; a++) {
    g->min_b[a] = 0;
    g->div[a] = 0;
  }
  for (int a = 0; a < 3; a++) {
    const float fd = (mx[a] - mn[a]) * g->inv;
    if (!(fd < kTwo31)) return kFlagPassthrough;  // also NaN / inf: beyond every int64 count
    prod *= (long long)fd + 1;
    if (prod > 2147483647LL) return kFlagPassthrough;
  }
  prod = 1;
  long long dv[3];
  for (int a = 0; a < 3; a++) {
    const float fl = floorf(mn[a] * g->inv), fh = floorf(mx[a] * g->inv);
    if (!(fabsf(fl) < kTwo31) || !(fabsf(fh) < kTwo31)) return kFlagUnsupported;  // PCL's conversion to int would overflow
    g->min_b[a] = (int)fl;
    dv[a] = (long long)(int)fh - (long long)g->min_b[a] + 1;
  }
  for (int a = 0; a < 3; a++) {
    prod *= dv[a];
    if (prod > 2147483647LL) return kFlagUnsupported;  // PCL's int product would overflow
  }
  for (int a = 0; a < 3; a++) g->div[a] = (int)dv[a];
  return 0;
}

// ------------------------------------------------------------------ stable LSD radix sort of (key, val) pairs, 8 bits a pass
// n_dev (may be null): the element count when only the device knows it; the grid is sized for the host's upper bound.

static __global__ __launch_bounds__(kThreads) void k_lm_hist(const unsigned* __restrict__ key, int n, const int* __restrict__ n_dev, int shift,
                                                      int* __restrict__ hist, int nblk) {
  __shared__ int h[kBins];
  if (n_dev) n = min(n, *n_dev);
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  for (int r = 0; r < kItems; r++) {
    const int i = blockIdx.x * kTile + r * kThreads + tid;
    if (i < n) atomicAdd(&h[(key[i] >> shift) & (kBins - 1)], 1);  // a count: the order of arrival does not matter
  }
  __syncthreads();
  hist[tid * nblk + blockIdx.x] = h[tid];
}

static __global__ __launch_bounds__(kThreads) void k_lm_scatter(const unsigned* __restrict__ key, const unsigned* __restrict__ val, int n,
                                                         const int* __restrict__ n_dev, int shift, const int* __restrict__ hist, int nblk,
                                                         unsigned* __restrict__ key_out, unsigned* __restrict__ val_out) {
  __shared__ int off[kBins], sh[kThreads];
  if (n_dev) n = min(n, *n_dev);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // this tile's first position for digit tid: every pair with a lower digit, and the pairs with this digit in the tiles in front
  // (every workgroup sums the small table itself: no scan kernel between the histogram and the scatter)
  int total = 0, before = 0;
  for (int b = 0; b < nblk; b++) {
    const int v = hist[tid * nblk + b];
    total += v;
    if (b < (int)blockIdx.x) before += v;
  }
  int all;
  off[tid] = block_scan<kThreads>(total, sh, &all) + before;
  __syncthreads();
  for (int r = 0; r < kItems; r++) {
    const int i = blockIdx.x * kTile + r * kThreads + tid;
    const bool valid = i < n;
    const unsigned k = valid ? key[i] : 0u, v = valid ? val[i] : 0u;
    const int d = (int)((k >> shift) & (kBins - 1));
    unsigned long long same = __ballot(valid);  // the valid lanes of this wave with the same digit
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull)), cnt = __popcll(same);
    int pos = 0;
    for (int w = 0; w < kThreads / 64; w++) {  // the waves take their turn in index order
      if (wave == w && valid) pos = off[d] + rank;
      __builtin_amdgcn_wave_barrier();
      if (wave == w && valid && rank == 0) off[d] += cnt;
      __syncthreads();
    }
    if (valid) {
      key_out[pos] = k;
      val_out[pos] = v;
    }
  }
}

// The float sums of the run of sorted positions [j, m) whose key equals skey[j]: the voxel's points in ascending input index; returns
// m.  kBatch keys, indices and points are loaded at a time (clamped to the array, used only while the key matches): a one-by-one
// walk is two dependent round trips to memory per point
__device__ __forceinline__ int voxel_run_sum(const unsigned* __restrict__ skey, const unsigned* __restrict__ sval,
                                             const float4* __restrict__ world, int n, int j, float* s0_, float* s1_, float* s2_) {
  const unsigned k = skey[j];
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  constexpr int kBatch = 8;
  int m = j;
  for (bool more = true; more;) {
    unsigned kk[kBatch], vv[kBatch];
    float4 P[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
      const int mm = min(m + b, n - 1);
      kk[b] = skey[mm];
      vv[b] = sval[mm];
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) P[b] = world[vv[b]];
    int taken = 0;
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
      if (more && m + b < n && kk[b] == k) {
        s0 = s0 + P[b].x;
        s1 = s1 + P[b].y;
        s2 = s2 + P[b].z;
        taken++;
      } else {
        more = false;
      }
    }
    m += taken;
  }
  *s0_ = s0;
  *s1_ = s1;
  *s2_ = s2;
  return m;
}

}  // namespace gfs_voxel
