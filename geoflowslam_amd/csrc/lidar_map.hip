// The lidar local map of LidarMapping::viewer (reference src/LidarMapping.cc:130-185) on MI355X: the last key-frames' downsampled
// clouds are transformed to the world by toMatrix4d(Tcw.inverse()) (transformPointCloud, :107-127), concatenated, run through
// pcl::VoxelGrid at LidarMapping.LocalResolution, and the result is laid out in the search grid the association kernels of
// lidar_assoc.hpp walk -- the layout gfs_lidar_map_set builds on the host.  DESIGN.md section 11 states the filter's rule; the
// sequential restatement is tests/host/lidar_map_restatement.cpp.
//
// One call, one stream, no allocation:
//   k_lm_init       one lane per key-frame: M = init_pose_f(q, t); lane 0 resets the control block
//   k_lm_transform  one thread per point: the double expression of transformPointCloud stored as float; per-block min / max of the
//                   three axes folded into the control block with atomics on an order-preserving encoding (min and max do not
//                   depend on order); a point that is not finite or beyond 1e6 m raises the refusal flag
//   k_lm_keys       every thread derives inv, d, min_b, div from the six folded floats and writes (idx, i); passthrough: idx = i
//   radix sort      4 passes of 8 bits, least significant first: block histogram, then a scatter whose workgroups each sum the
//                   histogram table for their tile's offsets and place the pairs by their rank inside the tile.  The rank comes
//                   from ballots inside a wave and a running offset handed from wave to wave in wave order: stable, and no
//                   atomic decides a position
//   k_lm_heads      heads of the runs of equal idx, counted per block
//   k_lm_centroid   a voxel's slot = heads in front of it; one thread per voxel adds its points in sorted (= input) order and
//                   divides; it also writes the voxel's grid bucket (the hash of its 1.25 m cell, nb = next_pow2(2 n_out))
//   radix sort      of (bucket, map index), as many 8-bit passes as the largest possible nb needs
//   k_lm_grid       only if nothing was refused: the bucket-sorted points with their index words and the bucket offsets (a binary
//                   search per bucket) go straight into the gfs_lidar_map; a refused build has written nothing there
// and the control block (n_out, nb, flags, div) is read back: the call's one synchronisation.
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "block_layouts.hpp"
#include "gfs_common.hpp"
#include "lidar_assoc.hpp"
#include "voxel_filter_dev.hpp"

using namespace gfs_lidar;
using namespace gfs_voxel;

namespace {

struct Ctl {
  unsigned lo[3], hi[3];  // encoded per-axis min / max of the transformed points
  int flags, n_out, nb;
  int div[3];
};

size_t next_pow2(size_t v) {  // as gfs_lidar_map_set
  size_t p = 64;
  while (p < v) p <<= 1;
  return p;
}

__global__ void k_lm_init(const float* __restrict__ q, const float* __restrict__ t, int n_kf, double* __restrict__ M, Ctl* c) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) {
    for (int a = 0; a < 3; a++) {
      c->lo[a] = 0xffffffffu;
      c->hi[a] = 0u;
      c->div[a] = 0;
    }
    c->flags = 0;
    c->n_out = 0;
    c->nb = 0;
  }
  if (k < n_kf) init_pose_f(q + 4 * k, t + 3 * k, M + 12 * k);
}

// M == nullptr: the points are taken as they are (gfs_voxel_grid_filter)
__global__ __launch_bounds__(kThreads) void k_lm_transform(const float* __restrict__ cloud, int n, const int* __restrict__ cb, int n_kf,
                                                           const double* __restrict__ M, float4* __restrict__ world, Ctl* c) {
  __shared__ unsigned s_lo[3][kThreads / 64], s_hi[3][kThreads / 64];
  __shared__ int s_bad;
  const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (i < n) {
    const float x = cloud[3 * i], y = cloud[3 * i + 1], z = cloud[3 * i + 2];
    float p[3] = {x, y, z};
    if (M) {
      int a = 0, b = n_kf;  // the key-frame k with cb[k] <= i < cb[k + 1] (empty clouds repeat an offset)
      while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (cb[m] <= i) a = m; else b = m;
      }
      const double* Mk = M + 12 * a;
#pragma unroll
      for (int r = 0; r < 3; r++)
        p[r] = (float)(((Mk[4 * r] * (double)x + Mk[4 * r + 1] * (double)y) + Mk[4 * r + 2] * (double)z) + Mk[4 * r + 3]);
    }
    world[i] = make_float4(p[0], p[1], p[2], 0.0f);
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 3; r++) bad = bad || !(isfinite(p[r]) && fabsf(p[r]) < kBound);
    if (bad) {
      s_bad = 1;
    } else {
#pragma unroll
      for (int r = 0; r < 3; r++) lo[r] = hi[r] = f_enc(p[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {
    for (int o = 32; o >= 1; o >>= 1) {
      lo[r] = min(lo[r], (unsigned)__shfl_xor((int)lo[r], o));
      hi[r] = max(hi[r], (unsigned)__shfl_xor((int)hi[r], o));
    }
    if ((tid & 63) == 0) {
      s_lo[r][tid >> 6] = lo[r];
      s_hi[r][tid >> 6] = hi[r];
    }
  }
  __syncthreads();
  if (tid < 3) {
    unsigned l = s_lo[tid][0], h = s_hi[tid][0];
    for (int w = 1; w < kThreads / 64; w++) {
      l = min(l, s_lo[tid][w]);
      h = max(h, s_hi[tid][w]);
    }
    atomicMin(&c->lo[tid], l);
    atomicMax(&c->hi[tid], h);
  }
  if (tid == 0 && s_bad) atomicOr(&c->flags, kFlagBad);
}

__global__ __launch_bounds__(kThreads) void k_lm_keys(const float4* __restrict__ world, int n, float leaf, Ctl* c, unsigned* __restrict__ key,
                                                      unsigned* __restrict__ val) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool bad = (c->flags & kFlagBad) != 0;
  int mode = 0;
  VoxelGridDims g;
  if (!bad) {
    float mn[3], mx[3];
    for (int a = 0; a < 3; a++) {
      mn[a] = f_dec(c->lo[a]);
      mx[a] = f_dec(c->hi[a]);
    }
    mode = voxel_grid_dims(mn, mx, leaf, &g);
    if (i == 0) {
      if (mode) atomicOr(&c->flags, mode);
      for (int a = 0; a < 3; a++) c->div[a] = g.div[a];
    }
  }
  if (i >= n) return;
  unsigned k = 0;
  if (mode == kFlagPassthrough) {
    k = (unsigned)i;
  } else if (!bad && mode == 0) {
    const float4 P = world[i];
    const unsigned i0 = (unsigned)(int)(floorf(P.x * g.inv) - (float)g.min_b[0]);
    const unsigned i1 = (unsigned)(int)(floorf(P.y * g.inv) - (float)g.min_b[1]);
    const unsigned i2 = (unsigned)(int)(floorf(P.z * g.inv) - (float)g.min_b[2]);
    k = i0 + i1 * (unsigned)g.div[0] + i2 * (unsigned)g.div[0] * (unsigned)g.div[1];
  }
  key[i] = k;
  val[i] = (unsigned)i;
}

// ------------------------------------------------------------------ runs and centroids
// thread t of a block owns the kItems consecutive sorted positions from blockIdx.x * kTile + t * kItems

__global__ __launch_bounds__(kThreads) void k_lm_heads(const unsigned* __restrict__ skey, int n, int* __restrict__ blkcnt) {
  __shared__ int sh[kThreads];
  const int j0 = blockIdx.x * kTile + threadIdx.x * kItems;
  int cnt = 0;
  for (int u = 0; u < kItems; u++) {
    const int j = j0 + u;
    if (j < n && (j == 0 || skey[j] != skey[j - 1])) cnt++;
  }
  int total;
  block_scan<kThreads>(cnt, sh, &total);
  if (threadIdx.x == 0) blkcnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_lm_centroid(const unsigned* __restrict__ skey, const unsigned* __restrict__ sval,
                                                          const float4* __restrict__ world, int n, const int* __restrict__ blkcnt, int nblk,
                                                          Ctl* c, float4* __restrict__ out, unsigned* __restrict__ gkey,
                                                          unsigned* __restrict__ gval) {
  __shared__ int sh[kThreads];
  const int flags = c->flags;
  if (flags & (kFlagBad | kFlagUnsupported)) return;  // n_out stays 0
  const int tid = threadIdx.x;
  int before = 0, all = 0;
  for (int b = tid; b < nblk; b += kThreads) {
    const int v = blkcnt[b];
    all += v;
    if (b < (int)blockIdx.x) before += v;
  }
  int n_out, base;
  block_scan<kThreads>(all, sh, &n_out);
  block_scan<kThreads>(before, sh, &base);
  int nb = 64;
  while (nb < 2 * n_out) nb <<= 1;
  if (blockIdx.x == 0 && tid == 0) {
    c->n_out = n_out;
    c->nb = nb;
  }
  const int j0 = blockIdx.x * kTile + tid * kItems;
  bool head[kItems];
  int cnt = 0;
  for (int u = 0; u < kItems; u++) {
    const int j = j0 + u;
    head[u] = j < n && (j == 0 || skey[j] != skey[j - 1]);
    cnt += head[u];
  }
  int unused;
  int slot = base + block_scan<kThreads>(cnt, sh, &unused);
  for (int u = 0; u < kItems; u++) {
    if (!head[u]) continue;
    const int j = j0 + u;
    float4 o;
    if (flags & kFlagPassthrough) {
      o = world[sval[j]];
    } else {
      float s0, s1, s2;
      const int m = voxel_run_sum(skey, sval, world, n, j, &s0, &s1, &s2);  // the voxel's points in ascending input index
      const float fc = (float)(m - j);
      o = make_float4(s0 / fc, s1 / fc, s2 / fc, 0.0f);
    }
    out[slot] = o;
    gkey[slot] = cell_hash(cell_of((double)o.x), cell_of((double)o.y), cell_of((double)o.z), nb);
    gval[slot] = (unsigned)slot;
    slot++;
  }
}

// the map's two arrays, written only when the build stands (the host takes the same decision from the control block)
__global__ __launch_bounds__(kThreads) void k_lm_grid(const unsigned* __restrict__ skey, const unsigned* __restrict__ sval,
                                                      const float4* __restrict__ out, const Ctl* __restrict__ c, float4* __restrict__ map_pts,
                                                      int* __restrict__ map_start, int map_max) {
  const int n = c->n_out, nb = c->nb;
  if ((c->flags & (kFlagBad | kFlagUnsupported)) || n < 5 || n > map_max) return;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) {
    const unsigned mi = sval[i];
    float4 P = out[mi];
    P.w = __int_as_float((int)mi);
    map_pts[i] = P;
  }
  if (i <= nb) {  // the first sorted position whose bucket is >= i
    int a = 0, b = n;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (skey[m] < (unsigned)i) a = m + 1; else b = m;
    }
    map_start[i] = a;
  }
}

}  // namespace

struct gfs_lidar_mapper {
  int device, max_points, max_kf, max_blk;
  hipStream_t stream;
  std::mutex mu;
  gfs::LidarMapLayout Y{0, 0};  // staging: cloud_begin | q | t | cloud, at the handle's capacity
  gfs::Mirror in;
  gfs::DevBuf<double> d_M;
  gfs::DevBuf<float4> d_world, d_out;
  gfs::DevBuf<unsigned> d_key[2], d_val[2];
  gfs::DevBuf<int> d_hist, d_blk;
  gfs::DevBuf<Ctl> d_ctl;
  gfs::PinBuf<Ctl> h_ctl;
  gfs::PinBuf<float4> h_out;
};

namespace {

// Sorts (key[from], val[from]) by the low 8 * passes bits of the key; returns the buffer index holding the result.
int radix_sort(gfs_lidar_mapper* h, int from, int n, const int* n_dev, int passes, int* rc) {
  const int nblk = gfs::div_up(n, kTile);
  hipStream_t s = h->stream;
  auto pass = [&](int src, int shift) -> int {
    GFS_LAUNCH("k_lm_hist", k_lm_hist, dim3(nblk), dim3(kThreads), 0, s, h->d_key[src].p, n, n_dev, shift, h->d_hist.p, nblk);
    GFS_LAUNCH("k_lm_scatter", k_lm_scatter, dim3(nblk), dim3(kThreads), 0, s, h->d_key[src].p, h->d_val[src].p, n, n_dev, shift,
               h->d_hist.p, nblk, h->d_key[src ^ 1].p, h->d_val[src ^ 1].p);
    return GFS_OK;
  };
  *rc = GFS_OK;
  for (int p = 0; p < passes && !*rc; p++, from ^= 1) *rc = pass(from, 8 * p);
  return from;
}

// Upload done: transform (M null: none), filter.  Leaves the sorted pairs' centroids in d_out, the grid pairs in buffer 1.
int launch_filter(gfs_lidar_mapper* h, int n, int n_kf, float leaf) {
  hipStream_t s = h->stream;
  const uint8_t* di = h->in.d.p;
  const float *d_q = h->Y.q.at(di), *d_t = h->Y.t.at(di), *d_cloud = h->Y.cloud.at(di);
  const int* d_cb = h->Y.cloud_begin.at(di);
  const int nblk = gfs::div_up(n, kTile), nb256 = gfs::div_up(n, kThreads);
  GFS_LAUNCH("k_lm_init", k_lm_init, dim3(gfs::div_up(std::max(n_kf, 1), 64)), dim3(64), 0, s, d_q, d_t, n_kf, h->d_M.p, h->d_ctl.p);
  GFS_LAUNCH("k_lm_transform", k_lm_transform, dim3(nb256), dim3(kThreads), 0, s, d_cloud, n, d_cb, n_kf,
             n_kf > 0 ? (const double*)h->d_M.p : (const double*)nullptr, h->d_world.p, h->d_ctl.p);
  GFS_LAUNCH("k_lm_keys", k_lm_keys, dim3(nb256), dim3(kThreads), 0, s, h->d_world.p, n, leaf, h->d_ctl.p, h->d_key[0].p, h->d_val[0].p);
  int rc;
  const int at = radix_sort(h, 0, n, nullptr, 4, &rc);  // 4 passes: back in buffer 0
  if (rc) return rc;
  GFS_LAUNCH("k_lm_heads", k_lm_heads, dim3(nblk), dim3(kThreads), 0, s, h->d_key[at].p, n, h->d_blk.p);
  GFS_LAUNCH("k_lm_centroid", k_lm_centroid, dim3(nblk), dim3(kThreads), 0, s, h->d_key[at].p, h->d_val[at].p, h->d_world.p, n,
             h->d_blk.p, nblk, h->d_ctl.p, h->d_out.p, h->d_key[at ^ 1].p, h->d_val[at ^ 1].p);
  return GFS_OK;
}

void fill_info(gfs_lidar_map_info* info, int n_in, const Ctl& c) {
  if (!info) return;
  info->n_in = n_in;
  info->n_out = c.n_out;
  info->passthrough = (c.flags & kFlagPassthrough) ? 1 : 0;
  for (int a = 0; a < 3; a++) info->div[a] = c.div[a];
}

}  // namespace

extern "C" {

int gfs_lidar_mapper_create(int device, int max_points_in, int max_keyframes, gfs_lidar_mapper** out) {
  GFS_REQUIRE(out && max_points_in >= 1 && max_points_in <= (1 << 28) && max_keyframes >= 1, GFS_ERR_INVALID_ARG,
              "gfs_lidar_mapper_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_lidar_mapper> h(new gfs_lidar_mapper);
  h->device = device;
  h->max_points = max_points_in;
  h->max_kf = max_keyframes;
  h->max_blk = gfs::div_up(max_points_in, kTile);
  const size_t N = (size_t)max_points_in, K = (size_t)max_keyframes;
  h->Y = gfs::LidarMapLayout{K, N};
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  int rc = 0;
  if (!rc) rc = h->in.alloc(h->Y.in.bytes());
  if (!rc) rc = h->d_M.alloc(12 * K);
  if (!rc) rc = h->d_world.alloc(N);
  if (!rc) rc = h->d_out.alloc(N);
  for (int k = 0; k < 2; k++) {
    if (!rc) rc = h->d_key[k].alloc(N);
    if (!rc) rc = h->d_val[k].alloc(N);
  }
  if (!rc) rc = h->d_hist.alloc((size_t)kBins * h->max_blk);
  if (!rc) rc = h->d_blk.alloc((size_t)h->max_blk);
  if (!rc) rc = h->d_ctl.alloc(1);
  if (!rc) rc = h->h_ctl.alloc(1);
  if (!rc) rc = h->h_out.alloc(N);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_lidar_mapper_destroy(gfs_lidar_mapper* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_lidar_map_build(gfs_lidar_mapper* h, const gfs_lidar_map_input* in, gfs_lidar_map* map, gfs_lidar_map_info* info) {
  GFS_REQUIRE(h && in && map, GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: invalid argument");
  GFS_REQUIRE(map->device == h->device, GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: map on another device");
  GFS_REQUIRE(std::isfinite(in->leaf) && in->leaf > 0.0f, GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: leaf %g is not positive and finite",
              (double)in->leaf);
  const int K = in->n_keyframes;
  GFS_REQUIRE(K >= 0 && (K == 0 || (in->q && in->t && in->cloud_begin)), GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: invalid key-frame list");
  GFS_REQUIRE(K <= h->max_kf, GFS_ERR_CAPACITY, "gfs_lidar_map_build: %d key-frames exceed capacity %d", K, h->max_kf);
  const int n = K > 0 ? in->cloud_begin[K] : 0;
  for (int k = 0; k < K; k++)
    GFS_REQUIRE(in->cloud_begin[0] == 0 && in->cloud_begin[k + 1] >= in->cloud_begin[k], GFS_ERR_INVALID_ARG,
                "gfs_lidar_map_build: cloud_begin is not an ascending list of offsets from 0");
  GFS_REQUIRE(n <= h->max_points, GFS_ERR_CAPACITY, "gfs_lidar_map_build: %d points exceed capacity %d", n, h->max_points);
  if (info) *info = gfs_lidar_map_info{n, 0, 0, {0, 0, 0}};
  GFS_REQUIRE(n >= 5, GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: %d points (the consumers read the 5th neighbour)", n);
  GFS_REQUIRE(in->cloud, GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: NULL cloud");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs::LidarMapLayout& Y = h->Y;
  uint8_t* hi = h->in.h.p;
  Y.cloud_begin.put(hi, 0, in->cloud_begin, (size_t)K + 1);
  Y.q.put(hi, 0, in->q, (size_t)K);
  Y.t.put(hi, 0, in->t, (size_t)K);
  Y.cloud.put(hi, 0, in->cloud, (size_t)n);
  hipStream_t s = h->stream;
  // one copy up to the end of the cloud (the offsets, the poses and the cloud lie in one staging block)
  if (int rc = h->in.upload(s, 0, Y.cloud.off + Y.cloud.bytes((size_t)n))) return rc;
  int rc = launch_filter(h, n, K, in->leaf);
  if (rc) return rc;
  // the grid: n_out <= n is known to the device only; the passes cover the largest nb it can give
  const size_t nb_max = next_pow2(2 * (size_t)n);
  int bits = 0;
  while (((size_t)1 << bits) < nb_max) bits++;
  const int at = radix_sort(h, 1, n, &h->d_ctl.p->n_out, (bits + 7) / 8, &rc);
  if (rc) return rc;
  const int cells = (int)std::max((size_t)n, nb_max + 1);
  GFS_LAUNCH("k_lm_grid", k_lm_grid, dim3(gfs::div_up(cells, kThreads)), dim3(kThreads), 0, s, h->d_key[at].p, h->d_val[at].p, h->d_out.p,
             h->d_ctl.p, map->d_pts.p, map->d_start.p, map->max_points);
  GFS_HIP(hipMemcpyAsync(h->h_ctl.p, h->d_ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  const Ctl c = *h->h_ctl.p;
  fill_info(info, n, c);
  GFS_REQUIRE(!(c.flags & kFlagBad), GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: a transformed point is not finite or beyond 1e6 m");
  GFS_REQUIRE(!(c.flags & kFlagUnsupported), GFS_ERR_UNSUPPORTED,
              "gfs_lidar_map_build: the voxel grid's index range exceeds int (pcl::VoxelGrid would overflow)");
  GFS_REQUIRE(c.n_out <= map->max_points, GFS_ERR_CAPACITY, "gfs_lidar_map_build: %d map points exceed the map's capacity %d", c.n_out,
              map->max_points);
  GFS_REQUIRE(c.n_out >= 5, GFS_ERR_INVALID_ARG, "gfs_lidar_map_build: %d map points (the consumers read the 5th neighbour)", c.n_out);
  map->n = c.n_out;
  map->nb = c.nb;
  return GFS_OK;
}

int gfs_lidar_map_fetch(const gfs_lidar_map* map, float* xyz, int cap, int32_t* n) {
  GFS_REQUIRE(map && n && cap >= 0 && (xyz || cap == 0), GFS_ERR_INVALID_ARG, "gfs_lidar_map_fetch: invalid argument");
  *n = map->n;
  const int m = map->n;
  if (m == 0 || cap == 0) return GFS_OK;
  GFS_HIP(hipSetDevice(map->device));
  std::vector<float4> pts((size_t)m);
  GFS_HIP(hipMemcpy(pts.data(), map->d_pts.p, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost));
  for (int j = 0; j < m; j++) {  // the grid's copy is sorted by bucket; w is the map index
    int mi;
    memcpy(&mi, &pts[j].w, 4);
    GFS_REQUIRE(mi >= 0 && mi < m, GFS_ERR_INVALID_ARG, "gfs_lidar_map_fetch: map index %d out of range (the map was never set)", mi);
    if (mi < cap) {
      xyz[3 * mi] = pts[j].x;
      xyz[3 * mi + 1] = pts[j].y;
      xyz[3 * mi + 2] = pts[j].z;
    }
  }
  return GFS_OK;
}

int gfs_voxel_grid_filter(gfs_lidar_mapper* h, const float* xyz, int n, float leaf, float* out_xyz, int cap, gfs_lidar_map_info* info) {
  GFS_REQUIRE(h && xyz && n >= 1 && cap >= 0 && (out_xyz || cap == 0), GFS_ERR_INVALID_ARG, "gfs_voxel_grid_filter: invalid argument");
  GFS_REQUIRE(std::isfinite(leaf) && leaf > 0.0f, GFS_ERR_INVALID_ARG, "gfs_voxel_grid_filter: leaf %g is not positive and finite", (double)leaf);
  GFS_REQUIRE(n <= h->max_points, GFS_ERR_CAPACITY, "gfs_voxel_grid_filter: %d points exceed capacity %d", n, h->max_points);
  if (info) *info = gfs_lidar_map_info{n, 0, 0, {0, 0, 0}};
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs::LidarMapLayout& Y = h->Y;
  Y.cloud.put(h->in.h.p, 0, xyz, (size_t)n);
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, Y.cloud.off, Y.cloud.off + Y.cloud.bytes((size_t)n))) return rc;
  int rc = launch_filter(h, n, 0, leaf);
  if (rc) return rc;
  // n_out <= n: the whole possible output comes back with the control block, one synchronisation
  GFS_HIP(hipMemcpyAsync(h->h_out.p, h->d_out.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipMemcpyAsync(h->h_ctl.p, h->d_ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  const Ctl c = *h->h_ctl.p;
  fill_info(info, n, c);
  GFS_REQUIRE(!(c.flags & kFlagBad), GFS_ERR_INVALID_ARG, "gfs_voxel_grid_filter: a point is not finite or beyond 1e6 m");
  GFS_REQUIRE(!(c.flags & kFlagUnsupported), GFS_ERR_UNSUPPORTED,
              "gfs_voxel_grid_filter: the voxel grid's index range exceeds int (pcl::VoxelGrid would overflow)");
  GFS_REQUIRE(c.n_out <= cap, GFS_ERR_CAPACITY, "gfs_voxel_grid_filter: %d output points exceed cap %d", c.n_out, cap);
  for (int i = 0; i < c.n_out; i++) {
    out_xyz[3 * i] = h->h_out.p[i].x;
    out_xyz[3 * i + 1] = h->h_out.p[i].y;
    out_xyz[3 * i + 2] = h->h_out.p[i].z;
  }
  return GFS_OK;
}

int gfs_test_lidar_map_grid(const gfs_lidar_map* map, int32_t* start, int cap_start, float* pts, int32_t* index, int cap_pts, int32_t* nb,
                            int32_t* n) {
  GFS_REQUIRE(map && nb && n && cap_start >= 0 && cap_pts >= 0, GFS_ERR_INVALID_ARG, "gfs_test_lidar_map_grid: invalid argument");
  *nb = map->nb;
  *n = map->n;
  if (map->n == 0) return GFS_OK;
  GFS_HIP(hipSetDevice(map->device));
  if (start && cap_start >= map->nb + 1)
    GFS_HIP(hipMemcpy(start, map->d_start.p, (size_t)(map->nb + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (pts && index && cap_pts >= map->n) {
    std::vector<float4> p((size_t)map->n);
    GFS_HIP(hipMemcpy(p.data(), map->d_pts.p, (size_t)map->n * sizeof(float4), hipMemcpyDeviceToHost));
    for (int j = 0; j < map->n; j++) {
      pts[3 * j] = p[j].x;
      pts[3 * j + 1] = p[j].y;
      pts[3 * j + 2] = p[j].z;
      memcpy(&index[j], &p[j].w, 4);
    }
  }
  return GFS_OK;
}

}  // extern "C"
