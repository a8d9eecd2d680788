// The frame cloud of the Frame constructor (reference src/Frame.cc:378-393) on MI355X: LaserProcessingClass::featureExtraction
// (src/LidarProcess.cc:20-204) on the camera-frame cloud ConvertDepthToPointCloud left on the device, surf + edge, pcl::VoxelGrid at
// downsizeResolution().  DESIGN.md section 17 states the rule (frame_cloud_rule.hpp holds its constants and expressions); the
// sequential restatement is tests/host/frame_cloud_restatement.cpp.
//
// One call, one stream, no allocation, one upload and one read-back on the device-split path:
//   k_fc_reset     the control block; the point count is read from device memory and clamped to the capacity
//   k_fc_prep      one thread per point: refusal of a non-finite / far / zero-norm point; angle = atan2(y, z) in degrees
//   k_fc_split     ONE wave walks the break chain, 64 points a step: a ballot finds the first break after the last one; writes the scan
//                  table (begin, count, pad flags, first candidate slot).  A comparison on the walked chain that lies within the
//                  angle guard of its threshold raises kFcAmbiguous: the host then redoes the table with its own atan2
//   k_fc_scan      one wave per scan: padded scan and curvatures in LDS, vqs::wave_std_sort on (value bits, position), one lane walks
//                  the picks, the wave writes the edge points (pick order) and the surf points (ascending sorted order) to the
//                  scan's slots
//   k_fc_gather    one wave per scan: the slots are closed up into edge_raw / surf_raw (every block sums the small count table itself)
//   voxel filter   (x 3: edge_raw, surf_raw, surf ++ edge) bounding box, keys, 4 radix passes, heads, centroids; every kernel reads
//                  its element count from the control block and the grids are sized by the capacity
//   radius filter  (x 2) points hashed by their cell (edge = 1.001 r: neighbours within r lie in the 27 cells around) and radix
//                  sorted by bucket, bucket offsets, one thread per point counts the others with (double)d2 <= r * r and stops at
//                  min_pts, stable compaction (surf first, edge behind it: the cloud)
// and the control block, the downsampled cloud and (if asked for) the cloud are read back in one copy.
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "frame_cloud_rule.hpp"
#include "gfs_common.hpp"
#include "voxel_filter_dev.hpp"
#include "wave_std_sort.hpp"

using namespace gfs_voxel;
using namespace gfs_fc;

namespace {

enum { kFcBad = 1, kFcCapacity = 8, kFcScanTooLong = 16, kFcAmbiguous = 32 };
constexpr int kScanLds = kMaxCandidates + 2 * kPad + 2;  // the longest padded scan (no pads: count = candidates + 10)
constexpr double kCellScale = 1.001;                     // radius grid: cell edge / radius

struct VoxCtl {
  unsigned lo[3], hi[3];
  int flags, div[3];
};

struct Ctl {
  int n_in, flags, n_scans, n_cand;
  int n_edge_raw, n_surf_raw, n_edge_voxel, n_surf_voxel, n_edge, n_surf, n_cloud, n_down;
  VoxCtl vox[3];  // edge, surf, final
};

struct Params {
  double half_angle, max_distance, guard, r2, inv_cell;
  float leaf_edge, leaf_surf, leaf_down;
};

__global__ void k_fc_reset(const int* __restrict__ n_dev, int max_points, int host_scans, int host_cand, int host_flags, Ctl* c) {
  // host_scans >= 0: the scan table (its rows, candidates and flags) came from the host: the second pass
  const int n = *n_dev;
  c->n_in = (n < 0 || n > max_points) ? 0 : n;
  c->flags = (n < 0 || n > max_points) ? kFcCapacity : host_flags;
  c->n_scans = host_scans >= 0 ? host_scans : 0;
  c->n_cand = host_scans >= 0 ? host_cand : 0;
  c->n_edge_raw = c->n_surf_raw = c->n_edge_voxel = c->n_surf_voxel = c->n_edge = c->n_surf = c->n_cloud = c->n_down = 0;
  for (int v = 0; v < 3; v++) {
    for (int a = 0; a < 3; a++) {
      c->vox[v].lo[a] = 0xffffffffu;
      c->vox[v].hi[a] = 0u;
      c->vox[v].div[a] = 0;
    }
    c->vox[v].flags = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_fc_prep(const float4* __restrict__ in, Ctl* c, double* __restrict__ angle) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= c->n_in) return;
  const float4 P = in[i];
  const float p[3] = {P.x, P.y, P.z};
  bool bad = false;
#pragma unroll
  for (int r = 0; r < 3; r++) bad = bad || !(isfinite(p[r]) && fabsf(p[r]) < kCoordBound);
  bad = bad || !(P.x * P.x + P.y * P.y + P.z * P.z > 0.0f);  // the curvature divides by it
  if (bad) atomicOr(&c->flags, kFcBad);
  angle[i] = bad ? 0.0 : angle_deg(P.y, P.z);
}

// |v - threshold| <= guard: the device's atan2 may decide this comparison differently from the host's
__device__ __forceinline__ bool near_threshold(double v, double threshold, double guard) { return fabs(v - threshold) <= guard; }

__global__ __launch_bounds__(64) void k_fc_split(const float4* __restrict__ in, const double* __restrict__ angle, Params P, int max_scans,
                                                 Ctl* c, Scan* __restrict__ scans) {
  const int lane = threadIdx.x, n = c->n_in;
  if (n <= 0 || (c->flags & kFcBad)) return;
  double last = angle[0];
  int run = 0, pos = 0, n_scans = 0, cand = 0, flags = 0;
  while (pos < n) {
    const int i = pos + lane;
    const double a = angle[min(i, n - 1)];
    const double d = fabs(a - last);
    const bool brk = i < n && d > kScanBreakDeg;
    const unsigned long long bb = __ballot(brk);
    const int first = bb ? __builtin_ctzll(bb) : 64;
    // the comparisons the sequential walk makes against this `last`: up to and including the first break
    if (__ballot(i < n && lane <= first && near_threshold(d, kScanBreakDeg, P.guard))) flags |= kFcAmbiguous;
    if (first == 64) {
      pos += 64;
      continue;
    }
    const int ib = pos + first;
    if (ib - run > kMinScanCount && n_scans < max_scans) {
      const float4 A = in[run], B = in[ib - 1];
      const double sa = angle_deg(A.x, A.z), ea = angle_deg(B.x, B.z);
      const double st = -P.half_angle + kPadMarginDeg, et = P.half_angle - kPadMarginDeg;
      if (near_threshold(sa, st, P.guard) || near_threshold(ea, et, P.guard)) flags |= kFcAmbiguous;
      const int pad = (sa > st ? kPadStart : 0) | (ea < et ? kPadEnd : 0);
      const int nc = candidates_of(ib - run, pad);
      if (nc > kMaxCandidates) flags |= kFcScanTooLong;
      if (lane == 0) scans[n_scans] = Scan{run, ib - run, pad, cand};
      cand += nc;
      n_scans++;
    }
    run = ib;
    last = __shfl(a, first);
    pos = ib + 1;
  }
  if (lane == 0) {
    c->n_scans = n_scans;
    c->n_cand = cand;
    if (flags) atomicOr(&c->flags, flags);
  }
}

// One wave per scan.  edge_slot [scan][10], surf_slot [candidate slot]: closed up by k_fc_gather.
__global__ __launch_bounds__(64) void k_fc_scan(const float4* __restrict__ in, const Ctl* __restrict__ c, const Scan* __restrict__ scans,
                                                float max_distance, float4* __restrict__ edge_slot, float4* __restrict__ surf_slot,
                                                int* __restrict__ n_edge_of) {
  __shared__ float X[kScanLds], Y[kScanLds], Z[kScanLds];
  __shared__ vqs::u64 K[kMaxCandidates];
  __shared__ unsigned short Pm[kMaxCandidates], l0[kMaxCandidates], l1[kMaxCandidates], cl[kMaxCandidates], st[3 * 40];
  __shared__ unsigned char picked[kScanLds], is_edge[kScanLds];
  __shared__ int s_edge[kMaxEdgePicks], s_ne;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= c->n_scans || (c->flags & (kFcBad | kFcCapacity | kFcScanTooLong))) return;
  const Scan sc = scans[s];
  const int ps = (sc.pad & kPadStart) ? kPad : 0, pe = (sc.pad & kPadEnd) ? kPad : 0;
  const int size = sc.count + ps + pe, nc = size - 2 * kPad;
  if (nc > kMaxCandidates || nc < 1) return;
  for (int j = lane; j < size; j += 64) {
    const int k = j - ps;  // position in the run
    const float4 Q = in[sc.begin + min(max(k, 0), sc.count - 1)];
    X[j] = Q.x;
    Y[j] = Q.y;
    Z[j] = (k < 0 || k >= sc.count) ? max_distance : Q.z;
    picked[j] = 0;
    is_edge[j] = 0;
  }
  __syncthreads();
  for (int q = lane; q < nc; q += 64) {
    const double v = curvature(X, Y, Z, q + kPad);
    K[q] = (vqs::u64)__double_as_longlong(v);  // values are >= +0 (or +inf): the order of the bits is the order of the doubles
    Pm[q] = (unsigned short)(q + kPad);
  }
  __syncthreads();
  vqs::wave_std_sort<vqs::u64>(K, Pm, l0, l1, cl, st, nc);
  __syncthreads();
  if (lane == 0) {
    int ne = 0, largest = 0;
    for (int i = nc - 1; i >= 0; i--) {
      const int ind = Pm[i];
      if (picked[ind]) continue;
      if (__longlong_as_double((long long)K[i]) <= kEdgeMinValue) break;
      largest++;
      picked[ind] = 1;
      if (largest > kMaxEdgePicks) break;
      s_edge[ne++] = ind;
      is_edge[ind] = 1;
      for (int k = -kPickHalo; k <= kPickHalo; k++) picked[ind + k] = 1;  // ind in [5, size - 5): inside the padded scan
    }
    s_ne = ne;
    n_edge_of[s] = ne;
  }
  __syncthreads();
  const int ne = s_ne;
  if (lane < ne) {
    const int ind = s_edge[lane];
    edge_slot[(size_t)s * kMaxEdgePicks + lane] = make_float4(X[ind], Y[ind], Z[ind], 0.0f);
  }
  int out = sc.cand_begin;
  for (int q0 = 0; q0 < nc; q0 += 64) {
    const int q = q0 + lane;
    const int ind = q < nc ? Pm[q] : 0;
    const bool surf = q < nc && !is_edge[ind];
    const unsigned long long b = __ballot(surf);
    if (surf) surf_slot[out + __popcll(b & ((1ull << lane) - 1ull))] = make_float4(X[ind], Y[ind], Z[ind], 0.0f);
    out += __popcll(b);
  }
}

__global__ __launch_bounds__(64) void k_fc_gather(Ctl* c, const Scan* __restrict__ scans, const int* __restrict__ n_edge_of,
                                                  const float4* __restrict__ edge_slot, const float4* __restrict__ surf_slot,
                                                  float4* __restrict__ edge_raw, float4* __restrict__ surf_raw) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const bool off = (c->flags & (kFcBad | kFcCapacity | kFcScanTooLong)) != 0;
  const int n_scans = off ? 0 : c->n_scans;
  if (s >= n_scans && s != 0) return;
  int before = 0, total = 0;
  for (int t = lane; t < n_scans; t += 64) {
    const int v = n_edge_of[t];
    total += v;
    if (t < s) before += v;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    before += __shfl_xor(before, o);
    total += __shfl_xor(total, o);
  }
  if (s == 0 && lane == 0) {
    c->n_edge_raw = total;
    c->n_surf_raw = (off ? 0 : c->n_cand) - total;
  }
  if (s >= n_scans) return;
  const Scan sc = scans[s];
  const int ne = n_edge_of[s], ns = candidates_of(sc.count, sc.pad) - ne;
  if (lane < ne) edge_raw[before + lane] = edge_slot[(size_t)s * kMaxEdgePicks + lane];
  for (int q = lane; q < ns; q += 64) surf_raw[sc.cand_begin - before + q] = surf_slot[sc.cand_begin + q];
}

// ------------------------------------------------------------------ pcl::VoxelGrid on a device-counted cloud

__global__ __launch_bounds__(kThreads) void k_fc_bbox(const float4* __restrict__ pts, const int* __restrict__ n_dev, VoxCtl* v) {
  __shared__ unsigned s_lo[3][kThreads / 64], s_hi[3][kThreads / 64];
  const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid, n = *n_dev;
  if (blockIdx.x * kThreads >= n) return;
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (i < n) {
    const float4 P = pts[i];
    lo[0] = hi[0] = f_enc(P.x);
    lo[1] = hi[1] = f_enc(P.y);
    lo[2] = hi[2] = f_enc(P.z);
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
    atomicMin(&v->lo[tid], l);
    atomicMax(&v->hi[tid], h);
  }
}

__global__ __launch_bounds__(kThreads) void k_fc_keys(const float4* __restrict__ pts, const int* __restrict__ n_dev, float leaf, VoxCtl* v,
                                                      unsigned* __restrict__ key, unsigned* __restrict__ val) {
  const int i = blockIdx.x * kThreads + threadIdx.x, n = *n_dev;
  if (n <= 0) return;  // an empty cloud: no grid, no flag
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) {
    mn[a] = f_dec(v->lo[a]);
    mx[a] = f_dec(v->hi[a]);
  }
  VoxelGridDims g;
  const int mode = voxel_grid_dims(mn, mx, leaf, &g);
  if (i == 0) {
    if (mode) atomicOr(&v->flags, mode);
    for (int a = 0; a < 3; a++) v->div[a] = g.div[a];
  }
  if (i >= n) return;
  unsigned k = 0;
  if (mode == kFlagPassthrough) {
    k = (unsigned)i;
  } else if (mode == 0) {
    const float4 P = pts[i];
    const unsigned i0 = (unsigned)(int)(floorf(P.x * g.inv) - (float)g.min_b[0]);
    const unsigned i1 = (unsigned)(int)(floorf(P.y * g.inv) - (float)g.min_b[1]);
    const unsigned i2 = (unsigned)(int)(floorf(P.z * g.inv) - (float)g.min_b[2]);
    k = i0 + i1 * (unsigned)g.div[0] + i2 * (unsigned)g.div[0] * (unsigned)g.div[1];
  }
  key[i] = k;
  val[i] = (unsigned)i;
}

__global__ __launch_bounds__(kThreads) void k_fc_heads(const unsigned* __restrict__ skey, const int* __restrict__ n_dev, int* __restrict__ blkcnt) {
  __shared__ int sh[kThreads];
  const int n = *n_dev, j0 = blockIdx.x * kTile + threadIdx.x * kItems;
  int cnt = 0;
  for (int u = 0; u < kItems; u++) {
    const int j = j0 + u;
    if (j < n && (j == 0 || skey[j] != skey[j - 1])) cnt++;
  }
  int total;
  block_scan<kThreads>(cnt, sh, &total);
  if (threadIdx.x == 0) blkcnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_fc_centroid(const unsigned* __restrict__ skey, const unsigned* __restrict__ sval,
                                                          const float4* __restrict__ pts, const int* __restrict__ n_dev,
                                                          const int* __restrict__ blkcnt, int nblk, const VoxCtl* __restrict__ v,
                                                          float4* __restrict__ out, int* n_out) {
  __shared__ int sh[kThreads];
  const int flags = v->flags, n = *n_dev;
  if ((flags & kFlagUnsupported) || n <= 0) return;  // n_out stays 0
  const int tid = threadIdx.x;
  int before = 0, all = 0;
  for (int b = tid; b < nblk; b += kThreads) {
    const int c = blkcnt[b];
    all += c;
    if (b < (int)blockIdx.x) before += c;
  }
  int total, base;
  block_scan<kThreads>(all, sh, &total);
  block_scan<kThreads>(before, sh, &base);
  if (blockIdx.x == 0 && tid == 0) *n_out = total;
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
      o = pts[sval[j]];
    } else {
      float s0, s1, s2;
      const int m = voxel_run_sum(skey, sval, pts, n, j, &s0, &s1, &s2);
      const float fc = (float)(m - j);
      o = make_float4(s0 / fc, s1 / fc, s2 / fc, 0.0f);
    }
    out[slot++] = o;
  }
}

// ------------------------------------------------------------------ RadiusOutlierRemoval

struct Cell {
  long long x, y, z;
};
__device__ __forceinline__ Cell cell_of_point(const float4& P, double inv_cell) {
  return Cell{(long long)floor((double)P.x * inv_cell), (long long)floor((double)P.y * inv_cell), (long long)floor((double)P.z * inv_cell)};
}
__device__ __forceinline__ unsigned cell_bucket(const Cell& q, unsigned nb) {
  const unsigned long long h = (unsigned long long)q.x * 73856093ull ^ (unsigned long long)q.y * 19349663ull ^ (unsigned long long)q.z * 83492791ull;
  return (unsigned)((h ^ (h >> 32)) & (nb - 1));
}

__global__ __launch_bounds__(kThreads) void k_fc_rad_keys(const float4* __restrict__ pts, const int* __restrict__ n_dev, double inv_cell,
                                                          unsigned nb, unsigned* __restrict__ key, unsigned* __restrict__ val) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= *n_dev) return;
  key[i] = cell_bucket(cell_of_point(pts[i], inv_cell), nb);
  val[i] = (unsigned)i;
}

__global__ __launch_bounds__(kThreads) void k_fc_rad_starts(const unsigned* __restrict__ skey, const int* __restrict__ n_dev, unsigned nb,
                                                            int* __restrict__ start) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x;
  if (i > nb) return;
  int a = 0, b = *n_dev;  // the first sorted position whose bucket is >= i
  while (a < b) {
    const int m = (a + b) >> 1;
    if (skey[m] < i) a = m + 1; else b = m;
  }
  start[i] = a;
}

__global__ __launch_bounds__(kThreads) void k_fc_rad_count(const float4* __restrict__ pts, const unsigned* __restrict__ sval,
                                                           const int* __restrict__ start, const int* __restrict__ n_dev, double r2,
                                                           double inv_cell, unsigned nb, int min_pts, unsigned char* __restrict__ keep,
                                                           int* __restrict__ blkcnt) {
  __shared__ int sh[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x, n = *n_dev;
  int kept = 0;
  if (i < n) {
    const float4 P = pts[i];
    const Cell c0 = cell_of_point(P, inv_cell);
    int cnt = 0;
    for (int d = 0; d < 27 && cnt < min_pts; d++) {
      const Cell q{c0.x + d % 3 - 1, c0.y + (d / 3) % 3 - 1, c0.z + d / 9 - 1};
      const unsigned b = cell_bucket(q, nb);
      const int e = start[b + 1];
      for (int j = start[b]; j < e && cnt < min_pts; j++) {
        const int o = (int)sval[j];
        if (o == i) continue;
        const float4 Q = pts[o];
        const Cell cq = cell_of_point(Q, inv_cell);  // a bucket may hold several cells: a point counts under its own cell only
        if (cq.x != q.x || cq.y != q.y || cq.z != q.z) continue;
        if ((double)dist2(Q.x, Q.y, Q.z, P.x, P.y, P.z) <= r2) cnt++;
      }
    }
    kept = cnt >= min_pts ? 1 : 0;
    keep[i] = (unsigned char)kept;
  }
  int total;
  block_scan<kThreads>(kept, sh, &total);
  if (threadIdx.x == 0) blkcnt[blockIdx.x] = total;
}

// kept points in input order to out[*base + ...]; *n_out = the kept count, *n_sum (may be null) = *base + the kept count
__global__ __launch_bounds__(kThreads) void k_fc_rad_compact(const float4* __restrict__ pts, const unsigned char* __restrict__ keep,
                                                             const int* __restrict__ blkcnt, int nblk, const int* __restrict__ n_dev,
                                                             const int* __restrict__ base_dev, float4* __restrict__ out, int* n_out,
                                                             int* n_sum) {
  __shared__ int sh[kThreads];
  const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid, n = *n_dev;
  const int nb_used = min(nblk, (n + kThreads - 1) / kThreads);
  const int base = base_dev ? *base_dev : 0;
  int before = 0, all = 0;
  for (int b = tid; b < nb_used; b += kThreads) {
    const int c = blkcnt[b];
    all += c;
    if (b < (int)blockIdx.x) before += c;
  }
  int total, off;
  block_scan<kThreads>(all, sh, &total);
  block_scan<kThreads>(before, sh, &off);
  if (blockIdx.x == 0 && tid == 0) {
    *n_out = total;
    if (n_sum) *n_sum = base + total;
  }
  const int k = i < n ? keep[i] : 0;
  int unused;
  const int rank = block_scan<kThreads>(k, sh, &unused);
  if (k) out[base + off + rank] = pts[i];
}

size_t next_pow2(size_t v) {
  size_t p = 64;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace

struct gfs_frame_cloud {
  int device, max_points, max_scans, max_blk;
  gfs_frame_cloud_config cfg;
  Params P;
  hipStream_t stream;
  std::mutex mu;
  size_t res_bytes;  // the result block: Ctl | down [cap] | cloud [cap]
  gfs::DevBuf<uint8_t> d_in, d_res, d_keep;
  gfs::PinBuf<uint8_t> h_in, h_res;
  gfs::DevBuf<double> d_angle;
  gfs::DevBuf<Scan> d_scans;
  gfs::PinBuf<Scan> h_scans;
  gfs::DevBuf<int> d_nedge, d_hist, d_blk, d_start;
  gfs::DevBuf<float4> d_edge_slot, d_surf_slot, d_edge_raw, d_surf_raw, d_edge_vox, d_surf_vox;
  gfs::DevBuf<unsigned> d_key[2], d_val[2];
  // the last call, for gfs_test_frame_cloud_stages
  bool last_ok = false;
  int last_cap = 0;
  Ctl last{};
};

namespace {

constexpr size_t kHead = 256;  // the control block's / the point count's slot in front of the arrays

Ctl* ctl_of(gfs_frame_cloud* h) { return reinterpret_cast<Ctl*>(h->d_res.p); }
float4* down_of(gfs_frame_cloud* h) { return reinterpret_cast<float4*>(h->d_res.p + kHead); }
float4* cloud_of(gfs_frame_cloud* h, int cap) { return reinterpret_cast<float4*>(h->d_res.p + kHead) + cap; }

// Sorts (key[0], val[0]) by the low 8 * passes bits; returns the buffer index holding the result.
int radix_sort(gfs_frame_cloud* h, int cap, const int* n_dev, int passes, int* at) {
  const int nblk = gfs::div_up(cap, kTile);
  hipStream_t s = h->stream;
  int from = 0;
  for (int p = 0; p < passes; p++, from ^= 1) {
    GFS_LAUNCH("k_lm_hist", k_lm_hist, dim3(nblk), dim3(kThreads), 0, s, h->d_key[from].p, cap, n_dev, 8 * p, h->d_hist.p, nblk);
    GFS_LAUNCH("k_lm_scatter", k_lm_scatter, dim3(nblk), dim3(kThreads), 0, s, h->d_key[from].p, h->d_val[from].p, cap, n_dev, 8 * p,
               h->d_hist.p, nblk, h->d_key[from ^ 1].p, h->d_val[from ^ 1].p);
  }
  *at = from;
  return GFS_OK;
}

int voxel_filter(gfs_frame_cloud* h, int cap, const float4* in, const int* n_dev, float leaf, int which, float4* out, int* n_out) {
  hipStream_t s = h->stream;
  VoxCtl* v = &ctl_of(h)->vox[which];
  const int nblk = gfs::div_up(cap, kTile), nb256 = gfs::div_up(cap, kThreads);
  GFS_LAUNCH("k_fc_bbox", k_fc_bbox, dim3(nb256), dim3(kThreads), 0, s, in, n_dev, v);
  GFS_LAUNCH("k_fc_keys", k_fc_keys, dim3(nb256), dim3(kThreads), 0, s, in, n_dev, leaf, v, h->d_key[0].p, h->d_val[0].p);
  int at;
  const int rc = radix_sort(h, cap, n_dev, 4, &at);
  if (rc) return rc;
  GFS_LAUNCH("k_fc_heads", k_fc_heads, dim3(nblk), dim3(kThreads), 0, s, h->d_key[at].p, n_dev, h->d_blk.p);
  GFS_LAUNCH("k_fc_centroid", k_fc_centroid, dim3(nblk), dim3(kThreads), 0, s, h->d_key[at].p, h->d_val[at].p, in, n_dev, h->d_blk.p, nblk,
             v, out, n_out);
  return GFS_OK;
}

int radius_filter(gfs_frame_cloud* h, int cap, const float4* in, const int* n_dev, int min_pts, const int* base_dev, float4* out, int* n_out,
                  int* n_sum) {
  hipStream_t s = h->stream;
  const unsigned nb = (unsigned)next_pow2(2 * (size_t)cap);
  int bits = 0;
  while ((1u << bits) < nb) bits++;
  const int nb256 = gfs::div_up(cap, kThreads);
  GFS_LAUNCH("k_fc_rad_keys", k_fc_rad_keys, dim3(nb256), dim3(kThreads), 0, s, in, n_dev, h->P.inv_cell, nb, h->d_key[0].p, h->d_val[0].p);
  int at;
  const int rc = radix_sort(h, cap, n_dev, (bits + 7) / 8, &at);
  if (rc) return rc;
  GFS_LAUNCH("k_fc_rad_starts", k_fc_rad_starts, dim3(gfs::div_up((int)nb + 1, kThreads)), dim3(kThreads), 0, s, h->d_key[at].p, n_dev, nb,
             h->d_start.p);
  GFS_LAUNCH("k_fc_rad_count", k_fc_rad_count, dim3(nb256), dim3(kThreads), 0, s, in, h->d_val[at].p, h->d_start.p, n_dev, h->P.r2,
             h->P.inv_cell, nb, min_pts, h->d_keep.p, h->d_blk.p);
  GFS_LAUNCH("k_fc_rad_compact", k_fc_rad_compact, dim3(nb256), dim3(kThreads), 0, s, in, h->d_keep.p, h->d_blk.p, nb256, n_dev, base_dev, out,
             n_out, n_sum);
  return GFS_OK;
}

// Everything behind the scan table, and the read-back of the result block.
int run_from_scans(gfs_frame_cloud* h, const float4* d_xyzw, int cap, bool want_cloud) {
  hipStream_t s = h->stream;
  Ctl* c = ctl_of(h);
  const int max_scans = std::min(h->max_scans, cap / (kMinScanCount + 1) + 1);
  GFS_LAUNCH("k_fc_scan", k_fc_scan, dim3(max_scans), dim3(64), 0, s, d_xyzw, c, h->d_scans.p, (float)h->cfg.max_distance, h->d_edge_slot.p,
             h->d_surf_slot.p, h->d_nedge.p);
  GFS_LAUNCH("k_fc_gather", k_fc_gather, dim3(max_scans), dim3(64), 0, s, c, h->d_scans.p, h->d_nedge.p, h->d_edge_slot.p, h->d_surf_slot.p,
             h->d_edge_raw.p, h->d_surf_raw.p);
  const int cap_edge = std::min(cap, max_scans * kMaxEdgePicks);
  int rc = voxel_filter(h, cap_edge, h->d_edge_raw.p, &c->n_edge_raw, h->P.leaf_edge, 0, h->d_edge_vox.p, &c->n_edge_voxel);
  if (!rc) rc = voxel_filter(h, cap, h->d_surf_raw.p, &c->n_surf_raw, h->P.leaf_surf, 1, h->d_surf_vox.p, &c->n_surf_voxel);
  float4* cloud = cloud_of(h, cap);
  if (!rc) rc = radius_filter(h, cap, h->d_surf_vox.p, &c->n_surf_voxel, kSurfMinNeighbors, nullptr, cloud, &c->n_surf, nullptr);
  if (!rc) rc = radius_filter(h, cap_edge, h->d_edge_vox.p, &c->n_edge_voxel, kEdgeMinNeighbors, &c->n_surf, cloud, &c->n_edge, &c->n_cloud);
  if (!rc) rc = voxel_filter(h, cap, cloud, &c->n_cloud, h->P.leaf_down, 2, down_of(h), &c->n_down);
  if (rc) return rc;
  const size_t bytes = kHead + (size_t)cap * sizeof(float4) * (want_cloud ? 2 : 1);
  GFS_HIP(hipMemcpyAsync(h->h_res.p, h->d_res.p, bytes, hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  return GFS_OK;
}

void fill_info(gfs_frame_cloud_info* info, const Ctl& c, int host_split) {
  if (!info) return;
  *info = gfs_frame_cloud_info{c.n_in,   c.n_scans, c.n_edge_raw, c.n_surf_raw, c.n_edge_voxel, c.n_surf_voxel,
                               c.n_edge, c.n_surf,  c.n_down,     host_split,   {0, 0, 0}};
  for (int v = 0; v < 3; v++) info->passthrough[v] = (c.vox[v].flags & kFlagPassthrough) ? 1 : 0;
}

// d_xyzw / d_count: device memory; cap: the host's upper bound of the point count (sizes the grids and the result block)
int extract_common(gfs_frame_cloud* h, const float4* d_xyzw, const int* d_count, int cap, float* cloud_xyz, int cap_cloud, float* down_xyz,
                   int cap_down, gfs_frame_cloud_info* info) {
  hipStream_t s = h->stream;
  Ctl* c = ctl_of(h);
  h->last_ok = false;
  const int max_scans = std::min(h->max_scans, cap / (kMinScanCount + 1) + 1);
  GFS_LAUNCH("k_fc_reset", k_fc_reset, dim3(1), dim3(1), 0, s, d_count, h->max_points, -1, 0, 0, c);
  GFS_LAUNCH("k_fc_prep", k_fc_prep, dim3(gfs::div_up(cap, kThreads)), dim3(kThreads), 0, s, d_xyzw, c, h->d_angle.p);
  GFS_LAUNCH("k_fc_split", k_fc_split, dim3(1), dim3(64), 0, s, d_xyzw, h->d_angle.p, h->P, max_scans, c, h->d_scans.p);
  const bool want_cloud = cloud_xyz != nullptr;
  int rc = run_from_scans(h, d_xyzw, cap, want_cloud);
  if (rc) return rc;
  Ctl r = *reinterpret_cast<const Ctl*>(h->h_res.p);
  int host_split = 0;
  if ((r.flags & kFcAmbiguous) && !(r.flags & (kFcBad | kFcCapacity))) {
    // a comparison on the walked chain was too close to call with the device's atan2: the table again with the host's
    host_split = 1;
    const int n = r.n_in;
    std::vector<float> pts((size_t)n * 4);
    GFS_HIP(hipMemcpyAsync(pts.data(), d_xyzw, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    GFS_HIP(hipStreamSynchronize(s));
    bool too_long;
    const int n_scans = split_host(pts.data(), n, h->cfg.horizontal_angle, h->h_scans.p, &too_long);
    if (n_scans > 0) GFS_HIP(hipMemcpyAsync(h->d_scans.p, h->h_scans.p, (size_t)n_scans * sizeof(Scan), hipMemcpyHostToDevice, s));
    int cand = 0;
    if (n_scans > 0) {
      const Scan& e = h->h_scans.p[n_scans - 1];
      cand = e.cand_begin + candidates_of(e.count, e.pad);
    }
    GFS_LAUNCH("k_fc_reset", k_fc_reset, dim3(1), dim3(1), 0, s, d_count, h->max_points, n_scans, cand, too_long ? kFcScanTooLong : 0, c);
    rc = run_from_scans(h, d_xyzw, cap, want_cloud);
    if (rc) return rc;
    r = *reinterpret_cast<const Ctl*>(h->h_res.p);
  }
  h->last = r;
  h->last_cap = cap;
  int unsupported = 0;
  for (int v = 0; v < 3; v++) unsupported |= r.vox[v].flags & kFlagUnsupported;
  if (info) *info = gfs_frame_cloud_info{r.n_in, 0, 0, 0, 0, 0, 0, 0, 0, host_split, {0, 0, 0}};
  GFS_REQUIRE(!(r.flags & kFcCapacity), GFS_ERR_CAPACITY, "gfs_frame_cloud_extract: the device's point count is negative or exceeds capacity %d",
              h->max_points);
  GFS_REQUIRE(r.n_in >= 1, GFS_ERR_INVALID_ARG, "gfs_frame_cloud_extract: an empty cloud (the reference reads points[0])");
  GFS_REQUIRE(!(r.flags & kFcBad), GFS_ERR_INVALID_ARG,
              "gfs_frame_cloud_extract: a point is not finite, beyond 1e6 m, or at the origin (the curvature divides by its squared norm)");
  GFS_REQUIRE(!(r.flags & kFcScanTooLong), GFS_ERR_CAPACITY, "gfs_frame_cloud_extract: a scan has more than %d candidates", kMaxCandidates);
  GFS_REQUIRE(!unsupported, GFS_ERR_UNSUPPORTED,
              "gfs_frame_cloud_extract: a voxel grid's index range exceeds int (pcl::VoxelGrid would overflow)");
  fill_info(info, r, host_split);
  h->last_ok = true;
  const int n_cloud = r.n_surf + r.n_edge;
  GFS_REQUIRE(!want_cloud || n_cloud <= cap_cloud, GFS_ERR_CAPACITY, "gfs_frame_cloud_extract: %d cloud points exceed cap %d", n_cloud, cap_cloud);
  GFS_REQUIRE(r.n_down <= cap_down, GFS_ERR_CAPACITY, "gfs_frame_cloud_extract: %d downsampled points exceed cap_down %d", r.n_down, cap_down);
  const float4* down = reinterpret_cast<const float4*>(h->h_res.p + kHead);
  for (int i = 0; i < r.n_down; i++) {
    down_xyz[3 * i] = down[i].x;
    down_xyz[3 * i + 1] = down[i].y;
    down_xyz[3 * i + 2] = down[i].z;
  }
  if (want_cloud) {
    const float4* cl = down + cap;
    for (int i = 0; i < n_cloud; i++) {
      cloud_xyz[3 * i] = cl[i].x;
      cloud_xyz[3 * i + 1] = cl[i].y;
      cloud_xyz[3 * i + 2] = cl[i].z;
    }
  }
  return GFS_OK;
}

bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

int fetch3(const float4* d, int n, float* out, int cap) {
  if (!out || n == 0) return GFS_OK;
  GFS_REQUIRE(n <= cap, GFS_ERR_CAPACITY, "gfs_test_frame_cloud_stages: %d points exceed cap_points %d", n, cap);
  std::vector<float4> t((size_t)n);
  GFS_HIP(hipMemcpy(t.data(), d, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    out[3 * i] = t[i].x;
    out[3 * i + 1] = t[i].y;
    out[3 * i + 2] = t[i].z;
  }
  return GFS_OK;
}

}  // namespace

extern "C" {

void gfs_frame_cloud_default_config(gfs_frame_cloud_config* cfg) {
  if (!cfg) return;
  cfg->horizontal_angle = kDefaultHorizontalAngle;
  cfg->max_distance = kDefaultMaxDistance;
  cfg->local_map_resolution = kDefaultLocalMapResolution;
  cfg->downsize_resolution = 0.05f;
  cfg->angle_guard_deg = kDefaultAngleGuardDeg;
}

int gfs_frame_cloud_create(int device, int max_points, const gfs_frame_cloud_config* cfg, gfs_frame_cloud** out) {
  GFS_REQUIRE(out && cfg && max_points >= 1 && max_points <= (1 << 26), GFS_ERR_INVALID_ARG, "gfs_frame_cloud_create: invalid argument");
  GFS_REQUIRE(positive_finite(cfg->local_map_resolution) && positive_finite((double)cfg->downsize_resolution) &&
                  positive_finite((double)(float)(cfg->local_map_resolution / kEdgeLeafDivisor)),
              GFS_ERR_INVALID_ARG, "gfs_frame_cloud_create: resolutions %g / %g are not positive and finite", cfg->local_map_resolution,
              (double)cfg->downsize_resolution);
  GFS_REQUIRE(std::isfinite(cfg->horizontal_angle) && std::isfinite(cfg->max_distance) && std::fabs(cfg->max_distance) < (double)kCoordBound &&
                  cfg->max_distance != 0.0 && std::isfinite(cfg->angle_guard_deg) && cfg->angle_guard_deg >= 0.0,
              GFS_ERR_INVALID_ARG, "gfs_frame_cloud_create: horizontal_angle, max_distance or angle_guard_deg out of range");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_frame_cloud> h(new gfs_frame_cloud);
  h->device = device;
  h->max_points = max_points;
  h->max_scans = max_points / (kMinScanCount + 1) + 1;
  h->max_blk = gfs::div_up(max_points, kThreads);
  h->cfg = *cfg;
  const double r = cfg->local_map_resolution;
  h->P = Params{cfg->horizontal_angle / 2.0, cfg->max_distance, cfg->angle_guard_deg, r * r, 1.0 / (r * kCellScale),
                (float)(r / kEdgeLeafDivisor), (float)(r / kSurfLeafDivisor), cfg->downsize_resolution};
  const size_t N = (size_t)max_points;
  h->res_bytes = kHead + 2 * N * sizeof(float4);
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  int rc = 0;
#define A(x) if (!rc) rc = (x)
  A(h->d_in.alloc(kHead + N * sizeof(float4)));
  A(h->h_in.alloc(kHead + N * sizeof(float4)));
  A(h->d_res.alloc(h->res_bytes));
  A(h->h_res.alloc(h->res_bytes));
  A(h->d_keep.alloc(N));
  A(h->d_angle.alloc(N));
  A(h->d_scans.alloc((size_t)h->max_scans));
  A(h->h_scans.alloc((size_t)h->max_scans));
  A(h->d_nedge.alloc((size_t)h->max_scans));
  A(h->d_hist.alloc((size_t)kBins * gfs::div_up(max_points, kTile)));
  A(h->d_blk.alloc((size_t)h->max_blk));
  A(h->d_start.alloc(next_pow2(2 * N) + 1));
  A(h->d_edge_slot.alloc((size_t)h->max_scans * kMaxEdgePicks));
  A(h->d_surf_slot.alloc(N));
  A(h->d_edge_raw.alloc((size_t)h->max_scans * kMaxEdgePicks));
  A(h->d_surf_raw.alloc(N));
  A(h->d_edge_vox.alloc((size_t)h->max_scans * kMaxEdgePicks));
  A(h->d_surf_vox.alloc(N));
  for (int k = 0; k < 2; k++) {
    A(h->d_key[k].alloc(N));
    A(h->d_val[k].alloc(N));
  }
#undef A
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_frame_cloud_destroy(gfs_frame_cloud* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_frame_cloud_extract(gfs_frame_cloud* h, const float* xyzw, int n, float* cloud_xyz, int cap, float* down_xyz, int cap_down,
                            gfs_frame_cloud_info* info) {
  GFS_REQUIRE(h && xyzw && n >= 0 && cap >= 0 && cap_down >= 0 && (down_xyz || cap_down == 0), GFS_ERR_INVALID_ARG,
              "gfs_frame_cloud_extract: invalid argument");
  if (info) *info = gfs_frame_cloud_info{n, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
  GFS_REQUIRE(n >= 1, GFS_ERR_INVALID_ARG, "gfs_frame_cloud_extract: an empty cloud (the reference reads points[0])");
  GFS_REQUIRE(n <= h->max_points, GFS_ERR_CAPACITY, "gfs_frame_cloud_extract: %d points exceed capacity %d", n, h->max_points);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  memcpy(h->h_in.p, &n, sizeof(int));
  memcpy(h->h_in.p + kHead, xyzw, (size_t)n * 16);
  GFS_HIP(hipMemcpyAsync(h->d_in.p, h->h_in.p, kHead + (size_t)n * 16, hipMemcpyHostToDevice, h->stream));  // the count and the points: one copy
  return extract_common(h, reinterpret_cast<const float4*>(h->d_in.p + kHead), reinterpret_cast<const int*>(h->d_in.p), n, cloud_xyz, cap,
                        down_xyz, cap_down, info);
}

int gfs_frame_cloud_extract_device(gfs_frame_cloud* h, const void* dev_xyzw, const void* dev_count, float* cloud_xyz, int cap, float* down_xyz,
                                   int cap_down, gfs_frame_cloud_info* info) {
  GFS_REQUIRE(h && dev_xyzw && dev_count && cap >= 0 && cap_down >= 0 && (down_xyz || cap_down == 0), GFS_ERR_INVALID_ARG,
              "gfs_frame_cloud_extract_device: invalid argument");
  if (info) *info = gfs_frame_cloud_info{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  return extract_common(h, static_cast<const float4*>(dev_xyzw), static_cast<const int*>(dev_count), h->max_points, cloud_xyz, cap, down_xyz,
                        cap_down, info);
}

int gfs_test_frame_cloud_stages(gfs_frame_cloud* h, gfs_test_frame_cloud_stage_buffers* out) {
  GFS_REQUIRE(h && out && out->cap_scans >= 0 && out->cap_points >= 0, GFS_ERR_INVALID_ARG, "gfs_test_frame_cloud_stages: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_REQUIRE(h->last_ok, GFS_ERR_INVALID_ARG, "gfs_test_frame_cloud_stages: the handle's last call was refused (or none was made)");
  GFS_HIP(hipSetDevice(h->device));
  const Ctl& c = h->last;
  if (out->scans && c.n_scans > 0) {
    GFS_REQUIRE(c.n_scans <= out->cap_scans, GFS_ERR_CAPACITY, "gfs_test_frame_cloud_stages: %d scans exceed cap_scans %d", c.n_scans,
                out->cap_scans);
    static_assert(sizeof(Scan) == 4 * sizeof(int32_t), "the scan table is copied out as it is");
    GFS_HIP(hipMemcpy(out->scans, h->d_scans.p, (size_t)c.n_scans * sizeof(Scan), hipMemcpyDeviceToHost));
  }
  const float4* cloud = cloud_of(h, h->last_cap);
  int rc = fetch3(h->d_edge_raw.p, c.n_edge_raw, out->edge_raw, out->cap_points);
  if (!rc) rc = fetch3(h->d_surf_raw.p, c.n_surf_raw, out->surf_raw, out->cap_points);
  if (!rc) rc = fetch3(h->d_edge_vox.p, c.n_edge_voxel, out->edge_voxel, out->cap_points);
  if (!rc) rc = fetch3(h->d_surf_vox.p, c.n_surf_voxel, out->surf_voxel, out->cap_points);
  if (!rc) rc = fetch3(cloud + c.n_surf, c.n_edge, out->edge, out->cap_points);
  if (!rc) rc = fetch3(cloud, c.n_surf, out->surf, out->cap_points);
  return rc;
}

int gfs_test_frame_cloud_radius(gfs_frame_cloud* h, const float* xyz, int n, int min_pts, float* out_xyz, int cap, int32_t* n_out) {
  GFS_REQUIRE(h && xyz && out_xyz && n_out && n >= 1 && n <= h->max_points && min_pts >= 0 && cap >= n, GFS_ERR_INVALID_ARG,
              "gfs_test_frame_cloud_radius: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  h->last_ok = false;
  hipStream_t s = h->stream;
  Ctl* c = ctl_of(h);
  float4* in = reinterpret_cast<float4*>(h->h_in.p + kHead);
  for (int i = 0; i < n; i++) in[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
  memcpy(h->h_in.p, &n, sizeof(int));
  GFS_HIP(hipMemcpyAsync(h->d_in.p, h->h_in.p, kHead + (size_t)n * 16, hipMemcpyHostToDevice, s));
  GFS_LAUNCH("k_fc_reset", k_fc_reset, dim3(1), dim3(1), 0, s, reinterpret_cast<const int*>(h->d_in.p), h->max_points, -1, 0, 0, c);
  const int rc = radius_filter(h, n, reinterpret_cast<const float4*>(h->d_in.p + kHead), &c->n_in, min_pts, nullptr, cloud_of(h, n), &c->n_surf,
                               nullptr);
  if (rc) return rc;
  GFS_HIP(hipMemcpyAsync(h->h_res.p, h->d_res.p, kHead + 2 * (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  const Ctl r = *reinterpret_cast<const Ctl*>(h->h_res.p);
  const float4* kept = reinterpret_cast<const float4*>(h->h_res.p + kHead) + n;
  *n_out = r.n_surf;
  for (int i = 0; i < r.n_surf; i++) {
    out_xyz[3 * i] = kept[i].x;
    out_xyz[3 * i + 1] = kept[i].y;
    out_xyz[3 * i + 2] = kept[i].z;
  }
  return GFS_OK;
}

}  // extern "C"
