// The per-map-point rule of MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:376-448) and
// MapPoint::UpdateNormalAndDepth (:468-532) for single-camera key frames, stated once for the device and the host (DESIGN.md
// section 15).  Integer results equal the reference's; float, every operation rounded once, sums left to right in list order; the
// translation units that include this are built with -ffp-contract=off.  k_map_points (map_points.hip) runs it a wave per point;
// update_point below runs it on the host for one point (gfs_host::map_points_update_host, gfs_adaptors.hpp).
#pragma once
#include <cmath>
#include <cstdint>

#if !defined(GFS_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFS_HD __host__ __device__ inline
#else
#define GFS_HD inline
#endif
#endif

namespace gfs_mp {

constexpr int kObsInNormal = 1, kObsInDesc = 2;  // GFS_MAP_POINT_OBS_* of include/gfs_abi.h
constexpr int kNormalSet = 1, kDescSet = 2;      // GFS_MAP_POINT_*_SET

// vDists[0.5 * (N - 1)] (:436): the index the double product converts to; even N takes the lower middle
GFS_HD int median_index(int n) { return (int)(0.5 * (n - 1)); }

// `median < BestMedian` (:438): a later row replaces the best only with a strictly smaller median
GFS_HD bool better_median(int median, int best) { return median < best; }

// ORBmatcher::DescriptorDistance on eight 32-bit words
GFS_HD int hamming256(const uint32_t* a, const uint32_t* b) {
  int d = 0;
  for (int k = 0; k < 8; k++) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// normali = Pos - Owi; normali / normali.norm() (:496-497), the norm grouped as fuse_rule.hpp's dist3D: (x x + y y) + z z
GFS_HD float norm3(const float* v) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
GFS_HD void normal_term(const float* pos, const float* Ow, float* t) {
  const float d[3] = {pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]};
  const float n = norm3(d);
  for (int k = 0; k < 3; k++) t[k] = d[k] / n;
}

// :508-531 after the sum: mNormalVector = normal / n, mfMaxDistance = dist * levelScaleFactor, mfMinDistance = mfMaxDistance / max scale
GFS_HD void finish_normal(const float* sum, int n, const float* pos, const float* ref_Ow, float level_scale, float max_scale, float* normal,
                          float* min_dist, float* max_dist) {
  const float fn = (float)n;
  for (int k = 0; k < 3; k++) normal[k] = sum[k] / fn;
  const float pc[3] = {pos[0] - ref_Ow[0], pos[1] - ref_Ow[1], pos[2] - ref_Ow[2]};
  const float dist = norm3(pc);
  *max_dist = dist * level_scale;
  *min_dist = *max_dist / max_scale;
}

#if !defined(__HIP_DEVICE_COMPILE__)
struct PointResult {
  int best_obs, best_median, status;
  float normal[3], min_dist, max_dist;
};

// One point on the host.  Ow [n][3], desc [n][32] (not read when !with_desc), flags [n]: the point's observations in list order.
// The k-th smallest of a row is found by counting (a 257-bin histogram), which is what sorting the row and indexing it gives.
inline PointResult update_point(int n, const float* Ow, const uint8_t* desc, const uint8_t* flags, const float* pos, const float* ref_Ow,
                                float level_scale, float max_scale, bool with_desc) {
  PointResult R{-1, -1, 0, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f};
  if (n <= 0) return R;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    if (!(flags[i] & kObsInNormal)) continue;
    float t[3];
    normal_term(pos, Ow + 3 * (size_t)i, t);
    for (int k = 0; k < 3; k++) sum[k] = sum[k] + t[k];
    cnt++;
  }
  finish_normal(sum, cnt, pos, ref_Ow, level_scale, max_scale, R.normal, &R.min_dist, &R.max_dist);
  R.status |= kNormalSet;
  if (!with_desc) return R;
  int nd = 0;
  for (int i = 0; i < n; i++) nd += (flags[i] & kObsInDesc) ? 1 : 0;
  if (nd == 0) return R;
  const int k = median_index(nd);
  int best = 0x7fffffff;  // INT_MAX (:431)
  for (int i = 0; i < n; i++) {
    if (!(flags[i] & kObsInDesc)) continue;
    uint32_t a[8], b[8];
    __builtin_memcpy(a, desc + 32 * (size_t)i, 32);
    int hist[257] = {0};
    for (int j = 0; j < n; j++) {
      if (!(flags[j] & kObsInDesc)) continue;
      __builtin_memcpy(b, desc + 32 * (size_t)j, 32);
      hist[hamming256(a, b)]++;  // (j == i gives the row's own 0)
    }
    int v = 0;
    for (int c = hist[0]; c <= k; c += hist[v]) v++;
    if (better_median(v, best)) {
      best = v;
      R.best_obs = i;
    }
  }
  R.best_median = best;
  R.status |= kDescSet;
  return R;
}
#endif

}  // namespace gfs_mp
