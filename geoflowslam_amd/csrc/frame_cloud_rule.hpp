// The rule of the frame cloud: LaserProcessingClass::featureExtraction (reference src/LidarProcess.cc:20-204)
// and the tail of the Frame constructor (src/Frame.cc:378-393), as constants and as the expressions whose evaluation order decides
// bits.  Shared by the kernels of frame_cloud.hip, by the host scan split the library falls back to when a device atan2 comparison is
// too close to its threshold, and by the adaptor.  Host and device evaluate the same source: build with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFS_FC_HD __host__ __device__ __forceinline__
#else
#define GFS_FC_HD inline
#endif

namespace gfs_fc {

constexpr double kScanBreakDeg = 0.05;  // fabs(angle - last_angle) > 0.05 starts a new run            LidarProcess.cc:40
constexpr int kMinScanCount = 20;       // a run becomes a scan iff count > 20                         :41
constexpr int kPad = 5;                 // 5 copies of (x, y, max_distance) in front / behind          :50, :67
constexpr double kPadMarginDeg = 5.0;   // start_angle > -H / 2 + 5.0, end_angle < H / 2 - 5.0         :49, :66
constexpr double kEdgeMinValue = 0.1;   // the walk stops at the first unpicked value <= 0.1           :176
constexpr int kMaxEdgePicks = 10;       // largestPickedNum <= 10 are edge points; the 11th ends it    :183
constexpr int kPickHalo = 5;            // ind - 5 .. ind + 5 join picked_points                       :191
constexpr int kEdgeMinNeighbors = 3;    // edge_noise_filter.setMinNeighborsInRadius(3)                :15
constexpr int kSurfMinNeighbors = 14;   // surf_noise_filter.setMinNeighborsInRadius(14)               :17
constexpr double kEdgeLeafDivisor = 4.0;  // edge leaf = map_resolution / 4.0                          :9
constexpr double kSurfLeafDivisor = 2.0;  // surf leaf = map_resolution / 2.0                          :11
constexpr double kDefaultHorizontalAngle = 70.0, kDefaultMaxDistance = 9.0, kDefaultLocalMapResolution = 0.05;  // Lidar.cc:100-128
constexpr int kMaxCandidates = 1024;    // the std::sort replica's limit (wave_std_sort.hpp)
constexpr double kDefaultAngleGuardDeg = 1e-9;
constexpr float kCoordBound = 1e6f;

enum { kPadStart = 1, kPadEnd = 2 };

struct Scan {  // one row of the scan table
  int32_t begin, count, pad, cand_begin;  // points [begin, begin + count); kPad* flags; candidates of the scans in front
};

GFS_FC_HD double angle_deg(float a, float b) { return atan2((double)a, (double)b) * 180 / M_PI; }

GFS_FC_HD int candidates_of(int count, int pad) {
  return count + ((pad & kPadStart) ? kPad : 0) + ((pad & kPadEnd) ? kPad : 0) - 2 * kPad;
}

// cloudCurvature of padded-scan position j: float sums left to right, widened; only the Z term is divided.
// X / Y / Z: the padded scan's coordinates
GFS_FC_HD double curvature(const float* X, const float* Y, const float* Z, int j) {
  const float pd = X[j] * X[j] + Y[j] * Y[j] + Z[j] * Z[j];
  const float dx = X[j - 5] + X[j - 4] + X[j - 3] + X[j - 2] + X[j - 1] - 10 * X[j] + X[j + 1] + X[j + 2] + X[j + 3] + X[j + 4] + X[j + 5];
  const float dy = Y[j - 5] + Y[j - 4] + Y[j - 3] + Y[j - 2] + Y[j - 1] - 10 * Y[j] + Y[j + 1] + Y[j + 2] + Y[j + 3] + Y[j + 4] + Y[j + 5];
  const float dz = Z[j - 5] + Z[j - 4] + Z[j - 3] + Z[j - 2] + Z[j - 1] - 10 * Z[j] + Z[j + 1] + Z[j + 2] + Z[j + 3] + Z[j + 4] + Z[j + 5];
  const double point_distance = pd, diffX = dx, diffY = dy, diffZ = dz;
  return diffX * diffX + diffY * diffY + diffZ * diffZ / point_distance;
}

// FLANN L2_Simple on three floats, as the radius filter's rule takes it
GFS_FC_HD float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// The scan split with the host's atan2 (the reference's own): xyzw [n][4] -> scans (at most n / 21 rows); returns the row count.
// *too_long is set when a scan has more than kMaxCandidates candidates.
inline int split_host(const float* xyzw, int n, double horizontal_angle, Scan* scans, bool* too_long) {
  int n_scans = 0, run = 0, cand = 0;
  *too_long = false;
  if (n <= 0) return 0;
  double last = angle_deg(xyzw[1], xyzw[2]);
  for (int i = 0; i < n; i++) {
    const double a = angle_deg(xyzw[4 * i + 1], xyzw[4 * i + 2]);
    if (fabs(a - last) > kScanBreakDeg) {
      if (i - run > kMinScanCount) {
        int pad = 0;
        if (angle_deg(xyzw[4 * run], xyzw[4 * run + 2]) > -horizontal_angle / 2.0 + kPadMarginDeg) pad |= kPadStart;
        if (angle_deg(xyzw[4 * (i - 1)], xyzw[4 * (i - 1) + 2]) < horizontal_angle / 2.0 - kPadMarginDeg) pad |= kPadEnd;
        scans[n_scans++] = Scan{run, i - run, pad, cand};
        const int c = candidates_of(i - run, pad);
        if (c > kMaxCandidates) *too_long = true;
        cand += c;
      }
      run = i;
      last = a;
    }
  }
  return n_scans;
}

}  // namespace gfs_fc
