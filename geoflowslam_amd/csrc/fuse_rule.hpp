// The per-(map point, key frame) rule of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th, bRight = false)
// (reference src/ORBmatcher.cc:1424-1526) for single-camera pinhole key frames, stated once for the device and the host
// (DESIGN.md section 13): float, every operation rounded once, sums left to right; the translation units that include this are
// built with -ffp-contract=off.  k_fuse (fuse.hip) runs it with the key frame's grid in LDS; search_point below runs it on the
// host for ONE pair, for the adaptor's replay when a point's descriptor changed after the upload (gfs_adaptors.hpp).
#pragma once
#include <cstdint>

#include "glibc_math.hpp"

namespace gfs_fuse {

constexpr int kGridCols = 64, kGridRows = 48;
constexpr int kThLow = 50;                 // ORBmatcher::TH_LOW
constexpr float kMinDistFactor = 0.8f;     // MapPoint::GetMinDistanceInvariance
constexpr float kMaxDistFactor = 1.2f;     // MapPoint::GetMaxDistanceInvariance
constexpr double kViewCosHalf = 0.5;       // PO.dot(Pn) < 0.5 * dist3D (:1459)
constexpr double kChi2Stereo = 7.8;        // :1505
constexpr double kChi2Mono = 5.99;         // :1513

// where the loop body of :1424-1544 ends for a point (GFS_FUSE_* of include/gfs_abi.h)
enum Exit { kNegDepth = 0, kNotInImage = 1, kTooNear = 2, kTooFar = 3, kViewAngle = 4, kEmptyWindow = 5, kNoCandidate = 6, kMatched = 7 };

struct KeyFrame {  // what the rule reads of a key frame
  float q[4], t[3], Ow[3];  // GetPose() as unit quaternion (x, y, z, w) + translation, GetCameraCenter()
  float fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y, grid_w_inv, grid_h_inv, log_scale_factor, th;
  int n_levels, n_kp;
  float scale[16], inv_sigma2[16];
};

struct Proj {
  int exit;  // kNegDepth .. kViewAngle, or kEmptyWindow when GetFeaturesInArea returns before its loops, else -1: search the window
  int level, x0, x1, y0, y1;
  float u, v, ur, radius;
};

// SO3f * p (Thirdparty/Sophus/sophus/so3.hpp:358-367): uv = q.vec x p; uv += uv; p + w * uv + q.vec x uv
GFS_HD void so3_act(const float* q, const float* p, float* o) {
  float uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int k = 0; k < 3; k++) uv[k] += uv[k];
  const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int k = 0; k < 3; k++) o[k] = (p[k] + q[3] * uv[k]) + c[k];
}

// MapPoint::PredictScale(currentDist, KeyFrame*) (src/MapPoint.cc:549-563); a quotient no int holds gives level 0 (chosen rule 2 of
// what x86-64's conversion, INT_MIN, and the clamp produce)
GFS_HD int predict_scale(float max_dist, float dist, float log_scale_factor, int n_levels) {
  const float c = ceilf(gfs_glibc::logf(max_dist / dist) / log_scale_factor);
  int lv = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : 0;
  return lv < 0 ? 0 : (lv >= n_levels ? n_levels - 1 : lv);
}

// every field defined, for a point that leaves before its window is known
GFS_HD Proj no_projection() {
  Proj R;
  R.exit = R.level = 0;
  R.x0 = R.x1 = R.y0 = R.y1 = 0;
  R.u = R.v = R.ur = R.radius = 0.0f;
  return R;
}

// Tcw * p3Dw
GFS_HD void camera_point(const KeyFrame& K, const float* P, float* Pc) {
  so3_act(K.q, P, Pc);
  for (int k = 0; k < 3; k++) Pc[k] += K.t[k];
}

// KeyFrame::IsInImage (src/KeyFrame.cc:848-850): half open; NaN and +-inf fail it by themselves
GFS_HD bool in_image(const KeyFrame& K, float u, float v) {
  if (!(u >= K.min_x && u < K.max_x && v >= K.min_y && v < K.max_y)) return false;
  return true;
}

// From the distance gates to the cell range of KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:802-827) for a point that projects to
// (R.u, R.v) inside the image (:1444-1470; the Sim3 searches of sim3_search_rule.hpp run the same steps): sets R.exit, R.level,
// R.radius and the cell range.
GFS_HD void gates_and_window(const KeyFrame& K, const float* P, const float* Pn, float min_dist, float max_dist, Proj& R) {
  const float u = R.u, v = R.v;
  const float PO[3] = {P[0] - K.Ow[0], P[1] - K.Ow[1], P[2] - K.Ow[2]};
  const float dist = sqrtf((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
  if (dist < kMinDistFactor * min_dist) return (void)(R.exit = kTooNear);
  if (dist > kMaxDistFactor * max_dist) return (void)(R.exit = kTooFar);
  const float dot = (PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2];
  if ((double)dot < kViewCosHalf * (double)dist) return (void)(R.exit = kViewAngle);
  R.level = predict_scale(max_dist, dist, K.log_scale_factor, K.n_levels);
  R.radius = K.th * K.scale[R.level];
  R.exit = kEmptyWindow;
  R.x0 = (int)floorf((u - K.min_x - R.radius) * K.grid_w_inv);
  if (R.x0 < 0) R.x0 = 0;
  if (R.x0 >= kGridCols) return;
  R.x1 = (int)ceilf((u - K.min_x + R.radius) * K.grid_w_inv);
  if (R.x1 > kGridCols - 1) R.x1 = kGridCols - 1;
  if (R.x1 < 0) return;
  R.y0 = (int)floorf((v - K.min_y - R.radius) * K.grid_h_inv);
  if (R.y0 < 0) R.y0 = 0;
  if (R.y0 >= kGridRows) return;
  R.y1 = (int)ceilf((v - K.min_y + R.radius) * K.grid_h_inv);
  if (R.y1 > kGridRows - 1) R.y1 = kGridRows - 1;
  if (R.y1 < 0) return;
  R.exit = -1;
}

// :1424-1470 up to the cell range
GFS_HD Proj project(const KeyFrame& K, const float* P, const float* Pn, float min_dist, float max_dist) {
  Proj R = no_projection();
  float Pc[3];
  camera_point(K, P, Pc);
  if (Pc[2] < 0.0f) return R.exit = kNegDepth, R;
  const float invz = 1.0f / Pc[2];
  const float u = K.fx * Pc[0] / Pc[2] + K.cx, v = K.fy * Pc[1] / Pc[2] + K.cy;
  if (!in_image(K, u, v)) return R.exit = kNotInImage, R;
  R.u = u;
  R.v = v;
  R.ur = u - K.bf * invz;
  gates_and_window(K, P, Pn, min_dist, max_dist, R);
  return R;
}

// the membership test of GetFeaturesInArea (src/KeyFrame.cc:837-840)
GFS_HD bool in_window(const Proj& R, float kx, float ky) {
  const float distx = kx - R.u, disty = ky - R.v;
  return fabsf(distx) < R.radius && fabsf(disty) < R.radius;
}

// the filters of the candidate loop before the descriptor distance (:1491-1514)
GFS_HD bool candidate_ok(const KeyFrame& K, const Proj& R, float kx, float ky, float kur, int oct) {
  if (oct < R.level - 1 || oct > R.level) return false;
  const float ex = R.u - kx, ey = R.v - ky;
  if (kur >= 0) {
    const float er = R.ur - kur;
    const float e2 = (ex * ex + ey * ey) + er * er;
    if ((double)(e2 * K.inv_sigma2[oct]) > kChi2Stereo) return false;
  } else {
    const float e2 = ex * ex + ey * ey;
    if ((double)(e2 * K.inv_sigma2[oct]) > kChi2Mono) return false;
  }
  return true;
}

// the exit of a point whose window was searched
GFS_HD int search_exit(bool any_in_window, int best_dist) { return !any_in_window ? kEmptyWindow : (best_dist <= kThLow ? kMatched : kNoCandidate); }

#if !defined(__HIP_DEVICE_COMPILE__)
struct PointResult {
  int exit, best_idx, best_dist, level;
};

// One (map point, key frame) search on the host, without a grid: a key-point is visited iff its cell (Frame::PosInGrid: roundf) lies
// in the window's cell range and it passes the membership test; the reference visits cells ix outer, iy inner, a cell's key-points
// in index order, and keeps the best under strict `<`, so the winner is the minimum of (distance, ix, iy, index).
// kx / ky / kur / koct: the key frame's mvKeysUn positions, mvuRight and octaves; kdesc [n_kp][32]; desc: the point's descriptor.
inline PointResult search_point(const KeyFrame& K, const float* P, const float* Pn, float min_dist, float max_dist, const uint8_t* desc,
                                const float* kx, const float* ky, const float* kur, const int32_t* koct, const uint8_t* kdesc) {
  const Proj R = project(K, P, Pn, min_dist, max_dist);
  PointResult o{R.exit, -1, 256, R.level};
  if (R.exit >= 0) return o;
  bool any = false;
  int bx = 0, by = 0;
  for (int j = 0; j < K.n_kp; j++) {
    const int px = (int)roundf((kx[j] - K.min_x) * K.grid_w_inv), py = (int)roundf((ky[j] - K.min_y) * K.grid_h_inv);
    if (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) continue;  // not in the grid at all
    if (px < R.x0 || px > R.x1 || py < R.y0 || py > R.y1) continue;
    if (!in_window(R, kx[j], ky[j])) continue;
    any = true;
    if (!candidate_ok(K, R, kx[j], ky[j], kur[j], koct[j])) continue;
    int d = 0;
    for (int b = 0; b < 32; b++) d += __builtin_popcount((unsigned)(desc[b] ^ kdesc[32 * (size_t)j + b]));
    const bool earlier = px < bx || (px == bx && (py < by || (py == by && j < o.best_idx)));
    if (d < o.best_dist || (d == o.best_dist && o.best_idx >= 0 && earlier)) {
      o.best_dist = d;
      o.best_idx = j;
      bx = px;
      by = py;
    }
  }
  o.exit = search_exit(any, o.best_dist);
  return o;
}
#endif

}  // namespace gfs_fuse
