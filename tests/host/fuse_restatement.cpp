// TEST INFRASTRUCTURE — NOT PRODUCT CODE.  Sequential CPU restatement of the search of ORBmatcher::Fuse(KeyFrame*, const
// vector<MapPoint*>&, th, bRight = false) (reference src/ORBmatcher.cc:1424-1526) for single-camera pinhole key frames: the SE3f
// action (Thirdparty/Sophus/sophus/so3.hpp:358-367), Pinhole::project (src/CameraModels/Pinhole.cpp:43-49), KeyFrame::IsInImage and
// GetFeaturesInArea (src/KeyFrame.cc:848-850, 802-846) over a plain vector<vector<>> grid filled as Frame::AssignFeaturesToGrid
// fills it (src/Frame.cc:734-761, 1073-1084), MapPoint::PredictScale (src/MapPoint.cc:549-563) calling the HOST's logf, and the
// candidate loop.  The checker of gfs_fuse_search (geoflowslam_amd/csrc/fuse.hip) and of the host rule the adaptor replays with; it
// shares no code with either.  The tests build it with g++ -O2 -std=c++17 -ffp-contract=off.
//
// Float arithmetic, one rounding per operation, sums left to right.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gfs_abi.h"

namespace {

constexpr int TH_LOW = 50;
constexpr int kCols = 64, kRows = 48;
constexpr float kMinDistFactor = 0.8f;  // GetMinDistanceInvariance: 0.8f * mfMinDistance
constexpr float kMaxDistFactor = 1.2f;  // GetMaxDistanceInvariance: 1.2f * mfMaxDistance

struct Stats {
  int64_t stereo = 0, mono = 0, stereo_rejected = 0, mono_rejected = 0, ties = 0, ties_other_cell = 0;
};

typedef std::vector<std::vector<std::vector<int>>> Grid;

Grid assign_features_to_grid(const gfs_fuse_keyframe& k) {
  Grid g(kCols, std::vector<std::vector<int>>(kRows));
  for (int i = 0; i < k.n_kp; i++) {
    const int posX = (int)std::round((k.kps_un[i].x - k.min_x) * k.grid_w_inv);
    const int posY = (int)std::round((k.kps_un[i].y - k.min_y) * k.grid_h_inv);
    if (posX < 0 || posX >= kCols || posY < 0 || posY >= kRows) continue;
    g[posX][posY].push_back(i);
  }
  return g;
}

std::vector<int> features_in_area(const gfs_fuse_keyframe& k, const Grid& g, float x, float y, float r) {
  std::vector<int> vIndices;
  const int nMinCellX = std::max(0, (int)std::floor((x - k.min_x - r) * k.grid_w_inv));
  if (nMinCellX >= kCols) return vIndices;
  const int nMaxCellX = std::min(kCols - 1, (int)std::ceil((x - k.min_x + r) * k.grid_w_inv));
  if (nMaxCellX < 0) return vIndices;
  const int nMinCellY = std::max(0, (int)std::floor((y - k.min_y - r) * k.grid_h_inv));
  if (nMinCellY >= kRows) return vIndices;
  const int nMaxCellY = std::min(kRows - 1, (int)std::ceil((y - k.min_y + r) * k.grid_h_inv));
  if (nMaxCellY < 0) return vIndices;
  for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
    for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
      for (int j : g[ix][iy]) {
        const float distx = k.kps_un[j].x - x;
        const float disty = k.kps_un[j].y - y;
        if (std::fabs(distx) < r && std::fabs(disty) < r) vIndices.push_back(j);
      }
  return vIndices;
}

int predict_scale(float max_distance, float dist, float log_scale_factor, int n_levels) {
  volatile float ratio = max_distance / dist;  // (volatile: the call below is the library's logf, never a folded constant)
  const float c = std::ceil(::logf(ratio) / log_scale_factor);
  int n = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : INT_MIN;
  if (n < 0)
    n = 0;
  else if (n >= n_levels)
    n = n_levels - 1;
  return n;
}

int descriptor_distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

struct Out {
  int exit, best_idx, best_dist, level;
};

Out fuse_point(const gfs_fuse_keyframe& k, const Grid& g, const float* P, const float* Pn, float min_d, float max_d, const uint8_t* dMP,
               Stats& st) {
  Out o{GFS_FUSE_NEG_DEPTH, -1, 256, 0};
  const float* q = k.Tcw_q;
  float uv3[3] = {q[1] * P[2] - q[2] * P[1], q[2] * P[0] - q[0] * P[2], q[0] * P[1] - q[1] * P[0]};
  for (int c = 0; c < 3; c++) uv3[c] += uv3[c];
  const float cr[3] = {q[1] * uv3[2] - q[2] * uv3[1], q[2] * uv3[0] - q[0] * uv3[2], q[0] * uv3[1] - q[1] * uv3[0]};
  float p3Dc[3];
  for (int c = 0; c < 3; c++) p3Dc[c] = ((P[c] + q[3] * uv3[c]) + cr[c]) + k.Tcw_t[c];
  if (p3Dc[2] < 0.0f) return o;
  const float invz = 1 / p3Dc[2];
  const float u = k.fx * p3Dc[0] / p3Dc[2] + k.cx;
  const float v = k.fy * p3Dc[1] / p3Dc[2] + k.cy;
  if (!(u >= k.min_x && u < k.max_x && v >= k.min_y && v < k.max_y)) return o.exit = GFS_FUSE_NOT_IN_IMAGE, o;
  const float ur = u - k.bf * invz;
  const float maxDistance = kMaxDistFactor * max_d, minDistance = kMinDistFactor * min_d;
  const float PO[3] = {P[0] - k.Ow[0], P[1] - k.Ow[1], P[2] - k.Ow[2]};
  const float dist3D = std::sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
  if (dist3D < minDistance) return o.exit = GFS_FUSE_TOO_NEAR, o;
  if (dist3D > maxDistance) return o.exit = GFS_FUSE_TOO_FAR, o;
  const float dot = (PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2];
  if (dot < 0.5 * dist3D) return o.exit = GFS_FUSE_VIEW_ANGLE, o;
  const int nPredictedLevel = predict_scale(max_d, dist3D, k.log_scale_factor, k.n_levels);
  o.level = nPredictedLevel;
  const float radius = k.th * k.scale_factors[nPredictedLevel];
  const std::vector<int> vIndices = features_in_area(k, g, u, v, radius);
  if (vIndices.empty()) return o.exit = GFS_FUSE_EMPTY_WINDOW, o;
  int bestDist = 256, bestIdx = -1;
  for (int idx : vIndices) {
    const gfs_keypoint& kp = k.kps_un[idx];
    const int kpLevel = kp.octave;
    if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
    if (k.u_right[idx] >= 0) {
      const float ex = u - kp.x, ey = v - kp.y, er = ur - k.u_right[idx];
      const float e2 = ex * ex + ey * ey + er * er;
      st.stereo++;
      if (e2 * k.inv_level_sigma2[kpLevel] > 7.8) {
        st.stereo_rejected++;
        continue;
      }
    } else {
      const float ex = u - kp.x, ey = v - kp.y;
      const float e2 = ex * ex + ey * ey;
      st.mono++;
      if (e2 * k.inv_level_sigma2[kpLevel] > 5.99) {
        st.mono_rejected++;
        continue;
      }
    }
    const int dist = descriptor_distance(dMP, k.desc + 32 * (size_t)idx);
    if (dist == bestDist && bestIdx >= 0) {
      st.ties++;
      const gfs_keypoint& b = k.kps_un[bestIdx];
      if ((int)std::round((b.x - k.min_x) * k.grid_w_inv) != (int)std::round((kp.x - k.min_x) * k.grid_w_inv) ||
          (int)std::round((b.y - k.min_y) * k.grid_h_inv) != (int)std::round((kp.y - k.min_y) * k.grid_h_inv))
        st.ties_other_cell++;
    }
    if (dist < bestDist) {
      bestDist = dist;
      bestIdx = idx;
    }
  }
  o.best_idx = bestIdx;
  o.best_dist = bestDist;
  o.exit = bestDist <= TH_LOW ? GFS_FUSE_MATCHED : GFS_FUSE_NO_CANDIDATE;
  return o;
}

}  // namespace

// gfs_fuse_search, point after point.  stats [6] may be NULL: chi2 tests on the stereo / mono branch, rejections of each, Hamming
// ties met (a candidate equal to the best so far), ties whose two key-points sit in different cells.
extern "C" int fr_fuse_search(const gfs_fuse_points* lists, int n_lists, const gfs_fuse_keyframe* kfs, int B, gfs_fuse_result* results,
                              int64_t* stats) {
  Stats st;
  for (int f = 0; f < B; f++) {
    const gfs_fuse_keyframe& k = kfs[f];
    if (k.list < 0 || k.list >= n_lists) return -1;
    const gfs_fuse_points& L = lists[k.list];
    const Grid g = assign_features_to_grid(k);
    int matched = 0;
    for (int i = 0; i < L.n_mp; i++) {
      const Out o = fuse_point(k, g, L.mp_xw + 3 * i, L.mp_normal + 3 * i, L.mp_min_dist[i], L.mp_max_dist[i], L.mp_desc + 32 * (size_t)i, st);
      results[f].exit[i] = (uint8_t)o.exit;
      results[f].best_idx[i] = o.best_idx;
      results[f].best_dist[i] = o.best_dist;
      results[f].level[i] = o.level;
      matched += o.exit == GFS_FUSE_MATCHED;
    }
    results[f].n_matched = matched;
  }
  if (stats) {
    const int64_t s[6] = {st.stereo, st.mono, st.stereo_rejected, st.mono_rejected, st.ties, st.ties_other_cell};
    std::memcpy(stats, s, sizeof(s));
  }
  return 0;
}

// one (point, key frame) search with the descriptor given apart (the sequential loop of the adaptor's test: the live descriptor)
extern "C" void fr_fuse_point(const gfs_fuse_keyframe* k, const float* P, const float* Pn, float min_d, float max_d, const uint8_t* desc,
                              int32_t* out4) {
  Stats st;
  const Out o = fuse_point(*k, assign_features_to_grid(*k), P, Pn, min_d, max_d, desc, st);
  out4[0] = o.exit;
  out4[1] = o.best_idx;
  out4[2] = o.best_dist;
  out4[3] = o.level;
}

// TH_LOW and the distance factors as compiled in
extern "C" void fr_constants(float* out) {
  out[0] = (float)TH_LOW;
  out[1] = kMinDistFactor;
  out[2] = kMaxDistFactor;
}
