// The per-(map point, key frame) rule of the three Sim3 searches of loop closing (reference src/ORBmatcher.cc), stated once for the
// device and the host: float, every operation rounded once, sums left to right; the translation units that
// include this are built with -ffp-contract=off.
//   kFuse    Fuse(KeyFrame*, Sim3f& Scw, points, th, vpReplacePoint)                                   :1550-1654
//   kSbp     SearchByProjection(KeyFrame*, Sim3f&, points, vpMatched, th, ratioHamming)                :432-529
//   kSbpKfs  SearchByProjection(KeyFrame*, Sim3f&, points, vpPointsKFs, vpMatched, vpMatchedKF, ...)   :531-636
// The SE3 action, the distance and viewing-angle gates, PredictScale and the window are those of fuse_rule.hpp; there is no chi2
// gate and no mvuRight here.  k_sim3_search (sim3_search.hip) runs the rule with the key frame's grid in LDS; search_point below runs
// it on the host for ONE pair against a live taken set: for the replay of gfs_sim3_search when a point's listed candidates are all
// taken, and for the adaptor's replay when a point's descriptor changed after the upload (gfs_adaptors.hpp).
#pragma once
#include "fuse_rule.hpp"

namespace gfs_sim3 {

using gfs_fuse::KeyFrame;  // bf and inv_sigma2 are not read
using gfs_fuse::Proj;      // ur is not set

enum Mode { kFuse = 0, kSbp = 1, kSbpKfs = 2 };  // GFS_SIM3_* of include/gfs_abi.h
constexpr int kSkipped = 8;                      // GFS_FUSE_SKIPPED: isBad() || spAlreadyFound.count(pMP) (:457, :559, :1576)
constexpr int kListed = 4;                       // candidates the kernel lists per point in the projection modes
constexpr int kIntMax = 2147483647;              // bestDist = INT_MAX (:1621)

// what bestDist starts at: INT_MAX in Fuse (:1621), 256 in the projection searches (:500, :606)
GFS_HD int first_best_dist(int mode) { return mode == kFuse ? kIntMax : 256; }

// the acceptance test: bestDist <= TH_LOW (:1641); bestDist <= TH_LOW * ratioHamming, an int against a float product (:522, :628)
GFS_HD bool accepted(int mode, int best_dist, float ratio_hamming) {
  return mode == kFuse ? best_dist <= gfs_fuse::kThLow : (float)best_dist <= (float)gfs_fuse::kThLow * ratio_hamming;
}

// the ratios gfs_sim3_search takes: 256 (nothing survived, bestIdx = -1) must fail the acceptance test
inline bool ratio_ok(float ratio_hamming) { return ratio_hamming >= 0.0f && (float)gfs_fuse::kThLow * ratio_hamming < 256.0f; }

// steps 1 - 9 and the cell range.  Fuse and the first projection search call Pinhole::project (fx * Pc0 / Pc2 + cx); the second
// projection search multiplies by invz first (:571-576), one more rounding
GFS_HD Proj project(const KeyFrame& K, int mode, const float* P, const float* Pn, float min_dist, float max_dist) {
  Proj R = gfs_fuse::no_projection();
  float Pc[3];
  gfs_fuse::camera_point(K, P, Pc);
  if (Pc[2] < 0.0f) return R.exit = gfs_fuse::kNegDepth, R;
  float u, v;
  if (mode == kSbpKfs) {
    const float invz = 1.0f / Pc[2];
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    u = K.fx * x + K.cx;
    v = K.fy * y + K.cy;
  } else {
    u = K.fx * Pc[0] / Pc[2] + K.cx;
    v = K.fy * Pc[1] / Pc[2] + K.cy;
  }
  if (!gfs_fuse::in_image(K, u, v)) return R.exit = gfs_fuse::kNotInImage, R;
  R.u = u;
  R.v = v;
  gfs_fuse::gates_and_window(K, P, Pn, min_dist, max_dist, R);
  return R;
}

// the level filter of the candidate loop (:510, :616, :1628)
GFS_HD bool level_ok(const Proj& R, int oct) { return !(oct < R.level - 1 || oct > R.level); }

// the exit of a point whose window was searched
GFS_HD int search_exit(int mode, bool any_in_window, int best_dist, float ratio_hamming) {
  return !any_in_window ? gfs_fuse::kEmptyWindow : (accepted(mode, best_dist, ratio_hamming) ? gfs_fuse::kMatched : gfs_fuse::kNoCandidate);
}

struct PointResult {
  int exit, best_idx, best_dist, level;
};

// One (map point, key frame) search on the host, without a grid (as gfs_fuse::search_point): the reference's bestIdx / bestDist for
// this point when the key-points with taken[j] != 0 are skipped (taken may be NULL; it is not read in kFuse mode).  The winner is the
// minimum of (distance, ix, iy, index) over the candidates, which is what the visiting order and the strict `<` give.
// kp(j, &x, &y, &octave): the key frame's mvKeysUn; kdesc [n_kp][32]; desc: the point's descriptor.
template <class KpAt>
inline PointResult search_point(const KeyFrame& K, int mode, float ratio_hamming, const float* P, const float* Pn, float min_dist, float max_dist,
                         const uint8_t* desc, KpAt&& kp, const uint8_t* kdesc, const uint8_t* taken) {
  const Proj R = project(K, mode, P, Pn, min_dist, max_dist);
  PointResult o{R.exit, -1, first_best_dist(mode), R.level};
  if (R.exit >= 0) return o;
  bool any = false;
  int bx = 0, by = 0;
  for (int j = 0; j < K.n_kp; j++) {
    float x, y;
    int oct;
    kp(j, &x, &y, &oct);
    const int px = (int)roundf((x - K.min_x) * K.grid_w_inv), py = (int)roundf((y - K.min_y) * K.grid_h_inv);
    if (px < 0 || px >= gfs_fuse::kGridCols || py < 0 || py >= gfs_fuse::kGridRows) continue;  // not in the grid at all
    if (px < R.x0 || px > R.x1 || py < R.y0 || py > R.y1) continue;
    if (!gfs_fuse::in_window(R, x, y)) continue;
    any = true;
    if (mode != kFuse && taken && taken[j]) continue;
    if (!level_ok(R, oct)) continue;
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
  o.exit = search_exit(mode, any, o.best_dist, ratio_hamming);
  return o;
}

}  // namespace gfs_sim3
