// Test harness for gfs_host::SearchLocalPoints / LocalPointsSearcher (geoflowslam_amd/host/gfs_adaptors.hpp): Tracking::SearchLocalPoints
// (reference src/Tracking.cc:4294-4359) over plain-struct Frame / MapPoint classes (bad points, points the frame already holds,
// key-points holding a bad point).  The numeric core is the CPU restatement (tests/host/local_points_restatement.cpp through dlopen)
// or the GPU library.  Built by tests/test_local_points_adaptor.py.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <map>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

namespace {
struct MockMapPoint {
  bool bad = false;
  int visible = 0, obs = 1;
  unsigned long mnId = 0;
  long unsigned int mnLastFrameSeen = 0;
  bool mbTrackInView = true, mbTrackInViewR = true;  // stale values: the function must not rely on them
  float mTrackProjX = -7, mTrackProjY = -7, mTrackProjXR = -7, mTrackViewCos = -7, mTrackDepth = -7;
  int mnTrackScaleLevel = -7;
  float xw[3], normal[3], min_d, max_d;
  uint8_t desc[32];
  bool isBad() const { return bad; }
  void IncreaseVisible(int n = 1) { visible += n; }
  int Observations() const { return obs; }
};
struct MockFrame {
  int Nleft = -1, N = 0, mnScaleLevels = 0;
  long unsigned int mnId = 0;
  bool pinhole = true;
  std::vector<MockMapPoint*> mvpMapPoints;
  std::vector<float> mvuRight, mvScaleFactors;
  std::vector<gfs_keypoint> mvKeysUn;
  std::vector<uint8_t> mDescriptors;
  float mbf, mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv, mfLogScaleFactor;
  float R[9], t[3], Ow[3], k[4];
  std::map<long unsigned int, std::pair<float, float>> mmProjectPoints;
};
struct Access {
  static bool is_pinhole(const MockFrame& F) { return F.pinhole; }
  static void pose(const MockFrame& F, float* R, float* t, float* Ow) {
    std::memcpy(R, F.R, 36);
    std::memcpy(t, F.t, 12);
    std::memcpy(Ow, F.Ow, 12);
  }
  static void intrinsics(const MockFrame& F, float* k) { std::memcpy(k, F.k, 16); }
  static const gfs_keypoint* keys_un(const MockFrame& F) { return F.mvKeysUn.data(); }
  static const uint8_t* descriptors(const MockFrame& F) { return F.mDescriptors.data(); }
  static void set_project_point(MockFrame& F, unsigned long id, float x, float y) { F.mmProjectPoints[id] = {x, y}; }
  static void world_pos(const MockMapPoint* p, float* o) { std::memcpy(o, p->xw, 12); }
  static void normal(const MockMapPoint* p, float* o) { std::memcpy(o, p->normal, 12); }
  static void distances(const MockMapPoint* p, float* mn, float* mx) {
    *mn = p->min_d;
    *mx = p->max_d;
  }
  static void descriptor(const MockMapPoint* p, uint8_t* d) { std::memcpy(d, p->desc, 32); }
};
}  // namespace

// prob: the frame and ALL local map points (n_mp of them, in list order), as gfs_local_points_problem.  bad / obs [n_mp]: isBad(),
// Observations().  held [n_cur]: the local map point a key-point holds on entry (-1 none).  mode: 0 = restatement, 1 = GPU, 2 = a
// two-camera frame, 3 = a non-pinhole camera (both must throw: returns -200).  Outputs per local map point: visible, last_seen, in_view,
// track [n_mp][6] (proj x, y, xr, view cos, depth, level), project [n_mp][3] (1 if mmProjectPoints has the id, x, y); per key-point:
// final [n_cur] (local map point index or -1); counts[3] = listed, return value, status.
extern "C" int local_points_adaptor_test(const char* restatement_lib, int mode, const gfs_local_points_problem* prob, const uint8_t* bad,
                                         const int32_t* obs, const int32_t* held, float th, int32_t* visible, int32_t* last_seen,
                                         uint8_t* in_view, float* track, float* project, int32_t* final_mp, int32_t* counts) {
  try {
    const int n = prob->n_mp, nc = prob->n_cur;
    std::vector<MockMapPoint> mps((size_t)n);
    std::vector<MockMapPoint*> vpLocalMapPoints;
    for (int i = 0; i < n; i++) {
      MockMapPoint& m = mps[i];
      m.bad = bad[i] != 0;
      m.obs = obs[i];
      m.mnId = 1000 + 3 * (unsigned long)i;
      m.mnLastFrameSeen = 41;  // the previous frame
      std::memcpy(m.xw, prob->mp_xw + 3 * i, 12);
      std::memcpy(m.normal, prob->mp_normal + 3 * i, 12);
      m.min_d = prob->mp_min_dist[i];
      m.max_d = prob->mp_max_dist[i];
      std::memcpy(m.desc, prob->mp_desc + 32 * (size_t)i, 32);
      vpLocalMapPoints.push_back(&m);
    }
    MockFrame F;
    F.mnId = 42;
    F.N = nc;
    F.Nleft = mode == 2 ? nc / 2 : -1;
    F.pinhole = mode != 3;
    F.mnScaleLevels = prob->n_levels;
    F.mvScaleFactors.assign(prob->scale_factors, prob->scale_factors + prob->n_levels);
    F.mvuRight.assign(prob->cur_u_right, prob->cur_u_right + nc);
    F.mvKeysUn.assign(prob->cur_kps_un, prob->cur_kps_un + nc);
    F.mDescriptors.assign(prob->cur_desc, prob->cur_desc + 32 * (size_t)nc);
    for (int i = 0; i < nc; i++) F.mvpMapPoints.push_back(held[i] >= 0 ? &mps[held[i]] : nullptr);
    F.mbf = prob->bf;
    F.mnMinX = prob->min_x;
    F.mnMaxX = prob->max_x;
    F.mnMinY = prob->min_y;
    F.mnMaxY = prob->max_y;
    F.mfGridElementWidthInv = prob->grid_w_inv;
    F.mfGridElementHeightInv = prob->grid_h_inv;
    F.mfLogScaleFactor = prob->log_scale_factor;
    std::memcpy(F.R, prob->Rcw, 36);
    std::memcpy(F.t, prob->tcw, 12);
    std::memcpy(F.Ow, prob->Ow, 12);
    const float k[4] = {prob->fx, prob->fy, prob->cx, prob->cy};
    std::memcpy(F.k, k, 16);
    int ret = 0;
    counts[0] = -1;
    try {
      if (mode == 1) {
        gfs_host::LocalPointsSearcher searcher(std::max(n, 64), std::max(nc, 64));
        ret = gfs_host::SearchLocalPoints<Access>(F, vpLocalMapPoints, th, prob->far_points != 0, prob->th_far_points,
                                                  [&](const gfs_local_points_problem& p, gfs_local_points_result& r) {
                                                    counts[0] = p.n_mp;
                                                    return searcher.solve(p, r);
                                                  });
      } else {
        void* so = dlopen(restatement_lib, RTLD_NOW | RTLD_LOCAL);
        if (!so) return -101;
        typedef int (*fn_t)(const gfs_local_points_problem*, gfs_local_points_result*, int32_t*, int32_t*, int32_t*);
        fn_t fn = (fn_t)dlsym(so, "lpr_search_local_points");
        if (!fn) return -102;
        ret = gfs_host::SearchLocalPoints<Access>(F, vpLocalMapPoints, th, prob->far_points != 0, prob->th_far_points,
                                                  [&](const gfs_local_points_problem& p, gfs_local_points_result& r) {
                                                    counts[0] = p.n_mp;
                                                    if (p.view_cos_limit != 0.5f || p.nn_ratio != 0.8f) return -104;
                                                    return fn(&p, &r, nullptr, nullptr, nullptr);
                                                  });
      }
    } catch (const std::invalid_argument&) {
      return -200;
    }
    counts[1] = ret;
    for (int i = 0; i < n; i++) {
      const MockMapPoint& m = mps[i];
      visible[i] = m.visible;
      last_seen[i] = (int32_t)m.mnLastFrameSeen;
      in_view[i] = (m.mbTrackInView ? 1 : 0) | (m.mbTrackInViewR ? 2 : 0);
      const float tr[6] = {m.mTrackProjX, m.mTrackProjY, m.mTrackProjXR, m.mTrackViewCos, m.mTrackDepth, (float)m.mnTrackScaleLevel};
      std::memcpy(track + 6 * (size_t)i, tr, 24);
      auto it = F.mmProjectPoints.find(m.mnId);
      project[3 * i] = it != F.mmProjectPoints.end();
      project[3 * i + 1] = it != F.mmProjectPoints.end() ? it->second.first : 0.0f;
      project[3 * i + 2] = it != F.mmProjectPoints.end() ? it->second.second : 0.0f;
    }
    for (int i = 0; i < nc; i++) final_mp[i] = F.mvpMapPoints[i] ? (int32_t)(F.mvpMapPoints[i] - mps.data()) : -1;
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "local_points_adaptor_test: %s\n", ex.what());
    return -1;
  }
}
