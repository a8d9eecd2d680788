// Test harness for gfs_host::Fuse / SearchInNeighborsFuse / FuseSearcher (geoflowslam_amd/host/gfs_adaptors.hpp):
// LocalMapping::SearchInNeighbors from `ORBmatcher matcher;` on (reference src/LocalMapping.cc:1179-1234) over plain-struct KeyFrame /
// MapPoint classes whose Replace / AddObservation / AddMapPoint follow src/MapPoint.cc:129-160, 303-351 and src/KeyFrame.cc.  The numeric
// core is the CPU restatement (tests/host/fuse_restatement.cpp through dlopen) or the GPU library; the end state is compared with a
// plain sequential loop that runs the restatement point by point against the live state.  Built by tests/test_fuse_adaptor.py.
// Also exports the product's host rule (gfs_fuse::search_point) for a direct comparison with the restatement.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <map>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

namespace {
struct MockKeyFrame;
struct MockMapPoint {
  int id = 0;
  bool bad = false;
  int extra_obs = 0;  // observations in key frames outside the scene
  std::map<MockKeyFrame*, int> obs;
  MockMapPoint* replaced = nullptr;
  unsigned long mnFuseCandidateForKF = 0;
  float xw[3], normal[3], min_d, max_d;
  uint8_t desc[32], alt[32];
  bool has_alt = false;
  int n_cdd = 0, n_unad = 0;
  bool isBad() const { return bad; }
  bool IsInKeyFrame(MockKeyFrame* kf) const { return obs.count(kf) != 0; }
  int Observations() const { return (int)obs.size() + extra_obs; }
  void AddObservation(MockKeyFrame* kf, int idx) { obs[kf] = idx; }
  void ComputeDistinctiveDescriptors() {  // scripted: the descriptor the point has once its observations changed
    n_cdd++;
    if (has_alt) std::memcpy(desc, alt, 32);
  }
  void UpdateNormalAndDepth() { n_unad++; }
  void Replace(MockMapPoint* pMP);
};
struct MockKeyFrame {
  int NLeft = -1, N = 0, mnScaleLevels = 0;
  unsigned long mnId = 0;
  bool pinhole = true;
  float fx, fy, cx, cy, mbf, mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv, mfLogScaleFactor;
  std::vector<float> mvuRight, mvScaleFactors, mvInvLevelSigma2;
  std::vector<gfs_keypoint> mvKeysUn;
  std::vector<uint8_t> mDescriptors;
  std::vector<MockMapPoint*> mvpMapPoints;
  float q[4], t[3], Ow[3];
  int n_update_connections = 0;
  MockMapPoint* GetMapPoint(int idx) { return mvpMapPoints[idx]; }
  void AddMapPoint(MockMapPoint* p, int idx) { mvpMapPoints[idx] = p; }
  void ReplaceMapPointMatch(int idx, MockMapPoint* p) { mvpMapPoints[idx] = p; }
  void EraseMapPointMatch(int idx) { mvpMapPoints[idx] = nullptr; }
  std::vector<MockMapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  void UpdateConnections() { n_update_connections++; }
};
void MockMapPoint::Replace(MockMapPoint* pMP) {  // src/MapPoint.cc:303-351
  if (pMP->id == id) return;
  std::map<MockKeyFrame*, int> o = obs;
  obs.clear();
  bad = true;
  replaced = pMP;
  for (auto& kv : o) {
    if (!pMP->IsInKeyFrame(kv.first)) {
      kv.first->ReplaceMapPointMatch(kv.second, pMP);
      pMP->AddObservation(kv.first, kv.second);
    } else {
      kv.first->EraseMapPointMatch(kv.second);
    }
  }
  pMP->ComputeDistinctiveDescriptors();
}
struct Access {
  static bool is_pinhole(const MockKeyFrame& F) { return F.pinhole; }
  static void pose(const MockKeyFrame& F, float* q, float* t, float* Ow) {
    std::memcpy(q, F.q, 16);
    std::memcpy(t, F.t, 12);
    std::memcpy(Ow, F.Ow, 12);
  }
  static const gfs_keypoint* keys_un(const MockKeyFrame& F) { return F.mvKeysUn.data(); }
  static const uint8_t* descriptors(const MockKeyFrame& F) { return F.mDescriptors.data(); }
  static void world_pos(const MockMapPoint* p, float* o) { std::memcpy(o, p->xw, 12); }
  static void normal(const MockMapPoint* p, float* o) { std::memcpy(o, p->normal, 12); }
  static void distances(const MockMapPoint* p, float* mn, float* mx) {
    *mn = p->min_d;
    *mx = p->max_d;
  }
  static void descriptor(const MockMapPoint* p, uint8_t* d) { std::memcpy(d, p->desc, 32); }
};

typedef int (*search_fn)(const gfs_fuse_points*, int, const gfs_fuse_keyframe*, int, gfs_fuse_result*, int64_t*);
typedef void (*point_fn)(const gfs_fuse_keyframe*, const float*, const float*, float, float, const uint8_t*, int32_t*);

// ORBmatcher::Fuse as the reference writes it, the search of each point done by the restatement when its turn comes.
// stale: the descriptors the points had when the enclosing batch of Fuse calls began (what a replay without the recompute would use).
int fuse_sequential(point_fn fn, MockKeyFrame* pKF, const gfs_fuse_keyframe& k, const std::vector<MockMapPoint*>& vpMapPoints,
                    const std::map<MockMapPoint*, std::vector<uint8_t>>* stale) {
  int nFused = 0;
  for (MockMapPoint* pMP : vpMapPoints) {
    if (!pMP) continue;
    if (pMP->isBad()) continue;
    if (pMP->IsInKeyFrame(pKF)) continue;
    int32_t o[4];
    fn(&k, pMP->xw, pMP->normal, pMP->min_d, pMP->max_d, stale ? stale->at(pMP).data() : pMP->desc, o);
    if (o[0] != GFS_FUSE_MATCHED) continue;
    MockMapPoint* pMPinKF = pKF->GetMapPoint(o[1]);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) {
        if (pMPinKF->Observations() > pMP->Observations())
          pMP->Replace(pMPinKF);
        else
          pMPinKF->Replace(pMP);
      }
    } else {
      pMP->AddObservation(pKF, o[1]);
      pKF->AddMapPoint(pMP, o[1]);
    }
    nFused++;
  }
  return nFused;
}
}  // namespace

// The scene: key frame 0 is the current one, 1 .. B-1 the targets, all as gfs_fuse_keyframe (`list` unused); M map points as one
// gfs_fuse_points; slots [sum of n_kp]: the map point a key-point holds on entry (-1 none), key frame after key frame; bad / extra_obs
// [M]; alt [M][32] + has_alt [M]: the descriptor ComputeDistinctiveDescriptors gives the point.
// mode: 0 = adaptor over the restatement, 1 = adaptor over the GPU, 2 = the sequential loop (live descriptors), 3 = the sequential
// loop with the descriptors of each batch's start (a replay WITHOUT the recompute), 4 = a two-camera target, 5 = a non-pinhole target
// (both must throw: returns -200).
// Outputs: final_slots (as slots), point_state [M][5] (bad, Observations(), replaced id or -1, ComputeDistinctiveDescriptors calls,
// UpdateNormalAndDepth calls), counts [5] (fused in targets, fused in current, recomputed, UpdateConnections calls, device calls).
extern "C" int fuse_adaptor_test(const char* restatement_lib, int mode, const gfs_fuse_keyframe* kfs, int B, const gfs_fuse_points* pts,
                                 const int32_t* slots, const uint8_t* bad, const int32_t* extra_obs, const uint8_t* alt,
                                 const uint8_t* has_alt, int32_t* final_slots, int32_t* point_state, int32_t* counts) {
  try {
    void* so = dlopen(restatement_lib, RTLD_NOW | RTLD_LOCAL);
    if (!so) return -101;
    search_fn search = (search_fn)dlsym(so, "fr_fuse_search");
    point_fn point = (point_fn)dlsym(so, "fr_fuse_point");
    if (!search || !point) return -102;
    const int M = pts->n_mp;
    std::vector<MockMapPoint> mps((size_t)M);
    for (int i = 0; i < M; i++) {
      MockMapPoint& m = mps[i];
      m.id = i;
      m.bad = bad[i] != 0;
      m.extra_obs = extra_obs[i];
      std::memcpy(m.xw, pts->mp_xw + 3 * i, 12);
      std::memcpy(m.normal, pts->mp_normal + 3 * i, 12);
      m.min_d = pts->mp_min_dist[i];
      m.max_d = pts->mp_max_dist[i];
      std::memcpy(m.desc, pts->mp_desc + 32 * (size_t)i, 32);
      std::memcpy(m.alt, alt + 32 * (size_t)i, 32);
      m.has_alt = has_alt[i] != 0;
    }
    std::vector<MockKeyFrame> KF((size_t)B);
    size_t at = 0;
    for (int f = 0; f < B; f++) {
      const gfs_fuse_keyframe& k = kfs[f];
      MockKeyFrame& F = KF[f];
      F.mnId = 100 + (unsigned long)f;
      F.N = k.n_kp;
      F.mnScaleLevels = k.n_levels;
      F.fx = k.fx;
      F.fy = k.fy;
      F.cx = k.cx;
      F.cy = k.cy;
      F.mbf = k.bf;
      F.mnMinX = k.min_x;
      F.mnMaxX = k.max_x;
      F.mnMinY = k.min_y;
      F.mnMaxY = k.max_y;
      F.mfGridElementWidthInv = k.grid_w_inv;
      F.mfGridElementHeightInv = k.grid_h_inv;
      F.mfLogScaleFactor = k.log_scale_factor;
      F.mvScaleFactors.assign(k.scale_factors, k.scale_factors + k.n_levels);
      F.mvInvLevelSigma2.assign(k.inv_level_sigma2, k.inv_level_sigma2 + k.n_levels);
      F.mvuRight.assign(k.u_right, k.u_right + k.n_kp);
      F.mvKeysUn.assign(k.kps_un, k.kps_un + k.n_kp);
      F.mDescriptors.assign(k.desc, k.desc + 32 * (size_t)k.n_kp);
      std::memcpy(F.q, k.Tcw_q, 16);
      std::memcpy(F.t, k.Tcw_t, 12);
      std::memcpy(F.Ow, k.Ow, 12);
      for (int i = 0; i < k.n_kp; i++, at++) {
        MockMapPoint* p = slots[at] >= 0 ? &mps[slots[at]] : nullptr;
        F.mvpMapPoints.push_back(p);
        if (p && !p->IsInKeyFrame(&F)) p->AddObservation(&F, i);
      }
    }
    if (mode == 4) KF[B - 1].NLeft = KF[B - 1].N / 2;
    if (mode == 5) KF[B - 1].pinhole = false;
    MockKeyFrame* cur = &KF[0];
    std::vector<MockKeyFrame*> targets;
    for (int f = 1; f < B; f++) targets.push_back(&KF[f]);
    const float th = kfs[0].th;
    int n_calls = 0;
    counts[0] = counts[1] = counts[2] = counts[3] = counts[4] = 0;
    if (mode == 2 || mode == 3) {
      auto snapshot = [&](const std::vector<MockMapPoint*>& v) {
        std::map<MockMapPoint*, std::vector<uint8_t>> s;
        for (MockMapPoint* p : v)
          if (p) s[p] = std::vector<uint8_t>(p->desc, p->desc + 32);
        return s;
      };
      std::vector<MockMapPoint*> vpMapPointMatches = cur->GetMapPointMatches();
      auto s1 = snapshot(vpMapPointMatches);
      for (int f = 1; f < B; f++) {
        gfs_fuse_keyframe k = kfs[f];
        k.th = th;
        counts[0] += fuse_sequential(point, &KF[f], k, vpMapPointMatches, mode == 3 ? &s1 : nullptr);
      }
      std::vector<MockMapPoint*> vpFuseCandidates;
      for (MockKeyFrame* pKFi : targets)
        for (MockMapPoint* pMP : pKFi->GetMapPointMatches()) {
          if (!pMP) continue;
          if (pMP->isBad() || pMP->mnFuseCandidateForKF == cur->mnId) continue;
          pMP->mnFuseCandidateForKF = cur->mnId;
          vpFuseCandidates.push_back(pMP);
        }
      auto s2 = snapshot(vpFuseCandidates);
      counts[1] = fuse_sequential(point, cur, kfs[0], vpFuseCandidates, mode == 3 ? &s2 : nullptr);
      for (MockMapPoint* pMP : cur->GetMapPointMatches())
        if (pMP && !pMP->isBad()) {
          pMP->ComputeDistinctiveDescriptors();
          pMP->UpdateNormalAndDepth();
        }
      cur->UpdateConnections();
    } else {
      try {
        gfs_host::SearchInNeighborsCounts c;
        if (mode == 1) {
          gfs_host::FuseSearcher searcher(4096);
          c = gfs_host::SearchInNeighborsFuse<Access>(
              [&](const gfs_fuse_points* l, int nl, const gfs_fuse_keyframe* k, int nb, gfs_fuse_result* r) {
                n_calls++;
                return searcher.solve(l, nl, k, nb, r);
              },
              cur, targets, nullptr, th);
        } else {
          c = gfs_host::SearchInNeighborsFuse<Access>(
              [&](const gfs_fuse_points* l, int nl, const gfs_fuse_keyframe* k, int nb, gfs_fuse_result* r) {
                n_calls++;
                return search(l, nl, k, nb, r, nullptr);
              },
              cur, targets, nullptr, th);
        }
        counts[0] = c.fused_in_targets;
        counts[1] = c.fused_in_current;
        counts[2] = c.recomputed;
      } catch (const std::invalid_argument&) {
        return -200;
      }
    }
    counts[3] = cur->n_update_connections;
    counts[4] = n_calls;
    at = 0;
    for (int f = 0; f < B; f++)
      for (int i = 0; i < KF[f].N; i++, at++) final_slots[at] = KF[f].mvpMapPoints[i] ? KF[f].mvpMapPoints[i]->id : -1;
    for (int i = 0; i < M; i++) {
      const MockMapPoint& m = mps[i];
      const int32_t st[5] = {m.bad ? 1 : 0, m.Observations(), m.replaced ? m.replaced->id : -1, m.n_cdd, m.n_unad};
      std::memcpy(point_state + 5 * (size_t)i, st, sizeof(st));
    }
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "fuse_adaptor_test: %s\n", ex.what());
    return -1;
  }
}

// the product's host statement of the rule (csrc/fuse_rule.hpp) on every (point, key frame) pair of a call, as gfs_fuse_search delivers
extern "C" int fuse_host_rule(const gfs_fuse_points* lists, int n_lists, const gfs_fuse_keyframe* kfs, int B, gfs_fuse_result* results) {
  try {
    for (int f = 0; f < B; f++) {
      const gfs_fuse_points& L = lists[kfs[f].list];
      int matched = 0;
      for (int i = 0; i < L.n_mp; i++) {
        const gfs_fuse::PointResult o = gfs_host::fuse_search_point_host(kfs[f], L.mp_xw + 3 * i, L.mp_normal + 3 * i, L.mp_min_dist[i],
                                                                         L.mp_max_dist[i], L.mp_desc + 32 * (size_t)i);
        results[f].exit[i] = (uint8_t)o.exit;
        results[f].best_idx[i] = o.best_idx;
        results[f].best_dist[i] = o.best_dist;
        results[f].level[i] = o.level;
        matched += o.exit == GFS_FUSE_MATCHED;
      }
      results[f].n_matched = matched;
    }
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "fuse_host_rule: %s\n", ex.what());
    return -1;
  }
}
