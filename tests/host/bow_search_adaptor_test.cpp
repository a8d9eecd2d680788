// Test harness for gfs_host::SearchByBoW and gfs_host::BowMatchesOfCandidate (geoflowslam_amd/host/gfs_adaptors.hpp): plain-struct
// stand-ins for the members of KeyFrame / MapPoint that ORBmatcher::SearchByBoW (reference src/ORBmatcher.cc:936-1053) and the merge
// of LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:692-730) touch, filled from a flattened problem; the adaptor
// gathers, searches (the host restatement, bow_search_restatement.cpp, compiled in; or the device when use_device != 0) and maps the
// indices back to map points; the caller gets the lists as the adaptor left them, as indices.  Built by tests/test_bow_search_adaptor.py
// with g++.
#include <cstring>
#include <map>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"
#include "bow_search_restatement.cpp"

namespace {
struct MockMapPoint {
  int id = -1;
  bool bad = false;
  bool isBad() const { return bad; }
};
struct MockKeyFrame {
  int NLeft = -1, N = 0;
  bool bad = false;
  std::vector<gfs_keypoint> mvKeysUn;
  const uint8_t* mDescriptors = nullptr;
  std::map<unsigned, std::vector<unsigned>> mFeatVec;  // DBoW2::FeatureVector
  std::vector<MockMapPoint*> matches;
  bool isBad() const { return bad; }
  std::vector<MockMapPoint*> GetMapPointMatches() const { return matches; }
};
struct MockAccess {
  static const gfs_keypoint* keys_un(const MockKeyFrame& k) { return k.mvKeysUn.data(); }
  static const uint8_t* descriptors(const MockKeyFrame& k) { return k.mDescriptors; }
  template <class F>
  static void for_each_node(const MockKeyFrame& k, F&& f) {
    for (const auto& n : k.mFeatVec) f(n.first, n.second);
  }
};

// kind [n_kp]: 0 no map point, 1 a good one, 2 a bad one; mp_id [n_kp]: which point of the pool (one pool per side)
void fill(MockKeyFrame& K, const gfs_bow_keyframe& k, const uint8_t* kind, const int32_t* mp_id, std::vector<MockMapPoint>& pool) {
  K.N = k.n_kp;
  K.mvKeysUn.assign((size_t)k.n_kp + 1, gfs_keypoint{});
  for (int i = 0; i < k.n_kp; i++) K.mvKeysUn[i].angle = k.angle[i];
  K.mDescriptors = k.desc;
  for (int n = 0; n < k.n_nodes; n++)
    K.mFeatVec[(unsigned)k.node_id[n]] = std::vector<unsigned>(k.feat_idx + k.node_start[n], k.feat_idx + k.node_start[n + 1]);
  K.matches.assign((size_t)k.n_kp, nullptr);
  for (int i = 0; i < k.n_kp; i++) {
    if (kind[i] == 0) continue;
    MockMapPoint& P = pool[(size_t)mp_id[i]];
    P.id = mp_id[i];
    if (kind[i] == 2) P.bad = true;
    K.matches[i] = &P;
  }
}
}  // namespace

// One problem whose has_mp arrays hold the KIND of every key-point (0 none, 1 good, 2 bad); mp_id1 [n_kp1], mp_id2 [sum of the key
// frames 2' n_kp]: the identity of every map point, so that key frames 2 can share points; kf2_state [n_kf2]: 0 a key frame, 1 a null
// pointer, 2 a bad key frame; n_points: the size of the pool of side 2.
// Out: list_size [n_kf2] = vvpMatches12[j].size(); match_id [n_kf2][n_kp1] = the id of vvpMatches12[j][i] or -1; n_matches [n_kf2];
// merged_id [n_kp1], merged_kf [n_kp1] = vpMatchedPoints / the index of vpKeyFrameMatchedMP in vpCovKFi, or -1;
// summary [3] = numBoWMatches, nIndexMostBoWMatchesKF, nMostBoWNumMatches.
// Returns 0, -100 after std::invalid_argument, -101 after any other exception.
extern "C" int bow_adaptor_test(int use_device, const gfs_bow_problem* p, const int32_t* mp_id1, const int32_t* mp_id2, const int32_t* kf2_state,
                                int n_points, int two_cameras, int32_t* list_size, int32_t* match_id, int32_t* n_matches, int32_t* merged_id,
                                int32_t* merged_kf, int32_t* summary) {
  try {
    const int N = p->kf1.n_kp;
    std::vector<MockMapPoint> pool1((size_t)N + 1), pool2((size_t)n_points + 1);
    MockKeyFrame K1;
    fill(K1, p->kf1, p->kf1.has_mp, mp_id1, pool1);
    if (two_cameras) K1.NLeft = 10;
    std::vector<MockKeyFrame> K2((size_t)p->n_kf2);
    std::vector<MockKeyFrame*> vpCovKFi;
    size_t at = 0;
    for (int j = 0; j < p->n_kf2; j++) {
      fill(K2[j], p->kf2[j], p->kf2[j].has_mp, mp_id2 + at, pool2);
      at += (size_t)p->kf2[j].n_kp;
      K2[j].bad = kf2_state[j] == 2;
      vpCovKFi.push_back(kf2_state[j] == 1 ? nullptr : &K2[j]);
    }
    auto host = [](const gfs_bow_problem* q, int B, gfs_bow_result* const* r) { return bw_search_by_bow(q, B, r, nullptr); };
    std::vector<std::vector<MockMapPoint*>> vvpMatches12;
    std::vector<int> vnMatches;
    gfs_host::BowCandidateMatches<MockKeyFrame, MockMapPoint> merged;
    if (use_device) {
      gfs_host::BowSearcher dev(N > 64 ? N : 64);
      gfs_host::SearchByBoW<MockAccess>(dev.solver(), &K1, vpCovKFi, p->nn_ratio, p->check_orientation != 0, vvpMatches12, vnMatches);
      merged = gfs_host::BowMatchesOfCandidate<MockAccess, MockMapPoint>(dev.solver(), &K1, vpCovKFi, p->nn_ratio, p->check_orientation != 0);
    } else {
      gfs_host::SearchByBoW<MockAccess>(host, &K1, vpCovKFi, p->nn_ratio, p->check_orientation != 0, vvpMatches12, vnMatches);
      merged = gfs_host::BowMatchesOfCandidate<MockAccess, MockMapPoint>(host, &K1, vpCovKFi, p->nn_ratio, p->check_orientation != 0);
    }
    for (int j = 0; j < p->n_kf2; j++) {
      list_size[j] = (int32_t)vvpMatches12[j].size();
      n_matches[j] = vnMatches[j];
      for (int i = 0; i < N; i++) match_id[(size_t)j * N + i] = -1;
      for (size_t i = 0; i < vvpMatches12[j].size(); i++)
        if (vvpMatches12[j][i]) match_id[(size_t)j * N + i] = vvpMatches12[j][i]->id;
      if (merged.vvpMatchedMPs[j] != vvpMatches12[j]) return -102;  // the two entry points search alike
    }
    for (int i = 0; i < N; i++) {
      merged_id[i] = merged.vpMatchedPoints[i] ? merged.vpMatchedPoints[i]->id : -1;
      merged_kf[i] = -1;
      for (int j = 0; j < p->n_kf2; j++)
        if (merged.vpKeyFrameMatchedMP[i] && merged.vpKeyFrameMatchedMP[i] == vpCovKFi[j]) merged_kf[i] = j;
    }
    summary[0] = merged.numBoWMatches;
    summary[1] = merged.nIndexMostBoWMatchesKF;
    summary[2] = merged.nMostBoWNumMatches;
    return 0;
  } catch (const std::invalid_argument&) {
    return -100;
  } catch (...) {
    return -101;
  }
}
