// Test harness for gfs_host::UpdateMapPoints / ProcessNewKeyFrame / the batched tail of SearchInNeighborsFuse / MapPointUpdater /
// map_points_update_host (geoflowslam_amd/host/gfs_adaptors.hpp) over plain-struct KeyFrame / MapPoint classes whose
// ComputeDistinctiveDescriptors and UpdateNormalAndDepth are written out per point the way the reference writes them (src/MapPoint.cc:376-448,
// :468-532).  Two scenes are built from one seed; one runs the adaptor with a map-point solver (the CPU restatement through dlopen, the
// product's host rule, or the GPU library), the other the reference's per-point loops; their end states must agree bit for bit.
// Built by tests/test_map_point_adaptor.py as a shared library, and with -DMP_STANDALONE as a program of its own (main below) that
// needs neither the library nor python: that build runs under the address and undefined-behaviour sanitizers.
#include <dlfcn.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

#if defined(MP_STANDALONE)
extern "C" const char* gfs_last_error(void) { return "(host build)"; }
#endif

namespace {
struct MockKeyFrame;
struct MockMapPoint {
  int id = 0;
  bool bad = false;
  std::map<MockKeyFrame*, std::tuple<int, int>> mObservations;
  MockKeyFrame* mpRefKF = nullptr;
  MockMapPoint* replaced = nullptr;
  unsigned long mnFuseCandidateForKF = 0;
  float mWorldPos[3] = {0, 0, 0}, mNormalVector[3] = {9, 9, 9}, mfMinDistance = -1, mfMaxDistance = -1;
  uint8_t mDescriptor[32];
  int n_desc_set = 0, n_normal_set = 0;
  bool isBad() const { return bad; }
  bool IsInKeyFrame(MockKeyFrame* kf) const { return mObservations.count(kf) != 0; }
  int Observations() const { return (int)mObservations.size(); }
  std::map<MockKeyFrame*, std::tuple<int, int>> GetObservations() const { return mObservations; }
  void AddObservation(MockKeyFrame* kf, int idx) { mObservations[kf] = std::make_tuple(idx, -1); }
  void Replace(MockMapPoint*) {}
  void ComputeDistinctiveDescriptors();
  void UpdateNormalAndDepth();
};
struct MockKeyFrame {
  int NLeft = -1, N = 0, mnScaleLevels = 8, rows = 0;
  unsigned long mnId = 0;
  bool bad = false;
  float fx = 500, fy = 500, cx = 320, cy = 240, mbf = 40, mnMinX = 0, mnMaxX = 640, mnMinY = 0, mnMaxY = 480, mfGridElementWidthInv = 0.1f,
        mfGridElementHeightInv = 0.1f, mfLogScaleFactor = 0.18232f;
  std::vector<float> mvuRight, mvScaleFactors, mvInvLevelSigma2;
  std::vector<gfs_keypoint> mvKeysUn;
  std::vector<uint8_t> mDescriptors;  // [rows][32]
  std::vector<MockMapPoint*> mvpMapPoints;
  float Ow[3];
  int n_update_connections = 0;
  bool isBad() const { return bad; }
  MockMapPoint* GetMapPoint(int idx) { return mvpMapPoints[idx]; }
  void AddMapPoint(MockMapPoint* p, int idx) { mvpMapPoints[idx] = p; }
  std::vector<MockMapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  void UpdateConnections() { n_update_connections++; }
};

int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}
float Norm3(const float* v) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

void MockMapPoint::ComputeDistinctiveDescriptors() {  // src/MapPoint.cc:376-448, left indices
  std::vector<const uint8_t*> vDescriptors;
  if (bad) return;
  std::map<MockKeyFrame*, std::tuple<int, int>> observations = mObservations;
  if (observations.empty()) return;
  for (auto mit = observations.begin(); mit != observations.end(); mit++) {
    MockKeyFrame* pKF = mit->first;
    if (!pKF) continue;
    if (!pKF->isBad()) {
      const int leftIndex = std::get<0>(mit->second);
      if (leftIndex != -1 && leftIndex < pKF->rows) vDescriptors.push_back(&pKF->mDescriptors[32 * (size_t)leftIndex]);
    }
  }
  if (vDescriptors.empty()) return;
  const size_t N = vDescriptors.size();
  std::vector<float> Distances(N * N);
  for (size_t i = 0; i < N; i++) {
    Distances[i * N + i] = 0;
    for (size_t j = i + 1; j < N; j++) {
      int distij = DescriptorDistance(vDescriptors[i], vDescriptors[j]);
      Distances[i * N + j] = distij;
      Distances[j * N + i] = distij;
    }
  }
  int BestMedian = INT_MAX;
  int BestIdx = 0;
  for (size_t i = 0; i < N; i++) {
    std::vector<int> vDists(Distances.begin() + i * N, Distances.begin() + i * N + N);
    std::sort(vDists.begin(), vDists.end());
    int median = vDists[0.5 * (N - 1)];
    if (median < BestMedian) {
      BestMedian = median;
      BestIdx = i;
    }
  }
  std::memcpy(mDescriptor, vDescriptors[BestIdx], 32);
  n_desc_set++;
}

void MockMapPoint::UpdateNormalAndDepth() {  // src/MapPoint.cc:468-532, left indices
  if (bad) return;
  std::map<MockKeyFrame*, std::tuple<int, int>> observations = mObservations;
  MockKeyFrame* pRefKF = mpRefKF;
  if (observations.empty()) return;
  float normal[3] = {0, 0, 0};
  int n = 0;
  for (auto mit = observations.begin(); mit != observations.end(); mit++) {
    MockKeyFrame* pKF = mit->first;
    const int leftIndex = std::get<0>(mit->second);
    if (leftIndex != -1) {
      float normali[3];
      for (int c = 0; c < 3; c++) normali[c] = mWorldPos[c] - pKF->Ow[c];
      const float len = Norm3(normali);
      for (int c = 0; c < 3; c++) normal[c] = normal[c] + normali[c] / len;
      n++;
    }
  }
  float PC[3];
  for (int c = 0; c < 3; c++) PC[c] = mWorldPos[c] - pRefKF->Ow[c];
  const float dist = Norm3(PC);
  std::tuple<int, int> indexes = observations[pRefKF];
  const int level = pRefKF->mvKeysUn[std::get<0>(indexes)].octave;
  const float levelScaleFactor = pRefKF->mvScaleFactors[level];
  const int nLevels = pRefKF->mnScaleLevels;
  mfMaxDistance = dist * levelScaleFactor;
  mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
  for (int c = 0; c < 3; c++) mNormalVector[c] = normal[c] / n;
  n_normal_set++;
}

struct Access {
  static bool is_pinhole(const MockKeyFrame&) { return true; }
  static void pose(const MockKeyFrame& F, float* q, float* t, float* Ow) {
    q[0] = q[1] = q[2] = 0.0f;
    q[3] = 1.0f;
    for (int c = 0; c < 3; c++) t[c] = -F.Ow[c];
    std::memcpy(Ow, F.Ow, 12);
  }
  static const gfs_keypoint* keys_un(const MockKeyFrame& F) { return F.mvKeysUn.data(); }
  static const uint8_t* descriptors(const MockKeyFrame& F) { return F.mDescriptors.data(); }
  static void world_pos(const MockMapPoint* p, float* o) { std::memcpy(o, p->mWorldPos, 12); }
  static void normal(const MockMapPoint* p, float* o) { std::memcpy(o, p->mNormalVector, 12); }
  static void distances(const MockMapPoint* p, float* mn, float* mx) {
    *mn = p->mfMinDistance;
    *mx = p->mfMaxDistance;
  }
  static void descriptor(const MockMapPoint* p, uint8_t* d) { std::memcpy(d, p->mDescriptor, 32); }
  // the members of UpdateMapPoints
  static int descriptor_rows(const MockKeyFrame& F) { return F.rows; }
  static void camera_center(const MockKeyFrame& F, float* Ow) { std::memcpy(Ow, F.Ow, 12); }
  static MockKeyFrame* reference_keyframe(const MockMapPoint* p) { return p->mpRefKF; }
  static void set_descriptor(MockMapPoint* p, const uint8_t* row) {
    std::memcpy(p->mDescriptor, row, 32);
    p->n_desc_set++;
  }
  static void set_normal_and_depth(MockMapPoint* p, const float* n, float mn, float mx) {
    std::memcpy(p->mNormalVector, n, 12);
    p->mfMinDistance = mn;
    p->mfMaxDistance = mx;
    p->n_normal_set++;
  }
};

struct Scene {
  std::vector<MockKeyFrame> kfs;  // one array: std::map<KeyFrame*, ...> iterates in pointer order, which is then the index order in every scene
  std::vector<std::unique_ptr<MockMapPoint>> mps;
  std::vector<MockMapPoint*> listed;  // what UpdateMapPoints is given: nulls, bad points and a duplicate included
  MockKeyFrame* current = nullptr;    // the new key frame of ProcessNewKeyFrame / the current one of SearchInNeighbors
};

constexpr int kKp = 48;

// Key frame 3 is bad, key frame 5 has only 20 descriptor rows, the last key frame is the current one and observes nothing yet.
// Points: observations in 0..9 key frames; every 9th point is bad, every 11th has a reference key frame that does not observe it,
// point 4 carries a null key frame, point 6 an observation without an index; point 8 observes nothing.
void build(Scene& S, unsigned seed, int n_points) {
  std::mt19937 rng(seed);
  auto uni = [&rng](float a, float b) { return a + (b - a) * (float)(rng() % 100000) / 100000.0f; };
  const int K = 13;
  uint8_t base[6][32];
  for (auto& b : base)
    for (auto& x : b) x = (uint8_t)(rng() & 255);
  S.kfs.resize(K);
  for (int k = 0; k < K; k++) {
    MockKeyFrame* kf = &S.kfs[k];
    kf->mnId = 100 + k;
    kf->N = kKp;
    kf->rows = k == 5 ? 20 : kKp;
    kf->bad = k == 3;
    for (int c = 0; c < 3; c++) kf->Ow[c] = uni(-2.0f, 2.0f);
    float s = 1.0f;
    for (int l = 0; l < 8; l++, s *= 1.2f) {
      kf->mvScaleFactors.push_back(s);
      kf->mvInvLevelSigma2.push_back(1.0f / (s * s));
    }
    kf->mvuRight.assign(kKp, -1.0f);
    kf->mvKeysUn.resize(kKp);
    kf->mDescriptors.resize(32 * (size_t)kKp);
    kf->mvpMapPoints.assign(kKp, nullptr);
    for (int i = 0; i < kKp; i++) {
      kf->mvKeysUn[i] = gfs_keypoint{uni(10, 600), uni(10, 400), 31.0f, 0.0f, 1.0f, (int)(rng() % 8), -1};
      uint8_t* d = &kf->mDescriptors[32 * (size_t)i];
      std::memcpy(d, base[i % 6], 32);
      for (int f = (int)(rng() % 40); f > 0; f--) d[rng() % 32] ^= (uint8_t)(1u << (rng() % 8));
    }
  }
  S.current = &S.kfs[K - 1];
  for (int p = 0; p < n_points; p++) {
    auto mp = std::make_unique<MockMapPoint>();
    mp->id = p;
    mp->bad = p % 9 == 7;
    for (int c = 0; c < 3; c++) mp->mWorldPos[c] = uni(-5.0f, 5.0f);
    for (auto& x : mp->mDescriptor) x = (uint8_t)(rng() & 255);
    const int n = p == 8 ? 0 : 1 + (int)(rng() % 9);
    const int i6 = p % 6;  // the point's key-points share a base pattern
    for (int o = 0; o < n; o++) {
      MockKeyFrame* kf = &S.kfs[rng() % (K - 1)];
      mp->mObservations[kf] = std::make_tuple(i6 + 6 * (int)(rng() % (kKp / 6)), -1);
    }
    if (p == 4) mp->mObservations[nullptr] = std::make_tuple(-1, -1);
    if (p == 6) mp->mObservations[&S.kfs[1]] = std::make_tuple(-1, -1);
    mp->mpRefKF = (p % 11 == 10 || n == 0) ? &S.kfs[K - 2] : mp->mObservations.begin()->first ? mp->mObservations.begin()->first
                                                                                                 : &S.kfs[K - 2];
    if (p == 6) mp->mpRefKF = &S.kfs[K - 2];
    if (mp->mpRefKF == &S.kfs[K - 2]) mp->mObservations.erase(&S.kfs[K - 2]);  // a reference key frame that is absent
    S.mps.push_back(std::move(mp));
  }
  for (int p = 0; p < n_points; p++) {
    S.listed.push_back(S.mps[p].get());
    if (p % 10 == 3) S.listed.push_back(nullptr);
  }
  S.listed.push_back(S.mps[2].get());  // listed twice
  // the current key frame's slots: every second point, one of them in two slots, nulls between
  for (int i = 0, p = 0; i < kKp && p < n_points; i++) {
    if (i % 5 == 4) continue;
    S.current->mvpMapPoints[i] = S.mps[p].get();
    p += 2;
  }
  S.current->mvpMapPoints[kKp - 1] = S.current->mvpMapPoints[0];
}

std::string compare(const Scene& A, const Scene& B, const char* what) {
  char buf[256];
  for (size_t p = 0; p < A.mps.size(); p++) {
    const MockMapPoint &a = *A.mps[p], &b = *B.mps[p];
    const bool same = !std::memcmp(a.mDescriptor, b.mDescriptor, 32) && !std::memcmp(a.mNormalVector, b.mNormalVector, 12) &&
                      !std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) && !std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) &&
                      a.mObservations.size() == b.mObservations.size() && (a.n_desc_set > 0) == (b.n_desc_set > 0) &&
                      (a.n_normal_set > 0) == (b.n_normal_set > 0);
    if (!same) {
      std::snprintf(buf, sizeof buf, "%s: point %zu differs (normal %g %g %g / %g %g %g, max %g / %g, desc set %d / %d, normal set %d / %d)", what,
                    p, a.mNormalVector[0], a.mNormalVector[1], a.mNormalVector[2], b.mNormalVector[0], b.mNormalVector[1], b.mNormalVector[2],
                    a.mfMaxDistance, b.mfMaxDistance, a.n_desc_set, b.n_desc_set, a.n_normal_set, b.n_normal_set);
      return buf;
    }
  }
  return "";
}


// ---- the write-back of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:2001-2039) with the batched UpdateNormalAndDepth: classes
// with the members that adaptor uses (cv::KeyPoint-like key-points), a solver that moves every pose and point and fails some edges
namespace lba {
struct Map;
struct KeyFrame;
struct MapPoint {
  unsigned long mnBALocalForKF = 0;
  bool bad = false;
  Map* map = nullptr;
  std::map<KeyFrame*, std::tuple<int, int>> mObservations;
  KeyFrame* mpRefKF = nullptr;
  float mWorldPos[3], mNormalVector[3] = {9, 9, 9}, mfMinDistance = -1, mfMaxDistance = -1;
  bool isBad() const { return bad; }
  Map* GetMap() const { return map; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() const { return mObservations; }
  void EraseObservation(KeyFrame* kf) { mObservations.erase(kf); }
  void UpdateNormalAndDepth();
};
struct Pt {
  float x, y;
};
struct KeyPoint {
  Pt pt;
  int octave;
};
struct KeyFrame {
  unsigned long mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
  int NLeft = -1, mnScaleLevels = 8;
  Map* map = nullptr;
  void* mpCamera2 = nullptr;
  float fx = 500, fy = 500, cx = 320, cy = 240, mbf = 40, q[4] = {0, 0, 0, 1}, t[3];
  std::vector<KeyPoint> mvKeysUn;
  std::vector<gfs_keypoint> flat;
  std::vector<float> mvuRight, mvInvLevelSigma2, mvScaleFactors;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> neighbours;
  bool isBad() const { return false; }
  Map* GetMap() const { return map; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return neighbours; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
  void EraseMapPointMatch(MapPoint* p) {
    for (auto& m : mvpMapPoints)
      if (m == p) m = nullptr;
  }
};
struct Map {
  std::mutex mMutexMapUpdate;
  std::set<unsigned long> msOptKFs, msFixedKFs;
  int changes = 0;
  unsigned long GetInitKFid() const { return 1; }
  void IncreaseChangeIndex() { changes++; }
};
void MapPoint::UpdateNormalAndDepth() {  // src/MapPoint.cc:468-532 with GetCameraCenter() = t
  if (bad) return;
  std::map<KeyFrame*, std::tuple<int, int>> observations = mObservations;
  if (observations.empty()) return;
  float normal[3] = {0, 0, 0};
  int n = 0;
  for (auto& mit : observations) {
    if (std::get<0>(mit.second) != -1) {
      float normali[3];
      for (int c = 0; c < 3; c++) normali[c] = mWorldPos[c] - mit.first->t[c];
      const float len = Norm3(normali);
      for (int c = 0; c < 3; c++) normal[c] = normal[c] + normali[c] / len;
      n++;
    }
  }
  float PC[3];
  for (int c = 0; c < 3; c++) PC[c] = mWorldPos[c] - mpRefKF->t[c];
  const float dist = Norm3(PC);
  const int level = mpRefKF->mvKeysUn[std::get<0>(observations[mpRefKF])].octave;
  mfMaxDistance = dist * mpRefKF->mvScaleFactors[level];
  mfMinDistance = mfMaxDistance / mpRefKF->mvScaleFactors[mpRefKF->mnScaleLevels - 1];
  for (int c = 0; c < 3; c++) mNormalVector[c] = normal[c] / n;
}
struct Access {
  static void pose(const KeyFrame* F, float* q, float* t) {
    std::memcpy(q, F->q, 16);
    std::memcpy(t, F->t, 12);
  }
  static void set_pose(KeyFrame* F, const float* q, const float* t) {
    std::memcpy(F->q, q, 16);
    std::memcpy(F->t, t, 12);
  }
  static void world_pos(const MapPoint* p, float* o) { std::memcpy(o, p->mWorldPos, 12); }
  static void set_world_pos(MapPoint* p, const float* X) { std::memcpy(p->mWorldPos, X, 12); }
  static const gfs_keypoint* keys_un(const KeyFrame& F) { return F.flat.data(); }
  static const uint8_t* descriptors(const KeyFrame&) { return nullptr; }
  static int descriptor_rows(const KeyFrame&) { return 0; }
  static void camera_center(const KeyFrame& F, float* Ow) { std::memcpy(Ow, F.t, 12); }
  static KeyFrame* reference_keyframe(const MapPoint* p) { return p->mpRefKF; }
  static void set_descriptor(MapPoint*, const uint8_t*) {}
  static void set_normal_and_depth(MapPoint* p, const float* n, float mn, float mx) {
    std::memcpy(p->mNormalVector, n, 12);
    p->mfMinDistance = mn;
    p->mfMaxDistance = mx;
  }
};
struct Scene {
  Map map;
  std::vector<KeyFrame> kfs;
  std::vector<MapPoint> mps;
};
void build(Scene& S, unsigned seed) {
  std::mt19937 rng(seed);
  auto uni = [&rng](float a, float b) { return a + (b - a) * (float)(rng() % 100000) / 100000.0f; };
  const int K = 6, M = 80, kp = 40;
  S.kfs.resize(K);
  S.mps.resize(M);
  for (int k = 0; k < K; k++) {
    KeyFrame& F = S.kfs[k];
    F.mnId = k + 1;  // key frame 0 is the map's first: fixed
    F.map = &S.map;
    for (float& x : F.t) x = uni(-2, 2);
    float s = 1.0f;
    for (int l = 0; l < 8; l++, s *= 1.2f) {
      F.mvScaleFactors.push_back(s);
      F.mvInvLevelSigma2.push_back(1.0f / (s * s));
    }
    F.mvpMapPoints.assign(kp, nullptr);
    for (int i = 0; i < kp; i++) {
      const int oct = (int)(rng() % 8);
      F.mvKeysUn.push_back(KeyPoint{{uni(0, 640), uni(0, 480)}, oct});
      F.flat.push_back(gfs_keypoint{F.mvKeysUn[i].pt.x, F.mvKeysUn[i].pt.y, 31.0f, 0.0f, 1.0f, oct, -1});
      F.mvuRight.push_back(i % 3 ? uni(0, 600) : -1.0f);
    }
    if (k) S.kfs[0].neighbours.push_back(&F);
  }
  for (int p = 0; p < M; p++) {
    MapPoint& P = S.mps[p];
    P.map = &S.map;
    for (float& x : P.mWorldPos) x = uni(-5, 5);
    for (int o = 0, n = 1 + (int)(rng() % 4); o < n; o++) {
      KeyFrame* kf = &S.kfs[rng() % K];
      const int idx = (int)(rng() % kp);
      if (P.mObservations.count(kf) || kf->mvpMapPoints[idx]) continue;
      P.mObservations[kf] = std::make_tuple(idx, -1);
      kf->mvpMapPoints[idx] = &P;
    }
    P.mpRefKF = P.mObservations.empty() ? &S.kfs[0] : P.mObservations.begin()->first;
  }
}
template <class UpdatePoints>
std::string run(UpdatePoints&& update_points, unsigned seed) {
  Scene A, B;
  build(A, seed);
  build(B, seed);
  auto solve = [](const gfs_lba_problem& p, gfs_lba_solution& s, const bool*) {
    for (int i = 0; i < 4 * p.n_poses; i++) s.pose_q[i] = p.pose_q[i];
    for (int i = 0; i < 3 * p.n_poses; i++) s.pose_t[i] = p.pose_t[i] + 0.25;
    for (int i = 0; i < 3 * p.n_points; i++) s.points[i] = p.points[i] + 0.125;
    for (int e = 0; e < p.n_edges; e++) {
      s.edge_chi2[e] = e % 7 == 0 ? 100.0 : 0.0;
      s.edge_depth_positive[e] = 1;
    }
    return true;
  };
  int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  gfs_host::LocalBundleAdjustment<Access, KeyFrame, MapPoint, Map>(solve, &A.kfs[0], nullptr, &A.map, a[0], a[1], a[2], a[3], update_points);
  gfs_host::LocalBundleAdjustment<Access, KeyFrame, MapPoint, Map>(solve, &B.kfs[0], nullptr, &B.map, b[0], b[1], b[2], b[3]);
  if (std::memcmp(a, b, sizeof a) || a[3] < 50 || A.map.changes != 1) return "LocalBundleAdjustment: the counts differ";
  int moved = 0;
  for (size_t p = 0; p < A.mps.size(); p++) {
    const MapPoint &x = A.mps[p], &y = B.mps[p];
    if (std::memcmp(x.mWorldPos, y.mWorldPos, 12) || std::memcmp(x.mNormalVector, y.mNormalVector, 12) || std::memcmp(&x.mfMinDistance, &y.mfMinDistance, 4) ||
        std::memcmp(&x.mfMaxDistance, &y.mfMaxDistance, 4) || x.mObservations.size() != y.mObservations.size())
      return "LocalBundleAdjustment: point " + std::to_string(p) + " differs";
    moved += x.mfMaxDistance >= 0;
  }
  return moved < 50 ? "LocalBundleAdjustment: too few points were updated" : "";
}
}  // namespace lba

typedef int (*update_fn)(const gfs_map_points_problem*, gfs_map_points_result*, int32_t*);

template <class Solve>
std::string run_all(Solve&& solve, unsigned seed, int* n_updated) {
  std::string e;
  {  // UpdateMapPoints against the per-point calls, in both modes
    for (int mode : {GFS_MAP_POINTS_FULL, GFS_MAP_POINTS_NORMALS_ONLY}) {
      Scene A, B;
      build(A, seed, 60);
      build(B, seed, 60);
      gfs_host::UpdateMapPoints<Access>(solve, A.listed, mode);
      for (MockMapPoint* pMP : B.listed)
        if (pMP && !pMP->isBad()) {
          if (mode == GFS_MAP_POINTS_FULL) pMP->ComputeDistinctiveDescriptors();
          pMP->UpdateNormalAndDepth();
        }
      if (!(e = compare(A, B, mode ? "UpdateMapPoints, normals only" : "UpdateMapPoints")).empty()) return e;
      int set = 0, desc = 0;
      for (auto& m : A.mps) set += m->n_normal_set > 0, desc += m->n_desc_set > 0;
      if (set < 40 || (mode == GFS_MAP_POINTS_FULL) != (desc > 30)) return "UpdateMapPoints: the scene does not exercise the update";
      if (A.mps[7]->n_normal_set || A.mps[8]->n_normal_set) return "a bad or unobserved point was written";
      *n_updated = set;
    }
  }
  {  // ProcessNewKeyFrame (src/LocalMapping.cc:439-454)
    Scene A, B;
    build(A, seed + 1, 60);
    build(B, seed + 1, 60);
    A.mps[10]->AddObservation(A.current, 3);  // already observed by the new key frame: the else branch
    B.mps[10]->AddObservation(B.current, 3);
    std::list<MockMapPoint*> recentA, recentB;
    gfs_host::ProcessNewKeyFrame<Access>(solve, A.current, recentA);
    const std::vector<MockMapPoint*> v = B.current->GetMapPointMatches();
    for (size_t i = 0; i < v.size(); i++) {
      MockMapPoint* pMP = v[i];
      if (pMP) {
        if (!pMP->isBad()) {
          if (!pMP->IsInKeyFrame(B.current)) {
            pMP->AddObservation(B.current, (int)i);
            pMP->UpdateNormalAndDepth();
            pMP->ComputeDistinctiveDescriptors();
          } else {
            recentB.push_back(pMP);
          }
        }
      }
    }
    if (!(e = compare(A, B, "ProcessNewKeyFrame")).empty()) return e;
    if (recentA.size() != recentB.size() || recentA.size() < 2) return "ProcessNewKeyFrame: mlpRecentAddedMapPoints differs";
    auto ia = recentA.begin();
    for (auto ib = recentB.begin(); ib != recentB.end(); ++ia, ++ib)
      if ((*ia)->id != (*ib)->id) return "ProcessNewKeyFrame: mlpRecentAddedMapPoints order differs";
  }
  {  // the tail of SearchInNeighborsFuse (src/LocalMapping.cc:1219-1233); the Fuse searches match nothing here
    Scene A, B;
    build(A, seed + 2, 60);
    build(B, seed + 2, 60);
    auto no_match = [](const gfs_fuse_points*, int, const gfs_fuse_keyframe*, int, gfs_fuse_result*) { return 0; };
    for (Scene* S : {&A, &B})
      for (size_t i = 0; i < S->current->mvpMapPoints.size(); i++)
        if (MockMapPoint* p = S->current->mvpMapPoints[i]) p->AddObservation(S->current, (int)i);
    const std::vector<MockKeyFrame*> tA{&A.kfs[0], &A.kfs[1]}, tB{&B.kfs[0], &B.kfs[1]};
    gfs_host::SearchInNeighborsFuse<Access>(no_match, A.current, tA, nullptr, 3.0f, solve);
    gfs_host::SearchInNeighborsFuse<Access>(no_match, B.current, tB);
    if (!(e = compare(A, B, "SearchInNeighborsFuse")).empty()) return e;
    if (A.current->n_update_connections != 1 || B.current->n_update_connections != 1) return "SearchInNeighborsFuse: UpdateConnections";
  }
  if (!(e = lba::run(solve, seed + 3)).empty()) return e;
  {  // what the adaptor refuses
    Scene A;
    build(A, seed, 12);
    A.mps[0]->mObservations[&A.kfs[0]] = std::make_tuple(2, 5);  // a right index
    bool threw = false;
    try {
      gfs_host::UpdateMapPoints<Access>(solve, A.listed);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    if (!threw) return "a two-camera observation did not throw";
    if (A.mps[1]->n_normal_set) return "a refused call wrote a point";
  }
  return "";
}

int finish(const std::string& e, char* msg, int msg_len) {
  if (msg && msg_len > 0) std::snprintf(msg, (size_t)msg_len, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}
}  // namespace

// mode 0: the adaptor over the restatement (mr_update of restatement_lib), 1: over the product's host rule, 2: over the GPU library.
// -> 0 and the number of points written, or 1 and what differed in msg; -100 - x: an exception or a missing library.
extern "C" int map_point_adaptor_test(const char* restatement_lib, int mode, unsigned seed, int* n_updated, char* msg, int msg_len) {
  try {
    if (mode == 0) {
      void* so = dlopen(restatement_lib, RTLD_NOW | RTLD_LOCAL);
      if (!so) return -101;
      update_fn fn = (update_fn)dlsym(so, "mr_update");
      if (!fn) return -102;
      return finish(run_all([fn](const gfs_map_points_problem* p, gfs_map_points_result* r) { return fn(p, r, nullptr); }, seed, n_updated), msg,
                    msg_len);
    }
    if (mode == 1) return finish(run_all(gfs_host::map_points_update_host, seed, n_updated), msg, msg_len);
#if !defined(MP_STANDALONE)
    if (mode == 2) {
      gfs_host::MapPointUpdater gpu(16, 64);  // small: the reserve has to grow
      return finish(run_all(gpu.solver(), seed, n_updated), msg, msg_len);
    }
#endif
    return -103;
  } catch (const std::exception& e) {
    if (msg && msg_len > 0) std::snprintf(msg, (size_t)msg_len, "exception: %s", e.what());
    return -100;
  }
}

// the product's host statement of the rule on a whole problem (compared with the restatement by the tests)
extern "C" int map_point_host_rule(const gfs_map_points_problem* p, gfs_map_points_result* r) { return gfs_host::map_points_update_host(p, r); }

#if defined(MP_STANDALONE)
int main() {
  char msg[512] = "";
  for (unsigned seed = 1; seed <= 6; seed++) {
    int n = 0;
    const int rc = map_point_adaptor_test(nullptr, 1, seed, &n, msg, (int)sizeof msg);
    if (rc != 0) {
      std::printf("seed %u: rc %d %s\n", seed, rc, msg);
      return 1;
    }
  }
  {  // the host call's refusals, and an empty problem
    int32_t start[3] = {0, 2, 1};
    gfs_map_points_problem p{};
    gfs_map_points_result r{};
    p.n_points = 2;
    p.obs_start = start;
    if (gfs_host::map_points_update_host(&p, &r) != GFS_ERR_INVALID_ARG) return 2;
    start[0] = 1;
    start[2] = 3;
    if (gfs_host::map_points_update_host(&p, &r) != GFS_ERR_INVALID_ARG) return 3;
    start[0] = 0;
    p.n_points = 0;
    if (gfs_host::map_points_update_host(&p, &r) != GFS_OK) return 4;
  }
  std::printf("map_point_adaptor_test: ok\n");
  return 0;
}
#endif
