// Test harness for gfs_host::BundleAdjustment / GlobalBundleAdjustemnt (geoflowslam_amd/host/gfs_adaptors.hpp): plain-struct
// stand-ins for the members of KeyFrame / MapPoint / Map that Optimizer::BundleAdjustment touches (reference src/Optimizer.cc:47-363),
// filled from a flat synthetic map; the adaptor gathers, solves (the CPU oracle through dlopen) and writes back; the caller inspects
// the stand-ins.  Built by tests/test_gba_adaptor.py with g++.
#include <dlfcn.h>

#include <cstring>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

namespace {
struct MockMap;
struct MockMapPoint;
struct MockKeyFrame {
  unsigned long mnId = 0, mnBAGlobalForKF = 0;
  bool bad = false;
  MockMap* map = nullptr;
  float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
  double gba_q[4] = {0, 0, 0, 0}, gba_t[3] = {0, 0, 0};
  struct KP {
    struct {
      float x, y;
    } pt;
    int octave;
  };
  std::vector<KP> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  void* mpCamera2 = nullptr;
  int n_set_pose = 0, n_set_gba = 0;
  bool isBad() const { return bad; }
  MockMap* GetMap() const { return map; }
};
struct MockMapPoint {
  unsigned long mnId = 0, mnBAGlobalForKF = 0;
  bool bad = false;
  float pos[3] = {0, 0, 0}, pos_gba[3] = {0, 0, 0};
  std::map<MockKeyFrame*, std::tuple<int, int>> obs;
  int n_update = 0, n_set_pos = 0, n_set_gba = 0;
  bool isBad() const { return bad; }
  std::map<MockKeyFrame*, std::tuple<int, int>> GetObservations() const { return obs; }
  void UpdateNormalAndDepth() { n_update++; }
};
struct MockMap {
  unsigned long init_id = ~0ul;
  MockKeyFrame* origin = nullptr;
  std::vector<MockKeyFrame*> kfs;
  std::vector<MockMapPoint*> mps;
  unsigned long GetInitKFid() const { return init_id; }
  MockKeyFrame* GetOriginKF() const { return origin; }
  std::vector<MockKeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<MockMapPoint*> GetAllMapPoints() const { return mps; }
};
struct MockAccess {
  static void pose(const MockKeyFrame* k, float q[4], float t[3]) {
    std::memcpy(q, k->q, 16);
    std::memcpy(t, k->t, 12);
  }
  static void set_pose(MockKeyFrame* k, const float q[4], const float t[3]) {
    std::memcpy(k->q, q, 16);
    std::memcpy(k->t, t, 12);
    k->n_set_pose++;
  }
  static void set_pose_gba(MockKeyFrame* k, const double q[4], const double t[3]) {
    std::memcpy(k->gba_q, q, 32);
    std::memcpy(k->gba_t, t, 24);
    k->n_set_gba++;
  }
  static void world_pos(const MockMapPoint* p, float x[3]) { std::memcpy(x, p->pos, 12); }
  static void set_world_pos(MockMapPoint* p, const float x[3]) {
    std::memcpy(p->pos, x, 12);
    p->n_set_pos++;
  }
  static void set_pos_gba(MockMapPoint* p, const float x[3]) {
    std::memcpy(p->pos_gba, x, 12);
    p->n_set_gba++;
  }
};
}  // namespace

// The map has one more map point than `points` holds: the last one has no observation at all (nEdges == 0).
// second_camera: the first observation also carries a right-camera index on a rig key-frame (the adaptor must refuse it).
// counts [12]: what the solver saw {poses, points, edges, iterations, the caller's flag pointer handed down unchanged} and the calls
//   {SetPose, set_pose_gba, SetWorldPos, set_pos_gba, UpdateNormalAndDepth}, then the edge-less point's {calls of any setter, mnBAGlobalForKF}
extern "C" int gba_adaptor_test(const char* solver_lib, int n_poses, int n_points, int n_edges, const double* pose_q, const double* pose_t,
                                const double* points, const int32_t* edge_pose, const int32_t* edge_point, const double* edge_obs,
                                const double* edge_inv_sigma2, const uint8_t* edge_stereo, double fx, double fy, double cx, double cy,
                                double bf, int init_kf_pose, int bad_kf, int bad_point, int in_place, int robust, int iterations,
                                int stop_flag, int second_camera, float* out_pose_q, float* out_pose_t, double* out_gba_q,
                                double* out_gba_t, float* out_points, float* out_points_gba, int32_t* kf_gba_for, int32_t* mp_gba_for,
                                int32_t* counts, double* hubers) {
  try {
    MockMap map;
    std::vector<MockKeyFrame> kfs((size_t)n_poses);
    std::vector<MockMapPoint> mps((size_t)n_points + 1);
    for (int i = 0; i < n_poses; i++) {
      MockKeyFrame& k = kfs[i];
      k.mnId = 10 + (unsigned long)i;
      k.map = &map;
      for (int c = 0; c < 4; c++) k.q[c] = (float)pose_q[4 * i + c];
      for (int c = 0; c < 3; c++) k.t[c] = (float)pose_t[3 * i + c];
      k.fx = (float)fx;
      k.fy = (float)fy;
      k.cx = (float)cx;
      k.cy = (float)cy;
      k.mbf = (float)bf;
      map.kfs.push_back(&k);
    }
    map.init_id = kfs[init_kf_pose].mnId;
    map.origin = &kfs[0];
    if (bad_kf >= 0) kfs[bad_kf].bad = true;
    for (int j = 0; j <= n_points; j++) {
      mps[j].mnId = 1000 + (unsigned long)j;
      for (int c = 0; c < 3; c++) mps[j].pos[c] = j < n_points ? (float)points[3 * j + c] : 1.f;
      map.mps.push_back(&mps[j]);
    }
    if (bad_point >= 0) mps[bad_point].bad = true;
    for (int e = 0; e < n_edges; e++) {  // key-point e' of its key-frame: "octave" = its own index into mvInvLevelSigma2
      MockKeyFrame& k = kfs[edge_pose[e]];
      const int kp = (int)k.mvKeysUn.size();
      MockKeyFrame::KP u;
      u.pt.x = (float)edge_obs[3 * e];
      u.pt.y = (float)edge_obs[3 * e + 1];
      u.octave = kp;
      k.mvKeysUn.push_back(u);
      k.mvuRight.push_back(edge_stereo[e] ? (float)edge_obs[3 * e + 2] : -1.f);
      k.mvInvLevelSigma2.resize((size_t)kp + 1);
      k.mvInvLevelSigma2[kp] = (float)edge_inv_sigma2[e];
      mps[edge_point[e]].obs[&k] = std::make_tuple(kp, second_camera && e == 0 ? 0 : -1);
      if (second_camera && e == 0) k.mpCamera2 = &k;
    }
    void* so = dlopen(solver_lib, RTLD_NOW | RTLD_LOCAL);
    if (!so) return -101;
    typedef int (*fn_t)(const gfs_lba_problem*, gfs_lba_solution*);
    fn_t fn = (fn_t)dlsym(so, "gfso_lba_solve");
    if (!fn) return -102;
    bool stop = stop_flag == 1;
    bool* pstop = stop_flag >= 0 ? &stop : nullptr;
    int n_solves = 0;
    auto solve = [&](const gfs_lba_problem& p, gfs_lba_solution& s, const bool* st) {
      counts[0] = p.n_poses;
      counts[1] = p.n_points;
      counts[2] = p.n_edges;
      counts[3] = p.iterations;
      counts[4] = st == pstop ? 1 : 0;
      hubers[0] = p.huber_mono;
      hubers[1] = p.huber_stereo;
      n_solves++;
      fn(&p, &s);
    };
    // nLoopKF: the origin key-frame's id -> the in-place branch; any other -> the *GBA members
    const unsigned long nLoopKF = in_place ? map.origin->mnId : 77ul;
    gfs_host::GlobalBundleAdjustemnt<MockAccess>(solve, &map, iterations, pstop, nLoopKF, robust != 0);
    int n[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < n_poses; i++) {
      std::memcpy(out_pose_q + 4 * i, kfs[i].q, 16);
      std::memcpy(out_pose_t + 3 * i, kfs[i].t, 12);
      std::memcpy(out_gba_q + 4 * i, kfs[i].gba_q, 32);
      std::memcpy(out_gba_t + 3 * i, kfs[i].gba_t, 24);
      kf_gba_for[i] = (int32_t)kfs[i].mnBAGlobalForKF;
      n[0] += kfs[i].n_set_pose;
      n[1] += kfs[i].n_set_gba;
    }
    for (int j = 0; j < n_points; j++) {
      std::memcpy(out_points + 3 * j, mps[j].pos, 12);
      std::memcpy(out_points_gba + 3 * j, mps[j].pos_gba, 12);
      mp_gba_for[j] = (int32_t)mps[j].mnBAGlobalForKF;
      n[2] += mps[j].n_set_pos;
      n[3] += mps[j].n_set_gba;
      n[4] += mps[j].n_update;
    }
    for (int k = 0; k < 5; k++) counts[5 + k] = n[k];
    const MockMapPoint& lone = mps[n_points];
    counts[10] = lone.n_set_pos + lone.n_set_gba + lone.n_update;
    counts[11] = (int32_t)lone.mnBAGlobalForKF;
    return n_solves;
  } catch (const std::exception& ex) {
    fprintf(stderr, "gba_adaptor_test: %s\n", ex.what());
    return -1;
  }
}
