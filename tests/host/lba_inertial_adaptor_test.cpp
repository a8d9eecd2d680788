// Test harness for gfs_host::LocalInertialBA (geoflowslam_amd/host/gfs_adaptors.hpp): plain-struct stand-ins for the members of
// KeyFrame / MapPoint / Map / IMU::Preintegrated that the function touches (reference src/Optimizer.cc:3056-3702), built from the
// caller's arrays.  The adaptor gathers, "solves" with a recorder that keeps the flattened problem as the solver saw it and answers
// with a scripted solution, and writes back; the caller gets both.  Built by tests/test_lba_inertial_adaptor.py with g++.  No device.
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

namespace {
struct Point2f {
  float x, y;
};
struct KeyPoint {
  Point2f pt;
  int octave;
};
struct MockMap {
  std::mutex mMutexMapUpdate;
  int n_keyframes = 0, change_index = 0;
  int KeyFramesInMap() const { return n_keyframes; }
  void IncreaseChangeIndex() { change_index++; }
};
struct MockPreintegrated {
  float tag, bias_set = -1.f;
  void SetNewBias(float b) { bias_set = b; }
};
struct MockKeyFrame;
struct MockMapPoint {
  int id = 0;
  unsigned long mnBALocalForKF = 0;
  float pos[3] = {0, 0, 0}, mTrackDepth = 0;
  bool bad = false;
  std::map<MockKeyFrame*, std::tuple<int, int>> obs;
  int normal_updates = 0;
  std::vector<int> erased_from;
  bool isBad() const { return bad; }
  std::map<MockKeyFrame*, std::tuple<int, int>> GetObservations() const { return obs; }
  void EraseObservation(MockKeyFrame* kf);
  void UpdateNormalAndDepth() { normal_updates++; }
};
struct MockKeyFrame {
  unsigned long mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
  MockKeyFrame* mPrevKF = nullptr;
  bool bImu = true, bad = false, pinhole = true;
  void* mpCamera2 = nullptr;
  MockPreintegrated* mpImuPreintegrated = nullptr;
  MockMap* map = nullptr;
  std::vector<MockMapPoint*> matches;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  float bias = 0;
  gfs_imu_state written{};
  int n_written = 0;
  std::vector<int> erased_matches;
  bool isBad() const { return bad; }
  MockMap* GetMap() const { return map; }
  std::vector<MockMapPoint*> GetMapPointMatches() const { return matches; }
  float GetImuBias() const { return bias; }
  void EraseMapPointMatch(MockMapPoint* p) { erased_matches.push_back(p->id); }
};
void MockMapPoint::EraseObservation(MockKeyFrame* kf) { erased_from.push_back((int)kf->mnId); }
struct Access {
  static bool is_pinhole(const MockKeyFrame* k) { return k->pinhole; }
  static void calibration(const MockKeyFrame*, gfs_lba_inertial_problem& P) { P.fx = 607.0, P.bf = 45.0; }
  static void state(const MockKeyFrame* k, gfs_imu_state& s) { s.twb[0] = (double)k->mnId, s.Rcw[0] = 100.0 + (double)k->mnId, s.tcw[0] = 200.0 + (double)k->mnId; }
  static void preintegration(const MockPreintegrated* p, gfs_lba_inertial_edge& e) { e.dT = p->tag, e.info_gyro_rw[0] = p->bias_set; }
  static void world_pos(const MockMapPoint* p, float X[3]) { memcpy(X, p->pos, sizeof(p->pos)); }
  static void set_world_pos(MockMapPoint* p, const double X[3]) {
    for (int k = 0; k < 3; k++) p->pos[k] = (float)X[k];
  }
  static void set_pose_velocity_bias(MockKeyFrame* k, const gfs_imu_state& s) { k->written = s, k->n_written++; }
};
}  // namespace

extern "C" {

// A map of K key frames chained by mPrevKF (id k + 1; key frame K - 1 is pKF; chain_break: that key frame has no mPrevKF) and M points.
// obs_kf / obs_idx [n_obs]: point obs_point[j] is seen from key frame obs_kf[j] at key-point obs_idx[j]; matches are listed per key frame
// in observation order.  kp [K][n_kp][3] (x, y, octave), u_right [K][n_kp].  flags: kind 0 as it is, 1 a second camera on key frame
// `who`, 2 key frame `who` without IMU, 3 key frame `who` bad, 4 pbICPFlag.  The recorder answers err / err_end as given,
// edge_erase[e] = scripted[e], window[i].twb[0] = 1000 + i, points[l] = (l, l, l) + 0.5.
// Out: head [12] = n_opt, n_fixed, n_points, n_edges, iterations, lambda, refused, returned, reference calls, solves, change index,
// prev id; window_ids [n_opt]; fixed_ids [n_fixed]; edge_kf / edge_point-id / stereo / close [n_edges], begin [n_points + 1],
// dT [n_opt], bias_seen [n_opt]; after: kf_marks [K][2], kf_written [K] (twb[0] or -1), point_pos0 [M], point_updates [M],
// n_erased, erased [..][2] (key frame id, point id)
int lba_inertial_adaptor_test(int K, int M, int n_kp, int n_keyframes_in_map, int chain_break, int n_obs, const int* obs_point, const int* obs_kf,
                              const int* obs_idx, const float* kp, const float* u_right, const float* depth, const uint8_t* point_bad, int kind,
                              int who, int large, float err, float err_end, const uint8_t* scripted, double* head, int* window_ids, int* fixed_ids,
                              int* edge_kf, int* edge_point, uint8_t* stereo, uint8_t* close, int* begin, float* dT, float* bias_seen, int* kf_marks,
                              double* kf_written, float* point_pos0, int* point_updates, int* n_erased, int* erased) {
  MockMap map;
  map.n_keyframes = n_keyframes_in_map;
  std::vector<MockKeyFrame> kfs((size_t)K);
  std::vector<MockPreintegrated> pre((size_t)K);
  std::vector<MockMapPoint> pts((size_t)M);
  const float sigma[8] = {1.f, .5f, .25f, .125f, .0625f, .03125f, .015625f, .0078125f};
  for (int k = 0; k < K; k++) {
    MockKeyFrame& f = kfs[(size_t)k];
    f.mnId = (unsigned long)k + 1, f.map = &map, f.bias = 10.f + (float)k;
    f.mPrevKF = (k > 0 && k != chain_break) ? &kfs[(size_t)k - 1] : nullptr;
    pre[(size_t)k].tag = 0.1f * (float)(k + 1);
    f.mpImuPreintegrated = &pre[(size_t)k];
    for (int j = 0; j < n_kp; j++) {
      const float* q = kp + 3 * ((size_t)k * n_kp + j);
      f.mvKeysUn.push_back(KeyPoint{{q[0], q[1]}, (int)q[2]});
      f.mvuRight.push_back(u_right[(size_t)k * n_kp + j]);
    }
    f.mvInvLevelSigma2.assign(sigma, sigma + 8);
  }
  for (int l = 0; l < M; l++) pts[(size_t)l].id = l, pts[(size_t)l].pos[0] = (float)l, pts[(size_t)l].mTrackDepth = depth[l], pts[(size_t)l].bad = point_bad[l] != 0;
  for (int j = 0; j < n_obs; j++) {
    pts[(size_t)obs_point[j]].obs[&kfs[(size_t)obs_kf[j]]] = std::make_tuple(obs_idx[j], -1);
    kfs[(size_t)obs_kf[j]].matches.push_back(&pts[(size_t)obs_point[j]]);
  }
  int dummy_camera = 0;
  if (kind == 1) kfs[(size_t)who].mpCamera2 = &dummy_camera;
  if (kind == 2) kfs[(size_t)who].bImu = false;
  if (kind == 3) kfs[(size_t)who].bad = true;
  std::map<const MockKeyFrame*, int> id_of;
  int solves = 0, reference_calls = 0;
  head[11] = -1;
  auto recorder = [&](const gfs_lba_inertial_problem& P, gfs_lba_inertial_solution& S) {
    solves++;
    head[0] = P.n_opt, head[1] = P.n_fixed, head[2] = P.n_points, head[3] = P.n_edges, head[4] = P.iterations, head[5] = P.lambda_init;
    head[11] = P.prev.twb[0];
    for (int i = 0; i < P.n_opt; i++) window_ids[i] = (int)P.window[i].twb[0], dT[i] = P.inertial[i].dT, bias_seen[i] = (float)P.inertial[i].info_gyro_rw[0];
    for (int k = 0; k < P.n_fixed; k++) fixed_ids[k] = (int)P.fixed_Rcw[9 * k] - 100;
    for (int e = 0; e < P.n_edges; e++) edge_kf[e] = P.edge_kf[e], stereo[e] = P.stereo[e], close[e] = P.close[e], S.edge_erase[e] = scripted[e];
    for (int l = 0; l <= P.n_points; l++) begin[l] = P.point_edge_begin[l];
    for (int l = 0; l < P.n_points; l++) {
      for (int e = P.point_edge_begin[l]; e < P.point_edge_begin[l + 1]; e++) edge_point[e] = (int)P.points[3 * l];
      for (int k = 0; k < 3; k++) S.points[3 * l + k] = P.points[3 * l] + 0.5;
    }
    for (int i = 0; i < P.n_opt; i++) S.window[i].twb[0] = 1000.0 + i;
    S.err = err, S.err_end = err_end;
  };
  auto reference = [&](MockKeyFrame*, bool*, bool, MockMap*, int&, int&, int&, int&, bool, bool) { reference_calls++; };
  int a = 0, b = 0, c = 0, d = 0;
  bool stop = false, ret = false;
  head[6] = 0;
  try {
    ret = gfs_host::LocalInertialBA<Access>(recorder, reference, &kfs[(size_t)K - 1], &stop, kind == 4, &map, a, b, c, d, large != 0, false);
  } catch (const std::runtime_error&) {
    head[6] = 1;
  }
  head[7] = ret ? 1 : 0, head[8] = reference_calls, head[9] = solves, head[10] = map.change_index;
  *n_erased = 0;
  for (int k = 0; k < K; k++) {
    kf_marks[2 * k] = (int)kfs[(size_t)k].mnBALocalForKF, kf_marks[2 * k + 1] = (int)kfs[(size_t)k].mnBAFixedForKF;
    kf_written[k] = kfs[(size_t)k].n_written ? kfs[(size_t)k].written.twb[0] : -1.0;
    for (int pid : kfs[(size_t)k].erased_matches) erased[2 * *n_erased] = k + 1, erased[2 * *n_erased + 1] = pid, (*n_erased)++;
  }
  for (int l = 0; l < M; l++) {
    point_pos0[l] = pts[(size_t)l].pos[0], point_updates[l] = pts[(size_t)l].normal_updates;
    for (int kid : pts[(size_t)l].erased_from) {  // every EraseObservation has its EraseMapPointMatch
      bool found = false;
      for (int q = 0; q < *n_erased; q++) found = found || (erased[2 * q] == kid && erased[2 * q + 1] == l);
      if (!found) return 1;
    }
  }
  return 0;
}

}  // extern "C"
