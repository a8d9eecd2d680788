// Test harness for gfs_host::PoseInertialOptimizationLastKeyFrame / ...LastFrame (geoflowslam_amd/host/gfs_adaptors.hpp): plain-struct
// stand-ins for the members of Frame / KeyFrame / MapPoint / IMU::Preintegrated / ConstraintPoseImu that the two functions touch
// (reference src/Optimizer.cc:5899-6283, 6762-7171), filled from the caller's arrays.  The adaptor gathers, "solves" with a recorder
// that keeps the flattened problem as the solver saw it and answers with a scripted solution, and writes back; the caller gets both.
// Built by tests/test_pose_inertial_adaptor.py with g++.  No device.
#include <cstring>
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
struct MockMapPoint {
  float pos[3];
  float mTrackDepth;
};
struct MockPreintegrated {
  float tag;  // written into dT; the random-walk information carries it too, so that the test sees WHICH preintegration was read
};
struct MockConstraint {
  static int live;  // constructed - deleted
  double Rwb[9], twb[3], H00;
  int mode, made_by_adaptor;
  MockConstraint() { live++; }
  ~MockConstraint() { live--; }
};
int MockConstraint::live = 0;
struct MockKeyFrame {
  double tag;
};
struct MockFrame {
  int N = 0, Nleft = -1;
  bool pinhole = true;
  double tag = 0;
  std::vector<MockMapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  MockKeyFrame* mpLastKeyFrame = nullptr;
  MockFrame* mpPrevFrame = nullptr;
  MockPreintegrated *mpImuPreintegrated = nullptr, *mpImuPreintegratedFrame = nullptr;
  MockConstraint* mpcpi = nullptr;
  float f2f = -1.f, f2m = -1.f;
  gfs_imu_estimate written{};
  int n_written = 0;
  void SetFrame2FrameReprojError(float v) { f2f = v; }
  void SetFrame2MapReprojError(float v) { f2m = v; }
};
struct Access {
  static bool is_pinhole(const MockFrame* f) { return f->pinhole; }
  static void world_pos(const MockMapPoint* p, float X[3]) { memcpy(X, p->pos, sizeof(p->pos)); }
  static void calibration(const MockFrame*, gfs_pose_inertial_problem& P) { P.fx = 607.0, P.fy = 608.0, P.cx = 319.5, P.cy = 239.5, P.bf = 45.0; }
  static void state(const MockFrame* f, gfs_imu_state& s) { s.twb[0] = f->tag; }
  static void state(const MockKeyFrame* k, gfs_imu_state& s) { s.twb[0] = k->tag; }
  static void preintegration(const MockPreintegrated* p, gfs_pose_inertial_problem& P) { P.dT = p->tag; }
  static void random_walk_information(const MockPreintegrated* p, double* g, double* a) { g[0] = p->tag, a[0] = 2.0 * p->tag; }
  static void prior(const MockConstraint* c, gfs_pose_inertial_problem& P) { P.prior_H[0] = c->H00; }
  static void set_imu_pose_velocity_bias(MockFrame* f, const gfs_imu_estimate& e) { f->written = e, f->n_written++; }
  static MockConstraint* new_constraint(const gfs_imu_estimate& e, const double* H, int mode) {
    MockConstraint* c = new MockConstraint;
    memcpy(c->Rwb, e.Rwb, sizeof(e.Rwb)), memcpy(c->twb, e.twb, sizeof(e.twb));
    c->H00 = H[0], c->mode = mode, c->made_by_adaptor = 1;
    return c;
  }
};
}  // namespace

extern "C" {

// One call on a mock frame of N key-points.  has_mp / pos / depth / kp (x, y, octave as float) / u_right [N]; sigma [8].  kind: 0 as it
// is, 1 Nleft = 0, 2 not a pinhole, 3 no prior on the previous frame.  The recorder answers outlier[k] = scripted[k], n_good = 77,
// avg_reproj = 1.25, cur.twb = (5, 6, 7), H[0] = 42.
// Out: gathered n, idx-order arrays xw [n][3], obs [n][3], w [n], stereo [n], close [n]; head [12] = mode, n_rounds, rec_init, cur tag,
// other tag, dT, info_gyro[0], info_acc[0], prior_H[0], fx, bf, refused; back [10] = return value, f2f, f2m, written twb[0..2],
// n_written, new constraint's H00, its mode, live constraints after the call; outliers_after [N] (255 where untouched-false)
int pose_inertial_adaptor_test(int mode, int kind, int N, const uint8_t* has_mp, const float* pos, const float* depth, const float* kp,
                               const float* u_right, const float* sigma, const uint8_t* scripted, int rec_init, int f2f, int f2m, int n_rounds,
                               int* n_out, double* xw, double* obs, float* w, uint8_t* stereo, uint8_t* close, double* head, double* back,
                               uint8_t* outliers_after) {
  std::vector<MockMapPoint> mps((size_t)N);
  MockFrame F, prev;
  MockKeyFrame kf{11.0};
  MockPreintegrated pre_kf{0.4f}, pre_frame{0.05f};
  F.N = N, F.tag = 3.0, prev.tag = 2.0;
  F.Nleft = kind == 1 ? 0 : -1;
  F.pinhole = kind != 2;
  for (int i = 0; i < N; i++) {
    memcpy(mps[i].pos, pos + 3 * i, 3 * sizeof(float));
    mps[i].mTrackDepth = depth[i];
    F.mvpMapPoints.push_back(has_mp[i] ? &mps[i] : nullptr);
    F.mvbOutlier.push_back(true);  // the gather clears the flags of the edges it makes
    F.mvKeysUn.push_back(KeyPoint{{kp[3 * i], kp[3 * i + 1]}, (int)kp[3 * i + 2]});
    F.mvuRight.push_back(u_right[i]);
  }
  F.mvInvLevelSigma2.assign(sigma, sigma + 8);
  F.mpLastKeyFrame = &kf, F.mpPrevFrame = &prev, F.mpImuPreintegrated = &pre_kf, F.mpImuPreintegratedFrame = &pre_frame;
  MockConstraint::live = 0;
  if (kind != 3) {
    prev.mpcpi = new MockConstraint;
    prev.mpcpi->H00 = 9.0, prev.mpcpi->made_by_adaptor = 0;
  }
  int seen = 0;
  auto recorder = [&](const gfs_pose_inertial_problem& P, gfs_pose_inertial_solution& S) {
    seen++;
    *n_out = P.n_obs;
    memcpy(xw, P.xw, sizeof(double) * 3 * P.n_obs), memcpy(obs, P.obs, sizeof(double) * 3 * P.n_obs), memcpy(w, P.inv_sigma2, sizeof(float) * P.n_obs);
    memcpy(stereo, P.stereo, P.n_obs), memcpy(close, P.close, P.n_obs);
    const double hd[11] = {(double)P.mode, (double)P.n_rounds, (double)P.rec_init, P.cur.twb[0], P.other.twb[0], (double)P.dT, P.info_gyro_rw[0],
                           P.info_acc_rw[0], P.prior_H[0], P.fx, P.bf};
    memcpy(head, hd, sizeof(hd));
    for (int k = 0; k < P.n_obs; k++) S.outlier[k] = scripted[k];
    S.n_good = 77, S.avg_reproj = 1.25f, S.cur.twb[0] = 5, S.cur.twb[1] = 6, S.cur.twb[2] = 7, S.H[0] = 42.0;
  };
  head[11] = 0;
  int ret = -1;
  try {
    ret = mode == GFS_POSE_INERTIAL_LAST_FRAME
              ? gfs_host::PoseInertialOptimizationLastFrame<Access>(recorder, &F, rec_init != 0, f2f != 0, f2m != 0, n_rounds)
              : gfs_host::PoseInertialOptimizationLastKeyFrame<Access>(recorder, &F, rec_init != 0, f2f != 0, f2m != 0, n_rounds);
  } catch (const std::runtime_error&) {
    head[11] = 1;
  }
  back[0] = ret, back[1] = F.f2f, back[2] = F.f2m, back[3] = F.written.twb[0], back[4] = F.written.twb[1], back[5] = F.written.twb[2];
  back[6] = F.n_written, back[7] = F.mpcpi ? F.mpcpi->H00 : -1, back[8] = F.mpcpi ? F.mpcpi->mode : -1;
  for (int i = 0; i < N; i++) outliers_after[i] = F.mvbOutlier[i] ? 1 : 0;
  const bool prev_cleared = prev.mpcpi == nullptr;
  delete F.mpcpi;
  delete prev.mpcpi;
  back[9] = MockConstraint::live + (prev_cleared ? 100 : 0) + 1000 * seen;  // 0 live left; +100: the previous frame's prior was deleted and cleared
  return 0;
}

}  // extern "C"
