// Test harness for gfs_host::LocalVisualLidarBA and LocalBundleAdjuster::LocalVisualLidarBA (geoflowslam_amd/host/gfs_adaptors.hpp):
// the plain-struct stand-ins of tests/host/lba_adaptor_test.cpp, plus per key-frame mnMatchesInliers and a downsampled cloud.  The
// adaptor gathers, solves (the CPU restatement tests/host/lba_lidar_restatement.cpp through dlopen, recording what it was handed and
// what it returned; or the GPU library with the adaptor's owned map) and writes back.  Built by tests/test_lba_lidar_adaptor.py.
#include "lba_adaptor_test.cpp"

namespace {
const MockKeyFrame* g_base = nullptr;
const int32_t *g_inliers = nullptr, *g_cloud_begin = nullptr;
const float* g_cloud = nullptr;
struct LidarAccess : MockAccess {
  static int matches_inliers(const MockKeyFrame* k) { return g_inliers[k - g_base]; }
  static const float* cloud(const MockKeyFrame* k, int* n) {
    const long i = k - g_base;
    *n = g_cloud_begin[i + 1] - g_cloud_begin[i];
    return g_cloud + 3 * (size_t)g_cloud_begin[i];
  }
};
}  // namespace

// counts: num_fixedKF, num_OptKF, num_edges, change_index, erased, SetPose calls, UpdateNormalAndDepth calls, lidar edges (CPU solver).
// seen_sizes: n_poses, n_points, n_edges, cloud points handed to the solver (CPU solver only, like every seen_* / sol_* array).
extern "C" int lba_lidar_adaptor_test(const char* solver_lib, int n_poses, int n_points, int n_edges, const double* pose_q, const double* pose_t,
                                      const uint8_t* pose_fixed, const double* points, const int32_t* edge_pose, const int32_t* edge_point,
                                      const double* edge_obs, const double* edge_inv_sigma2, const uint8_t* edge_stereo, double fx, double fy,
                                      double cx, double cy, double bf, int init_kf_pose, int stop_flag, const int32_t* matches_inliers,
                                      const int32_t* cloud_begin, const float* cloud, const float* map_xyz, int n_map, float* out_pose_q,
                                      float* out_pose_t, float* out_points, int32_t* erased_pairs, int32_t* counts, double* seen_pose_t,
                                      double* seen_points, int32_t* seen_sizes, uint8_t* seen_pose_local, int32_t* seen_inliers,
                                      int32_t* seen_cloud_begin, float* seen_cloud, int32_t* seen_edge_pose, int32_t* seen_edge_point,
                                      double* sol_pose_q, double* sol_pose_t, double* sol_points, double* sol_edge_chi2, uint8_t* sol_depth,
                                      int32_t* sol_pose_lidar_edges) {
  try {
    MockMap map;
    std::vector<MockKeyFrame> kfs((size_t)n_poses);
    std::vector<MockMapPoint> mps((size_t)n_points);
    int pkf = -1;
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
      if (!pose_fixed[i] && pkf < 0) pkf = i;
    }
    if (pkf < 0) return -100;
    for (int i = 0; i < n_poses; i++)
      if (!pose_fixed[i] && i != pkf) kfs[pkf].covisible.push_back(&kfs[i]);
    if (init_kf_pose >= 0) map.init_id = kfs[init_kf_pose].mnId;
    for (int j = 0; j < n_points; j++) {
      mps[j].mnId = 1000 + (unsigned long)j;
      mps[j].map = &map;
      for (int c = 0; c < 3; c++) mps[j].pos[c] = (float)points[3 * j + c];
    }
    for (int e = 0; e < n_edges; e++) {
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
      k.mvpMapPoints.push_back(&mps[edge_point[e]]);
      mps[edge_point[e]].obs[&k] = std::make_tuple(kp, -1);
    }
    g_base = kfs.data();
    g_inliers = matches_inliers;
    g_cloud_begin = cloud_begin;
    g_cloud = cloud;
    bool stop = stop_flag != 0;
    int num_fixedKF = -1, num_OptKF = -1, num_MPs = -7, num_edges = -1;
    counts[7] = -1;
    if (solver_lib) {  // the CPU restatement: int lblr_solve(problem, lidar, map, n_map, solution, pose_edges, idx, plane, s)
      void* so = dlopen(solver_lib, RTLD_NOW | RTLD_LOCAL);
      if (!so) return -101;
      typedef int (*fn_t)(const gfs_lba_problem*, const gfs_lba_lidar*, const float*, int, gfs_lba_solution*, int32_t*, int32_t*, float*, float*);
      fn_t fn = (fn_t)dlsym(so, "lblr_solve");
      if (!fn) return -102;
      gfs_host::LocalVisualLidarBA<LidarAccess, MockKeyFrame, MockMapPoint, MockMap>(
          [&](const gfs_lba_problem& p, const gfs_lba_lidar& L, gfs_lba_solution& s, const bool*) {
            const int nc = L.cloud_begin[p.n_poses];
            seen_sizes[0] = p.n_poses;
            seen_sizes[1] = p.n_points;
            seen_sizes[2] = p.n_edges;
            seen_sizes[3] = nc;
            std::memcpy(seen_pose_t, p.pose_t, (size_t)p.n_poses * 24);
            std::memcpy(seen_points, p.points, (size_t)p.n_points * 24);
            std::memcpy(seen_pose_local, L.pose_local, (size_t)p.n_poses);
            std::memcpy(seen_inliers, L.matches_inliers, (size_t)p.n_poses * 4);
            std::memcpy(seen_cloud_begin, L.cloud_begin, (size_t)(p.n_poses + 1) * 4);
            std::memcpy(seen_cloud, L.cloud, (size_t)nc * 12);
            std::memcpy(seen_edge_pose, p.edge_pose, (size_t)p.n_edges * 4);
            std::memcpy(seen_edge_point, p.edge_point, (size_t)p.n_edges * 4);
            counts[7] = fn(&p, &L, map_xyz, n_map, &s, sol_pose_lidar_edges, nullptr, nullptr, nullptr);
            std::memcpy(sol_pose_q, s.pose_q, (size_t)p.n_poses * 32);
            std::memcpy(sol_pose_t, s.pose_t, (size_t)p.n_poses * 24);
            std::memcpy(sol_points, s.points, (size_t)p.n_points * 24);
            std::memcpy(sol_edge_chi2, s.edge_chi2, (size_t)p.n_edges * 8);
            std::memcpy(sol_depth, s.edge_depth_positive, (size_t)p.n_edges);
            return true;
          },
          &kfs[pkf], &stop, &map, num_fixedKF, num_OptKF, num_MPs, num_edges);
    } else {
      gfs_host::LocalBundleAdjuster lba(std::max(n_poses, 8), std::max(n_points, 64), std::max(n_edges, 64));
      lba.LocalVisualLidarBA<LidarAccess>(&kfs[pkf], map_xyz, n_map, &stop, &map, num_fixedKF, num_OptKF, num_MPs, num_edges);
    }
    for (int i = 0; i < n_poses; i++) {
      std::memcpy(out_pose_q + 4 * i, kfs[i].q, 16);
      std::memcpy(out_pose_t + 3 * i, kfs[i].t, 12);
    }
    for (int j = 0; j < n_points; j++) std::memcpy(out_points + 3 * j, mps[j].pos, 12);
    int ner = 0;
    for (int e = 0; e < n_edges; e++) {
      MockKeyFrame& k = kfs[edge_pose[e]];
      if (mps[edge_point[e]].obs.find(&k) == mps[edge_point[e]].obs.end()) {
        erased_pairs[2 * ner] = edge_pose[e];
        erased_pairs[2 * ner + 1] = edge_point[e];
        ner++;
      }
    }
    int n_set = 0, n_upd = 0;
    for (auto& k : kfs) n_set += k.n_set_pose;
    for (auto& m : mps) n_upd += m.n_update;
    counts[0] = num_fixedKF;
    counts[1] = num_OptKF;
    counts[2] = num_edges;
    counts[3] = map.change_index;
    counts[4] = ner;
    counts[5] = n_set;
    counts[6] = n_upd;
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "lba_lidar_adaptor_test: %s\n", ex.what());
    return -1;
  }
}
