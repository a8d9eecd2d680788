// The PoseLidarVisualInertialOptimization restatement and the rule headers as a program of its own, for a build under
// -fsanitize=address,undefined (CPU only; never loaded into python): a body at rest in front of a wall and above a floor, seen through
// n_obs = 0, 2, 7 and 65 visual edges and clouds of 0, 49, 50 and 130 points in both modes, every buffer allocated at its exact size,
// with a NaN cloud point, a far map and one to four rounds among them.  Prints one line a run, which
// tests/test_pose_lidar_inertial_restatement.py compares with the same program built without the sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pose_lidar_inertial_restatement.cpp"

static void identity(double* R) {
  for (int i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.0 : 0.0;
}
static void identity_f(float* R) {
  for (int i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.0f : 0.0f;
}
static void state(gfs_imu_state& s, double x) {
  identity(s.Rwb), identity(s.Rcw);
  s.twb[0] = x, s.tcw[0] = -x;
}

int main() {
  // the map: a wall z = 4 and a floor y = 1, a 0.1 m lattice with a deterministic ripple of a few millimetres
  std::vector<float> map;
  for (int i = -20; i <= 20; i++)
    for (int j = -10; j <= 10; j++) {
      const float r = 0.002f * ((i * 7 + j * 13) % 5);
      map.insert(map.end(), {0.1f * i, 0.1f * j, 4.0f + r});
      map.insert(map.end(), {0.1f * i, 1.0f + r, 3.0f + 0.1f * j});
    }
  const int n_map = (int)map.size() / 3;
  const int sizes[4] = {0, 2, 7, 65}, clouds[4] = {0, 49, 50, 130};
  int line = 0;
  for (int mode = 0; mode < 2; mode++)
    for (int n : sizes)
      for (int nc : clouds)
        for (int special = 0; special < 3; special++) {
          std::vector<double> xw(3 * n), obs(3 * n);
          std::vector<float> w(n), cloud(3 * nc);
          std::vector<uint8_t> st(n), close(n), outlier(n);
          const double fx = 607.0, cx = 319.5, cy = 239.5, bf = 45.0;
          for (int i = 0; i < n; i++) {
            const double z = 2.0 + (i * 37 % 11), x = ((i * 13) % 17 - 8) * 0.1 * z, y = ((i * 7) % 13 - 6) * 0.1 * z;
            xw[3 * i] = x, xw[3 * i + 1] = y, xw[3 * i + 2] = z;
            const double u = fx * x / z + cx, v = fx * y / z + cy, d = (i % 9 == 4) ? 30.0 : 0.3 * ((i % 5) - 2);
            st[i] = i % 3 != 0, close[i] = z < 10.0, w[i] = 1.0f / (1.0f + (i % 4));
            obs[3 * i] = u + d, obs[3 * i + 1] = v - d, obs[3 * i + 2] = st[i] ? u - bf / z + 0.1 * d : -1.0;
          }
          for (int i = 0; i < nc; i++) {  // alternately on the wall and on the floor, seen from the true pose (the origin)
            const float a = 0.13f * ((i * 11) % 23 - 11), b = 0.07f * ((i * 5) % 19 - 9);
            if (i % 2) cloud[3 * i] = a, cloud[3 * i + 1] = b, cloud[3 * i + 2] = 4.0f;
            else cloud[3 * i] = a, cloud[3 * i + 1] = 1.0f, cloud[3 * i + 2] = 3.0f + b;
          }
          if (special == 1 && nc > 3) cloud[4] = NAN, cloud[9] = 1e9f;  // a NaN coordinate, a point far outside the map
          gfs_pose_lidar_inertial_problem q{};
          gfs_pose_inertial_problem& p = q.vi;
          p.mode = mode, p.n_obs = n, p.n_rounds = 1 + (line % 4), p.rec_init = 0;
          p.xw = xw.data(), p.obs = obs.data(), p.inv_sigma2 = w.data(), p.stereo = st.data(), p.close = close.data();
          p.fx = p.fy = fx, p.cx = cx, p.cy = cy, p.bf = bf;
          identity(p.Rcb), identity(p.Rbc);
          state(p.cur, 0.01), state(p.other, 0.0);
          identity_f(p.dR);
          p.dT = 0.05f;
          p.dV[2] = 9.81f * p.dT, p.dP[2] = 0.5f * 9.81f * p.dT * p.dT;
          for (int k = 0; k < 3; k++) p.JRg[4 * k] = -p.dT, p.JVa[4 * k] = -p.dT, p.JPa[4 * k] = -0.5f * p.dT * p.dT;
          for (int k = 0; k < 9; k++) p.info_inertial[10 * k] = k < 3 ? 1e6 : 1e4;
          for (int k = 0; k < 3; k++) p.info_gyro_rw[4 * k] = 1e8, p.info_acc_rw[4 * k] = 1e6;
          identity(p.prior_Rwb);
          for (int k = 0; k < 15; k++) p.prior_H[16 * k] = 1e4;
          q.q[3] = 1.0f, q.t[0] = -0.01f, q.tcb_q[3] = 1.0f;
          q.kf_time_gap = special == 2 ? 0.9 : 0.4;
          q.n_cloud = nc, q.cloud = cloud.data();
          std::vector<float> far_map(map);
          if (special == 2 && mode == 1)
            for (float& v : far_map) v += 40.0f;
          std::vector<int32_t> e_idx(4 * (size_t)nc);
          std::vector<float> e_plane(16 * (size_t)nc), e_s(4 * (size_t)nc);
          gfs_pose_lidar_inertial_solution s{};
          s.vi.outlier = outlier.data();
          if (plir_optimize(&q, far_map.data(), n_map, &s, nullptr, e_idx.data(), e_plane.data(), e_s.data())) return 1;
          unsigned long long sum = 0;
          for (uint8_t v : outlier) sum += v;
          const int D = mode ? 30 : 15;
          double tr = 0;
          for (int k = 0; k < D; k++) tr += s.vi.H[D * k + k];
          printf("%d %d %d %d rounds %d good %d outliers %llu edges %d %d %d %d valid %d residual %.9g twb %.17g trace %.17g\n", mode, n, nc, special,
                 s.vi.rounds_run, s.vi.n_good, sum, s.round_edges[0], s.round_edges[1], s.round_edges[2], s.round_edges[3], s.n_lidar_inliers,
                 (double)s.residual, s.vi.cur.twb[0], std::isnan(tr) ? 0.0 : tr);
          line++;
        }
  gfs_pose_lidar_inertial_problem bad{};
  bad.vi.n_rounds = 5;
  gfs_pose_lidar_inertial_solution s{};
  if (plir_optimize(&bad, nullptr, 0, &s, nullptr, nullptr, nullptr, nullptr) != GFS_ERR_INVALID_ARG) return 2;
  printf("pose_lidar_inertial_restatement_main: ok\n");
  return 0;
}
