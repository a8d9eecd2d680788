// The LocalInertialBA restatement and the rule header as a program of its own, for a build under -fsanitize=address,undefined (CPU
// only; never loaded into python): small windows of a body at rest -- 1, 2 and 3 key frames, 0 and 2 other fixed key frames, 1, 5 and
// 40 points -- every buffer allocated at its exact size, with a NaN observation, a point behind a camera, a point without edges and a
// negative-definite random-walk information (a failed factorisation) among them, and iterations = 0.  Prints one line a run, which
// tests/test_lba_inertial_restatement.py compares with the same program built without the sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "lba_inertial_restatement.cpp"

static void identity(double* R) {
  for (int i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.0 : 0.0;
}
static void state(gfs_imu_state& s, double x) {
  identity(s.Rwb), identity(s.Rcw);
  s.twb[0] = x, s.tcw[0] = -x;
}

int main() {
  const int windows[3] = {1, 2, 3}, fixed_counts[2] = {0, 2}, point_counts[3] = {1, 5, 40};
  for (int N : windows)
    for (int F : fixed_counts)
      for (int P : point_counts)
        for (int special = 0; special < 5; special++) {
          const int K = N + 1 + F;
          const double fx = 607.0, cx = 319.5, cy = 239.5, bf = 45.0;
          std::vector<gfs_imu_state> window(N), out_window(N);
          std::vector<uint8_t> imu(N, 1);
          std::vector<gfs_lba_inertial_edge> inertial(N);
          std::vector<double> fixed_Rcw(9 * F), fixed_tcw(3 * F), points(3 * P), obs;
          std::vector<int32_t> begin{0}, edge_kf;
          std::vector<float> w;
          std::vector<uint8_t> st, close;
          std::vector<double> cam_x(K);  // every camera looks along z from (x, 0, 0): x = 0.05 k, the estimates a little off
          for (int k = 0; k < K; k++) cam_x[k] = 0.05 * k;
          for (int i = 0; i < N; i++) state(window[i], cam_x[i] + 0.004 * (i + 1));
          gfs_lba_inertial_problem p{};
          state(p.prev, cam_x[N]);
          for (int k = 0; k < F; k++) identity(&fixed_Rcw[9 * k]), fixed_tcw[3 * k] = -cam_x[N + 1 + k];
          for (int i = 0; i < N; i++) {
            gfs_lba_inertial_edge& e = inertial[i];
            for (int k = 0; k < 9; k++) e.dR[k] = k % 4 == 0 ? 1.0f : 0.0f;
            e.dT = 0.4f;
            e.dP[0] = -0.05f;  // key frame i stands 0.05 in front of key frame i + 1 along -x
            e.dV[2] = 9.81f * e.dT, e.dP[2] = 0.5f * 9.81f * e.dT * e.dT;
            for (int k = 0; k < 3; k++) e.JRg[4 * k] = -e.dT, e.JVa[4 * k] = -e.dT, e.JPa[4 * k] = -0.5f * e.dT * e.dT;
            for (int k = 0; k < 9; k++) e.info_inertial[10 * k] = k < 3 ? 1e6 : 1e4;
            for (int k = 0; k < 3; k++) e.info_gyro_rw[4 * k] = 1e8, e.info_acc_rw[4 * k] = (special == 3 && i == 0) ? -1e12 : 1e6;
          }
          for (int l = 0; l < P; l++) {
            const double z = 2.0 + (l * 37 % 11), x = ((l * 13) % 17 - 8) * 0.1 * z, y = ((l * 7) % 13 - 6) * 0.1 * z;
            points[3 * l] = x + 0.01, points[3 * l + 1] = y - 0.01, points[3 * l + 2] = z + 0.02;
            if (!(special == 2 && l == 1))  // special 2: point 1 has no edge
              for (int k = 0; k < K; k++) {
                if ((l + k) % 3 == 2 && k != l % N) continue;
                const double u = fx * (x - cam_x[k]) / z + cx, v = fx * y / z + cy, d = ((l + k) % 9 == 4) ? 30.0 : 0.3 * ((l % 5) - 2);
                const bool stereo = (l + k) % 4 != 0;
                obs.push_back(u + d), obs.push_back(v - d), obs.push_back(stereo ? u - bf / z + 0.1 * d : -1.0);
                edge_kf.push_back(k), w.push_back(1.0f / (1.0f + (l % 4))), st.push_back(stereo), close.push_back(z < 10.0);
              }
            begin.push_back((int32_t)edge_kf.size());
          }
          if (special == 1 && !obs.empty()) obs[0] = NAN;                 // a NaN observation
          if (special == 2) points[2] = -3.0;                             // a point behind every camera
          const int E = (int)edge_kf.size();
          p.n_opt = N, p.n_fixed = F, p.n_points = P, p.n_edges = E, p.n_cameras = 1;
          p.iterations = special == 4 ? 0 : 8, p.lambda_init = 1.0;
          p.fx = p.fy = fx, p.cx = cx, p.cy = cy, p.bf = bf;
          identity(p.Rcb), identity(p.Rbc);
          p.window = window.data(), p.window_imu = imu.data(), p.fixed_Rcw = fixed_Rcw.data(), p.fixed_tcw = fixed_tcw.data();
          p.inertial = inertial.data(), p.points = points.data(), p.point_edge_begin = begin.data(), p.edge_kf = edge_kf.data();
          p.obs = obs.data(), p.inv_sigma2 = w.data(), p.stereo = st.data(), p.close = close.data();
          std::vector<double> out_points(3 * P), chi2(E);
          std::vector<uint8_t> dp(E), erase(E);
          gfs_lba_inertial_solution s{};
          s.window = out_window.data(), s.points = out_points.data(), s.edge_chi2 = chi2.data(), s.edge_depth_positive = dp.data();
          s.edge_erase = erase.data();
          const int cap = 80;
          std::vector<double> lam(cap), temp(cap), rho(cap);
          std::vector<int32_t> acc(cap), ok2(cap), iter(cap);
          int32_t n_trials = 0;
          LirTrace t{};
          t.cap = cap, t.n_trials = &n_trials, t.lambda = lam.data(), t.temp_chi = temp.data(), t.rho = rho.data(), t.accepted = acc.data();
          t.ok2 = ok2.data(), t.iteration = iter.data();
          if (lir_solve(&p, &s, &t)) return 1;
          unsigned long long erased = 0, positive = 0, failed = 0;
          for (uint8_t v : erase) erased += v;
          for (uint8_t v : dp) positive += v;
          for (int k = 0; k < n_trials; k++) failed += !ok2[k];
          printf("%d %d %d %d edges %d iterations %d trials %d failed %llu erased %llu positive %llu twb %.17g lambda %.17g\n", N, F, P, special, E,
                 s.iterations_run, s.trials_run, failed, erased, positive, std::isnan(s.window[0].twb[0]) ? 0.0 : s.window[0].twb[0], s.final_lambda);
        }
  gfs_lba_inertial_problem bad{};
  gfs_lba_inertial_solution s{};
  if (lir_solve(&bad, &s, nullptr) != GFS_ERR_INVALID_ARG) return 2;
  printf("lba_inertial_restatement_main: ok\n");
  return 0;
}
