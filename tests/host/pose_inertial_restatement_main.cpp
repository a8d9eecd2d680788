// The PoseInertialOptimization restatement and the rule header as a program of its own, for a build under
// -fsanitize=address,undefined (CPU only; never loaded into python): a body at rest seen through n_obs = 0, 1, 6, 7, 65 and 300 visual
// edges in both modes, every buffer allocated at its exact size, with a NaN coordinate, a point behind the camera, a non-finite bias
// and an indefinite prior among them.  Prints one line a run, which tests/test_pose_inertial_restatement.py compares with the same
// program built without the sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pose_inertial_restatement.cpp"

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
  const int sizes[6] = {0, 1, 6, 7, 65, 300};
  for (int mode = 0; mode < 2; mode++)
    for (int n : sizes)
      for (int special = 0; special < 4; special++) {
        std::vector<double> xw(3 * n), obs(3 * n);
        std::vector<float> w(n);
        std::vector<uint8_t> st(n), close(n), outlier(n);
        const double fx = 607.0, cx = 319.5, cy = 239.5, bf = 45.0;
        for (int i = 0; i < n; i++) {
          const double z = 2.0 + (i * 37 % 11), x = ((i * 13) % 17 - 8) * 0.1 * z, y = ((i * 7) % 13 - 6) * 0.1 * z;
          xw[3 * i] = x, xw[3 * i + 1] = y, xw[3 * i + 2] = z;
          const double u = fx * x / z + cx, v = fx * y / z + cy, d = (i % 9 == 4) ? 30.0 : 0.3 * ((i % 5) - 2);  // every ninth a gross outlier
          st[i] = i % 3 != 0, close[i] = z < 10.0, w[i] = 1.0f / (1.0f + (i % 4));
          obs[3 * i] = u + d, obs[3 * i + 1] = v - d, obs[3 * i + 2] = st[i] ? u - bf / z + 0.1 * d : -1.0;
        }
        if (special == 1 && n > 1) xw[2] = -3.0, xw[3] = NAN;  // a point behind the camera, a NaN coordinate
        gfs_pose_inertial_problem p{};
        p.mode = mode, p.n_obs = n, p.n_rounds = 4, p.rec_init = special == 3;
        p.xw = xw.data(), p.obs = obs.data(), p.inv_sigma2 = w.data(), p.stereo = st.data(), p.close = close.data();
        p.fx = p.fy = fx, p.cx = cx, p.cy = cy, p.bf = bf;
        identity(p.Rcb), identity(p.Rbc);
        state(p.cur, 0.01), state(p.other, 0.0);
        if (special == 2) p.other.bg[1] = INFINITY;  // a non-finite gyro bias difference: the (1e-6, 1e-6, 1e-5) replacement
        identity_f(p.dR);
        p.dT = 0.05f;
        p.dV[2] = 9.81f * p.dT, p.dP[2] = 0.5f * 9.81f * p.dT * p.dT;
        for (int k = 0; k < 3; k++) p.JRg[4 * k] = -p.dT, p.JVa[4 * k] = -p.dT, p.JPa[4 * k] = -0.5f * p.dT * p.dT;
        for (int k = 0; k < 9; k++) p.info_inertial[10 * k] = k < 3 ? 1e6 : 1e4;
        for (int k = 0; k < 3; k++) p.info_gyro_rw[4 * k] = 1e8, p.info_acc_rw[4 * k] = 1e6;
        identity(p.prior_Rwb);
        for (int k = 0; k < 15; k++) p.prior_H[16 * k] = (special == 3 && k < 7) ? -1e12 : 1e4;  // special 3: an indefinite prior
        gfs_pose_inertial_solution s{};
        s.outlier = outlier.data();
        if (pir_optimize(&p, &s, nullptr)) return 1;
        unsigned long long sum = 0;
        for (uint8_t v : outlier) sum += v;
        const int D = mode ? 30 : 15;
        double tr = 0;
        for (int k = 0; k < D; k++) tr += s.H[D * k + k];
        printf("%d %d %d good %d inliers %d rounds %d outliers %llu twb %.17g trace %.17g\n", mode, n, special, s.n_good, s.n_inliers, s.rounds_run, sum,
               s.cur.twb[0], std::isnan(tr) ? 0.0 : tr);  // (the sign a NaN prints with is the compiler's)
      }
  gfs_pose_inertial_problem bad{};
  bad.n_rounds = 5;
  gfs_pose_inertial_solution s{};
  if (pir_optimize(&bad, &s, nullptr) != GFS_ERR_INVALID_ARG) return 2;
  printf("pose_inertial_restatement_main: ok\n");
  return 0;
}
