// The Sim3Solver restatement and the rule header as a program of its own, for a build under -fsanitize=address,undefined (CPU only;
// never loaded into python): N = 3 (the sampling empties its list's tail), N = 4 and 65, draws at both ends of their ranges, a
// degenerate triple, NaN and inf coordinates, z = 0, the too-few exit, both scale modes, with and without the early stop; every
// buffer allocated at its exact size.  Prints the solutions' byte sums, which tests/test_sim3_ransac_restatement.py compares with the
// same calls through the shared library.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sim3_ransac_restatement.cpp"

static float coord(int i, int k) { return (float)(((i * 37 + k * 11) % 29) / 7.0 - 2.0 + (k == 2 ? 4.5 : 0.0)); }

int main() {
  const int sizes[4] = {2, 3, 4, 65};
  for (int n : sizes)
    for (int fix = 0; fix < 2; fix++)
      for (int special = 0; special < 3; special++) {
        std::vector<float> x1(3 * n), x2(3 * n), m1(n), m2(n);
        for (int i = 0; i < n; i++) {
          for (int k = 0; k < 3; k++) {
            x2[3 * i + k] = coord(i, k);
            x1[3 * i + k] = 1.25f * coord(i, (k + 1) % 3 == 2 ? 2 : k) + 0.1f * k;  // not a rigid image: some pairs are outliers
          }
          m1[i] = (float)(13 + 7 * (i % 5));
          m2[i] = (float)(19 + 3 * (i % 7));
        }
        if (special == 1 && n > 2) {
          x1[0] = NAN;
          x2[4] = INFINITY;
          x2[3 * (n - 1) + 2] = 0.0f;
        }
        if (special == 2 && n > 3)
          for (int k = 0; k < 3; k++) x1[3 + k] = x1[k], x2[3 + k] = x2[k];  // two identical points
        const int H = 12;
        std::vector<int32_t> draws(3 * H);
        for (int it = 0; it < H; it++)
          for (int k = 0; k < 3; k++) {
            const int d = n - k > 0 ? n - k : 1;
            draws[3 * it + k] = it == 0 ? 0 : it == 1 ? d - 1 : (it * 7 + k * 5) % d;
          }
        gfs_sim3_ransac_problem p{};
        p.n_pairs = n;
        p.x3d_c1 = x1.data(), p.x3d_c2 = x2.data(), p.max_err1 = m1.data(), p.max_err2 = m2.data();
        p.fx1 = p.fy1 = 607.0f, p.cx1 = 319.5f, p.cy1 = 239.5f;
        p.fx2 = p.fy2 = 910.5f, p.cx2 = 639.5f, p.cy2 = 359.5f;
        p.fix_scale = fix, p.min_inliers = n > 3 ? 3 : n, p.n_iterations = H, p.draws = draws.data();
        for (int early = 0; early < 2; early++) {
          std::vector<uint8_t> mask(n);
          std::vector<int32_t> counts(H, -1);
          std::vector<float> e1(n), e2(n);
          gfs_sim3_ransac_solution s{};
          s.inlier = mask.data(), s.counts = counts.data();
          if (s3rr_solve(&p, early, &s, e1.data(), e2.data())) return 1;
          unsigned long long sum = 0;
          const unsigned char* b = reinterpret_cast<const unsigned char*>(&s);
          for (size_t k = 0; k < offsetof(gfs_sim3_ransac_solution, inlier); k++) sum += b[k];
          for (uint8_t v : mask) sum += v;
          printf("%d %d %d %d %d %d %d %llu\n", n, fix, special, early, s.status, s.iterations, s.n_inliers, sum);
        }
      }
  // the pick and the sampling at their smallest sizes
  const int32_t c1[1] = {0};
  int32_t out[3];
  s3rr_pick(c1, 1, 0, out);
  const int32_t r[3] = {2, 1, 0};
  int32_t idx[3];
  s3rr_resolve_draws(3, r, idx);
  printf("%d %d %d %d %d %d\n", out[0], out[1], out[2], idx[0], idx[1], idx[2]);
  printf("iterations %d %d %d\n", s3rr_iterations(20, 0.99, 15, 300), s3rr_iterations(10, 0.99, 15, 300), s3rr_iterations(0, 0.99, 15, 300));
  printf("sim3_ransac_restatement_main: ok\n");
  return 0;
}
