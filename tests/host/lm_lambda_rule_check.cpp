// Host check of geoflowslam_amd/csrc/lm_lambda_rule.hpp against the expression it restates, std::max(fabs(h), maxDiagonal) taken over
// the diagonal in order (g2o's computeLambdaInit): finite diagonals (signs, zeros, the maximum at every place), and a NaN first, in
// the middle, last, twice, and on every entry.  Equal means equal bits, or both NaN.
// Plain C++: g++ -std=c++17 -I <repo root>; exit code 0 and "ok" when all hold.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "geoflowslam_amd/csrc/lm_lambda_rule.hpp"

static double g2o_way(const double* d) {
  double maxDiagonal = 0.;
  for (int j = 0; j < 6; j++) maxDiagonal = std::max(std::fabs(d[j]), maxDiagonal);
  return maxDiagonal;
}
static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, 8) == 0; }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double base[6] = {3.0, -7.5, 0.0, 1e300, -2.0, 4.0};
  int bad = 0, checked = 0;
  auto check = [&](const double* d, const char* what) {
    double H21[21];
    for (int i = 0; i < 21; i++) H21[i] = 1e308;  // off-diagonal entries must not be read as diagonal ones
    for (int a = 0; a < 6; a++) H21[a * (a + 1) / 2 + a] = d[a];
    const double got = gfs_pose_lm::max_abs_diagonal6(H21), want = g2o_way(d);
    checked++;
    if (!same(got, want)) {
      bad++;
      printf("BAD %s: got %g want %g\n", what, got, want);
    }
    return got;
  };
  for (int rot = 0; rot < 6; rot++) {  // the maximum at every place
    double d[6];
    for (int a = 0; a < 6; a++) d[a] = base[(a + rot) % 6];
    if (check(d, "finite") != 1e300) bad++;
  }
  const double zeros[6] = {0.0, -0.0, 0.0, -0.0, 0.0, -0.0};
  const double z = check(zeros, "zeros");
  if (z != 0.0 || std::signbit(z)) bad++;
  for (int at = 0; at < 6; at++) {  // one NaN: kept only when it is last; before that, the maximum of what follows it
    double d[6];
    for (int a = 0; a < 6; a++) d[a] = a == at ? nan : base[a];
    const double got = check(d, "one NaN");
    double after = 0;
    for (int a = at + 1; a < 6; a++) after = std::fabs(d[a]) > after ? std::fabs(d[a]) : after;
    if (at == 5 ? !std::isnan(got) : got != after) {
      bad++;
      printf("BAD NaN at %d: got %g\n", at, got);
    }
  }
  const double two[6] = {nan, 5.0, nan, 2.0, -9.0, 1.0}, all[6] = {nan, nan, nan, nan, nan, nan}, infs[6] = {1.0, -inf, nan, 3.0, inf, 2.0};
  if (check(two, "two NaN") != 9.0) bad++;
  if (!std::isnan(check(all, "all NaN"))) bad++;
  if (check(infs, "inf and NaN") != inf) bad++;
  if (bad) return 1;
  printf("ok: %d diagonals\n", checked);
  return 0;
}
