// Host-side check of gfs_glibc::exp (geoflowslam_amd/csrc/glibc_math.hpp) against this machine's libm (glibc 2.35, FMA variant).
// usage: glibc_exp_check N  -> prints "exp <bad> of <N>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../geoflowslam_amd/csrc/glibc_math.hpp"

static bool same(double a, double b) { return (a != a && b != b) || memcmp(&a, &b, 8) == 0; }

int main(int argc, char** argv) {
  const long N = argc > 1 ? atol(argv[1]) : 1000000;
  uint64_t st = 88172645463325252ull;
  long bad = 0;
  auto check = [&](double x) {
    volatile double vx = x;
    if (!same(std::exp(vx), gfs_glibc::exp(x))) { if (bad++ < 5) printf("exp %a: %a vs %a\n", x, std::exp(vx), gfs_glibc::exp(x)); }
  };
  // the arguments OptimizeSim3 makes: +-1e-9 (the numeric Jacobian's step), 0 (fixed scale), and the small scale updates of a trial
  const double special[] = {0.0, -0.0, 1e-9, -1e-9, 1.0, -1.0, 1e-5, -1e-5, 9.9999e-6, 0.05, -0.05, 0x1p-54, -0x1p-54, 0x1p-55, 5e-324, -5e-324,
                            2.2250738585072014e-308, 709.0, 709.78, 709.79, 710.0, -708.0, -708.4, -745.0, -745.2, -746.0, 1e300, -1e300, 512.0,
                            -512.0, 1024.0, -1024.0, INFINITY, -INFINITY, NAN, 0.5, 2.0, 0.6931471805599453};
  for (double x : special) check(x);
  for (long i = 0; i < N; i++) {
    st ^= st << 13; st ^= st >> 7; st ^= st << 17;
    double x = ((st >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0);
    const int mode = i & 3;
    if (mode == 1) x = ldexp(x, -(int)((st >> 3) & 63));  // down to 2^-64: the tiny updates of a converged solve
    if (mode == 2) x *= 750.0;                            // through overflow, underflow and the subnormal results
    if (mode == 3) x *= 1e-8;                             // around the numeric step
    check(x);
  }
  printf("exp %ld of %ld\n", bad, N);
  return bad ? 1 : 0;
}
