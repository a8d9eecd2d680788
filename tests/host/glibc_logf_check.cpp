// Host-side check of gfs_glibc::logf (geoflowslam_amd/csrc/glibc_math.hpp) against this machine's libm on EVERY positive finite
// float (bit patterns 0x00000001 .. 0x7f7fffff) and on the special values.
// usage: glibc_logf_check [threads <= 16]  -> prints "logf <bad> of <count>"
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../geoflowslam_amd/csrc/glibc_math.hpp"

static bool same(float a, float b) { return (a != a && b != b) || memcmp(&a, &b, 4) == 0; }
static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  int nt = argc > 1 ? atoi(argv[1]) : (int)std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
  const uint32_t first = 1u, last = 0x7f7fffffu;
  std::atomic<long> bad{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; t++)
    pool.emplace_back([&, t] {
      const uint64_t n = (uint64_t)last - first + 1, a = first + n * t / nt, b = first + n * (t + 1) / nt;
      long mine = 0;
      for (uint64_t u = a; u < b; u++) {
        volatile float vx = from_bits((uint32_t)u);
        if (!same(::logf(vx), gfs_glibc::logf(from_bits((uint32_t)u)))) {
          if (mine++ < 3) printf("logf %a: %a vs %a\n", (double)vx, (double)::logf(vx), (double)gfs_glibc::logf(vx));
        }
      }
      bad += mine;
    });
  for (auto& th : pool) th.join();
  const float special[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, -1.0f, -1e-45f, -3.4e38f, 1.0f, 1.2f};
  for (float x : special) {
    volatile float vx = x;
    if (!same(::logf(vx), gfs_glibc::logf(x))) {
      printf("logf special %a: %a vs %a\n", (double)x, (double)::logf(vx), (double)gfs_glibc::logf(x));
      bad++;
    }
  }
  printf("logf %ld of %lu\n", bad.load(), (unsigned long)(last - first + 1) + sizeof(special) / sizeof(special[0]));
  return bad ? 1 : 0;
}
