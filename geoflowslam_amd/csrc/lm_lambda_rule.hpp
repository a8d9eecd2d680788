// computeLambdaInit's maximum (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:175-184), host and device:
//   maxDiagonal = 0;  for every diagonal entry h, in order:  maxDiagonal = std::max(fabs(h), maxDiagonal);
// std::max(a, b) is (a < b) ? b : a, so a NaN |h| REPLACES the running maximum (fmax would drop it) and the next entry replaces a NaN
// maximum in turn: the result is NaN exactly when the last entry is NaN, else the maximum of the entries after the last NaN.
// Plain C++ (tests/host/lm_lambda_rule_check.cpp compiles it with g++); pose_lm_dev.hpp calls it for k_pose_opt and k_pl_round.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GFS_LMR_HD __host__ __device__ __forceinline__
#else
#define GFS_LMR_HD inline
#endif

namespace gfs_pose_lm {

// Hp: the lower triangle of an N x N, packed a (a + 1) / 2 + c (N = 7: the Sim3 block of k_sim3_opt, sim3_opt.hip)
template <int N>
GFS_LMR_HD double max_abs_diagonal(const double* Hp) {
  double maxDiagonal = 0;
  for (int a = 0; a < N; a++) {
    const double h = fabs(Hp[a * (a + 1) / 2 + a]);
    maxDiagonal = h < maxDiagonal ? maxDiagonal : h;
  }
  return maxDiagonal;
}
GFS_LMR_HD double max_abs_diagonal6(const double* H21) { return max_abs_diagonal<6>(H21); }

}  // namespace gfs_pose_lm
