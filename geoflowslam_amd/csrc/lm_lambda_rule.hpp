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

// H21: the lower triangle of a 6x6, packed a (a + 1) / 2 + c
GFS_LMR_HD double max_abs_diagonal6(const double* H21) {
  double maxDiagonal = 0;
  for (int a = 0; a < 6; a++) {
    const double h = fabs(H21[a * (a + 1) / 2 + a]);
    maxDiagonal = h < maxDiagonal ? maxDiagonal : h;
  }
  return maxDiagonal;
}

}  // namespace gfs_pose_lm
