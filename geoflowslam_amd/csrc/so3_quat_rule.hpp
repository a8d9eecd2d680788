// The rotation matrix of a unit quaternion, computed in double and rounded to float once per entry: the written rule that stands for
// Sophus::SO3f::exp(v).matrix() wherever the reference calls it (rule B of sim3_ransac_rule.hpp, rule E of pose_inertial_rule.hpp).
// Stated once so that both rules share the bits.
#pragma once

#if !defined(GFS_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFS_HD __host__ __device__ inline
#else
#define GFS_HD inline
#endif
#endif

namespace gfs_so3 {

GFS_HD void quaternion_matrix(const double* q, float* R) {  // q = (w, x, y, z); R row-major
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = (float)(1.0 - 2.0 * (y * y + z * z));
  R[1] = (float)(2.0 * (x * y - w * z));
  R[2] = (float)(2.0 * (x * z + w * y));
  R[3] = (float)(2.0 * (x * y + w * z));
  R[4] = (float)(1.0 - 2.0 * (x * x + z * z));
  R[5] = (float)(2.0 * (y * z - w * x));
  R[6] = (float)(2.0 * (x * z - w * y));
  R[7] = (float)(2.0 * (y * z + w * x));
  R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
}

}  // namespace gfs_so3
