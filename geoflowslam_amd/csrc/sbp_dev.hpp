// Device pieces the matcher kernels of sbp.hip, local_points.hip and fuse.hip share: the frame grid, the LDS capacity of a frame's
// key-points, the pair header k_sbp reads (k_lp_compact patches its n_last) and the descriptor distance.
#pragma once
#include "gfs_common.hpp"

namespace gfs {

constexpr int kGridCols = 64, kGridRows = 48, kCells = kGridCols * kGridRows;  // include/Frame.h FRAME_GRID_COLS / ROWS
constexpr int kSbpMaxCur = 4096;                                               // key-points of the current frame (LDS tables)

struct SbpPair {
  int n_last, n_cur, n_levels, mono, check_orientation;
  int mode;  // 0 = frame to frame (:1853-2063), 1 = map points with Frame::isInFrustum projections (:43-206)
  float nn_ratio;
  float Tcw_q[4], Tcw_t[3], Tlw_q[4], Tlw_t[3];
  float fx, fy, cx, cy, bf, b, min_x, max_x, min_y, max_y, grid_w_inv, grid_h_inv, th;
  float scale[16];
};

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

}  // namespace gfs
