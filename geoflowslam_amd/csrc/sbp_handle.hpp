// The gfs_sbp handle as sbp.hip, local_points.hip, fuse.hip, sim3_search.hip, triangulate.hip and bow_search.hip see it: device, stream, lock and capacities, the
// staging of gfs_search_by_projection*, and one slot per feature that reserves a workspace of its own (defined in the feature's file,
// allocated by its gfs_sbp_reserve_*, freed with the handle).
#pragma once
#include <memory>
#include <vector>

#include "block_layouts.hpp"
#include "sbp_dev.hpp"

struct gfs_sbp_workspace {  // what a feature reserves: defined in the feature's file, allocated by its gfs_sbp_reserve_*
  virtual ~gfs_sbp_workspace() = default;
};

struct gfs_sbp {
  int device, max_last, max_cur, max_batch;
  hipStream_t stream;
  std::mutex mu;
  // One pinned arena that mirrors one device block for the inputs, one for the results: a call is ONE copy in, the kernel, ONE copy
  // out (ten + two copies before -- ~10 us of host time and a copy-engine round trip each, twice the kernel's time for one frame).
  // The per-frame arrays are strided by the CALL's largest counts (rounded up to 64), not by the handle's capacity.
  gfs::Mirror in, res;
  gfs::DevBuf<int> d_cand_cnt, d_lsel;
  gfs::DevBuf<unsigned> d_cand;
  std::unique_ptr<gfs_sbp_workspace> local, fuse, tri, sim3, bow;  // local_points.hip, fuse.hip, triangulate.hip, sim3_search.hip, bow_search.hip
};

namespace gfs {

using SbpBlocks = SbpLayout<SbpPair>;

// ---- sbp.hip, for the entry points that stage a current frame and run k_sbp ----
// the call's stride of a per-frame array: the largest count of the call rounded up to 64, within the capacity
template <class Count>
int sbp_stride(int B, int cap, Count&& count) {
  int S = 64;
  for (int f = 0; f < B; f++) S = std::max(S, (int)align_up((size_t)std::max(count(f), 0), 64));
  return std::min(S, (int)align_up((size_t)cap, 64));
}
// the header of a map search (mode 1: ORBmatcher.cc:43-206) with n_last map points
template <class Problem>
void sbp_map_pair(SbpPair& S, const Problem& p, int n_last) {
  memset(&S, 0, sizeof(S));
  S.n_last = n_last;
  S.n_cur = p.n_cur;
  S.n_levels = p.n_levels;
  S.mode = 1;
  S.nn_ratio = p.nn_ratio;
  S.min_x = p.min_x;
  S.min_y = p.min_y;
  S.grid_w_inv = p.grid_w_inv;
  S.grid_h_inv = p.grid_h_inv;
  S.th = p.th;
  for (int k = 0; k < 16; k++) S.scale[k] = k < p.n_levels ? p.scale_factors[k] : 0.f;
}
// ---- triangulate.hip and bow_search.hip: a key frame's feature vector (gfs_tri_keyframe, gfs_bow_keyframe) ----
// From the node arrays on (the caller has checked the counts and that they are not NULL): node_start begins at 0 and is a prefix sum
// within n_kp, the node ids ascend, every listed feature is a key-point and is listed once.  `seen` is scratch.
template <class KF>
int check_feature_vector(const char* who, const KF& k, const char* what, int b, int i, std::vector<uint8_t>& seen) {
  GFS_REQUIRE(k.node_start[0] == 0, GFS_ERR_INVALID_ARG, "%s: problem %d %s %d: node_start[0] != 0", who, b, what, i);
  for (int n = 0; n < k.n_nodes; n++) {
    GFS_REQUIRE(n == 0 || k.node_id[n] > k.node_id[n - 1], GFS_ERR_INVALID_ARG, "%s: problem %d %s %d: node ids not ascending at %d", who, b, what, i, n);
    GFS_REQUIRE(k.node_start[n + 1] >= k.node_start[n] && k.node_start[n + 1] <= k.n_kp, GFS_ERR_INVALID_ARG,
                "%s: problem %d %s %d: node_start not a prefix sum within n_kp at %d", who, b, what, i, n);
  }
  const int nf = k.node_start[k.n_nodes];
  GFS_REQUIRE(nf == 0 || k.feat_idx, GFS_ERR_INVALID_ARG, "%s: problem %d %s %d has a NULL feature list", who, b, what, i);
  seen.assign((size_t)k.n_kp, 0);
  for (int p = 0; p < nf; p++) {
    const int f = k.feat_idx[p];
    GFS_REQUIRE(f >= 0 && f < k.n_kp, GFS_ERR_INVALID_ARG, "%s: problem %d %s %d: feature index %d outside [0, %d)", who, b, what, i, f, k.n_kp);
    GFS_REQUIRE(!seen[f], GFS_ERR_INVALID_ARG, "%s: problem %d %s %d: feature index %d listed twice", who, b, what, i, f);
    seen[f] = 1;
  }
  return GFS_OK;
}
// copies frame f's key-point arrays into the pinned input block
void sbp_stage_cur(gfs_sbp* h, const SbpBlocks& Y, int f, int n_cur, const gfs_keypoint* kps, const float* u_right, const uint8_t* desc,
                   const uint8_t* has_mp_obs);
// launches k_sbp on the device input block; cur_match [B][Y.SC] and nmatches [B] are device pointers
int sbp_launch(gfs_sbp* h, int B, const SbpBlocks& Y, int* cur_match, int* nmatches);

}  // namespace gfs
