// Structure lists of the global bundle adjustment's Schur complement (gfs_gba_solve), built once per solve on the host: the graph does
// not change between iterations.  Plain C++, no HIP: tests/test_gba_lists.py checks it on the CPU through gfs_test_gba_lists.
//
// Edges are numbered landmark-major (the stable order gfs_lba_solve's preparation gives them: edges of landmark 0 first, each
// landmark's edges in the caller's order).  With f(e) the free-pose index of edge e's pose (-1: a fixed pose, which enters no list):
//   blocks   the lower 6 x 6 blocks (i >= j) of the reduced system that receive a term, in (i, j) order: EVERY diagonal block (i, i)
//            -- Hpp_i + lambda I is there whether pose i sees a landmark or not -- and every pair i > j with a common landmark;
//   contrib  per block, the pairs (e1, e2) with f(e1) = i, f(e2) = j on the same landmark, ordered by landmark, then by e1, then
//            by e2.  A diagonal block gets every combination of its pose's edges on the landmark, (e, e) and both orders of two
//            different edges, exactly as the e1 x e2 loops of BlockSolver's Schur product visit them (several edges may join one
//            pose and one point);
//   pose     per free pose, its edges in ascending order: the terms of the right-hand side bs_i.
// Counting sort: one pass counts the terms of every block of the packed lower triangle, a prefix sum turns the counts of the blocks
// that occur into offsets, a second pass in the same order fills the lists.  All counts are 64-bit.
#pragma once
#include <cstdint>
#include <vector>

namespace gba_sys {

struct Lists {
  std::vector<int32_t> blk_i, blk_j;        // [n_blocks]
  std::vector<int64_t> blk_begin;           // [n_blocks + 1] into contrib
  std::vector<int32_t> contrib;             // [n_contrib][2]: e1, e2
  std::vector<int64_t> pose_begin;          // [n_free + 1] into pose_edges
  std::vector<int32_t> pose_edges;
  std::vector<int64_t> slot;                // work: packed lower-triangle index -> count, then fill position
  int64_t n_blocks() const { return (int64_t)blk_i.size(); }
  int64_t n_contrib() const { return (int64_t)(contrib.size() / 2); }
};

inline int64_t tri64(int64_t i, int64_t j) { return i * (i + 1) / 2 + j; }

// pt_begin [n_points + 1]: the landmark-major edge ranges; e_free [n_edges]: f(e)
inline void build_lists(int64_t n_free, int64_t n_points, const int32_t* pt_begin, const int32_t* e_free, Lists& L) {
  const int64_t F = n_free, n_edges = n_points > 0 ? pt_begin[n_points] : 0;
  L.slot.assign((size_t)tri64(F, 0) + 1, 0);
  L.pose_begin.assign((size_t)F + 1, 0);
  auto for_each_term = [&](auto&& f) {
    for (int64_t l = 0; l < n_points; l++)
      for (int32_t e1 = pt_begin[l]; e1 < pt_begin[l + 1]; e1++) {
        const int64_t i = e_free[e1];
        if (i < 0) continue;
        for (int32_t e2 = pt_begin[l]; e2 < pt_begin[l + 1]; e2++) {
          const int64_t j = e_free[e2];
          if (j >= 0 && j <= i) f(tri64(i, j), e1, e2);
        }
      }
  };
  for_each_term([&](int64_t t, int32_t, int32_t) { L.slot[(size_t)t]++; });
  L.blk_i.clear();
  L.blk_j.clear();
  L.blk_begin.clear();
  int64_t at = 0;
  for (int64_t i = 0; i < F; i++)
    for (int64_t j = 0; j <= i; j++) {
      int64_t& s = L.slot[(size_t)tri64(i, j)];
      const int64_t cnt = s;
      s = at;  // from here on: where the block's next term goes
      if (cnt == 0 && i != j) continue;
      L.blk_i.push_back((int32_t)i);
      L.blk_j.push_back((int32_t)j);
      L.blk_begin.push_back(at);
      at += cnt;
    }
  L.blk_begin.push_back(at);
  L.contrib.assign((size_t)(2 * at), 0);
  for_each_term([&](int64_t t, int32_t e1, int32_t e2) {
    const int64_t k = L.slot[(size_t)t]++;
    L.contrib[(size_t)(2 * k)] = e1;
    L.contrib[(size_t)(2 * k + 1)] = e2;
  });
  for (int64_t e = 0; e < n_edges; e++)
    if (e_free[e] >= 0) L.pose_begin[(size_t)e_free[e] + 1]++;
  for (int64_t f = 0; f < F; f++) L.pose_begin[(size_t)f + 1] += L.pose_begin[(size_t)f];
  L.pose_edges.assign((size_t)L.pose_begin[(size_t)F], 0);
  std::vector<int64_t> pos(L.pose_begin.begin(), L.pose_begin.end() - 1);
  for (int64_t e = 0; e < n_edges; e++)
    if (e_free[e] >= 0) L.pose_edges[(size_t)pos[(size_t)e_free[e]]++] = (int32_t)e;
}

// The landmark-major numbering itself, for callers that hold a caller-order problem (the test hook): order[k] = caller's edge at
// landmark-major position k (stable), pt_begin and e_free as build_lists takes them.  Returns the number of free poses.
inline int64_t landmark_major(int64_t n_poses, int64_t n_points, int64_t n_edges, const uint8_t* pose_fixed, const int32_t* edge_pose,
                              const int32_t* edge_point, std::vector<int32_t>& order, std::vector<int32_t>& pt_begin,
                              std::vector<int32_t>& e_free) {
  std::vector<int32_t> free_index((size_t)n_poses, -1);
  int64_t F = 0;
  for (int64_t i = 0; i < n_poses; i++)
    if (!pose_fixed[i]) free_index[(size_t)i] = (int32_t)F++;
  pt_begin.assign((size_t)n_points + 1, 0);
  for (int64_t e = 0; e < n_edges; e++) pt_begin[(size_t)edge_point[e] + 1]++;
  for (int64_t l = 0; l < n_points; l++) pt_begin[(size_t)l + 1] += pt_begin[(size_t)l];
  std::vector<int32_t> pos(pt_begin.begin(), pt_begin.end() - 1);
  order.assign((size_t)n_edges, 0);
  e_free.assign((size_t)n_edges, -1);
  for (int64_t e = 0; e < n_edges; e++) {
    const int32_t k = pos[(size_t)edge_point[e]]++;
    order[(size_t)k] = (int32_t)e;
    e_free[(size_t)k] = free_index[(size_t)edge_pose[e]];
  }
  return F;
}

}  // namespace gba_sys
