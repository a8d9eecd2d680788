// Structure lists of the essential graph's pose system (gfs_essential_graph_optimize), built once per call on the host: the graph
// does not change between iterations.  Plain C++, no HIP: tests/test_pose_graph_lists.py checks it on the CPU through
// gfs_test_essential_graph_lists.
//
// With f(v) the free slot of vertex v (-1: fixed; free vertices are numbered in vertex order) an edge e = (i, j) gives
//   block (f(i), f(i))  4 e + 0   its J_i^T J_i          when i is free
//   block (f(j), f(j))  4 e + 1   its J_j^T J_j          when j is free
//   block (f(i), f(j))  4 e + 2   its J_i^T J_j          when both are free and f(i) > f(j)
//   block (f(j), f(i))  4 e + 3   ... transposed         when both are free and f(i) < f(j)
// blocks: the lower blocks (bi >= bj) that receive a term, in (bi, bj) order, and EVERY diagonal block -- lambda I is there whether
// the vertex has an edge or not.  Per block the terms in edge order (duplicate edges of one pair add up in the order they were
// made); on a diagonal block that list is also the list of the right-hand side's terms.  An edge between two fixed vertices enters
// no list.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace eg_sys {

struct Lists {
  std::vector<int32_t> free_index, free_vert;  // [n_vertices], [n_free]
  std::vector<int32_t> blk_i, blk_j;           // [n_blocks]
  std::vector<int64_t> blk_begin;              // [n_blocks + 1] into contrib
  std::vector<int32_t> contrib;                // 4 e + kind
  std::vector<int64_t> key;                    // work
  std::vector<int32_t> order;
  int64_t n_free() const { return (int64_t)free_vert.size(); }
  int64_t n_blocks() const { return (int64_t)blk_i.size(); }
  int64_t n_contrib() const { return (int64_t)contrib.size(); }
};

// edges with i == j or an index outside [0, n_vertices) are the caller's to refuse
inline void build_lists(int64_t n_vertices, int64_t n_edges, const uint8_t* fixed, const int32_t* edge_i, const int32_t* edge_j, Lists& L) {
  L.free_index.assign((size_t)n_vertices, -1);
  L.free_vert.clear();
  for (int64_t v = 0; v < n_vertices; v++)
    if (!fixed[v]) {
      L.free_index[(size_t)v] = (int32_t)L.free_vert.size();
      L.free_vert.push_back((int32_t)v);
    }
  const int64_t F = L.n_free();
  // one (block, term) pair per term, made in edge order, and a term-less pair per diagonal block in front of them; a stable sort by
  // block keeps the edge order inside every block
  L.key.clear();
  L.contrib.clear();
  for (int64_t f = 0; f < F; f++) {
    L.key.push_back(f * F + f);
    L.contrib.push_back(-1);
  }
  for (int64_t e = 0; e < n_edges; e++) {
    const int64_t fi = L.free_index[(size_t)edge_i[e]], fj = L.free_index[(size_t)edge_j[e]];
    auto term = [&](int64_t bi, int64_t bj, int kind) {
      L.key.push_back(bi * F + bj);
      L.contrib.push_back((int32_t)(4 * e + kind));
    };
    if (fi >= 0) term(fi, fi, 0);
    if (fj >= 0) term(fj, fj, 1);
    if (fi >= 0 && fj >= 0) {
      if (fi > fj) term(fi, fj, 2);
      if (fi < fj) term(fj, fi, 3);
    }
  }
  L.order.resize(L.key.size());
  for (size_t k = 0; k < L.order.size(); k++) L.order[k] = (int32_t)k;
  std::stable_sort(L.order.begin(), L.order.end(), [&](int32_t a, int32_t b) { return L.key[(size_t)a] < L.key[(size_t)b]; });
  std::vector<int32_t> sorted;
  sorted.reserve(L.contrib.size());
  L.blk_i.clear();
  L.blk_j.clear();
  L.blk_begin.clear();
  int64_t last = -1;
  for (int32_t k : L.order) {
    const int64_t key = L.key[(size_t)k];
    if (key != last) {
      L.blk_i.push_back((int32_t)(key / F));
      L.blk_j.push_back((int32_t)(key % F));
      L.blk_begin.push_back((int64_t)sorted.size());
      last = key;
    }
    if (L.contrib[(size_t)k] >= 0) sorted.push_back(L.contrib[(size_t)k]);
  }
  L.blk_begin.push_back((int64_t)sorted.size());
  L.contrib.swap(sorted);
}

}  // namespace eg_sys
