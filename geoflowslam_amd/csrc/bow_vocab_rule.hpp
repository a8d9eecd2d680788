// The rule of DBoW2::TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (reference
// Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1119-1259, BowVector.cpp:34-84) for TF_IDF weighting and L1_NORM scoring, and of the
// numeric core of KeyFrameDatabase::DetectNBestCandidates (src/KeyFrameDatabase.cc:596-645, ScoringObject.cpp:23-68), stated once for
// the device and the host.  The translation units that include this are built with -ffp-contract=off; every
// double operation below is one IEEE operation rounded once, in the order the reference performs it.
//
//   descent       from the root, at every level the child with the smallest 256-bit Hamming distance; strict `<` in the order of the
//                 node's children, so among equals the lowest POSITION wins: the minimum of child_key(distance, position)
//   nid           the node reached at level L - levelsup, node 0 when L - levelsup <= 0
//   accumulation  in feature order, a feature whose word weight is > 0 adds its weight to its word (first hit sets, later hits +=)
//                 and appends its index to its node's list; a stopped word (weight <= 0) contributes to neither
//   normalisation norm = sum of fabs(value) in ascending word id from 0.0; if norm > 0.0 every value is divided by it
//   score         over the common words in ascending id  score += fabs(vi - wi) - fabs(vi) - fabs(wi)  (left to right, then added),
//                 the result (float)(-score / 2.0); vi the query's value, wi the entry's
//   sharing list  a key frame's place in lKFsSharingWords is ordered by (its lowest common word id, its add sequence number)
//
// Two things the reference leaves undefined are fixed here: a leaf shallower than level L - levelsup (> 0) would leave *nid
// uninitialised, so such a (vocabulary, levelsup) pair is refused (nid_defined); and the root must be an inner node (the do-while of
// :1232-1254 reads children[0] of the root unconditionally).
#pragma once
#include <cmath>
#include <cstdint>

#if !defined(GFS_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFS_HD __host__ __device__ inline
#else
#define GFS_HD inline
#endif
#endif

#include <algorithm>
#include <vector>

#include "../../include/gfs_abi.h"

namespace gfs_bowv {

constexpr int kMaxK = 20;            // loadFromTextFile: m_k > 20 is refused (:1359)
constexpr int kMaxL = 10;            // ... and m_L < 1 || m_L > 10
constexpr int kScoringL1 = 0;        // DBoW2::L1_NORM
constexpr int kWeightingTfIdf = 0;   // DBoW2::TF_IDF
constexpr int kLevelsUp = 4;         // both ComputeBoW call sites (src/KeyFrame.cc:226, src/Frame.cc:1090)
constexpr float kMinCommonShare = 0.8f;   // int minCommonWords = maxCommonWords * 0.8f (src/KeyFrameDatabase.cc:627)
constexpr int kCovisibles = 10;           // GetBestCovisibilityKeyFrames(10) (:657)
constexpr int kLoopNumCandidates = 3;     // DetectNBestCandidates(mpCurrentKF, ..., 3) (src/LoopClosing.cc:519-520)
constexpr int kGroup = 16;           // lanes that share one feature's descent on the device
constexpr int kNoKey = 0x7fffffff;   // "no child yet": above every key

GFS_HD int popcount32(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}

// FORB::distance over the eight words of a descriptor
GFS_HD int hamming256(const unsigned* a, const unsigned* b) {
  int d = 0;
  for (int w = 0; w < 8; w++) d += popcount32(a[w] ^ b[w]);
  return d;
}

// (distance, position among the node's children) in one integer: the smaller key is the smaller distance, the lower position among
// equals -- what `if (d < best_d)` over the children in order leaves.  position < 256 (k <= 20), distance <= 256.
GFS_HD int child_key(int dist, int position) { return (dist << 8) | position; }
GFS_HD int key_position(int key) { return key & 0xff; }

GFS_HD int nid_level(int L, int levelsup) { return L - levelsup; }
GFS_HD bool stopped(double weight) { return !(weight > 0); }  // `if (w > 0)` (:1157)
// *nid is written for every feature iff the level is the root's or every leaf lies at or below it
GFS_HD bool nid_defined(int L, int levelsup, int min_leaf_depth) { return nid_level(L, levelsup) <= 0 || min_leaf_depth >= nid_level(L, levelsup); }

// one term of L1Scoring::score, and its end
GFS_HD double l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
GFS_HD float l1_finish(double score) { return (float)(-score / 2.0); }

// The repacked table: node p's children are the nodes first_child .. first_child + n_children - 1, in `children` order; the root is 0.
struct NodeMeta {
  int32_t first_child, n_children;  // n_children == 0: a leaf
};
struct TreeView {
  const NodeMeta* meta;     // [n_nodes]
  const unsigned* desc;     // [n_nodes][8]
  const int32_t* word;      // [n_nodes] word id of a leaf, -1 of an inner node
  const double* weight;     // [n_nodes]
  const int32_t* orig;      // [n_nodes] the caller's node id
};

// the descent of one feature, child by child (the device spreads the children over the lanes of a group and takes the same minimum)
GFS_HD void descend(const TreeView& T, const unsigned* f, int level_of_nid, int& word, double& weight, int& node) {
  int p = 0, level = 0, at = 0;
  while (T.meta[p].n_children > 0) {
    const NodeMeta m = T.meta[p];
    level++;
    int key = kNoKey;
    for (int c = 0; c < m.n_children; c++) {
      const int k = child_key(hamming256(f, T.desc + 8 * (size_t)(m.first_child + c)), c);
      key = k < key ? k : key;
    }
    p = m.first_child + key_position(key);
    if (level == level_of_nid) at = p;
  }
  weight = T.weight[p];
  word = stopped(weight) ? -1 : T.word[p];
  node = T.orig[at];
}

// the order of the surviving features in both vectors: (word or node, feature index) in one key
GFS_HD unsigned long long sort_key(int id, int feature) { return ((unsigned long long)(unsigned)id << 32) | (unsigned)feature; }

// ---- the host side: validation, repacking, and the host statement of both entries ----
struct PackedTree {
  std::vector<NodeMeta> meta;
  std::vector<unsigned> desc;
  std::vector<int32_t> word, orig;
  std::vector<double> weight;
  int L = 0, n_words = 0, min_leaf_depth = 0;
  TreeView view() const { return TreeView{meta.data(), desc.data(), word.data(), weight.data(), orig.data()}; }
};

// nullptr when the tree is what gfs_bow_create accepts, else the reason.  Fills depth[n_nodes] (root 0) and the breadth-first order.
inline const char* validate_tree(const gfs_bow_vocabulary* v, std::vector<int>& depth, std::vector<int>& order, int& n_words, int& min_leaf_depth) {
  if (!v) return "NULL vocabulary";
  if (v->k < 1 || v->k > kMaxK) return "k outside 1..20";
  if (v->L < 1 || v->L > kMaxL) return "L outside 1..10";
  if (v->scoring != kScoringL1 || v->weighting != kWeightingTfIdf) return "only L1_NORM scoring with TF_IDF weighting (header `k L 0 0`)";
  if (v->n_nodes < 2) return "fewer than two nodes";
  if (!v->parent || !v->child_start || !v->children || !v->desc || !v->weight || !v->word_id) return "NULL array";
  const int n = v->n_nodes;
  if (v->child_start[0] != 0) return "child_start does not start at 0";
  for (int i = 0; i < n; i++) {
    const long long nc = (long long)v->child_start[i + 1] - v->child_start[i];
    if (nc < 0) return "child_start decreases";
    if (v->child_start[i + 1] > n - 1) return "more child entries than non-root nodes";
    if (v->word_id[i] < -1) return "word id below -1";
    if (v->word_id[i] >= 0 && nc != 0) return "a leaf has children";
    if (v->word_id[i] == -1 && nc < 1) return "an inner node has no children";
    if (nc > v->k) return "a node has more than k children";
    if (!std::isfinite(v->weight[i])) return "a weight is not finite";
  }
  if (v->child_start[n] != n - 1) return "a non-root node is listed under no parent";
  if (v->word_id[0] != -1) return "the root is a leaf";
  std::vector<uint8_t> listed((size_t)n, 0);
  for (int i = 0; i < n; i++)
    for (int j = v->child_start[i]; j < v->child_start[i + 1]; j++) {
      const int c = v->children[j];
      if (c < 1 || c >= n) return "a child index is out of range";
      if (listed[c]) return "a node is listed as a child twice";
      listed[c] = 1;
      if (v->parent[c] != i) return "a node is listed under a node that is not its parent";
    }
  // every non-root node is listed exactly once: what is not reached from the root lies on a cycle
  depth.assign((size_t)n, -1);
  order.clear();
  order.reserve((size_t)n);
  order.push_back(0);
  depth[0] = 0;
  for (size_t q = 0; q < order.size(); q++) {
    const int i = order[q];
    for (int j = v->child_start[i]; j < v->child_start[i + 1]; j++) {
      depth[v->children[j]] = depth[i] + 1;
      order.push_back(v->children[j]);
    }
  }
  if ((int)order.size() != n) return "a cycle: nodes that the root does not reach";
  n_words = 0;
  min_leaf_depth = kMaxL + 1;
  for (int i = 0; i < n; i++) {
    if (depth[i] > v->L) return "a node deeper than L";
    if (v->word_id[i] >= 0) {
      n_words++;
      min_leaf_depth = std::min(min_leaf_depth, depth[i]);
    }
  }
  std::vector<uint8_t> seen((size_t)n_words, 0);
  for (int i = 0; i < n; i++)
    if (v->word_id[i] >= 0) {
      if (v->word_id[i] >= n_words || seen[v->word_id[i]]) return "word ids are not a permutation of 0..n_words-1";
      seen[v->word_id[i]] = 1;
    }
  return nullptr;
}

// Validates and repacks: breadth first, so a node's children take consecutive places in `children` order.
inline const char* pack_tree(const gfs_bow_vocabulary* v, PackedTree& P) {
  std::vector<int> depth, order;
  if (const char* why = validate_tree(v, depth, order, P.n_words, P.min_leaf_depth)) return why;
  const size_t n = (size_t)v->n_nodes;
  P.L = v->L;
  P.meta.assign(n, NodeMeta{0, 0});
  P.desc.assign(8 * n, 0u);
  P.word.assign(n, -1);
  P.orig.assign(n, 0);
  P.weight.assign(n, 0.0);
  // order[p] is the node at packed place p: the children of order[p] follow one another in `order` from `next` on
  int next = 1;
  for (size_t p = 0; p < n; p++) {
    const int i = order[p];
    const int nc = v->child_start[i + 1] - v->child_start[i];
    P.meta[p] = NodeMeta{nc ? next : 0, nc};
    next += nc;
    for (int w = 0; w < 8; w++) {
      const uint8_t* b = v->desc + 32 * (size_t)i + 4 * w;
      P.desc[8 * p + w] = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16 | (unsigned)b[3] << 24;
    }
    P.word[p] = v->word_id[i];
    P.orig[p] = i;
    P.weight[p] = v->weight[i];
  }
  return nullptr;
}

struct Vectors {  // one frame's output, as gfs_bow_vectors lays it out
  std::vector<int32_t> word_id, node_id, node_start, feat_idx, word_of_feature;
  std::vector<double> word_value;
};

// Host statement of one frame: the per-feature descent, then both vectors from the features sorted by (word, index) and by
// (node, index), the sums in that order -- the steps of k_bow_descend and k_bow_vectors, one after the other.
inline void transform_frame(const PackedTree& P, int levelsup, const uint8_t* desc, int n, Vectors& out) {
  const TreeView T = P.view();
  std::vector<double> w((size_t)n);
  std::vector<int> node((size_t)n);
  out.word_of_feature.assign((size_t)n, -1);
  std::vector<unsigned long long> by_word, by_node;
  for (int i = 0; i < n; i++) {
    unsigned f[8];
    for (int k = 0; k < 8; k++) {
      const uint8_t* b = desc + 32 * (size_t)i + 4 * k;
      f[k] = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16 | (unsigned)b[3] << 24;
    }
    descend(T, f, nid_level(P.L, levelsup), out.word_of_feature[i], w[i], node[i]);
    if (out.word_of_feature[i] < 0) continue;
    by_word.push_back(sort_key(out.word_of_feature[i], i));
    by_node.push_back(sort_key(node[i], i));
  }
  std::sort(by_word.begin(), by_word.end());
  std::sort(by_node.begin(), by_node.end());
  out.word_id.clear(), out.word_value.clear(), out.node_id.clear(), out.node_start.clear(), out.feat_idx.clear();
  for (size_t j = 0; j < by_word.size(); j++) {
    const int id = (int)(by_word[j] >> 32), i = (int)(by_word[j] & 0xffffffffu);
    if (j == 0 || id != out.word_id.back()) {
      out.word_id.push_back(id);
      out.word_value.push_back(w[i]);
    } else {
      out.word_value.back() += w[i];
    }
  }
  double norm = 0.0;
  for (double v : out.word_value) norm += fabs(v);
  if (norm > 0.0)
    for (double& v : out.word_value) v /= norm;
  for (size_t j = 0; j < by_node.size(); j++) {
    const int id = (int)(by_node[j] >> 32);
    if (j == 0 || id != out.node_id.back()) {
      out.node_id.push_back(id);
      out.node_start.push_back((int)j);
    }
    out.feat_idx.push_back((int)(by_node[j] & 0xffffffffu));
  }
  out.node_start.push_back((int)by_node.size());
}

// a BowVector as gfs_bow_db_add / gfs_bow_db_query accept it: ids strictly ascending from >= 0, values finite
inline bool valid_bow_vector(int n, const int32_t* id, const double* value) {
  for (int i = 0; i < n; i++)
    if (id[i] < 0 || (i && id[i] <= id[i - 1]) || !std::isfinite(value[i])) return false;
  return true;
}

// Host statement of one database slot against the query (the steps of one wave of k_bow_score): the entry's words in ascending id,
// each looked up in the query by binary search.
inline void score_entry(int nq, const int32_t* qid, const double* qval, int nd, const int32_t* did, const double* dval, int32_t& n_common,
                        int32_t& first_word, float& score) {
  n_common = 0;
  first_word = -1;
  double s = 0;
  for (int j = 0; j < nd; j++) {
    const int32_t* at = std::lower_bound(qid, qid + nq, did[j]);
    if (at == qid + nq || *at != did[j]) continue;
    if (n_common++ == 0) first_word = did[j];
    s += l1_term(qval[at - qid], dval[j]);
  }
  score = n_common ? l1_finish(s) : 0.0f;
}

}  // namespace gfs_bowv
