// TEST INFRASTRUCTURE — NOT PRODUCT CODE.  A program of its own (built by tests/test_bow_vocab_constants.py with
// g++ -fsanitize=address,undefined; CPU only, never loaded into python): the tree validator and the host build of the rule header
// (geoflowslam_amd/csrc/bow_vocab_rule.hpp) on a handful of malformed and well-formed trees, with every array sized EXACTLY, so that
// a read one element past an array is a report.  Prints one line per case; exit status 0 iff every case ended as its label says.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../geoflowslam_amd/csrc/bow_vocab_rule.hpp"

namespace {

struct Tree {  // arrays of exactly the sizes the ABI states
  int k, L, scoring = 0, weighting = 0;
  std::vector<int32_t> parent, child_start, children, word_id;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
  gfs_bow_vocabulary view() const {
    gfs_bow_vocabulary v{};
    v.k = k, v.L = L, v.scoring = scoring, v.weighting = weighting;
    v.n_nodes = (int32_t)parent.size();
    v.parent = parent.data(), v.child_start = child_start.data(), v.children = children.data();
    v.desc = desc.data(), v.weight = weight.data(), v.word_id = word_id.data();
    return v;
  }
};

// the complete k-ary tree of depth L; node i's descriptor has byte (i % 32) set to i
Tree complete(int k, int L) {
  Tree T;
  T.k = k, T.L = L;
  T.parent.assign(1, 0);
  std::vector<int> level(1, 0);
  std::vector<std::vector<int32_t>> kids(1);
  for (size_t i = 0; i < T.parent.size(); i++) {
    if (level[i] == L) continue;
    for (int c = 0; c < k; c++) {
      kids[i].push_back((int32_t)T.parent.size());
      T.parent.push_back((int32_t)i);
      level.push_back(level[i] + 1);
      kids.emplace_back();
    }
  }
  const size_t n = T.parent.size();
  T.child_start.assign(1, 0);
  int words = 0;
  for (size_t i = 0; i < n; i++) {
    T.children.insert(T.children.end(), kids[i].begin(), kids[i].end());
    T.child_start.push_back((int32_t)T.children.size());
    T.word_id.push_back(kids[i].empty() ? words++ : -1);
    T.weight.push_back(kids[i].empty() ? 0.5 + (double)(i % 7) : 0.0);
  }
  T.desc.assign(32 * n, 0);
  for (size_t i = 0; i < n; i++) T.desc[32 * i + i % 32] = (uint8_t)i, T.desc[32 * i + (i * 7) % 32] ^= (uint8_t)(i >> 3);
  return T;
}

int failures = 0;

void expect(const char* label, const Tree& T, const char* reason_part) {
  const gfs_bow_vocabulary v = T.view();
  gfs_bowv::PackedTree P;
  const char* why = gfs_bowv::pack_tree(&v, P);
  const bool ok = reason_part ? (why && strstr(why, reason_part)) : !why;
  printf("%-44s %s%s\n", label, why ? "refused: " : "accepted", why ? why : "");
  if (!ok) failures++;
  if (why) return;
  // the host statement on a few frames: every feature's word must be a word, every index listed once
  const int n = 37;
  std::vector<uint8_t> desc(32 * (size_t)n);
  for (size_t i = 0; i < desc.size(); i++) desc[i] = (uint8_t)((i * 2654435761u) >> 13);
  for (int levelsup = 0; levelsup <= T.L + 1; levelsup++) {
    if (!gfs_bowv::nid_defined(P.L, levelsup, P.min_leaf_depth)) continue;
    gfs_bowv::Vectors V;
    gfs_bowv::transform_frame(P, levelsup, desc.data(), n, V);
    double sum = 0;
    for (double x : V.word_value) sum += x;
    std::vector<int> seen((size_t)n, 0);
    for (int32_t i : V.feat_idx) seen[(size_t)i]++;
    bool good = V.node_start.size() == V.node_id.size() + 1 && (V.word_id.empty() || (sum > 0.999999 && sum < 1.000001));
    for (int i = 0; i < n; i++) good = good && seen[(size_t)i] == (V.word_of_feature[(size_t)i] >= 0 ? 1 : 0) && V.word_of_feature[(size_t)i] < P.n_words;
    printf("  levelsup %d: %zu words, %zu nodes, sum %.17g\n", levelsup, V.word_id.size(), V.node_id.size(), sum);
    if (!good) failures++;
  }
  gfs_bowv::Vectors E;
  gfs_bowv::transform_frame(P, T.L, nullptr, 0, E);  // an empty frame
  if (!E.word_id.empty() || E.node_start.size() != 1) failures++;
}

}  // namespace

int main() {
  expect("complete k=2 L=3", complete(2, 3), nullptr);
  expect("complete k=10 L=2", complete(10, 2), nullptr);
  expect("complete k=20 L=1", complete(20, 1), nullptr);
  expect("complete k=1 L=4", complete(1, 4), nullptr);
  {  // an early leaf: node 1 of k=2 L=2 loses its children (the nodes after it close ranks)
    Tree T = complete(2, 2);  // 0; 1 2; 3 4 5 6
    T.parent = {0, 0, 0, 2, 2};
    T.child_start = {0, 2, 2, 4, 4, 4};
    T.children = {1, 2, 3, 4};
    T.word_id = {-1, 0, -1, 1, 2};
    T.weight = {0, 1.5, 0, 0.0, 2.5};  // word 1 is stopped
    T.desc.resize(32 * 5);
    expect("an early leaf and a stopped word", T, nullptr);
  }
  {
    Tree T = complete(2, 2);
    T.parent = {0, 0, 0, 4, 3, 1, 1};
    T.child_start = {0, 2, 4, 4, 5, 6, 6, 6};
    T.children = {1, 2, 5, 6, 4, 3};
    T.word_id = {-1, -1, 0, -1, -1, 1, 2};
    expect("a cycle", T, "cycle");
  }
  {
    Tree T = complete(2, 2);
    T.children[5] = 3;
    expect("a child listed under two parents", T, "twice");
  }
  {
    Tree T = complete(2, 2);
    T.children[2] = 7;
    expect("an index out of range", T, "out of range");
    T.children[2] = -3;
    expect("a negative index", T, "out of range");
    T.children[2] = 0;
    expect("the root as a child", T, "out of range");
  }
  {
    Tree T = complete(2, 2);
    T.word_id[1] = 4;
    expect("a leaf with children", T, "leaf has children");
  }
  {
    Tree T = complete(2, 2);
    T.child_start[7] = 9;  // more entries than `children` holds: must be refused before any of them is read
    expect("child_start beyond the children array", T, "more child entries");
  }
  {
    Tree T = complete(2, 2);
    T.word_id[6] = 1 << 30;
    expect("a word id far out of range", T, "permutation");
  }
  {
    Tree T = complete(2, 2);
    T.L = 1;
    expect("deeper than L", T, "deeper");
  }
  // the score of one entry against a query
  {
    const int32_t qid[] = {1, 4, 9, 12}, did[] = {0, 4, 12, 40};
    const double qv[] = {0.1, 0.2, 0.3, 0.4}, dv[] = {0.25, 0.25, 0.25, 0.25};
    int32_t nc, fw;
    float s;
    gfs_bowv::score_entry(4, qid, qv, 4, did, dv, nc, fw, s);
    printf("score: %d common, first %d, %.9g\n", nc, fw, (double)s);
    if (nc != 2 || fw != 4 || !(s > 0.44f && s < 0.46f)) failures++;
    gfs_bowv::score_entry(0, qid, qv, 4, did, dv, nc, fw, s);
    if (nc != 0 || fw != -1 || s != 0.0f) failures++;
    gfs_bowv::score_entry(4, qid, qv, 0, did, dv, nc, fw, s);
    if (nc != 0 || fw != -1 || s != 0.0f) failures++;
  }
  printf(failures ? "bow_vocab_rule_check: %d FAILED\n" : "bow_vocab_rule_check: ok\n", failures);
  return failures ? 1 : 0;
}
