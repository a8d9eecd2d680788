// TEST INFRASTRUCTURE — NOT PRODUCT CODE.  Sequential CPU restatement of
//   DBoW2::TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)  (reference
//     Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1119-1259, BowVector.cpp:34-84, FeatureVector.cpp:28-42, FORB.cpp:81-101)
//   for TF_IDF / L1_NORM, and of the word-sharing walk and the scores of KeyFrameDatabase::DetectNBestCandidates (reference
//     src/KeyFrameDatabase.cc:596-645, ScoringObject.cpp:23-68),
// written from the reference's text: m_nodes with a `children` vector each, the per-feature do-while descent with `d < best_d`, the
// BowVector and FeatureVector as std::map, addWeight / addFeature / normalize, the inverted file as a vector of std::list, the merge
// loop of L1Scoring::score with lower_bound.  Nothing here comes from the rule header (geoflowslam_amd/csrc/bow_vocab_rule.hpp) but
// the bv_rule_* entry points, which run the rule's own host statement so that the tests can compare the two.
// The tests build it with g++ -O2 -std=c++17 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <vector>

#include "bow_vocab_rule.hpp"
#include "gfs_abi.h"

namespace {

typedef unsigned int WordId;
typedef unsigned int NodeId;
typedef double WordValue;
typedef std::map<WordId, WordValue> BowVector;
typedef std::map<NodeId, std::vector<unsigned int>> FeatureVector;

struct Node {  // TemplatedVocabulary::Node
  NodeId id = 0, parent = 0;
  std::vector<NodeId> children;
  const uint8_t* descriptor = nullptr;
  WordValue weight = 0;
  WordId word_id = 0;
  bool isLeaf() const { return children.empty(); }
};

struct Vocabulary {
  int m_k, m_L;
  std::vector<Node> m_nodes;
};

Vocabulary vocabulary(const gfs_bow_vocabulary& v) {
  Vocabulary V;
  V.m_k = v.k;
  V.m_L = v.L;
  V.m_nodes.resize((size_t)v.n_nodes);
  for (int i = 0; i < v.n_nodes; i++) {
    Node& n = V.m_nodes[i];
    n.id = i;
    n.parent = v.parent[i];
    n.children.assign(v.children + v.child_start[i], v.children + v.child_start[i + 1]);
    n.descriptor = v.desc + 32 * (size_t)i;
    n.weight = v.weight[i];
    n.word_id = (WordId)v.word_id[i];
  }
  return V;
}

double distance(const uint8_t* a, const uint8_t* b) {  // FORB::distance: 256 bits, 32 at a time
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    unsigned int pa, pb;
    memcpy(&pa, a + 4 * i, 4);
    memcpy(&pb, b + 4 * i, 4);
    unsigned int v = pa ^ pb;
    v = v - ((v >> 1) & 0x55555555);
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
    dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
  }
  return dist;
}

// :1218-1259.  nid_set: whether *nid was assigned at all (the reference leaves it uninitialised when the leaf is shallower)
void transform(const Vocabulary& V, const uint8_t* feature, WordId& word_id, WordValue& weight, NodeId* nid, int levelsup, bool& nid_set) {
  std::vector<NodeId> nodes;
  const int nid_level = V.m_L - levelsup;
  nid_set = false;
  if (nid_level <= 0 && nid != NULL) {
    *nid = 0;
    nid_set = true;
  }
  NodeId final_id = 0;
  int current_level = 0;
  do {
    ++current_level;
    nodes = V.m_nodes[final_id].children;
    final_id = nodes[0];
    double best_d = distance(feature, V.m_nodes[final_id].descriptor);
    for (std::vector<NodeId>::const_iterator nit = nodes.begin() + 1; nit != nodes.end(); ++nit) {
      NodeId id = *nit;
      double d = distance(feature, V.m_nodes[id].descriptor);
      if (d < best_d) {
        best_d = d;
        final_id = id;
      }
    }
    if (nid != NULL && current_level == nid_level) {
      *nid = final_id;
      nid_set = true;
    }
  } while (!V.m_nodes[final_id].isLeaf());
  word_id = V.m_nodes[final_id].word_id;
  weight = V.m_nodes[final_id].weight;
}

void addWeight(BowVector& v, WordId id, WordValue w) {  // BowVector.cpp:34-46
  BowVector::iterator vit = v.lower_bound(id);
  if (vit != v.end() && !(v.key_comp()(id, vit->first))) {
    vit->second += w;
  } else {
    v.insert(vit, BowVector::value_type(id, w));
  }
}

void addFeature(FeatureVector& fv, NodeId id, unsigned int i_feature) {  // FeatureVector.cpp:28-42
  FeatureVector::iterator vit = fv.lower_bound(id);
  if (vit != fv.end() && vit->first == id) {
    vit->second.push_back(i_feature);
  } else {
    vit = fv.insert(vit, FeatureVector::value_type(id, std::vector<unsigned int>()));
    vit->second.push_back(i_feature);
  }
}

void normalizeL1(BowVector& v) {  // BowVector.cpp:62-84
  double norm = 0.0;
  for (BowVector::iterator it = v.begin(); it != v.end(); ++it) norm += fabs(it->second);
  if (norm > 0.0) {
    for (BowVector::iterator it = v.begin(); it != v.end(); ++it) it->second /= norm;
  }
}

// :1119-1194 for TF_IDF with a scoring object that must normalise (L1).  false: some feature's node was never assigned
bool transform(const Vocabulary& V, const uint8_t* features, int n, BowVector& v, FeatureVector& fv, int levelsup, int32_t* word_of_feature) {
  v.clear();
  fv.clear();
  bool all_set = true;
  for (unsigned int i_feature = 0; i_feature < (unsigned)n; ++i_feature) {
    WordId id;
    NodeId nid = 0;
    WordValue w;
    bool nid_set;
    transform(V, features + 32 * (size_t)i_feature, id, w, &nid, levelsup, nid_set);
    all_set = all_set && nid_set;
    if (word_of_feature) word_of_feature[i_feature] = w > 0 ? (int32_t)id : -1;
    if (w > 0) {
      addWeight(v, id, w);
      addFeature(fv, nid, i_feature);
    }
  }
  normalizeL1(v);
  return all_set;
}

double L1score(const BowVector& v1, const BowVector& v2) {  // ScoringObject.cpp:23-68
  BowVector::const_iterator v1_it, v2_it;
  const BowVector::const_iterator v1_end = v1.end();
  const BowVector::const_iterator v2_end = v2.end();
  v1_it = v1.begin();
  v2_it = v2.begin();
  double score = 0;
  while (v1_it != v1_end && v2_it != v2_end) {
    const WordValue& vi = v1_it->second;
    const WordValue& wi = v2_it->second;
    if (v1_it->first == v2_it->first) {
      score += fabs(vi - wi) - fabs(vi) - fabs(wi);
      ++v1_it;
      ++v2_it;
    } else if (v1_it->first < v2_it->first) {
      v1_it = v1.lower_bound(v2_it->first);
    } else {
      v2_it = v2.lower_bound(v1_it->first);
    }
  }
  score = -score / 2.0;
  return score;
}

BowVector bow_vector(int n, const int32_t* id, const double* value) {
  BowVector v;
  for (int i = 0; i < n; i++) v[(WordId)id[i]] = value[i];
  return v;
}

// KeyFrameDatabase with slots for key frames: add (:41-50), erase (:52-71) and the walk of :596-614 without the connected set (which
// is the adaptor's)
struct Database {
  std::map<WordId, std::list<int>> mvInvertedFile;  // (a map, not a vector sized by the vocabulary: the same lists)
  std::vector<BowVector> mBowVec;
  std::vector<uint8_t> present;
};

}  // namespace

extern "C" {

// a vocabulary built once, for callers that transform many times (the arrays of *v must outlive it: the descriptors are not copied)
void* bv_vocabulary_create(const gfs_bow_vocabulary* v) { return new Vocabulary(vocabulary(*v)); }
void bv_vocabulary_destroy(void* V) { delete static_cast<Vocabulary*>(V); }

// out[b]: caller-owned arrays as gfs_bow_transform fills them.  0, or -2 where the reference would have left a node id uninitialised
int bv_vocabulary_transform(const void* vocab, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out) {
  const Vocabulary& V = *static_cast<const Vocabulary*>(vocab);
  bool all_set = true;
  for (int b = 0; b < B; b++) {
    BowVector bv;
    FeatureVector fv;
    all_set = transform(V, desc[b], n[b], bv, fv, levelsup, out[b].word_of_feature) && all_set;
    gfs_bow_vectors& o = out[b];
    o.n_words = 0;
    for (BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it, o.n_words++) {
      o.word_id[o.n_words] = (int32_t)it->first;
      o.word_value[o.n_words] = it->second;
    }
    o.n_nodes = 0;
    int at = 0;
    o.node_start[0] = 0;
    for (FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it, o.n_nodes++) {
      o.node_id[o.n_nodes] = (int32_t)it->first;
      for (unsigned int i : it->second) o.feat_idx[at++] = (int32_t)i;
      o.node_start[o.n_nodes + 1] = at;
    }
  }
  return all_set ? 0 : -2;
}

int bv_transform(const gfs_bow_vocabulary* v, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out) {
  const Vocabulary V = vocabulary(*v);
  return bv_vocabulary_transform(&V, desc, n, B, levelsup, out);
}

// the rule header's host build of the same call on a tree packed once: -2 for the shallow leaf
void* bv_rule_tree_create(const gfs_bow_vocabulary* v) {
  gfs_bowv::PackedTree* P = new gfs_bowv::PackedTree;
  if (gfs_bowv::pack_tree(v, *P)) {
    delete P;
    return nullptr;
  }
  return P;
}
void bv_rule_tree_destroy(void* P) { delete static_cast<gfs_bowv::PackedTree*>(P); }
int bv_rule_tree_transform(const void* tree, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out);

// ... and packed for this call: -1 with the validator's reason in why[cap] for a tree it refuses
int bv_rule_transform(const gfs_bow_vocabulary* v, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out,
                      char* why, int cap) {
  gfs_bowv::PackedTree P;
  if (const char* w = gfs_bowv::pack_tree(v, P)) {
    if (why && cap > 0) strncpy(why, w, (size_t)cap - 1), why[cap - 1] = 0;
    return -1;
  }
  return bv_rule_tree_transform(&P, desc, n, B, levelsup, out);
}

int bv_rule_tree_transform(const void* tree, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out) {
  const gfs_bowv::PackedTree& P = *static_cast<const gfs_bowv::PackedTree*>(tree);
  if (levelsup < 0 || !gfs_bowv::nid_defined(P.L, levelsup, P.min_leaf_depth)) return -2;
  for (int b = 0; b < B; b++) {
    gfs_bowv::Vectors V;
    gfs_bowv::transform_frame(P, levelsup, desc[b], n[b], V);
    gfs_bow_vectors& o = out[b];
    o.n_words = (int32_t)V.word_id.size();
    o.n_nodes = (int32_t)V.node_id.size();
    memcpy(o.word_id, V.word_id.data(), V.word_id.size() * sizeof(int32_t));
    memcpy(o.word_value, V.word_value.data(), V.word_value.size() * sizeof(double));
    memcpy(o.node_id, V.node_id.data(), V.node_id.size() * sizeof(int32_t));
    memcpy(o.node_start, V.node_start.data(), V.node_start.size() * sizeof(int32_t));
    memcpy(o.feat_idx, V.feat_idx.data(), V.feat_idx.size() * sizeof(int32_t));
    if (o.word_of_feature) memcpy(o.word_of_feature, V.word_of_feature.data(), V.word_of_feature.size() * sizeof(int32_t));
  }
  return 0;
}

// the validator alone: 0 and info = {n_words, min_leaf_depth}, or -1 and the reason
int bv_rule_validate(const gfs_bow_vocabulary* v, int32_t* info, char* why, int cap) {
  std::vector<int> depth, order;
  int n_words = 0, min_leaf_depth = 0;
  if (const char* w = gfs_bowv::validate_tree(v, depth, order, n_words, min_leaf_depth)) {
    if (why && cap > 0) strncpy(why, w, (size_t)cap - 1), why[cap - 1] = 0;
    return -1;
  }
  info[0] = n_words;
  info[1] = min_leaf_depth;
  return 0;
}

void* bv_db_create(int max_entries) {
  Database* D = new Database;
  D->mBowVec.resize((size_t)max_entries);
  D->present.assign((size_t)max_entries, 0);
  return D;
}
void bv_db_destroy(void* db) { delete static_cast<Database*>(db); }

void bv_db_erase(void* db, int slot) {  // :52-71
  Database& D = *static_cast<Database*>(db);
  if (!D.present[slot]) return;
  for (BowVector::const_iterator vit = D.mBowVec[slot].begin(), vend = D.mBowVec[slot].end(); vit != vend; vit++) {
    std::list<int>& lKFs = D.mvInvertedFile[vit->first];
    for (std::list<int>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
      if (slot == *lit) {
        lKFs.erase(lit);
        break;
      }
    }
  }
  D.present[slot] = 0;
  D.mBowVec[slot].clear();
}

void bv_db_add(void* db, int slot, int n_words, const int32_t* word_id, const double* word_value) {  // :41-50; an occupied slot is erased first
  Database& D = *static_cast<Database*>(db);
  bv_db_erase(db, slot);
  D.mBowVec[slot] = bow_vector(n_words, word_id, word_value);
  D.present[slot] = 1;
  for (BowVector::const_iterator vit = D.mBowVec[slot].begin(), vend = D.mBowVec[slot].end(); vit != vend; vit++)
    D.mvInvertedFile[vit->first].push_back(slot);
}

// n_common / first_word / score [max_entries] as gfs_bow_db_query fills them; list [max_entries]: lKFsSharingWords as slots in list
// order (:596-614 with an empty connected set), its length returned
static int db_query(void* db, int n_words, const int32_t* word_id, const double* word_value, int32_t* n_common, int32_t* first_word, float* score,
                    int32_t* list, bool only_above) {
  Database& D = *static_cast<Database*>(db);
  const BowVector q = bow_vector(n_words, word_id, word_value);
  const size_t E = D.present.size();
  std::vector<uint8_t> queried(E, 0);  // mnPlaceRecognitionQuery == pKF->mnId
  for (size_t s = 0; s < E; s++) n_common[s] = 0, first_word[s] = -1, score[s] = 0.0f;
  std::list<int> lKFsSharingWords;
  for (BowVector::const_iterator vit = q.begin(), vend = q.end(); vit != vend; vit++) {
    std::map<WordId, std::list<int>>::iterator f = D.mvInvertedFile.find(vit->first);
    if (f == D.mvInvertedFile.end()) continue;
    std::list<int>& lKFs = f->second;
    for (std::list<int>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
      const int pKFi = *lit;
      if (!queried[pKFi]) {
        n_common[pKFi] = 0;
        queried[pKFi] = 1;
        first_word[pKFi] = (int32_t)vit->first;
        lKFsSharingWords.push_back(pKFi);
      }
      n_common[pKFi]++;
    }
  }
  int maxCommonWords = 0;  // :619-627
  for (std::list<int>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++)
    if (n_common[*lit] > maxCommonWords) maxCommonWords = n_common[*lit];
  int minCommonWords = maxCommonWords * 0.8f;
  int n = 0;
  for (std::list<int>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
    list[n++] = *lit;
    if (only_above && !(n_common[*lit] > minCommonWords)) continue;
    float si = L1score(q, D.mBowVec[*lit]);  // float si = mpVoc->score(...) (:641)
    score[*lit] = si;
  }
  return n;
}

int bv_db_query(void* db, int n_words, const int32_t* word_id, const double* word_value, int32_t* n_common, int32_t* first_word, float* score,
                int32_t* list) {
  return db_query(db, n_words, word_id, word_value, n_common, first_word, score, list, false);
}

// as the reference runs it with an empty connected set: only the entries above minCommonWords are scored, the others keep 0
int bv_db_query_above(void* db, int n_words, const int32_t* word_id, const double* word_value, int32_t* n_common, int32_t* first_word,
                      float* score, int32_t* list) {
  return db_query(db, n_words, word_id, word_value, n_common, first_word, score, list, true);
}

// the rule's host statement of one slot
void bv_rule_score(int nq, const int32_t* qid, const double* qval, int nd, const int32_t* did, const double* dval, int32_t* n_common,
                   int32_t* first_word, float* score) {
  gfs_bowv::score_entry(nq, qid, qval, nd, did, dval, *n_common, *first_word, *score);
}

int bv_rule_valid_vector(int n, const int32_t* id, const double* value) { return gfs_bowv::valid_bow_vector(n, id, value) ? 1 : 0; }

// k and L bounds, the accepted scoring and weighting, levelsup of ComputeBoW, the two comparisons, and the constants of
// DetectNBestCandidates and of its call -- as the rule header compiles them in
void bv_constants(double* out) {
  out[0] = gfs_bowv::kMaxK;
  out[1] = gfs_bowv::kMaxL;
  out[2] = gfs_bowv::kScoringL1;
  out[3] = gfs_bowv::kWeightingTfIdf;
  out[4] = gfs_bowv::kLevelsUp;
  out[5] = gfs_bowv::stopped(0.0) && !gfs_bowv::stopped(5e-324) ? 1 : 0;                 // `w > 0`
  out[7] = gfs_bowv::kMinCommonShare;
  out[8] = gfs_bowv::kCovisibles;
  out[9] = gfs_bowv::kLoopNumCandidates;
  out[6] = gfs_bowv::child_key(7, 9) > gfs_bowv::child_key(7, 0) && gfs_bowv::child_key(6, 9) < gfs_bowv::child_key(7, 0) ? 1 : 0;  // `d < best_d`
}

}  // extern "C"
