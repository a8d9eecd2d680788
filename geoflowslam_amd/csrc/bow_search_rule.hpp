// The rule of ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (reference src/ORBmatcher.cc:936-1053) for
// single-camera key frames (NLeft == -1), stated once for the device and the host.  Everything is integer
// but the ratio test, which is one float multiplication rounded once; the translation units that include this are built with
// -ffp-contract=off.  The rotation bin and the three maxima are triangulate_rule.hpp's (the same lines of the reference).
//
// A feature index belongs to exactly one node of a feature vector, so vbMatched2 never crosses nodes: the common nodes of a pair of
// key frames are independent, and only the idx1 list of one node is walked in order.  For one idx1 the candidates are the node's
// list of key frame 2 in list order; what the sequential scan of :982-1006 leaves in bestDist1 / bestIdx2 / bestDist2 is
//   bestDist1, bestIdx2  the smallest distance, at the FIRST list position among equals (strict `dist < bestDist1`)
//   bestDist2            the smallest distance among all OTHER positions, an equal one included (`else if (dist < bestDist2)`)
// both starting at 256, which no candidate improves on.  `Best` holds them as a scan does, and two scans of disjoint position
// ranges are merged to what one scan of both would have left -- which is how the lanes of a wave share a list.
#pragma once
#include "triangulate_rule.hpp"

namespace gfs_bow {

constexpr int kThLow = 50;        // ORBmatcher::TH_LOW
constexpr int kHisto = 30;        // ORBmatcher::HISTO_LENGTH
constexpr int kInitDist = 256;    // int bestDist1 = 256, bestDist2 = 256 (:978, :980)
constexpr float kLoopNnRatio = 0.9f;         // ORBmatcher matcherBoW(0.9, true) (src/LoopClosing.cc:641-870)
constexpr int kLoopCheckOrientation = 1;
constexpr int kLoopMinBowMatches = 20;       // nBoWMatches
constexpr int kNoPosition = 0xffff;          // the position of "no candidate yet" in a key; list positions stay below it
static_assert(kHisto == gfs_tri::kHisto && kThLow == gfs_tri::kThLow, "one matcher, one set of constants");

GFS_HD int popcount32(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}

// ORBmatcher::DescriptorDistance over the eight words of a descriptor
GFS_HD int descriptor_distance(const unsigned* a, const unsigned* b) {
  int d = 0;
  for (int w = 0; w < 8; w++) d += popcount32(a[w] ^ b[w]);
  return d;
}

// (distance, list position) in one integer: the smaller key is the smaller distance, the earlier position among equals
GFS_HD int key_of(int dist, int position) { return (dist << 16) | position; }
GFS_HD int key_dist(int key) { return key >> 16; }
GFS_HD int key_position(int key) { return key & 0xffff; }

struct Best {  // the state of the scan :978-1006 over a set of positions
  int key1;    // key_of(bestDist1, position of bestIdx2)
  int dist2;   // bestDist2
};

GFS_HD Best best_init() { return Best{key_of(kInitDist, kNoPosition), kInitDist}; }

// one candidate, positions offered in ascending order (:999-1005)
GFS_HD void best_offer(Best& b, int dist, int position) {
  if (dist < key_dist(b.key1)) {
    b.dist2 = key_dist(b.key1);
    b.key1 = key_of(dist, position);
  } else if (dist < b.dist2) {
    b.dist2 = dist;
  }
}

// the scan of two disjoint sets of positions from their two states
GFS_HD Best best_merge(const Best& a, const Best& b) {
  const bool a_first = a.key1 < b.key1;
  const Best& w = a_first ? a : b;
  const Best& l = a_first ? b : a;
  Best r;
  r.key1 = w.key1;
  const int ld = key_dist(l.key1);
  r.dist2 = w.dist2 < ld ? w.dist2 : ld;
  return r;
}

// :1008-1010: TH_LOW is strict here (the triangulation and projection searches accept dist == TH_LOW), the ratio is one product
GFS_HD bool accept(int bestDist1, int bestDist2, float nn_ratio) {
  if (bestDist1 < kThLow) {
    if ((float)bestDist1 < nn_ratio * (float)bestDist2) return true;
  }
  return false;
}

// :1019 asserts 0 <= bin < HISTO_LENGTH, which holds for angles in [0, 360).  Written rule for other angles, where the reference's
// release build writes outside rotHist: such a match is in no bin, so it is counted nowhere and the orientation check removes it.
GFS_HD bool bin_in_histogram(int bin) { return bin >= 0 && bin < kHisto; }
GFS_HD bool bin_kept(int bin, int ind1, int ind2, int ind3) { return bin_in_histogram(bin) && (bin == ind1 || bin == ind2 || bin == ind3); }

// Host statement of one pair of key frames by the rule's pieces (node by node, the lists as given): match12[n_kp1] and the count.
// The device kernel (bow_search.hip) computes the same with the positions of a list spread over the lanes of a wave.
struct KeyFrameView {
  int n_kp;
  const float* angle;
  const uint8_t* desc;
  const uint8_t* has_mp;
  int n_nodes;
  const int* node_id;
  const int* node_start;
  const int* feat_idx;
};

#if !defined(__HIP_DEVICE_COMPILE__)
inline void load_words(const uint8_t* desc, int i, unsigned* w) {
  for (int k = 0; k < 8; k++) {
    const uint8_t* p = desc + 32 * (size_t)i + 4 * k;
    w[k] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
  }
}

// taken: scratch of n_kp2 bytes.  -> n_matches
inline int search_pair(const KeyFrameView& K1, const KeyFrameView& K2, float nn_ratio, bool check_orientation, int* match12, uint8_t* taken) {
  for (int i = 0; i < K1.n_kp; i++) match12[i] = -1;
  for (int i = 0; i < K2.n_kp; i++) taken[i] = 0;
  int hist[kHisto] = {0};
  for (int f1 = 0; f1 < K1.n_nodes; f1++) {
    int lo = 0, hi = K2.n_nodes;  // the node of key frame 2 with this id, if any
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (K2.node_id[mid] < K1.node_id[f1]) lo = mid + 1; else hi = mid;
    }
    if (lo >= K2.n_nodes || K2.node_id[lo] != K1.node_id[f1]) continue;
    const int b2 = K2.node_start[lo], n2 = K2.node_start[lo + 1] - b2;
    for (int i1 = K1.node_start[f1]; i1 < K1.node_start[f1 + 1]; i1++) {
      const int idx1 = K1.feat_idx[i1];
      if (!K1.has_mp[idx1]) continue;
      unsigned d1[8], d2[8];
      load_words(K1.desc, idx1, d1);
      Best b = best_init();
      for (int p = 0; p < n2; p++) {
        const int idx2 = K2.feat_idx[b2 + p];
        if (taken[idx2] || !K2.has_mp[idx2]) continue;
        load_words(K2.desc, idx2, d2);
        best_offer(b, descriptor_distance(d1, d2), p);
      }
      if (!accept(key_dist(b.key1), b.dist2, nn_ratio)) continue;
      const int idx2 = K2.feat_idx[b2 + key_position(b.key1)];
      match12[idx1] = idx2;
      taken[idx2] = 1;
      if (check_orientation) {
        const int bin = gfs_tri::rot_bin(K1.angle[idx1], K2.angle[idx2]);
        if (bin_in_histogram(bin)) hist[bin]++;
      }
    }
  }
  int n = 0;
  int ind1 = -1, ind2 = -1, ind3 = -1;
  if (check_orientation) gfs_tri::three_maxima(hist, ind1, ind2, ind3);
  for (int i = 0; i < K1.n_kp; i++) {
    if (match12[i] < 0) continue;
    if (check_orientation) {
      if (!bin_kept(gfs_tri::rot_bin(K1.angle[i], K2.angle[match12[i]]), ind1, ind2, ind3)) {
        match12[i] = -1;
        continue;
      }
    }
    n++;
  }
  return n;
}
#endif

}  // namespace gfs_bow
