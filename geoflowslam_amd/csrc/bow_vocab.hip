// ComputeBoW and the BoW database query on gfx950 (include/gfs_abi.h section 18): the vocabulary transform of
// DBoW2::TemplatedVocabulary::transform (TF_IDF, L1_NORM) for B frames in one call, and the common-word count and L1 score of a query
// against every slot of a database.  The rule is bow_vocab_rule.hpp's; this file spreads it over lanes without changing one rounding.
//
//   k_bow_descend   16 lanes per feature, four features per wave.  Every lane holds the feature's 32 bytes; lane c reads child c's
//                   descriptor and its (first child, child count) from the repacked table in one dependent round per level, the group
//                   takes the minimum of child_key(distance, position), and the winner's lane hands its child's entry to the group.
//   k_bow_vectors   one workgroup per frame.  The surviving features are sorted by (word, index) in LDS (bitonic); the first lane of a
//                   word's run adds the run's weights one after the other; one wave adds the norm in word order, 64 values a round
//                   handed from lane to lane; all lanes divide.  The same pass over (node, index) yields the feature vector.
//   k_bow_score     the query in LDS once per workgroup, one wave per database slot.  Each lane takes the slot's words strided and
//                   binary-searches the query; a ballot per 64 words gives the count and the order in which the terms are added.
#include <memory>
#include <mutex>

#include "bow_vocab_rule.hpp"
#include "gfs_common.hpp"
#include "staging.hpp"

namespace {

using namespace gfs_bowv;

constexpr int kDescendThreads = 256;
constexpr int kFeaturesPerBlock = kDescendThreads / kGroup;
constexpr int kVecThreads = 1024;      // block_scan_1024's width
constexpr int kVecPerThread = 4;
constexpr int kMaxFeatures = kVecThreads * kVecPerThread;  // the keys of one frame: 32 KB of LDS
constexpr int kScoreThreads = 256;
constexpr int kSlotsPerBlock = kScoreThreads / 64;
constexpr int kMaxWords = 4096;        // the query's ids and values: 48 KB of LDS
constexpr unsigned long long kNoFeature = ~0ull;  // sorts behind every key

struct FrameHead {
  int32_t n_words, n_nodes;  // -1, -1: the frame has more key-points than the handle or the stride holds (device entry)
  int32_t n;                 // the frame's count as the kernel read it
};

__device__ __forceinline__ int hamming_u4(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
         __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// the value of lane l (the same l in every lane) of a double
__device__ __forceinline__ double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// desc [B][in_stride][32], counts [B]; f_word / f_weight / f_node [B][out_stride]: the word id (-1 when stopped), the word's weight
// and the node at level_of_nid of every feature i < min(counts[b], in_stride, out_stride)
__global__ __launch_bounds__(kDescendThreads) void k_bow_descend(TreeView T, const uint4* __restrict__ desc, const int32_t* __restrict__ counts,
                                                                 int in_stride, int out_stride, int B, int level_of_nid,
                                                                 int32_t* __restrict__ f_word, double* __restrict__ f_weight,
                                                                 int32_t* __restrict__ f_node) {
  const int sub = threadIdx.x & (kGroup - 1);
  const long long g = (long long)blockIdx.x * kFeaturesPerBlock + threadIdx.x / kGroup;
  const int b = (int)(g / out_stride), i = (int)(g % out_stride);
  if (b >= B) return;  // (a whole group leaves together: the shuffles below stay within a group)
  if (i >= counts[b] || i >= in_stride) return;
  const uint4* fp = desc + 2 * ((size_t)b * in_stride + i);
  const uint4 f0 = fp[0], f1 = fp[1];
  NodeMeta m = T.meta[0];
  int p = 0, level = 0, at = 0;
  while (m.n_children > 0) {
    level++;
    int key = kNoKey;
    NodeMeta mine{0, 0};
    for (int c = sub; c < m.n_children; c += kGroup) {
      const size_t q = (size_t)m.first_child + c;
      const uint4* cp = reinterpret_cast<const uint4*>(T.desc + 8 * q);
      const uint4 c0 = cp[0], c1 = cp[1];
      const NodeMeta cm = T.meta[q];
      const int k = child_key(hamming_u4(f0, f1, c0, c1), c);
      if (k < key) key = k, mine = cm;
    }
    int best = key;
#pragma unroll
    for (int o = kGroup / 2; o >= 1; o >>= 1) best = min(best, __shfl_xor(best, o, kGroup));
    const int pos = key_position(best);
    p = m.first_child + pos;
    // the lane that looked at position pos holds the winning key, and with it the winner's entry
    m.first_child = __shfl(mine.first_child, pos & (kGroup - 1), kGroup);
    m.n_children = __shfl(mine.n_children, pos & (kGroup - 1), kGroup);
    if (level == level_of_nid) at = p;
  }
  if (sub == 0) {
    const size_t o = (size_t)b * out_stride + i;
    const double w = T.weight[p];
    f_weight[o] = w;
    f_word[o] = stopped(w) ? -1 : T.word[p];
    f_node[o] = T.orig[at];
  }
}

// ascending bitonic sort of s_key[0 .. P), P a power of two, by the whole workgroup
__device__ __forceinline__ void bitonic_sort(unsigned long long* s_key, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < P / 2; t += kVecThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = s_key[i], c = s_key[l];
        if ((a > c) == ((i & k) == 0)) s_key[i] = c, s_key[l] = a;
      }
      __syncthreads();
    }
}

// one workgroup per frame; the per-frame arrays have stride S (node_start S + 1)
__global__ __launch_bounds__(kVecThreads) void k_bow_vectors(const int32_t* __restrict__ counts, int in_stride, int S, int max_features,
                                                             const int32_t* __restrict__ f_word, const double* __restrict__ f_weight,
                                                             const int32_t* __restrict__ f_node, FrameHead* __restrict__ heads,
                                                             int32_t* __restrict__ word_id, double* word_value, int32_t* __restrict__ node_id,
                                                             int32_t* __restrict__ node_start, int32_t* __restrict__ feat_idx) {
  __shared__ unsigned long long s_key[kMaxFeatures];
  __shared__ int s_wave[16];
  __shared__ double s_norm;
  __shared__ int s_m;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = counts[b];
  f_word += (size_t)b * S, f_weight += (size_t)b * S, f_node += (size_t)b * S;
  word_id += (size_t)b * S, word_value += (size_t)b * S, node_id += (size_t)b * S, feat_idx += (size_t)b * S;
  node_start += (size_t)b * (S + 1);
  if (n < 0 || n > max_features || n > in_stride || n > S) {  // (the whole workgroup: n is the same in every thread)
    if (t == 0) heads[b] = FrameHead{-1, -1, n};
    return;
  }
  if (n == 0) {
    if (t == 0) heads[b] = FrameHead{0, 0, 0}, node_start[0] = 0;
    return;
  }
  int P = 64;
  while (P < n) P <<= 1;  // <= kMaxFeatures
  for (int pass = 0; pass < 2; pass++) {  // 0: the BowVector by (word, index); 1: the FeatureVector by (node, index)
    const int32_t* id = pass ? f_node : f_word;
    for (int i = t; i < P; i += kVecThreads) s_key[i] = (i < n && f_word[i] >= 0) ? sort_key(id[i], i) : kNoFeature;
    if (t == 0) s_m = 0;
    __syncthreads();
    bitonic_sort(s_key, P);
    // the first position of every run of one id, ranked in order
    bool head[kVecPerThread];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < kVecPerThread; e++) {
      const int j = kVecPerThread * t + e;
      head[e] = j < P && s_key[j] != kNoFeature && (j == 0 || (s_key[j] >> 32) != (s_key[j - 1] >> 32));
      cnt += head[e];
      if (j < P && s_key[j] != kNoFeature && (j + 1 == P || s_key[j + 1] == kNoFeature)) s_m = j + 1;  // the survivors
    }
    int total;
    int r = gfs::block_scan_1024(cnt, s_wave, &total);
    const int m = s_m;  // (written before the scan's barriers)
#pragma unroll
    for (int e = 0; e < kVecPerThread; e++) {
      const int j = kVecPerThread * t + e;
      if (j < m && pass) feat_idx[j] = (int)(s_key[j] & 0xffffffffu);
      if (!head[e]) continue;
      const int v = (int)(s_key[j] >> 32);
      if (pass) {
        node_id[r] = v;
        node_start[r] = j;
      } else {
        // addWeight in feature order: the first hit sets, every later one += (a word's features all carry the word's weight)
        const double w = f_weight[(int)(s_key[j] & 0xffffffffu)];
        double sum = w;
        for (int jj = j + 1; jj < m && (int)(s_key[jj] >> 32) == v; jj++) sum += w;
        word_id[r] = v;
        word_value[r] = sum;
      }
      r++;
    }
    if (pass) {
      if (t == 0) heads[b].n_nodes = total, node_start[total] = m;
      break;
    }
    if (t == 0) heads[b].n_words = total, heads[b].n = n;
    __syncthreads();
    // BowVector::normalize(L1): the norm from 0.0 in ascending word id, one addition after the other.  Wave 0 reads 64 values a round
    // and every lane adds them in lane order (a round's tail adds +0.0, which changes no bit of a sum that is never -0.0).
    if (t < 64) {
      double norm = 0.0;
      for (int base = 0; base < total; base += 64) {
        const double v = base + t < total ? fabs(word_value[base + t]) : 0.0;
#pragma unroll
        for (int l = 0; l < 64; l++) norm += lane_value(v, l);
      }
      if (t == 0) s_norm = norm;
    }
    __syncthreads();
    const double norm = s_norm;
    if (norm > 0.0)
      for (int q = t; q < total; q += kVecThreads) word_value[q] /= norm;
    __syncthreads();  // s_key and s_m are rewritten by the next pass
  }
}

// qid / qval [nq] the query; counts [max_entries], db_id / db_val [max_entries][max_words] the store
__global__ __launch_bounds__(kScoreThreads) void k_bow_score(int nq, const int32_t* __restrict__ qid, const double* __restrict__ qval,
                                                             int max_entries, int max_words, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ db_id, const double* __restrict__ db_val,
                                                             int32_t* __restrict__ n_common, int32_t* __restrict__ first_word,
                                                             float* __restrict__ score) {
  __shared__ int32_t s_qid[kMaxWords];
  __shared__ double s_qval[kMaxWords];
  for (int i = threadIdx.x; i < nq; i += kScoreThreads) s_qid[i] = qid[i], s_qval[i] = qval[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, slot = blockIdx.x * kSlotsPerBlock + (threadIdx.x >> 6);
  if (slot >= max_entries) return;  // (a whole wave, after the only barrier)
  const int nd = counts[slot];
  const int32_t* id = db_id + (size_t)slot * max_words;
  const double* val = db_val + (size_t)slot * max_words;
  int cnt = 0, first = 0x7fffffff;
  double s = 0;
  for (int base = 0; base < nd; base += 64) {
    const int j = base + lane;
    bool hit = false;
    double term = 0;
    if (j < nd) {
      const int w = id[j];
      int lo = 0, hi = nq;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_qid[mid] < w) lo = mid + 1; else hi = mid;
      }
      hit = lo < nq && s_qid[lo] == w;
      if (hit) {
        term = l1_term(s_qval[lo], val[j]);
        first = min(first, w);
      }
    }
    // the common words of this block in ascending id are the set lanes in ascending order: every lane adds their terms in that order
    unsigned long long mask = __ballot(hit);
    cnt += __popcll(mask);
    while (mask) {
      const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
      s += lane_value(term, l);
      mask &= mask - 1;
    }
  }
  first = gfs::wave_min_i32(first);
  if (lane == 0) {
    n_common[slot] = cnt;
    first_word[slot] = cnt ? first : -1;
    score[slot] = cnt ? l1_finish(s) : 0.0f;
  }
}

}  // namespace

struct gfs_bow_vocab {
  int device, max_batch, max_features;
  hipStream_t stream;
  std::mutex mu;
  int L, min_leaf_depth, n_words, n_nodes;
  gfs::DevBuf<NodeMeta> d_meta;
  gfs::DevBuf<unsigned> d_desc;
  gfs::DevBuf<int32_t> d_word, d_orig;
  gfs::DevBuf<double> d_weight;
  // one pinned block mirroring one device block for the inputs, one for the outputs: a call is one copy in, two kernels, one copy out
  struct Layout {  // S: features per frame
    gfs::Block<256> in, res;
    gfs::Field<int32_t> counts;
    gfs::Field<uint8_t, 32> desc;
    gfs::Field<FrameHead> heads;
    gfs::Field<int32_t> word_id, node_id, node_start, feat_idx, f_word;
    gfs::Field<double> word_value;
    Layout(size_t B, size_t S)
        : counts(in, B), desc(in, B * S), heads(res, B), word_id(res, B * S), node_id(res, B * S), node_start(res, B * (S + 1)),
          feat_idx(res, B * S), f_word(res, B * S), word_value(res, B * S) {}
  };
  gfs::Mirror in, res;
  gfs::DevBuf<double> d_f_weight;
  gfs::DevBuf<int32_t> d_f_node;
  TreeView view() const { return TreeView{d_meta.p, d_desc.p, d_word.p, d_weight.p, d_orig.p}; }
};

struct gfs_bow_db {
  int device, max_entries, max_words;
  hipStream_t stream;
  std::mutex mu;
  struct Layout {
    gfs::Block<256> in, res;
    gfs::Field<int32_t> counts, qid;
    gfs::Field<double> qval;
    gfs::Field<int32_t> n_common, first_word;
    gfs::Field<float> score;
    Layout(size_t E, size_t W) : counts(in, E), qid(in, W), qval(in, W), n_common(res, E), first_word(res, E), score(res, E) {}
  };
  gfs::Mirror in, res;  // in.h's counts are the store's occupancy: they travel with every query
  gfs::PinBuf<uint8_t> stage;  // one slot on its way up: ids, then values
  gfs::DevBuf<int32_t> d_id;
  gfs::DevBuf<double> d_val;
};

namespace {

int check_vectors(const gfs_bow_vectors* out, int B, const char* who) {
  for (int b = 0; b < B; b++)
    GFS_REQUIRE(out[b].word_id && out[b].word_value && out[b].node_id && out[b].node_start && out[b].feat_idx, GFS_ERR_INVALID_ARG,
                "%s: frame %d has NULL output arrays", who, b);
  return GFS_OK;
}

// the two kernels, the download and the synchronisation of both entries
int run_transform(gfs_bow_vocab* h, const gfs_bow_vocab::Layout& L, const uint8_t* d_descs, const int32_t* d_counts, int in_stride, int S, int B, int levelsup,
                  gfs_bow_vectors* out, const char* who) {
  hipStream_t s = h->stream;
  uint8_t* dr = h->res.d.p;
  const long long slots = (long long)B * S;
  GFS_LAUNCH("k_bow_descend", k_bow_descend, dim3((unsigned)((slots + kFeaturesPerBlock - 1) / kFeaturesPerBlock)), dim3(kDescendThreads), 0, s,
             h->view(), reinterpret_cast<const uint4*>(d_descs), d_counts, in_stride, S, B, nid_level(h->L, levelsup), L.f_word.at(dr),
             h->d_f_weight.p, h->d_f_node.p);
  GFS_LAUNCH("k_bow_vectors", k_bow_vectors, dim3(B), dim3(kVecThreads), 0, s, d_counts, in_stride, S, h->max_features, L.f_word.at(dr),
             h->d_f_weight.p, h->d_f_node.p, L.heads.at(dr), L.word_id.at(dr), L.word_value.at(dr), L.node_id.at(dr), L.node_start.at(dr),
             L.feat_idx.at(dr));
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  for (int b = 0; b < B; b++)
    GFS_REQUIRE(L.heads.at(hr)[b].n_words >= 0, GFS_ERR_CAPACITY, "%s: frame %d has more key-points than the handle's %d or the stride %d", who, b,
                h->max_features, in_stride);
  for (int b = 0; b < B; b++) {
    const FrameHead& H = L.heads.at(hr)[b];
    gfs_bow_vectors& o = out[b];
    o.n_words = H.n_words;
    o.n_nodes = H.n_nodes;
    L.word_id.get(o.word_id, hr, (size_t)b * S, (size_t)H.n_words);
    L.word_value.get(o.word_value, hr, (size_t)b * S, (size_t)H.n_words);
    L.node_id.get(o.node_id, hr, (size_t)b * S, (size_t)H.n_nodes);
    L.node_start.get(o.node_start, hr, (size_t)b * (S + 1), (size_t)H.n_nodes + 1);
    const int m = L.node_start.at(hr, (size_t)b * (S + 1))[H.n_nodes];
    L.feat_idx.get(o.feat_idx, hr, (size_t)b * S, (size_t)m);
    if (o.word_of_feature) L.f_word.get(o.word_of_feature, hr, (size_t)b * S, (size_t)H.n);
  }
  return GFS_OK;
}

}  // namespace

extern "C" {

int gfs_bow_create(int device, const gfs_bow_vocabulary* v, int max_batch, int max_features, gfs_bow_vocab** out) {
  GFS_REQUIRE(out && v && max_batch > 0 && max_features > 0, GFS_ERR_INVALID_ARG, "gfs_bow_create: invalid argument");
  GFS_REQUIRE(max_features <= kMaxFeatures, GFS_ERR_UNSUPPORTED, "gfs_bow_create: max_features %d above %d (one workgroup sorts a frame in LDS)",
              max_features, kMaxFeatures);
  PackedTree P;
  if (const char* why = pack_tree(v, P)) {
    gfs::set_error("gfs_bow_create: %s", why);
    return GFS_ERR_INVALID_ARG;
  }
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_bow_vocab> h(new gfs_bow_vocab);
  h->device = device;
  h->max_batch = max_batch;
  h->max_features = max_features;
  h->L = P.L;
  h->min_leaf_depth = P.min_leaf_depth;
  h->n_words = P.n_words;
  h->n_nodes = v->n_nodes;
  const size_t n = (size_t)v->n_nodes, Smax = gfs::align_up((size_t)max_features, kGroup);
  const gfs_bow_vocab::Layout L{(size_t)max_batch, Smax};
  int rc = h->d_meta.alloc(n);
  if (!rc) rc = h->d_desc.alloc(8 * n);
  if (!rc) rc = h->d_word.alloc(n);
  if (!rc) rc = h->d_orig.alloc(n);
  if (!rc) rc = h->d_weight.alloc(n);
  if (!rc) rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->d_f_weight.alloc(max_batch * Smax);
  if (!rc) rc = h->d_f_node.alloc(max_batch * Smax);
  if (rc) return rc;
  GFS_HIP(hipMemcpy(h->d_meta.p, P.meta.data(), n * sizeof(NodeMeta), hipMemcpyHostToDevice));
  GFS_HIP(hipMemcpy(h->d_desc.p, P.desc.data(), 8 * n * sizeof(unsigned), hipMemcpyHostToDevice));
  GFS_HIP(hipMemcpy(h->d_word.p, P.word.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  GFS_HIP(hipMemcpy(h->d_orig.p, P.orig.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  GFS_HIP(hipMemcpy(h->d_weight.p, P.weight.data(), n * sizeof(double), hipMemcpyHostToDevice));
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  *out = h.release();
  return GFS_OK;
}

void gfs_bow_destroy(gfs_bow_vocab* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_bow_transform(gfs_bow_vocab* h, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out) {
  GFS_REQUIRE(h && B >= 0 && (B == 0 || (desc && n && out)), GFS_ERR_INVALID_ARG, "gfs_bow_transform: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_bow_transform: batch %d exceeds capacity %d", B, h->max_batch);
  GFS_REQUIRE(levelsup >= 0, GFS_ERR_INVALID_ARG, "gfs_bow_transform: levelsup = %d", levelsup);
  GFS_REQUIRE(nid_defined(h->L, levelsup, h->min_leaf_depth), GFS_ERR_INVALID_ARG,
              "gfs_bow_transform: the vocabulary has a leaf at depth %d, above level L - levelsup = %d: the reference leaves its node undefined",
              h->min_leaf_depth, nid_level(h->L, levelsup));
  int S = kGroup;
  for (int b = 0; b < B; b++) {
    GFS_REQUIRE(n[b] >= 0, GFS_ERR_INVALID_ARG, "gfs_bow_transform: frame %d has n = %d", b, n[b]);
    GFS_REQUIRE(n[b] <= h->max_features, GFS_ERR_CAPACITY, "gfs_bow_transform: frame %d has %d features (capacity %d)", b, n[b], h->max_features);
    GFS_REQUIRE(n[b] == 0 || desc[b], GFS_ERR_INVALID_ARG, "gfs_bow_transform: frame %d has NULL descriptors", b);
    S = std::max(S, (int)gfs::align_up((size_t)n[b], kGroup));
  }
  if (int rc = check_vectors(out, B, "gfs_bow_transform")) return rc;
  if (B == 0) return GFS_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_bow_vocab::Layout L{(size_t)B, (size_t)S};
  uint8_t* hi = h->in.h.p;
  for (int b = 0; b < B; b++) {
    L.counts.at(hi)[b] = n[b];
    L.desc.put(hi, (size_t)b * S, desc[b], (size_t)n[b]);
  }
  if (int rc = h->in.upload(h->stream, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  return run_transform(h, L, L.desc.at(di), L.counts.at(di), S, S, B, levelsup, out, "gfs_bow_transform");
}

int gfs_bow_transform_device(gfs_bow_vocab* h, const void* dev_desc, const void* dev_counts, int stride, int B, int levelsup, gfs_bow_vectors* out) {
  GFS_REQUIRE(h && B >= 0 && (B == 0 || (dev_desc && dev_counts && out && stride > 0)), GFS_ERR_INVALID_ARG,
              "gfs_bow_transform_device: invalid argument");
  GFS_REQUIRE(((uintptr_t)dev_desc & 15) == 0, GFS_ERR_INVALID_ARG, "gfs_bow_transform_device: dev_desc is not 16-byte aligned");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_bow_transform_device: batch %d exceeds capacity %d", B, h->max_batch);
  GFS_REQUIRE(levelsup >= 0, GFS_ERR_INVALID_ARG, "gfs_bow_transform_device: levelsup = %d", levelsup);
  GFS_REQUIRE(nid_defined(h->L, levelsup, h->min_leaf_depth), GFS_ERR_INVALID_ARG,
              "gfs_bow_transform_device: the vocabulary has a leaf at depth %d, above level L - levelsup = %d", h->min_leaf_depth,
              nid_level(h->L, levelsup));
  if (int rc = check_vectors(out, B, "gfs_bow_transform_device")) return rc;
  if (B == 0) return GFS_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  // the counts are on the device: the outputs take the handle's full stride
  const int S = (int)gfs::align_up((size_t)h->max_features, kGroup);
  const gfs_bow_vocab::Layout L{(size_t)B, (size_t)S};
  return run_transform(h, L, (const uint8_t*)dev_desc, (const int32_t*)dev_counts, stride, S, B, levelsup, out, "gfs_bow_transform_device");
}

int gfs_bow_db_create(int device, int max_entries, int max_words, gfs_bow_db** out) {
  GFS_REQUIRE(out && max_entries > 0 && max_words > 0, GFS_ERR_INVALID_ARG, "gfs_bow_db_create: invalid argument");
  GFS_REQUIRE(max_words <= kMaxWords, GFS_ERR_UNSUPPORTED, "gfs_bow_db_create: max_words %d above %d (the query lives in LDS)", max_words, kMaxWords);
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_bow_db> h(new gfs_bow_db);
  h->device = device;
  h->max_entries = max_entries;
  h->max_words = max_words;
  const gfs_bow_db::Layout L{(size_t)max_entries, (size_t)max_words};
  int rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->stage.alloc((size_t)max_words * (sizeof(int32_t) + sizeof(double)));
  if (!rc) rc = h->d_id.alloc((size_t)max_entries * max_words);
  if (!rc) rc = h->d_val.alloc((size_t)max_entries * max_words);
  if (rc) return rc;
  memset(L.counts.at(h->in.h.p), 0, L.counts.bytes((size_t)max_entries));
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  *out = h.release();
  return GFS_OK;
}

void gfs_bow_db_destroy(gfs_bow_db* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_bow_db_add(gfs_bow_db* h, int slot, int n_words, const int32_t* word_id, const double* word_value) {
  GFS_REQUIRE(h && n_words >= 0 && (n_words == 0 || (word_id && word_value)), GFS_ERR_INVALID_ARG, "gfs_bow_db_add: invalid argument");
  GFS_REQUIRE(slot >= 0 && slot < h->max_entries, GFS_ERR_INVALID_ARG, "gfs_bow_db_add: slot %d outside [0, %d)", slot, h->max_entries);
  GFS_REQUIRE(n_words <= h->max_words, GFS_ERR_CAPACITY, "gfs_bow_db_add: %d words (capacity %d)", n_words, h->max_words);
  GFS_REQUIRE(valid_bow_vector(n_words, word_id, word_value), GFS_ERR_INVALID_ARG,
              "gfs_bow_db_add: word ids not strictly ascending from >= 0, or a value that is not finite");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_bow_db::Layout L{(size_t)h->max_entries, (size_t)h->max_words};
  if (n_words) {
    int32_t* ids = reinterpret_cast<int32_t*>(h->stage.p + (size_t)h->max_words * sizeof(double));
    double* vals = reinterpret_cast<double*>(h->stage.p);
    memcpy(ids, word_id, (size_t)n_words * sizeof(int32_t));
    memcpy(vals, word_value, (size_t)n_words * sizeof(double));
    GFS_HIP(hipMemcpyAsync(h->d_id.p + (size_t)slot * h->max_words, ids, (size_t)n_words * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    GFS_HIP(hipMemcpyAsync(h->d_val.p + (size_t)slot * h->max_words, vals, (size_t)n_words * sizeof(double), hipMemcpyHostToDevice, h->stream));
    GFS_HIP(hipStreamSynchronize(h->stream));
  }
  L.counts.at(h->in.h.p)[slot] = n_words;
  return GFS_OK;
}

int gfs_bow_db_erase(gfs_bow_db* h, int slot) {
  GFS_REQUIRE(h, GFS_ERR_INVALID_ARG, "gfs_bow_db_erase: invalid argument");
  GFS_REQUIRE(slot >= 0 && slot < h->max_entries, GFS_ERR_INVALID_ARG, "gfs_bow_db_erase: slot %d outside [0, %d)", slot, h->max_entries);
  std::lock_guard<std::mutex> lk(h->mu);
  const gfs_bow_db::Layout L{(size_t)h->max_entries, (size_t)h->max_words};
  L.counts.at(h->in.h.p)[slot] = 0;
  return GFS_OK;
}

int gfs_bow_db_query(gfs_bow_db* h, int n_words, const int32_t* word_id, const double* word_value, int32_t* n_common, int32_t* first_word,
                     float* score) {
  GFS_REQUIRE(h && n_words >= 0 && (n_words == 0 || (word_id && word_value)) && n_common && first_word && score, GFS_ERR_INVALID_ARG,
              "gfs_bow_db_query: invalid argument");
  GFS_REQUIRE(n_words <= h->max_words, GFS_ERR_CAPACITY, "gfs_bow_db_query: %d words (capacity %d)", n_words, h->max_words);
  GFS_REQUIRE(valid_bow_vector(n_words, word_id, word_value), GFS_ERR_INVALID_ARG,
              "gfs_bow_db_query: word ids not strictly ascending from >= 0, or a value that is not finite");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const size_t E = (size_t)h->max_entries;
  const gfs_bow_db::Layout L{E, (size_t)h->max_words};
  uint8_t* hi = h->in.h.p;
  L.qid.put(hi, 0, word_id, (size_t)n_words);
  L.qval.put(hi, 0, word_value, (size_t)n_words);
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  uint8_t* dr = h->res.d.p;
  GFS_LAUNCH("k_bow_score", k_bow_score, dim3(gfs::div_up(h->max_entries, kSlotsPerBlock)), dim3(kScoreThreads), 0, s, n_words, L.qid.at(di),
             L.qval.at(di), h->max_entries, h->max_words, L.counts.at(di), h->d_id.p, h->d_val.p, L.n_common.at(dr), L.first_word.at(dr),
             L.score.at(dr));
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  L.n_common.get(n_common, hr, 0, E);
  L.first_word.get(first_word, hr, 0, E);
  L.score.get(score, hr, 0, E);
  return GFS_OK;
}

}  // extern "C"
