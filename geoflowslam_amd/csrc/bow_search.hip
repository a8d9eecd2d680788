// ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (reference src/ORBmatcher.cc:936-1053) on the gfs_sbp handle: gfs_sbp_reserve_bow
// and gfs_search_by_bow (include/gfs_abi.h).  The rule is bow_search_rule.hpp, shared with the host.
//
// One launch.  k_bow_search: one workgroup per slot, a slot being one (key frame 1, key frame 2) pair.  The waves take the nodes of
// key frame 1 in turn, find the node in key frame 2's ascending ids by binary search (the merge walk visits exactly the common ids)
// and walk the node's idx1 list in order.  The lanes hold the node's idx2 list, position 64 c + lane in chunk c: the descriptors of
// chunk 0 stay in registers, later chunks are read again per idx1; one bit per chunk and lane says "has a map point and is not yet
// matched" (vbMatched2: the lists of different nodes are disjoint, so no other wave ever needs the bit).  Every lane scans its own
// positions with the rule's best_offer; two wave reductions merge the 64 scans as the rule's best_merge does: the minimum key
// (distance, then position) and the minimum over everything else.  There is no distance matrix.  After a barrier the workgroup
// counts the rotation bins in LDS (integer adds: any order gives the same counts), one thread picks the three maxima and the
// matches outside them go back to -1.  No global atomics; the results do not depend on scheduling.
#include <algorithm>
#include <climits>

#include "bow_search_rule.hpp"
#include "sbp_handle.hpp"

namespace {

constexpr int kBowThreads = 1024, kBowWaves = kBowThreads / 64;
constexpr int kMaxKp = 4096;  // key-points of a key frame (the handle's limit): 64 chunks of 64 list positions, one bit each
static_assert(kMaxKp <= 64 * 64 && kMaxKp - 1 < gfs_bow::kNoPosition, "a list position fits a lane's chunk mask and a key's low half");

struct BowFrame {  // a key frame on the device: its counts and the byte offsets of its arrays in the input block
  int n_kp, n_nodes;
  unsigned o_ang, o_hasmp, o_desc, o_nid, o_nstart, o_feat;
};

struct BowSlot {  // one (key frame 1, key frame 2)
  int f1, f2;        // the two frames
  unsigned out_at;   // element index of the slot's match12
  float nn_ratio;
  int check_orientation;
};

struct Desc {
  uint4 a, b;
};

__device__ __forceinline__ Desc load_desc(const uint8_t* __restrict__ desc, int i) {
  const uint4* d = reinterpret_cast<const uint4*>(desc) + 2 * (size_t)i;
  return Desc{d[0], d[1]};
}

__device__ __forceinline__ int desc_distance(const Desc& p, const Desc& q) {
  const unsigned x[8] = {p.a.x, p.a.y, p.a.z, p.a.w, p.b.x, p.b.y, p.b.z, p.b.w};
  const unsigned y[8] = {q.a.x, q.a.y, q.a.z, q.a.w, q.b.x, q.b.y, q.b.z, q.b.w};
  return gfs_bow::descriptor_distance(x, y);
}

__global__ __launch_bounds__(kBowThreads) void k_bow_search(const uint8_t* __restrict__ in, const BowSlot* __restrict__ slots,
                                                            const BowFrame* __restrict__ frames, int* __restrict__ o_match) {
  __shared__ int s_hist[gfs_bow::kHisto], s_ind[3];
  const BowSlot S = slots[blockIdx.x];
  const BowFrame F1 = frames[S.f1], F2 = frames[S.f2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N1 = F1.n_kp;
  int* match12 = o_match + S.out_at;
  for (int i = tid; i < N1; i += kBowThreads) match12[i] = -1;
  if (tid < gfs_bow::kHisto) s_hist[tid] = 0;
  __syncthreads();
  const int* nid1 = reinterpret_cast<const int*>(in + F1.o_nid);
  const int* ns1 = reinterpret_cast<const int*>(in + F1.o_nstart);
  const int* nid2 = reinterpret_cast<const int*>(in + F2.o_nid);
  const int* ns2 = reinterpret_cast<const int*>(in + F2.o_nstart);
  const uint8_t *has1 = in + F1.o_hasmp, *has2 = in + F2.o_hasmp, *desc1 = in + F1.o_desc, *desc2 = in + F2.o_desc;
  // ---- the search: the merge loop of :964-1034, a node per wave
  for (int node = wave; node < F1.n_nodes; node += kBowWaves) {
    const int j = gfs::find_node(nid2, F2.n_nodes, nid1[node]);
    if (j < 0) continue;
    const int b1 = ns1[node], n1 = ns1[node + 1] - b1, b2 = ns2[j], n2 = ns2[j + 1] - b2;
    if (n1 <= 0 || n2 <= 0) continue;
    const int* feat1 = reinterpret_cast<const int*>(in + F1.o_feat) + b1;
    const int* feat2 = reinterpret_cast<const int*>(in + F2.o_feat) + b2;
    const int chunks = (n2 + 63) >> 6;  // <= 64: n2 <= n_kp <= kMaxKp
    unsigned long long open = 0;        // bit c: this lane's position 64 c + lane has a map point and is not matched yet
    Desc d0 = Desc{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    for (int c = 0; c < chunks; c++) {
      const int p = 64 * c + lane;
      if (p < n2) {
        const int idx2 = feat2[p];
        if (has2[idx2]) open |= 1ull << c;
        if (c == 0) d0 = load_desc(desc2, idx2);
      }
    }
    for (int i1b = 0; i1b < n1; i1b += 64) {
      // 64 list entries of key frame 1 at once: their indices and pMP1 flags; the walk then visits the eligible ones in order
      int my1 = 0;
      bool eligible = false;
      if (i1b + lane < n1) {
        my1 = feat1[i1b + lane];
        eligible = has1[my1] != 0;
      }
      unsigned long long todo = __ballot(eligible);
      if (todo == 0) continue;
      int idx1 = __builtin_amdgcn_readfirstlane(__shfl(my1, __builtin_ctzll(todo)));
      todo &= todo - 1;
      Desc d1 = load_desc(desc1, idx1);
      for (;;) {
        const bool more = todo != 0;  // the next idx1's descriptor is on its way while this one is scanned
        int idx1_next = 0;
        Desc d1_next = d1;
        if (more) {
          idx1_next = __builtin_amdgcn_readfirstlane(__shfl(my1, __builtin_ctzll(todo)));
          todo &= todo - 1;
          d1_next = load_desc(desc1, idx1_next);
        }
        gfs_bow::Best b = gfs_bow::best_init();
        if (open & 1ull) gfs_bow::best_offer(b, desc_distance(d1, d0), lane);
        for (int c = 1; c < chunks; c++) {
          if (open >> c & 1ull) {
            const int p = 64 * c + lane;
            gfs_bow::best_offer(b, desc_distance(d1, load_desc(desc2, feat2[p])), p);
          }
        }
        // the 64 scans merged (gfs_bow::best_merge, all at once): the smallest key wins, bestDist2 is the smallest of the winner's
        // own second and every other lane's best
        const int key1 = gfs::wave_min_i32(b.key1);
        const int dist2 = gfs::wave_min_i32(b.key1 == key1 ? b.dist2 : gfs_bow::key_dist(b.key1));
        if (gfs_bow::accept(gfs_bow::key_dist(key1), dist2, S.nn_ratio)) {
          const int p = gfs_bow::key_position(key1);
          if ((p & 63) == lane) {
            open &= ~(1ull << (p >> 6));  // vbMatched2[bestIdx2] = true
            match12[idx1] = feat2[p];
          }
        }
        if (!more) break;
        idx1 = idx1_next;
        d1 = d1_next;
      }
    }
  }
  __syncthreads();
  // ---- the rotation histogram (:1014-1021, :1036-1050)
  if (S.check_orientation) {
    const float* ang1 = reinterpret_cast<const float*>(in + F1.o_ang);
    const float* ang2 = reinterpret_cast<const float*>(in + F2.o_ang);
    for (int i = tid; i < N1; i += kBowThreads) {
      const int m = match12[i];
      if (m < 0) continue;
      const int bin = gfs_tri::rot_bin(ang1[i], ang2[m]);
      if (gfs_bow::bin_in_histogram(bin)) atomicAdd(&s_hist[bin], 1);
    }
    __syncthreads();
    if (tid == 0) gfs_tri::three_maxima(s_hist, s_ind[0], s_ind[1], s_ind[2]);
    __syncthreads();
    const int ind1 = s_ind[0], ind2 = s_ind[1], ind3 = s_ind[2];
    for (int i = tid; i < N1; i += kBowThreads) {  // (the thread that read match12[i] above)
      const int m = match12[i];
      if (m < 0) continue;
      if (!gfs_bow::bin_kept(gfs_tri::rot_bin(ang1[i], ang2[m]), ind1, ind2, ind3)) match12[i] = -1;
    }
  }
}

using HeadLayout = gfs::BowHeadLayout<BowSlot, BowFrame>;

}  // namespace

struct gfs_bow_workspace : gfs_sbp_workspace {
  int max_problems = 0, max_kf2 = 0;
  gfs::Mirror in, out;
  size_t in_bytes = 0, out_elems = 0;
};

namespace {

int validate_kf(const gfs_bow_keyframe& k, int max_cur, const char* what, int b, int i, std::vector<uint8_t>& seen) {
  GFS_REQUIRE(k.n_kp >= 0 && k.n_kp <= max_cur, GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d %s %d has %d key-points (the handle's limit is %d)",
              b, what, i, k.n_kp, max_cur);
  GFS_REQUIRE(k.n_nodes >= 0 && k.n_nodes <= max_cur, GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d %s %d has %d nodes (the handle's limit is %d)",
              b, what, i, k.n_nodes, max_cur);
  GFS_REQUIRE(k.n_kp == 0 || (k.angle && k.desc && k.has_mp), GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d %s %d has NULL key-point arrays", b,
              what, i);
  GFS_REQUIRE(k.node_start && (k.n_nodes == 0 || k.node_id), GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d %s %d has NULL node arrays", b, what, i);
  return gfs::check_feature_vector("gfs_search_by_bow", k, what, b, i, seen);
}

// takes a key frame's arrays from the staging block's cursor, copies them there and fills its device header
void stage_kf(const gfs_bow_keyframe& k, uint8_t* base, gfs::Block<256>& in, BowFrame& F) {
  const size_t n = (size_t)k.n_kp, m = (size_t)k.n_nodes, nf = (size_t)k.node_start[k.n_nodes];
  const gfs::BowKfArrays A{in, n, m, nf};
  F.n_kp = k.n_kp;
  F.n_nodes = k.n_nodes;
  F.o_ang = (unsigned)A.ang.off;
  F.o_hasmp = (unsigned)A.hasmp.off;
  F.o_desc = (unsigned)A.desc.off;
  F.o_nid = (unsigned)A.nid.off;
  F.o_nstart = (unsigned)A.nstart.off;
  F.o_feat = (unsigned)A.feat.off;
  A.ang.put(base, 0, k.angle, n);
  A.hasmp.put(base, 0, k.has_mp, n);
  A.desc.put(base, 0, k.desc, n);
  A.nid.put(base, 0, k.node_id, m);
  A.nstart.put(base, 0, k.node_start, m + 1);
  A.feat.put(base, 0, k.feat_idx, nf);
}

}  // namespace

extern "C" {

int gfs_sbp_reserve_bow(gfs_sbp* h, int max_problems, int max_kf2_per_call) {
  GFS_REQUIRE(h && max_problems > 0 && max_kf2_per_call > 0, GFS_ERR_INVALID_ARG, "gfs_sbp_reserve_bow: invalid argument");
  GFS_REQUIRE(h->max_cur <= kMaxKp, GFS_ERR_UNSUPPORTED, "gfs_sbp_reserve_bow: the handle's max_cur %d is above %d", h->max_cur, kMaxKp);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipStreamSynchronize(h->stream));
  h->bow.reset();
  std::unique_ptr<gfs_bow_workspace> w(new gfs_bow_workspace);
  const size_t P = (size_t)max_problems, K2 = (size_t)max_kf2_per_call, SC = gfs::align_up((size_t)h->max_cur, 64);
  gfs::Block<256> one_kf;
  const gfs::BowKfArrays widest{one_kf, SC, SC, SC};  // a key frame of the capacity: SC key-points, as many nodes, every key-point listed
  w->in_bytes = HeadLayout{K2, P + K2}.in.bytes() + (P + K2) * widest.in.bytes();
  GFS_REQUIRE(w->in_bytes < 0xffffffffull, GFS_ERR_UNSUPPORTED, "gfs_sbp_reserve_bow: the input block would exceed 4 GiB");
  w->out_elems = K2 * SC;
  int rc = 0;
  if (!rc) rc = w->in.alloc(w->in_bytes);
  if (!rc) rc = w->out.alloc(w->out_elems * sizeof(int));
  if (rc) return rc;
  w->max_problems = max_problems;
  w->max_kf2 = max_kf2_per_call;
  h->bow = std::move(w);
  return GFS_OK;
}

int gfs_search_by_bow(gfs_sbp* h, const gfs_bow_problem* problems, int B, gfs_bow_result* const* results) {
  GFS_REQUIRE(h && B >= 0 && (B == 0 || (problems && results)), GFS_ERR_INVALID_ARG, "gfs_search_by_bow: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_bow_workspace* w = static_cast<gfs_bow_workspace*>(h->bow.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_search_by_bow: call gfs_sbp_reserve_bow first");
  GFS_REQUIRE(B <= w->max_problems, GFS_ERR_CAPACITY, "gfs_search_by_bow: %d problems exceed the reserve %d", B, w->max_problems);
  // every refusal comes before anything is staged or written
  std::vector<uint8_t> seen;
  size_t n_slots = 0, out_elems = 0;
  for (int b = 0; b < B; b++) {
    const gfs_bow_problem& Q = problems[b];
    GFS_REQUIRE(Q.n_kf2 >= 0, GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d has %d key frames 2", b, Q.n_kf2);
    GFS_REQUIRE(n_slots + (size_t)Q.n_kf2 <= (size_t)w->max_kf2, GFS_ERR_CAPACITY, "gfs_search_by_bow: more than %d key frames 2 in the call (reserve)",
                w->max_kf2);
    GFS_REQUIRE(Q.n_kf2 == 0 || (Q.kf2 && results[b]), GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d has NULL key frames 2 or results", b);
    if (int rc = validate_kf(Q.kf1, h->max_cur, "key frame 1", b, 0, seen)) return rc;
    for (int i = 0; i < Q.n_kf2; i++) {
      if (int rc = validate_kf(Q.kf2[i], h->max_cur, "key frame 2", b, i, seen)) return rc;
      GFS_REQUIRE(Q.kf1.n_kp == 0 || results[b][i].match12, GFS_ERR_INVALID_ARG, "gfs_search_by_bow: problem %d key frame 2 %d has a NULL match12", b, i);
    }
    n_slots += (size_t)Q.n_kf2;
    out_elems += (size_t)Q.n_kf2 * gfs::align_up((size_t)Q.kf1.n_kp, 64);
  }
  if (n_slots == 0) return GFS_OK;
  GFS_HIP(hipSetDevice(h->device));
  // ---- stage: the headers, then every key frame's arrays; key frame 1 once per problem (all within the reserve: checked above)
  uint8_t* hb = w->in.h.p;
  HeadLayout Y{n_slots, n_slots + (size_t)B};
  BowSlot* slots = Y.slots.at(hb);
  BowFrame* frames = Y.frames.at(hb);
  size_t slot = 0, frame = 0, out_at = 0;
  for (int b = 0; b < B; b++) {
    const gfs_bow_problem& Q = problems[b];
    if (Q.n_kf2 == 0) continue;
    const int f1 = (int)frame;
    stage_kf(Q.kf1, hb, Y.in, frames[frame++]);
    for (int i = 0; i < Q.n_kf2; i++) {
      BowSlot& S = slots[slot++];
      S.f1 = f1;
      S.f2 = (int)frame;
      S.out_at = (unsigned)out_at;
      S.nn_ratio = Q.nn_ratio;
      S.check_orientation = Q.check_orientation;
      out_at += gfs::align_up((size_t)Q.kf1.n_kp, 64);
      stage_kf(Q.kf2[i], hb, Y.in, frames[frame++]);
    }
  }
  const size_t at = Y.in.bytes();
  if (at > w->in_bytes || out_elems > w->out_elems) {  // (cannot happen: the reserve bounds every term above)
    gfs::set_error("gfs_search_by_bow: internal: staged %zu of %zu bytes", at, w->in_bytes);
    return GFS_ERR_CAPACITY;
  }
  if (out_elems > 0) {
    hipStream_t s = h->stream;
    const uint8_t* di = w->in.d.p;
    if (int rc = w->in.upload(s, 0, at)) return rc;
    GFS_LAUNCH("k_bow_search", k_bow_search, dim3((unsigned)n_slots), dim3(kBowThreads), 0, s, di, Y.slots.at(di), Y.frames.at(di),
               reinterpret_cast<int*>(w->out.d.p));
    if (int rc = w->out.download(s, 0, out_elems * sizeof(int))) return rc;
    GFS_HIP(hipStreamSynchronize(s));  // the call's one synchronisation
  }
  const int* ho = reinterpret_cast<const int*>(w->out.h.p);
  slot = 0;
  for (int b = 0; b < B; b++) {
    const size_t n = (size_t)problems[b].kf1.n_kp;
    for (int i = 0; i < problems[b].n_kf2; i++, slot++) {
      gfs_bow_result& R = results[b][i];
      if (n) memcpy(R.match12, ho + slots[slot].out_at, n * sizeof(int));
      int nm = 0;
      for (size_t p = 0; p < n; p++) nm += R.match12[p] >= 0;
      R.n_matches = nm;
    }
  }
  return GFS_OK;
}

}  // extern "C"
