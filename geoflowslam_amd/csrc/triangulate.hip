// LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:803-1127) on the gfs_sbp handle: gfs_sbp_reserve_triangulation and
// gfs_create_new_map_points (include/gfs_abi.h).  The rule is triangulate_rule.hpp, shared with the host.
//
// Two launches, and the kernel boundary is the only hand-off between workgroups:
//   k_tri_candidates  one workgroup per (problem, neighbour, node of the current key frame): finds the node in the neighbour's ids
//                     by binary search and writes one byte per key-point pair of the node into its n1 x n2 matrix: the Hamming
//                     distance 0..50 of a pair that passes the entry-state filters and the gates, 255 otherwise.  Nothing here
//                     depends on what the call creates: map-point state only grows, so a pair out at entry stays out.
//   k_tri_resolve     one workgroup per problem, the neighbours in order.  The dependency between neighbours (a created point takes
//                     its idx1 out of the later searches) is a bitset in LDS.  Per neighbour: the waves take the common nodes in
//                     turn and walk a node's idx1 list sequentially, a wave reduction picks the minimum distance, last position on
//                     ties, among the idx2 not yet taken (vbMatched2: the lists of different nodes are disjoint, so a lane keeps
//                     the taken flags of its own idx2 in a register); then the rotation histogram; then one thread per match runs
//                     the rule's triangulation and gates.
// No global atomics; the results do not depend on scheduling.
#include <algorithm>
#include <climits>

#include "sbp_handle.hpp"
#include "triangulate_rule.hpp"

namespace {

constexpr int kCandThreads = 256, kTile = 64;
constexpr int kResThreads = 512, kResWaves = kResThreads / 64;
constexpr int kMaxKp = 4096;  // key-points of a key frame (the handle's limit): 128 words of has_mp1 bits, 64 chunks of 64 idx2
constexpr int kPrefetch = 8;  // rows of a node's matrix a wave has in flight before it resolves them

static_assert(gfs_tri::kNoMatch == GFS_TRI_NO_MATCH && gfs_tri::kLowParallax == GFS_TRI_LOW_PARALLAX && gfs_tri::kSvdWZero == GFS_TRI_SVD_W_ZERO &&
                  gfs_tri::kUnprojectFailed == GFS_TRI_UNPROJECT_FAILED && gfs_tri::kBehind1 == GFS_TRI_BEHIND_1 &&
                  gfs_tri::kBehind2 == GFS_TRI_BEHIND_2 && gfs_tri::kReproj1 == GFS_TRI_REPROJ_1 && gfs_tri::kReproj2 == GFS_TRI_REPROJ_2 &&
                  gfs_tri::kZeroDist == GFS_TRI_ZERO_DIST && gfs_tri::kFar == GFS_TRI_FAR && gfs_tri::kScale == GFS_TRI_SCALE &&
                  gfs_tri::kCreated == GFS_TRI_CREATED, "the rule's exits are the ABI's");

struct TriFrame {  // a key frame on the device: the rule's view and the byte offsets of its arrays in the input block
  gfs_tri::Cam cam;
  float ep[2], F12[9];
  int n_kp, n_nodes;
  unsigned o_un, o_kps, o_ang, o_oct, o_ur, o_depth, o_desc, o_hasmp, o_nid, o_nstart, o_feat;
};

struct TriSlot {  // one (problem, neighbour)
  int problem, cur, nb;         // the problem and the two frames
  int pair_at;                  // index of the slot's matrix offsets: one per node of the current key frame, -1 = not common
  unsigned out_at;              // element index of the slot's result arrays
  unsigned long long mat_base;  // where the slot's matrices begin
};

struct TriProb {
  int first_slot, n_slots, cur;
  int only_stereo, coarse, check_orientation, inertial, far_points;
  float th_far, ratio_factor;
};

// bit 0: not out by the entry state (no map point; stereo when only_stereo), bit 1: stereo
__device__ __forceinline__ int kp_flags(const uint8_t* __restrict__ in, const TriFrame& F, int i, int only_stereo) {
  const bool st = reinterpret_cast<const float*>(in + F.o_ur)[i] >= 0;
  const bool in_play = in[F.o_hasmp + i] == 0 && (!only_stereo || st);
  return (in_play ? 1 : 0) | (st ? 2 : 0);
}

__global__ __launch_bounds__(kCandThreads) void k_tri_candidates(const uint8_t* __restrict__ in, const TriProb* __restrict__ probs,
                                                                 const TriSlot* __restrict__ slots, const TriFrame* __restrict__ frames,
                                                                 const int* __restrict__ pair_off, uint8_t* __restrict__ mat) {
  // descriptors of side 1 row-wise (a wave reads one row: broadcast), of side 2 word-wise (64 lanes read 64 consecutive words)
  __shared__ unsigned s_d1[kTile][8], s_d2[8][kTile];
  __shared__ gfs_tri::Line s_l1[kTile];
  __shared__ float s_x2[kTile], s_y2[kTile], s_sc2[kTile], s_sg2[kTile];
  __shared__ int s_f1[kTile], s_f2[kTile];
  const TriSlot S = slots[blockIdx.y];
  const TriFrame& F1 = frames[S.cur];
  const TriFrame& F2 = frames[S.nb];
  const int node = blockIdx.x, tid = threadIdx.x;
  if (node >= F1.n_nodes) return;  // (uniform: the grid is sized by the call's longest node list)
  const int off = pair_off[S.pair_at + node];
  const int j = gfs::find_node(reinterpret_cast<const int*>(in + F2.o_nid), F2.n_nodes, reinterpret_cast<const int*>(in + F1.o_nid)[node]);
  if (j < 0 || off < 0) return;  // (the host's merge, which laid the matrices out, and this search agree)
  const int only_stereo = probs[S.problem].only_stereo;
  const bool coarse = probs[S.problem].coarse != 0;
  const int* ns1 = reinterpret_cast<const int*>(in + F1.o_nstart);
  const int* ns2 = reinterpret_cast<const int*>(in + F2.o_nstart);
  const int b1 = ns1[node], n1 = ns1[node + 1] - b1, b2 = ns2[j], n2 = ns2[j + 1] - b2;
  const int* feat1 = reinterpret_cast<const int*>(in + F1.o_feat) + b1;
  const int* feat2 = reinterpret_cast<const int*>(in + F2.o_feat) + b2;
  uint8_t* M = mat + S.mat_base + (unsigned)off;
  const float ep[2] = {F2.ep[0], F2.ep[1]};
  for (int t1 = 0; t1 < n1; t1 += kTile) {
    __syncthreads();
    if (tid < kTile && t1 + tid < n1) {
      const int i = feat1[t1 + tid];
      const uint4* d = reinterpret_cast<const uint4*>(in + F1.o_desc) + 2 * (size_t)i;
      const uint4 a = d[0], b = d[1];
      s_d1[tid][0] = a.x; s_d1[tid][1] = a.y; s_d1[tid][2] = a.z; s_d1[tid][3] = a.w;
      s_d1[tid][4] = b.x; s_d1[tid][5] = b.y; s_d1[tid][6] = b.z; s_d1[tid][7] = b.w;
      const float2 xy = reinterpret_cast<const float2*>(in + F1.o_un)[i];
      s_l1[tid] = gfs_tri::epipolar_line(F2.F12, xy.x, xy.y);
      s_f1[tid] = kp_flags(in, F1, i, only_stereo);
    }
    for (int t2 = 0; t2 < n2; t2 += kTile) {
      __syncthreads();
      if (tid < kTile && t2 + tid < n2) {
        const int i = feat2[t2 + tid];
        const uint4* d = reinterpret_cast<const uint4*>(in + F2.o_desc) + 2 * (size_t)i;
        const uint4 a = d[0], b = d[1];
        s_d2[0][tid] = a.x; s_d2[1][tid] = a.y; s_d2[2][tid] = a.z; s_d2[3][tid] = a.w;
        s_d2[4][tid] = b.x; s_d2[5][tid] = b.y; s_d2[6][tid] = b.z; s_d2[7][tid] = b.w;
        const float2 xy = reinterpret_cast<const float2*>(in + F2.o_un)[i];
        s_x2[tid] = xy.x;
        s_y2[tid] = xy.y;
        const int oct = in[F2.o_oct + i];
        s_sc2[tid] = F2.cam.scale[oct];
        s_sg2[tid] = F2.cam.sigma2[oct];
        s_f2[tid] = kp_flags(in, F2, i, only_stereo);
      }
      __syncthreads();
      const int i2 = tid & (kTile - 1);
      if (t2 + i2 < n2) {
        const int f2 = s_f2[i2];
        for (int i1 = tid / kTile; i1 < kTile && t1 + i1 < n1; i1 += kCandThreads / kTile) {
          const int f1 = s_f1[i1];
          int out = gfs_tri::kNoCandidate;
          if ((f1 & 1) && (f2 & 1)) {
            int d = 0;
#pragma unroll
            for (int w = 0; w < 8; w++) d += __popc(s_d1[i1][w] ^ s_d2[w][i2]);
            if (d <= gfs_tri::kThLow &&
                gfs_tri::candidate_ok(s_l1[i1], ep, (f1 & 2) != 0, (f2 & 2) != 0, s_x2[i2], s_y2[i2], s_sc2[i2], s_sg2[i2], coarse))
              out = d;
          }
          M[(size_t)(t1 + i1) * n2 + (t2 + i2)] = (uint8_t)out;
        }
      }
    }
  }
}

__device__ __forceinline__ gfs_tri::Kp load_kp(const uint8_t* __restrict__ in, const TriFrame& F, int i) {
  gfs_tri::Kp k;
  const float2 un = reinterpret_cast<const float2*>(in + F.o_un)[i], raw = reinterpret_cast<const float2*>(in + F.o_kps)[i];
  k.x = un.x;
  k.y = un.y;
  k.kx = raw.x;
  k.ky = raw.y;
  k.angle = reinterpret_cast<const float*>(in + F.o_ang)[i];
  k.ur = reinterpret_cast<const float*>(in + F.o_ur)[i];
  k.depth = reinterpret_cast<const float*>(in + F.o_depth)[i];
  k.oct = in[F.o_oct + i];
  return k;
}

__global__ __launch_bounds__(kResThreads) void k_tri_resolve(const uint8_t* __restrict__ in, const TriProb* __restrict__ probs,
                                                             const TriSlot* __restrict__ slots, const TriFrame* __restrict__ frames,
                                                             const int* __restrict__ pair_off, const uint8_t* __restrict__ mat,
                                                             int* __restrict__ o_match, uint8_t* __restrict__ o_exit, float* __restrict__ o_x3d,
                                                             uint8_t* __restrict__ o_stereo) {
  __shared__ unsigned s_has1[kMaxKp / 32];  // GetMapPoint(idx1) != nullptr of the current key frame, carried across the neighbours
  __shared__ int s_hist[gfs_tri::kHisto], s_ind[3];
  const TriProb P = probs[blockIdx.x];
  const TriFrame& F1 = frames[P.cur];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N1 = F1.n_kp;
  for (int w = tid; w < kMaxKp / 32; w += kResThreads) {
    unsigned bits = 0;
    for (int b = 0; b < 32; b++) {
      const int i = 32 * w + b;
      if (i < N1 && in[F1.o_hasmp + i]) bits |= 1u << b;
    }
    s_has1[w] = bits;
  }
  const int* nid1 = reinterpret_cast<const int*>(in + F1.o_nid);
  const int* ns1 = reinterpret_cast<const int*>(in + F1.o_nstart);
  const int* feat1_all = reinterpret_cast<const int*>(in + F1.o_feat);
  const float* ang1 = reinterpret_cast<const float*>(in + F1.o_ang);
  for (int s = 0; s < P.n_slots; s++) {
    const TriSlot S = slots[P.first_slot + s];
    const TriFrame& F2 = frames[S.nb];
    int* match12 = o_match + S.out_at;
    uint8_t* exit_ = o_exit + S.out_at;
    float* x3d = o_x3d + 3 * (size_t)S.out_at;
    uint8_t* stereo = o_stereo + S.out_at;
    for (int i = tid; i < N1; i += kResThreads) {
      match12[i] = -1;
      exit_[i] = gfs_tri::kNoMatch;
      x3d[3 * i] = x3d[3 * i + 1] = x3d[3 * i + 2] = 0.0f;
      stereo[i] = 0;
    }
    if (tid < gfs_tri::kHisto) s_hist[tid] = 0;
    __syncthreads();  // (also: s_has1 as the previous neighbour left it)
    // ---- the search: SearchForTriangulation's merge loop, a node per wave
    const int* nid2 = reinterpret_cast<const int*>(in + F2.o_nid);
    const int* ns2 = reinterpret_cast<const int*>(in + F2.o_nstart);
    for (int node = wave; node < F1.n_nodes; node += kResWaves) {
      const int off = pair_off[S.pair_at + node];
      if (off < 0) continue;
      const int j = gfs::find_node(nid2, F2.n_nodes, nid1[node]);
      if (j < 0) continue;
      const int b1 = ns1[node], n1 = ns1[node + 1] - b1, b2 = ns2[j], n2 = ns2[j + 1] - b2;
      const int* feat1 = feat1_all + b1;
      const int* feat2 = reinterpret_cast<const int*>(in + F2.o_feat) + b2;
      const uint8_t* M = mat + S.mat_base + (unsigned)off;
      unsigned long long taken = 0;  // bit c: this lane's idx2 of chunk c (position 64 c + lane) is matched (vbMatched2)
      for (int i1b = 0; i1b < n1; i1b += kPrefetch) {
        int idx1[kPrefetch], d0[kPrefetch];  // the rows' first chunk, loaded together
#pragma unroll
        for (int u = 0; u < kPrefetch; u++) {
          const int r = min(i1b + u, n1 - 1);
          idx1[u] = feat1[r];
          d0[u] = lane < n2 ? M[(size_t)r * n2 + lane] : gfs_tri::kNoCandidate;
        }
#pragma unroll
        for (int u = 0; u < kPrefetch; u++) {
          if (i1b + u >= n1) break;
          if (s_has1[idx1[u] >> 5] >> (idx1[u] & 31) & 1) continue;  // pMP1: at entry or created at an earlier neighbour
          int best = INT_MAX;  // (distance, last position first): min picks the minimum distance, the last position on ties
          if (d0[u] != gfs_tri::kNoCandidate && !(taken & 1ull)) best = (d0[u] << 16) | (0xffff - lane);
          const uint8_t* row = M + (size_t)(i1b + u) * n2;
          for (int c = 1; c * 64 < n2; c++) {
            const int i2 = c * 64 + lane;
            if (i2 < n2 && !(taken >> c & 1ull)) {
              const int d = row[i2];
              if (d != gfs_tri::kNoCandidate) best = min(best, (d << 16) | (0xffff - i2));
            }
          }
          best = gfs::wave_min_i32(best);
          if (best == INT_MAX) continue;
          const int i2 = 0xffff - (best & 0xffff);
          if ((i2 & 63) == lane) {
            taken |= 1ull << (i2 >> 6);
            match12[idx1[u]] = feat2[i2];
          }
        }
      }
    }
    __syncthreads();
    // ---- the rotation histogram (src/ORBmatcher.cc:1331-1365)
    if (P.check_orientation) {
      const float* ang2 = reinterpret_cast<const float*>(in + F2.o_ang);
      for (int i = tid; i < N1; i += kResThreads) {
        const int m = match12[i];
        if (m >= 0) atomicAdd(&s_hist[gfs_tri::rot_bin(ang1[i], ang2[m])], 1);
      }
      __syncthreads();
      if (tid == 0) gfs_tri::three_maxima(s_hist, s_ind[0], s_ind[1], s_ind[2]);
      __syncthreads();
      const int ind1 = s_ind[0], ind2 = s_ind[1], ind3 = s_ind[2];
      for (int i = tid; i < N1; i += kResThreads) {  // (the thread that reads match12[i] below)
        const int m = match12[i];
        if (m < 0) continue;
        const int bin = gfs_tri::rot_bin(ang1[i], ang2[m]);
        if (bin != ind1 && bin != ind2 && bin != ind3) match12[i] = -1;
      }
    }
    // ---- every match: parallax, triangulation or UnprojectStereo, the gates (src/LocalMapping.cc:904-1100)
    for (int i = tid; i < N1; i += kResThreads) {
      const int m = match12[i];
      if (m < 0) continue;
      const gfs_tri::Kp k1 = load_kp(in, F1, i), k2 = load_kp(in, F2, m);
      float X[3];
      int ps;
      const int ex = gfs_tri::triangulate_match(F1.cam, F2.cam, k1, k2, P.inertial != 0, P.far_points != 0, P.th_far, P.ratio_factor, X, &ps);
      exit_[i] = (uint8_t)ex;
      x3d[3 * i] = X[0];
      x3d[3 * i + 1] = X[1];
      x3d[3 * i + 2] = X[2];
      stereo[i] = (uint8_t)ps;
      if (ex == gfs_tri::kCreated) atomicOr(&s_has1[i >> 5], 1u << (i & 31));  // mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
    }
    __syncthreads();
  }
}

using HeadLayout = gfs::TriHeadLayout<TriProb, TriSlot, TriFrame>;

}  // namespace

struct gfs_tri_workspace : gfs_sbp_workspace {
  int max_neighbours = 0;
  long long max_pairs = 0;
  gfs::Mirror in, out;
  gfs::DevBuf<uint8_t> d_mat;
  size_t in_bytes = 0, mat_bytes = 0;
};

namespace {

int validate_kf(const gfs_tri_keyframe& k, int max_cur, const char* what, int b, int i, std::vector<uint8_t>& seen) {
  GFS_REQUIRE(k.n_kp >= 0 && k.n_kp <= max_cur, GFS_ERR_CAPACITY, "gfs_create_new_map_points: problem %d %s %d has %d key-points (capacity %d)",
              b, what, i, k.n_kp, max_cur);
  GFS_REQUIRE(k.n_nodes >= 0 && k.n_nodes <= max_cur, GFS_ERR_CAPACITY, "gfs_create_new_map_points: problem %d %s %d has %d nodes (capacity %d)",
              b, what, i, k.n_nodes, max_cur);
  GFS_REQUIRE(k.n_levels >= 1 && k.n_levels <= 16 && k.scale_factors && k.level_sigma2, GFS_ERR_INVALID_ARG,
              "gfs_create_new_map_points: problem %d %s %d needs 1..16 scale factors and level variances", b, what, i);
  GFS_REQUIRE(k.n_kp == 0 || (k.kps_un && k.kps && k.u_right && k.depth && k.desc && k.has_mp), GFS_ERR_INVALID_ARG,
              "gfs_create_new_map_points: problem %d %s %d has NULL key-point arrays", b, what, i);
  GFS_REQUIRE(k.node_start && (k.n_nodes == 0 || k.node_id), GFS_ERR_INVALID_ARG, "gfs_create_new_map_points: problem %d %s %d has NULL node arrays",
              b, what, i);
  for (int p = 0; p < k.n_kp; p++)
    GFS_REQUIRE(k.kps_un[p].octave >= 0 && k.kps_un[p].octave < k.n_levels, GFS_ERR_INVALID_ARG,
                "gfs_create_new_map_points: problem %d %s %d key-point %d has octave %d outside [0, %d)", b, what, i, p, k.kps_un[p].octave,
                k.n_levels);
  return gfs::check_feature_vector("gfs_create_new_map_points", k, what, b, i, seen);
}

// takes a key frame's arrays from the staging block's cursor, copies them there and fills its device header
void stage_kf(const gfs_tri_keyframe& k, const float* ep, const float* F12, uint8_t* base, gfs::Block<256>& in, TriFrame& F) {
  memset(&F, 0, sizeof(F));
  memcpy(F.cam.Tcw, k.Tcw, sizeof(k.Tcw));
  memcpy(F.cam.Ow, k.Ow, sizeof(k.Ow));
  memcpy(F.cam.Rwc, k.Rwc, sizeof(k.Rwc));
  memcpy(F.cam.twc, k.twc, sizeof(k.twc));
  F.cam.fx = k.fx;
  F.cam.fy = k.fy;
  F.cam.cx = k.cx;
  F.cam.cy = k.cy;
  F.cam.invfx = k.invfx;
  F.cam.invfy = k.invfy;
  F.cam.mbf = k.mbf;
  F.cam.mb = k.mb;
  F.cam.n_levels = k.n_levels;
  for (int l = 0; l < k.n_levels; l++) {
    F.cam.scale[l] = k.scale_factors[l];
    F.cam.sigma2[l] = k.level_sigma2[l];
  }
  if (ep) memcpy(F.ep, ep, 8);
  if (F12) memcpy(F.F12, F12, 36);
  F.n_kp = k.n_kp;
  F.n_nodes = k.n_nodes;
  const size_t n = (size_t)k.n_kp, m = (size_t)k.n_nodes, nf = (size_t)k.node_start[k.n_nodes];
  const gfs::TriKfArrays A{in, n, m, nf};
  F.o_un = (unsigned)A.un.off;
  F.o_kps = (unsigned)A.kps.off;
  F.o_ang = (unsigned)A.ang.off;
  F.o_ur = (unsigned)A.ur.off;
  F.o_depth = (unsigned)A.depth.off;
  F.o_oct = (unsigned)A.oct.off;
  F.o_hasmp = (unsigned)A.hasmp.off;
  F.o_desc = (unsigned)A.desc.off;
  F.o_nid = (unsigned)A.nid.off;
  F.o_nstart = (unsigned)A.nstart.off;
  F.o_feat = (unsigned)A.feat.off;
  float2 *un = A.un.at(base), *raw = A.kps.at(base);
  float* ang = A.ang.at(base);
  uint8_t *oct = A.oct.at(base), *hasmp = A.hasmp.at(base);
  for (size_t i = 0; i < n; i++) {
    un[i] = make_float2(k.kps_un[i].x, k.kps_un[i].y);
    raw[i] = make_float2(k.kps[i].x, k.kps[i].y);
    ang[i] = k.kps_un[i].angle;
    oct[i] = (uint8_t)k.kps_un[i].octave;
    hasmp[i] = k.has_mp[i] ? 1 : 0;
  }
  A.ur.put(base, 0, k.u_right, n);
  A.depth.put(base, 0, k.depth, n);
  A.desc.put(base, 0, k.desc, n);
  A.nid.put(base, 0, k.node_id, m);
  A.nstart.put(base, 0, k.node_start, m + 1);
  A.feat.put(base, 0, k.feat_idx, nf);
}

}  // namespace

extern "C" {

int gfs_sbp_reserve_triangulation(gfs_sbp* h, int max_neighbours, int64_t max_candidate_pairs) {
  GFS_REQUIRE(h && max_neighbours > 0 && max_candidate_pairs > 0 && max_candidate_pairs <= INT_MAX, GFS_ERR_INVALID_ARG,
              "gfs_sbp_reserve_triangulation: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipStreamSynchronize(h->stream));
  h->tri.reset();
  std::unique_ptr<gfs_tri_workspace> w(new gfs_tri_workspace);
  const size_t B = (size_t)h->max_batch, NB = (size_t)max_neighbours, SC = gfs::align_up((size_t)h->max_cur, 64);
  gfs::Block<256> one_kf;
  const gfs::TriKfArrays widest{one_kf, SC, SC, SC};  // a key frame of the capacity: SC key-points, as many nodes, every key-point listed
  w->in_bytes = HeadLayout{B, B * NB, B * (NB + 1), B * NB * SC}.in.bytes() + B * (NB + 1) * widest.in.bytes();
  GFS_REQUIRE(w->in_bytes < 0xffffffffull, GFS_ERR_UNSUPPORTED, "gfs_sbp_reserve_triangulation: the input block would exceed 4 GiB");
  w->mat_bytes = gfs::align_up(B * (size_t)max_candidate_pairs, 256);
  int rc = 0;
  if (!rc) rc = w->in.alloc(w->in_bytes);
  if (!rc) rc = w->out.alloc(gfs::TriOutLayout{B * NB * SC}.out.bytes());
  if (!rc) rc = w->d_mat.alloc(w->mat_bytes);
  if (rc) return rc;
  w->max_neighbours = max_neighbours;
  w->max_pairs = max_candidate_pairs;
  h->tri = std::move(w);
  return GFS_OK;
}

int gfs_create_new_map_points(gfs_sbp* h, const gfs_tri_problem* problems, int B, gfs_tri_result* const* results) {
  GFS_REQUIRE(h && problems && results && B > 0, GFS_ERR_INVALID_ARG, "gfs_create_new_map_points: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  gfs_tri_workspace* w = static_cast<gfs_tri_workspace*>(h->tri.get());
  GFS_REQUIRE(w, GFS_ERR_CAPACITY, "gfs_create_new_map_points: call gfs_sbp_reserve_triangulation first");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_create_new_map_points: batch %d exceeds capacity %d", B, h->max_batch);
  GFS_HIP(hipSetDevice(h->device));
  // every refusal comes before anything is staged
  std::vector<uint8_t> seen;
  std::vector<int> pair_off;  // per (slot, node of the current key frame): the matrix's offset within the slot's problem, -1 = not common
  std::vector<size_t> slot_pair_at;
  std::vector<long long> prob_pairs((size_t)B);
  size_t n_slots = 0, out_elems = 0;
  int max_nodes1 = 0;
  for (int b = 0; b < B; b++) {
    const gfs_tri_problem& Q = problems[b];
    GFS_REQUIRE(Q.n_neighbours >= 0 && Q.n_neighbours <= w->max_neighbours, GFS_ERR_CAPACITY,
                "gfs_create_new_map_points: problem %d has %d neighbours (reserve %d)", b, Q.n_neighbours, w->max_neighbours);
    GFS_REQUIRE(Q.n_neighbours == 0 || (Q.neighbours && results[b]), GFS_ERR_INVALID_ARG, "gfs_create_new_map_points: problem %d has NULL neighbours or results", b);
    if (int rc = validate_kf(Q.cur, h->max_cur, "current key frame", b, 0, seen)) return rc;
    long long pairs = 0;
    for (int i = 0; i < Q.n_neighbours; i++) {
      const gfs_tri_keyframe& K2 = Q.neighbours[i].kf;
      if (int rc = validate_kf(K2, h->max_cur, "neighbour", b, i, seen)) return rc;
      const gfs_tri_result& R = results[b][i];
      GFS_REQUIRE(Q.cur.n_kp == 0 || (R.match12 && R.exit && R.x3d && R.point_stereo), GFS_ERR_INVALID_ARG,
                  "gfs_create_new_map_points: problem %d neighbour %d has NULL result arrays", b, i);
      slot_pair_at.push_back(pair_off.size());
      int p2 = 0;  // the merge of the two ascending id lists
      for (int p1 = 0; p1 < Q.cur.n_nodes; p1++) {
        while (p2 < K2.n_nodes && K2.node_id[p2] < Q.cur.node_id[p1]) p2++;
        if (p2 < K2.n_nodes && K2.node_id[p2] == Q.cur.node_id[p1]) {
          const long long n1 = Q.cur.node_start[p1 + 1] - Q.cur.node_start[p1], n2 = K2.node_start[p2 + 1] - K2.node_start[p2];
          GFS_REQUIRE(pairs + n1 * n2 <= w->max_pairs, GFS_ERR_CAPACITY, "gfs_create_new_map_points: problem %d has more than %lld candidate pairs",
                      b, w->max_pairs);
          pair_off.push_back((int)pairs);
          pairs += n1 * n2;
        } else {
          pair_off.push_back(-1);
        }
      }
      n_slots++;
      out_elems += gfs::align_up((size_t)Q.cur.n_kp, 64);
    }
    prob_pairs[b] = pairs;
    if (Q.n_neighbours > 0) max_nodes1 = std::max(max_nodes1, Q.cur.n_nodes);
  }
  if (n_slots == 0) return GFS_OK;
  // ---- stage: headers, the matrix offsets, then every key frame's arrays (all within the reserve: counts and sizes were checked)
  uint8_t* hb = w->in.h.p;
  HeadLayout Y{(size_t)B, n_slots, n_slots + (size_t)B, pair_off.size()};
  Y.pairs.put(hb, 0, pair_off.data(), pair_off.size());
  TriProb* probs = Y.probs.at(hb);
  TriSlot* slots = Y.slots.at(hb);
  TriFrame* frames = Y.frames.at(hb);
  size_t slot = 0, frame = 0, out_at = 0;
  unsigned long long mat_at = 0;
  for (int b = 0; b < B; b++) {
    const gfs_tri_problem& Q = problems[b];
    TriProb& P = probs[b];
    P.first_slot = (int)slot;
    P.n_slots = Q.n_neighbours;
    P.cur = (int)frame;
    P.only_stereo = Q.only_stereo;
    P.coarse = Q.coarse;
    P.check_orientation = Q.check_orientation;
    P.inertial = Q.inertial;
    P.far_points = Q.far_points;
    P.th_far = Q.th_far_points;
    P.ratio_factor = Q.ratio_factor;
    stage_kf(Q.cur, nullptr, nullptr, hb, Y.in, frames[frame++]);
    for (int i = 0; i < Q.n_neighbours; i++) {
      TriSlot& S = slots[slot];
      S.problem = b;
      S.cur = P.cur;
      S.nb = (int)frame;
      S.pair_at = (int)slot_pair_at[slot];
      S.out_at = (unsigned)out_at;
      S.mat_base = mat_at;
      out_at += gfs::align_up((size_t)Q.cur.n_kp, 64);
      stage_kf(Q.neighbours[i].kf, Q.neighbours[i].ep, Q.neighbours[i].F12, hb, Y.in, frames[frame++]);
      slot++;
    }
    mat_at += (unsigned long long)prob_pairs[b];
  }
  const size_t at = Y.in.bytes();
  if (at > w->in_bytes || mat_at > w->mat_bytes) {  // (cannot happen: the reserve bounds every term above)
    gfs::set_error("gfs_create_new_map_points: internal: staged %zu of %zu bytes", at, w->in_bytes);
    return GFS_ERR_CAPACITY;
  }
  const gfs::TriOutLayout Z{out_elems};
  if (out_elems > 0) {
    hipStream_t s = h->stream;
    const uint8_t* di = w->in.d.p;
    uint8_t* dq = w->out.d.p;
    if (int rc = w->in.upload(s, 0, at)) return rc;
    const TriProb* dprob = Y.probs.at(di);
    const TriSlot* dslot = Y.slots.at(di);
    const TriFrame* dframe = Y.frames.at(di);
    const int* dpair = Y.pairs.at(di);
    if (max_nodes1 > 0 && mat_at > 0)
      GFS_LAUNCH("k_tri_candidates", k_tri_candidates, dim3(max_nodes1, (unsigned)n_slots), dim3(kCandThreads), 0, s, di, dprob,
                 dslot, dframe, dpair, w->d_mat.p);
    GFS_LAUNCH("k_tri_resolve", k_tri_resolve, dim3(B), dim3(kResThreads), 0, s, di, dprob, dslot, dframe, dpair,
               (const uint8_t*)w->d_mat.p, Z.match.at(dq), Z.exit.at(dq), Z.x3d.at(dq), Z.stereo.at(dq));
    if (int rc = w->out.download(s, 0, Z.out.bytes())) return rc;
    GFS_HIP(hipStreamSynchronize(s));  // the call's one synchronisation
  }
  const uint8_t* ho = w->out.h.p;
  slot = 0;
  for (int b = 0; b < B; b++) {
    const size_t n = (size_t)problems[b].cur.n_kp;
    for (int i = 0; i < problems[b].n_neighbours; i++, slot++) {
      gfs_tri_result& R = results[b][i];
      const size_t o = slots[slot].out_at;
      int nm = 0, ncr = 0;
      Z.match.get(R.match12, ho, o, n);
      Z.exit.get(R.exit, ho, o, n);
      Z.stereo.get(R.point_stereo, ho, o, n);
      Z.x3d.get(R.x3d, ho, o, n);
      for (size_t p = 0; p < n; p++) {
        nm += R.match12[p] >= 0;
        ncr += R.exit[p] == GFS_TRI_CREATED;
      }
      R.n_matches = nm;
      R.n_created = ncr;
    }
  }
  return GFS_OK;
}

}  // extern "C"
