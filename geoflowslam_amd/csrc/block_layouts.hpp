// The staging blocks of the handles that make one copy in and one copy out per call (staging.hpp): which arrays a block holds, in which
// order, of what element type.  A layout is an aggregate built as Layout{sizes...} for the sizes of ONE call (or, at create / reserve
// time, for the capacity), so what travels is what the call holds; the cursors follow the sizes, so one size too many does not compile.
// The fields are taken in the order they are declared, and that order is part of the contract: several uploads are partial and end or
// begin at a field.  The headers of a block are device structs of the files that own them; they enter only through their size, as a
// type parameter.  Plain C++ apart from float2: tests/host/staging_layout_check.cpp builds the same layouts on the host.
#pragma once
#include "../../include/gfs_abi.h"
#include "staging.hpp"

namespace gfs {

#if defined(__HIPCC__)
using xy_t = float2;
#else
struct alignas(8) xy_t {
  float x, y;
};
#endif

// gfs_search_by_projection / _map (sbp.hip): B frames, the per-frame arrays strided by SL map points / SC key-points.
// gfs_search_local_points uploads the headers and [kp, end of the block) only: the map-point arrays in between are filled on the device.
template <class Pair>
struct SbpLayout {
  size_t B;
  int SL, SC;
  Block<256> in, res;
  size_t L = (size_t)SL * B, C = (size_t)SC * B;
  Field<Pair> pairs{in, B};
  Field<float, 3> xw{in, L};
  Field<uint8_t, 32> desc{in, L};
  Field<int> oct{in, L};
  Field<float> ang{in, L};
  Field<uint8_t> lobs{in, L};
  Field<gfs_keypoint> kp{in, C};
  Field<float> ur{in, C};
  Field<uint8_t, 32> cdesc{in, C};
  Field<uint8_t> cobs{in, C};
  Field<int> match{res, C}, nm{res, B};  // the result block
};

// gfs_search_local_points (local_points.hip): the listed map points, strided by SM; the results with k_sbp's cur_match / nmatches behind them
template <class Frame, class Meta>
struct LocalLayout {
  size_t B;
  int SM, SL, SC;
  Block<256> in, out;
  size_t M = (size_t)SM * B, NL = (size_t)SL * B, NC = (size_t)SC * B;
  Field<Frame> frames{in, B};
  Field<float, 3> xw{in, M}, nrm{in, M};
  Field<float> dmin{in, M}, dmax{in, M};
  Field<uint8_t, 32> desc{in, M};
  Field<uint8_t> obs{in, M};
  Field<Meta> meta{out, B};
  Field<uint8_t> view{out, M};
  Field<float, 3> proj{out, M};
  Field<float> depth{out, M}, cos{out, M};
  Field<int> level{out, M}, index{out, NL}, match{out, NC}, nm{out, B};
};

// The point block of gfs_fuse_search and gfs_sim3_search (point_search.hpp stages it): the T points of all lists
struct PointListFields {
  Block<256>& pts;
  size_t T;
  Field<float, 3> xw{pts, T}, nrm{pts, T};
  Field<float> dmin{pts, T}, dmax{pts, T};
  Field<uint8_t, 32> desc{pts, T};
};

// gfs_fuse_search (fuse.hip): T points of all lists, B key frames of SC key-points, O result slots -- three blocks
template <class Problem>
struct FuseLayout {
  size_t T, B, SC, O;
  Block<256> pts, kf, out;
  PointListFields p{pts, T};
  Field<Problem> problems{kf, B};
  Field<xy_t> xy{kf, B * SC};
  Field<float> ur{kf, B * SC};
  Field<uint8_t> oct{kf, B * SC};
  Field<uint8_t, 32> kdesc{kf, B * SC};
  Field<uint8_t> exit{out, O};
  Field<int> idx{out, O}, dist{out, O}, level{out, O};
};

// gfs_sim3_search (sim3_search.hip): T points of all lists, B problems of SC key-points, O result slots and OC listed candidates
template <class Problem>
struct Sim3SearchLayout {
  size_t T, B, SC, O, OC;
  Block<256> pts, kf, out;
  PointListFields p{pts, T};
  Field<Problem> problems{kf, B};
  Field<xy_t> xy{kf, B * SC};
  Field<uint8_t> oct{kf, B * SC};  // the octave, bit 7 = the key-point is taken at entry
  Field<uint8_t, 32> kdesc{kf, B * SC};
  Field<uint8_t> exit{out, O};
  Field<int> level{out, O}, count{out, O}, cidx{out, OC}, cdist{out, OC};
};

// gfs_create_new_map_points (triangulate.hip): the arrays of one key frame (n key-points, m nodes, nf listed features), taken from
// the call's running input block -- and from an empty block, the bytes a key frame of the capacity needs
struct TriKfArrays {
  Block<256>& in;
  size_t n, m, nf;
  Field<xy_t> un{in, n}, kps{in, n};
  Field<float> ang{in, n}, ur{in, n}, depth{in, n};
  Field<uint8_t> oct{in, n}, hasmp{in, n};
  Field<uint8_t, 32> desc{in, n};
  Field<int> nid{in, m}, nstart{in, m + 1}, feat{in, nf};
};
// the headers of the input block; the key frames' arrays follow them on the same cursor
template <class Prob, class Slot, class Frame>
struct TriHeadLayout {
  size_t B, n_slots, n_frames, n_pairs;
  Block<256> in;
  Field<Prob> probs{in, B};
  Field<Slot> slots{in, n_slots};
  Field<Frame> frames{in, n_frames};
  Field<int> pairs{in, n_pairs};
};
struct TriOutLayout {
  size_t n;
  Block<256> out;
  Field<int> match{out, n};
  Field<uint8_t> exit{out, n}, stereo{out, n};
  Field<float, 3> x3d{out, n};
};

// gfs_search_by_bow (bow_search.hip): the arrays of one key frame, as TriKfArrays; then the headers of the input block, the key
// frames' arrays behind them on the same cursor; the results are one int per (slot, key-point of key frame 1)
struct BowKfArrays {
  Block<256>& in;
  size_t n, m, nf;
  Field<float> ang{in, n};
  Field<uint8_t> hasmp{in, n};
  Field<uint8_t, 32> desc{in, n};
  Field<int> nid{in, m}, nstart{in, m + 1}, feat{in, nf};
};
template <class Slot, class Frame>
struct BowHeadLayout {
  size_t n_slots, n_frames;
  Block<256> in;
  Field<Slot> slots{in, n_slots};
  Field<Frame> frames{in, n_frames};
};

// gfs_map_points_update (map_points.hip): P points, O observations; blocks aligned to 64
struct MpLayout {
  size_t P, O;
  Block<64> in, out;
  Field<int> obs_start{in, P + 1}, dsc_start{in, P + 1};
  Field<float, 3> pos{in, P}, ref{in, P};
  Field<float> lscale{in, P}, mscale{in, P};
  Field<float, 3> Ow{in, O};
  Field<int> dsc_obs{in, O};
  Field<uint8_t> flags{in, O};
  Field<uint32_t, 8> words{in, O};  // last: a normals-only call does not upload it, a full call only the IN_DESC rows
  Field<int> best{out, P}, median{out, P};
  Field<float, 3> normal{out, P};
  Field<float> dmin{out, P}, dmax{out, P};
  Field<uint8_t> status{out, P};
};

// gfs_pose_optimize (pose.hip): B frames, B x stride observations
template <class Frame, class Out>
struct PoseLayout {
  size_t B, stride;
  Block<256> in, res;
  Field<Frame> frames{in, B};
  Field<double, 3> xw{in, B * stride}, obs{in, B * stride};
  Field<float> w{in, B * stride};
  Field<uint8_t> stereo{in, B * stride};
  Field<Out> out{res, B};
  Field<double> chi2{res, B * stride};
  Field<uint8_t> outlier{res, B * stride};
};

// gfs_pose_lidar_optimize (pose_lidar.hip): B frames of S observations and SC cloud points
template <class Frame>
struct PoseLidarLayout {
  size_t B, S, SC;
  Block<256> in;
  Field<Frame> frames{in, B};
  Field<double, 3> xw{in, B * S}, obs{in, B * S};
  Field<float> w{in, B * S};
  Field<uint8_t> stereo{in, B * S};
  Field<float, 3> cloud{in, B * SC};
};

// gfs_lidar_map_build (lidar_map.hip): K key frames, N cloud points; fixed at the handle's capacity.  The cloud is last: a call
// uploads up to the end of its own points.
struct LidarMapLayout {
  size_t K, N;
  Block<256> in;
  Field<int> cloud_begin{in, K + 1};
  Field<float, 4> q{in, K};
  Field<float, 3> t{in, K}, cloud{in, N};
};

}  // namespace gfs
