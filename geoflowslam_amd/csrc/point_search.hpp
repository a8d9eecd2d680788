// The host half that gfs_fuse_search (fuse.hip) and gfs_sim3_search (sim3_search.hip) share: both search the key-points of B key
// frames for the points of shared lists (gfs_fuse_points), from three staging blocks -- the points, the key frames, the results.
// Every check takes the entry point's name (`who`) and what it calls a key frame (`what`) for its error text; a check returns the
// code of its first refusal and stages nothing.
#pragma once
#include <vector>

#include "fuse_rule.hpp"
#include "sbp_handle.hpp"

namespace gfs {

// what gfs_sbp_reserve_fuse / gfs_sbp_reserve_sim3_search allocate: the reserve's sizes and a pinned block mirrored by a device block
// for each of the three
struct PointSearchWorkspace : gfs_sbp_workspace {
  int lists = 0, points = 0, kfs = 0;
  Mirror pts, kf, out;
  int alloc(size_t pts_bytes, size_t kf_bytes, size_t out_bytes, int max_lists, int max_points_per_list, int max_kfs) {
    int rc = pts.alloc(pts_bytes);
    if (!rc) rc = kf.alloc(kf_bytes);
    if (!rc) rc = out.alloc(out_bytes);
    if (rc) return rc;
    lists = max_lists;
    points = max_points_per_list;
    kfs = max_kfs;
    return GFS_OK;
  }
  // the call's device half: the two input blocks up, launch(), the results down, the call's one synchronisation
  template <class Launch>
  int run(hipStream_t s, size_t pts_bytes, size_t kf_bytes, size_t out_bytes, Launch&& launch) {
    if (int rc = pts.upload(s, 0, pts_bytes)) return rc;
    if (int rc = kf.upload(s, 0, kf_bytes)) return rc;
    if (int rc = launch()) return rc;
    if (int rc = out.download(s, 0, out_bytes)) return rc;
    GFS_HIP(hipStreamSynchronize(s));
    return GFS_OK;
  }
};

// the lists against the reserve; list_base[l] = the first slot of list l in the point block, *T = the slots of all lists
inline int check_point_lists(const char* who, const gfs_fuse_points* lists, int n_lists, int max_points, std::vector<size_t>& list_base,
                             size_t* T) {
  list_base.resize((size_t)n_lists);
  *T = 0;
  for (int l = 0; l < n_lists; l++) {
    const gfs_fuse_points& L = lists[l];
    GFS_REQUIRE(L.n_mp >= 0 && L.n_mp <= max_points, GFS_ERR_CAPACITY, "%s: list %d has %d map points (reserve %d)", who, l, L.n_mp, max_points);
    GFS_REQUIRE(L.n_mp == 0 || (L.mp_xw && L.mp_normal && L.mp_min_dist && L.mp_max_dist && L.mp_desc), GFS_ERR_INVALID_ARG,
                "%s: list %d has NULL arrays", who, l);
    list_base[l] = *T;
    *T += align_up((size_t)L.n_mp, 64);
  }
  return GFS_OK;
}

inline void stage_point_lists(const PointListFields& Y, uint8_t* hp, const gfs_fuse_points* lists, int n_lists, const std::vector<size_t>& list_base) {
  for (int l = 0; l < n_lists; l++) {
    const gfs_fuse_points& L = lists[l];
    const size_t at = list_base[l], n = (size_t)L.n_mp;
    Y.xw.put(hp, at, L.mp_xw, n);
    Y.nrm.put(hp, at, L.mp_normal, n);
    Y.dmin.put(hp, at, L.mp_min_dist, n);
    Y.dmax.put(hp, at, L.mp_max_dist, n);
    Y.desc.put(hp, at, L.mp_desc, n);
  }
}

// Key frame f of a call, in two parts with the entry point's own pointer checks between them.  The head: the key-point count against
// the handle, the level count and tables (have_tables = the level tables the entry needs are given; `tables` names them), the list.
template <class KF>
int check_search_kf_head(const char* who, const char* what, int f, const KF& k, int max_cur, bool have_tables, const char* tables, int n_lists) {
  GFS_REQUIRE(k.n_kp >= 0 && k.n_kp <= max_cur, GFS_ERR_CAPACITY, "%s: %s %d has %d key-points (capacity %d)", who, what, f, k.n_kp, max_cur);
  GFS_REQUIRE(k.n_levels > 0 && k.n_levels <= 16 && have_tables, GFS_ERR_INVALID_ARG, "%s: %s %d needs 1..16 %s", who, what, f, tables);
  GFS_REQUIRE(k.list >= 0 && k.list < n_lists, GFS_ERR_INVALID_ARG, "%s: %s %d names list %d of %d", who, what, f, k.list, n_lists);
  return GFS_OK;
}
// The tail: result arrays for the n points of its list, every octave inside the pyramid (k.kps_un is checked by then).
template <class KF, class Result>
int check_search_kf_tail(const char* who, const char* what, int f, const KF& k, int n, const Result& r) {
  GFS_REQUIRE(n == 0 || (r.exit && r.best_idx && r.best_dist && r.level), GFS_ERR_INVALID_ARG, "%s: %s %d has NULL result arrays", who, what, f);
  for (int i = 0; i < k.n_kp; i++)
    GFS_REQUIRE(k.kps_un[i].octave >= 0 && k.kps_un[i].octave < k.n_levels, GFS_ERR_INVALID_ARG,
                "%s: %s %d key-point %d has octave %d outside [0, %d)", who, what, f, i, k.kps_un[i].octave, k.n_levels);
  return GFS_OK;
}

// the rule's view of a key frame from gfs_fuse_keyframe or gfs_sim3_search_problem: every field both have (K is zeroed before)
template <class KF>
void fill_search_keyframe(gfs_fuse::KeyFrame& K, const KF& k) {
  for (int c = 0; c < 4; c++) K.q[c] = k.Tcw_q[c];
  for (int c = 0; c < 3; c++) {
    K.t[c] = k.Tcw_t[c];
    K.Ow[c] = k.Ow[c];
  }
  K.fx = k.fx;
  K.fy = k.fy;
  K.cx = k.cx;
  K.cy = k.cy;
  K.min_x = k.min_x;
  K.max_x = k.max_x;
  K.min_y = k.min_y;
  K.max_y = k.max_y;
  K.grid_w_inv = k.grid_w_inv;
  K.grid_h_inv = k.grid_h_inv;
  K.log_scale_factor = k.log_scale_factor;
  K.th = k.th;
  K.n_levels = k.n_levels;
  K.n_kp = k.n_kp;
  for (int c = 0; c < k.n_levels; c++) K.scale[c] = k.scale_factors[c];
}

// the positions and octaves of n key-points as the kernels load them
inline void stage_xy_oct(const gfs_keypoint* kps, int n, xy_t* xy, uint8_t* oct) {
  for (int i = 0; i < n; i++) {
    xy[i] = make_float2(kps[i].x, kps[i].y);
    oct[i] = (uint8_t)kps[i].octave;
  }
}

}  // namespace gfs
