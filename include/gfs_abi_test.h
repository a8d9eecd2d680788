/* gfs_abi_test.h — test hooks of libgfs_hip.so.  NOT part of the drop-in boundary (include/gfs_abi.h): nothing a maintainer of the
 * reference binds.  They expose internal replicas of third-party behaviour (libstdc++ std::sort, small_gicp's quick_sort_omp, glibc's
 * sin / cos / pow) and the counter-calibration kernels so that tests/ and profiles/calibrate.sh can check them in isolation.
 */
#ifndef GFS_ABI_TEST_H_
#define GFS_ABI_TEST_H_

#include "gfs_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host test hooks for the libstdc++ std::sort replica used by the device quadtree (sorts (size, x) pairs in place). */
int gfs_test_sort_replica(int32_t* size_key, int32_t* x_key, int32_t* payload, int n);
int gfs_test_heap_sort_replica(int32_t* size_key, int32_t* x_key, int32_t* payload, int n);

/* Host test hook: the order in which k_blur7 takes the 64 x 32 tiles of a frame's pyramid (rows x cols, nlevels levels at
 * scale_factor): level_tx_ty[3 i ..] = (level, tile column, tile row) of list position i, at most cap entries; returns the number of
 * tiles.  The 2 x 2 tiles over the same 128-byte lines sit at positions p, p + 8, p + 16, p + 24 (one XCD's L2 serves them). */
int gfs_test_orb_blur_tiles(int rows, int cols, int nlevels, float scale_factor, int32_t* level_tx_ty, int cap);

/* Host test hook (no GPU): what OrbGeometry::build (csrc/orb_host.cpp) decides for an image of rows x cols under an extractor of
 * nfeatures / nlevels / scale_factor -- the very object gfs_orb_create sizes a handle from and every call lays its tables out from,
 * not a second statement of its rules.  *info is always filled; levels[0 .. min(nlevels, cap_levels)) when supported.  Returns the
 * number of levels, or GFS_ERR_UNSUPPORTED when build refuses the size (a level smaller than one FAST cell, an integer level ratio,
 * 4096 pixels or more), GFS_ERR_INVALID_ARG for arguments gfs_orb_create refuses. */
typedef struct gfs_test_orb_geometry_info {
  int32_t supported;
  int32_t pyr_strips, pyr_strips_fine; /* row strips of the pyramid kernel: the coarse cut, the fine cut (0 = none); both 0 with one level */
  int32_t pyr_in_lds;                  /* the strips fit the LDS (k_pyr_area_lds); 0 = k_pyr_area_hbm, or no pyramid kernel at all */
  int32_t xtab_in_lds, xtab_in_lds_fine; /* the x tables sit in LDS behind the strips of the coarse / fine cut; 0 = read from memory */
  int32_t kp_cap;                      /* key points a frame can give: the sum of the levels' kp_cap.  A handle holds its max size's + 8 */
  int32_t octree_on_device;            /* every level within k_octree; 0 = the whole call runs the host quadtree */
  int32_t oct_node_cap;                /* nodes k_octree's LDS list is sized for */
  int32_t n_cells, n_blur_tiles;       /* FAST cells and 64 x 32 blur tiles of all levels */
  int32_t fast_lds_wave;               /* LDS bytes of the largest cell in k_fast_cells */
} gfs_test_orb_geometry_info;
typedef struct gfs_test_orb_level_info {
  int32_t rows, cols;
  int32_t n_cell_cols, n_cell_rows, w_cell, h_cell; /* the FAST cell grid (src/ORBextractor.cc:778-806) */
  int32_t n_cells;                                  /* cells that are launched (the reference skips a cell that starts in the border) */
  int32_t max_cell_w, max_cell_h;                   /* the largest cell's window, its 3-pixel FAST margins included */
  int32_t quota;                                    /* mnFeaturesPerLevel */
  int32_t n_ini;                                    /* DistributeOctTree's initial nodes (:573), at least 1 */
  int32_t kp_cap;                                   /* quota + 3 + 4 n_ini */
  int32_t octree_on_device;                         /* k_octree takes this level: n_ini <= 4 and quota + 4 n_ini + 8 <= 768 */
} gfs_test_orb_level_info;
int gfs_test_orb_geometry(int rows, int cols, int nfeatures, int nlevels, float scale_factor, gfs_test_orb_geometry_info* info,
                          gfs_test_orb_level_info* levels, int cap_levels);

/* Test hook: the paths the handle's last extract call took, from the flags the call itself branched on. */
#define GFS_TEST_ORB_PYR_NONE 0 /* nlevels = 1: no level above 0, no pyramid launch */
#define GFS_TEST_ORB_PYR_LDS 1  /* k_pyr_area_lds */
#define GFS_TEST_ORB_PYR_HBM 2  /* k_pyr_area_hbm */
typedef struct gfs_test_orb_paths {
  int32_t octree_on_device; /* 1 = k_octree; 0 = the host quadtree (GFS_ORB_OCTREE=host, or a level k_octree does not take) */
  int32_t pyr_kernel;       /* GFS_TEST_ORB_PYR_* */
  int32_t pyr_fine_cut;     /* 1 = the fine cut of row strips (few frames), 0 = the coarse cut or no LDS pyramid kernel */
  int32_t geometry_builds;  /* times the handle (re)wrote its geometry tables since gfs_orb_create; a refused call does not count */
  int32_t last_batch, rows, cols; /* the last accepted call; 0 before the first */
} gfs_test_orb_paths;
int gfs_test_orb_last_paths(gfs_orb* h, gfs_test_orb_paths* out);

/* GPU test hook: sin(x), cos(x), pow(x, 3.0) of n doubles evaluated on the device with the restated glibc 2.35 arithmetic
 * (csrc/glibc_math.hpp) that the pose / window / registration optimizers use for SE3Quat::exp
 * (Thirdparty/g2o/g2o/types/se3quat.h:223-257) and the Levenberg step control (core/optimization_algorithm_levenberg.cpp:127). */
int gfs_test_glibc_math(int device, const double* x, int n, double* sin_out, double* cos_out, double* pow3_out);
/* GPU test hook: exp(x) of n doubles on the device with the restated glibc 2.35 arithmetic (csrc/glibc_math.hpp) that k_sim3_opt uses
 * for the scale of a VertexSim3Expmap update (Thirdparty/g2o/g2o/types/sim3.h:82). */
int gfs_test_glibc_exp(int device, const double* x, int n, double* out);
/* GPU test hook: logf(x) of n floats on the device with the restated glibc 2.35 arithmetic (csrc/glibc_math.hpp) that the frustum
 * kernel uses for MapPoint::PredictScale (src/MapPoint.cc:565-579). */
int gfs_test_glibc_logf(int device, const float* x, int n, float* out);
/* GPU test hook for calibrating the HBM counters (profiles/calibrate.sh): a kernel with a KNOWN byte count -- mode 0 streaming read,
 * 1 per-lane gathers of 32-byte records out of a table of `table` records, 2 streaming write; n records (mode 1: n threads x per_thread
 * gathers).  *bytes_out = the bytes the kernel asked for. */
int gfs_test_traffic(int device, int mode, long long n, long long table, int per_thread, long long* bytes_out);

/* GPU test hook: the voxel sort of the preprocessing — the device replica of small_gicp's quick_sort_omp
 * (util/sort_omp.hpp:58-85: 3-way quicksort above 1024 elements, libstdc++ std::sort below), whose permutation of
 * equal keys decides the 1024-block splits of voxelgrid_sampling_omp (util/downsampling_omp.hpp:57-90) — on n <=
 * max_points caller keys (3 x 21-bit voxel fields, or all ones = invalid).  perm_out[i] = input index of the i-th
 * element of the sorted sequence. */
int gfs_test_voxel_sort(gfs_gicp* h, const unsigned long long* keys, int n, unsigned* perm_out);
/* GPU test hook: on which path the leaf ranges (< 1024 elements) of the handle's last voxel sort -- gfs_test_voxel_sort or the
 * preprocessing of the last align call, all its clouds together -- ended (csrc/voxel_qsort.hpp k_voxel_qsort_leaf): out3 = {ranges
 * without equal keys (any sort gives the reference's permutation), ranges whose equal keys cannot change a voxel mean (kept in
 * position order), ranges that ran the libstdc++ introsort replica}.  Waits for the handle's stream. */
int gfs_test_voxel_sort_paths(gfs_gicp* h, int32_t out3[3]);
/* GPU test hook: the one-wave std::sort replica (csrc/wave_std_sort.hpp: the voxel sort's leaves, sort_omp.hpp:61, and the quadtree's
 * (size, x) list, ORBextractor.cc:697-698) on n <= 1024 caller keys; perm_out[i] = original index of the element left at position i. */
int gfs_test_wave_std_sort(int device, const unsigned* keys, int n, unsigned short* perm_out);

/* Test hooks (no kernel is launched): the process-wide workgroup budget of the cooperative LM kernel (csrc/gicp.hip CoopBudget), held
 * as another handle's launch in flight would hold it, so that a test decides how many workgroups the next call of a handle is granted.
 * gfs_test_gicp_coop_hold takes exactly n workgroups of h's device out of the budget h's own calls reserve against (half of what the
 * device holds at once: out[3] of gfs_gicp_coop_stats), or none and GFS_ERR_CAPACITY when n are not free.  They are NOT booked on the
 * handle: only gfs_test_gicp_coop_release(h, n) gives them back, and the caller must (a budget left held makes every later call of
 * the process run its launch-per-step rounds).  gfs_test_gicp_coop_in_use = workgroups of the device's budget that are taken now. */
int gfs_test_gicp_coop_hold(gfs_gicp* h, int n);
int gfs_test_gicp_coop_release(gfs_gicp* h, int n);
int gfs_test_gicp_coop_in_use(int device);

/* GPU test hook: a map's search grid as the association kernels read it -- the bucket offsets start[nb + 1] and the bucket-sorted
 * points pts[n][3] with their map-index words index[n] (copied when the caps suffice); *nb, *n = the map's sizes. */
int gfs_test_lidar_map_grid(const gfs_lidar_map* map, int32_t* start, int cap_start, float* pts, int32_t* index, int cap_pts, int32_t* nb,
                            int32_t* n);

/* Test hook: a SCRIPTED stop flag for the calling thread's next gfs_lba_solve, gfs_lba_solve_bool, gfs_lba_solve_lidar(_bool) or
 * gfs_lba_solve_batch call.  Every evaluation of the caller's stop flag by that call is a "look": look 0 is the entry check
 * (src/Optimizer.cc:1955-1956), look 1 and every later top of an LM iteration is g2o's `i < iterations && !terminate()`
 * (core/sparse_optimizer.cpp), and one more follows every rejected trial that is to be retried (`rho < 0 && qmax < max &&
 * !terminate()`, core/optimization_algorithm_levenberg.cpp); the batched entry looks once per round of trials.  Armed with look >= 0,
 * the looks number look, look + 1, ... read as raised, whatever the caller's memory holds; the call needs a non-NULL stop pointer
 * (a NULL one is never looked at).  A negative value disarms; the script disarms itself when the call returns.  A call made while
 * the hook is not armed queues exactly what it queued without the hook. */
int gfs_test_lba_stop_at_look(int look);
/* What the calling thread's last such call did: the looks it made; the iterations that had run ahead of a raised flag and were
 * discarded (k_lba_restore); the forced decides it queued (a trial closed without a rho test); *ahead_at_stop = 1 / 0 when the flag
 * was seen up with / without an iteration queued ahead of the host's knowledge, -1 when it was not seen up after the entry check. */
int gfs_test_lba_last_looks(int32_t* looks, int32_t* discarded, int32_t* forced_decides, int32_t* ahead_at_stop);

/* GPU test hook: the linear step of the FIRST Levenberg-Marquardt trial of a window, stage by stage.  The problem is staged as
 * gfs_lba_solve stages it; init, the build group of iteration 0 and the first trial run up to and including k_lba_update, through
 * the dispatch of the product (the Schur kernel, one 128 x 128 block or several, the LDS or the HBM factorisation, the LDS sizes):
 * the hook is a tap in that sequence, not a second copy of it.  Hs / bs are copied out, stream-ordered, between the Schur launches
 * and k_lba_solve (the HBM factorisation works in place).  The blocks Hpp / Hll / Hpl / bp / bl of the same state are what
 * gfs_lba_linearize reports for the same handle and problem.  Every pointer is required (sizes for F free poses, n_points landmarks). */
typedef struct gfs_test_lba_trial {
  double* Dinv;     /* [n_points][6]  (Hll + lambda I)^-1: xx, xy, xz, yy, yz, zz */
  double* Hs;       /* [6F (6F + 1) / 2]  the reduced system as the Schur stage left it: packed lower triangle, row by row */
  double* bs;       /* [6F] */
  double* xp;       /* [6F]  the pose step */
  double* xl;       /* [n_points][3]  the landmark step */
  double lambda;    /* as k_lba_begin set it (computeLambdaInit) */
  double scale;     /* computeScale: the partial sums of k_lba_update added in block order */
  int32_t solve_ok; /* the reduced solve met no zero or non-finite pivot */
} gfs_test_lba_trial;
int gfs_test_lba_first_trial(gfs_lba* h, const gfs_lba_problem* p, gfs_test_lba_trial* out);

/* GPU test hook: the same tap in gfs_gba_solve's sequence (gfs_test_lba_stop_at_look scripts that entry's flag too; its look 0 is
 * the top of iteration 0).  Hs is delivered as the packed lower triangle row by row, whatever the tiling, copied out between the
 * assembly and the in-place factorisation. */
int gfs_test_gba_first_trial(gfs_gba* h, const gfs_lba_problem* p, gfs_test_lba_trial* out);
/* Rows of a tile of the tiled reduced system (csrc/gba_tiles.hpp: kP). */
int gfs_test_gba_panel_rows(void);
/* Host test hook (no GPU): the structure lists of csrc/gba_lists.hpp for a caller-order problem.  counts = {free poses, listed
 * blocks, contributions} is always filled; GFS_ERR_CAPACITY when a cap is too small.  order [n_edges]: the caller's edge at each
 * landmark-major position (the numbering of every edge id below); blk_ij [blocks][2]; blk_begin [blocks + 1]; contrib
 * [contributions][2] = (e1, e2); pose_begin [free poses + 1]; pose_edges [edges on free poses]. */
int gfs_test_gba_lists(int n_poses, int n_points, int n_edges, const uint8_t* pose_fixed, const int32_t* edge_pose, const int32_t* edge_point,
                       int64_t* counts, int32_t* order, int32_t* blk_ij, int64_t* blk_begin, int64_t cap_blocks, int32_t* contrib,
                       int64_t cap_contrib, int64_t* pose_begin, int32_t* pose_edges);
/* Host test hook (no GPU): csrc/gba_tiles.hpp for a system of n rows and its element (r, c), r >= c: out = {panels, bytes of the
 * storage, index of the element's tile, byte offset of the element}. */
int gfs_test_gba_tile_layout(int64_t n, int64_t r, int64_t c, uint64_t* out);

/* GPU test hook: the first trial of gfs_essential_graph_optimize's sequence (the estimates set, iteration 0 linearised, lambda =
 * lambda_init, the system assembled -- copied out here, ahead of the in-place factorisation -- factored and solved, the step applied,
 * the errors at the trial estimate).  n = dimension x free vertices.  Every pointer is required. */
typedef struct gfs_test_essential_graph_trial {
  double* H;        /* [n (n + 1) / 2] packed lower triangle, row by row, lambda on the diagonal */
  double* b;        /* [n] */
  double* x;        /* [n] */
  double chi2;      /* at the estimate as it came, summed in edge order */
  double trial_chi2; /* at the trial estimate */
  double scale;     /* computeScale: the vertices' terms added in vertex order */
  int32_t n_free, dimension;
  int32_t solve_ok;
} gfs_test_essential_graph_trial;
int gfs_test_essential_graph_first_trial(gfs_essential_graph* h, const gfs_essential_graph_problem* p, gfs_test_essential_graph_trial* out);
/* Host test hook (no GPU): the structure lists of csrc/eg_lists.hpp.  counts = {free vertices, listed blocks, terms} is always filled;
 * GFS_ERR_CAPACITY when a cap is too small.  free_index [n_vertices]; blk_ij [blocks][2]; blk_begin [blocks + 1]; contrib [terms] =
 * 4 edge + kind. */
int gfs_test_essential_graph_lists(int n_vertices, int n_edges, const uint8_t* vertex_fixed, const int32_t* edge_i, const int32_t* edge_j,
                                   int64_t* counts, int32_t* free_index, int32_t* blk_ij, int64_t* blk_begin, int64_t cap_blocks,
                                   int32_t* contrib, int64_t cap_contrib);

/* Test hook: how many workgroups a gfs_sim3_search launch of this handle may hold (csrc/sim3_search.hip: beyond the cap a workgroup
 * keeps its grid and walks several 256-point chunks).  0 = the default, what the device holds at once; < 0 = a workgroup a chunk;
 * > 0 = that many.  The results do not depend on it.  After gfs_sbp_reserve_sim3_search; a new reserve resets it. */
int gfs_test_sim3_search_groups(gfs_sbp* h, int max_groups);

/* GPU test hook: the stages of the handle's last gfs_frame_cloud_extract(_device) call, as they lie on the device: the scan table
 * (rows of begin, count, pad flags 1 = start | 2 = end, candidates in the scans in front), edge_raw / surf_raw, the two voxel
 * filters' outputs and the two radius filters' outputs.  Their sizes are the call's info; a NULL pointer skips a stage.  Refused
 * after a refused call. */
typedef struct gfs_test_frame_cloud_stage_buffers {
  int32_t* scans; /* [cap_scans][4] */
  int32_t cap_scans;
  float *edge_raw, *surf_raw, *edge_voxel, *surf_voxel, *edge, *surf; /* [cap_points][3] each */
  int32_t cap_points;
} gfs_test_frame_cloud_stage_buffers;
int gfs_test_frame_cloud_stages(gfs_frame_cloud* h, gfs_test_frame_cloud_stage_buffers* out);
/* GPU test hook: the handle's radius filter on its own (radius = the handle's local_map_resolution): the points of xyz [n][3] with
 * at least min_pts others within the radius, in input order -> out_xyz [cap >= n][3], *n_out.  Duplicates reach the filter only
 * here (inside the chain a voxel filter runs in front of it). */
int gfs_test_frame_cloud_radius(gfs_frame_cloud* h, const float* xyz, int n, int min_pts, float* out_xyz, int cap, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* GFS_ABI_TEST_H_ */
