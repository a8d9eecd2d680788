/* gfs_abi.h — C ABI of the MI355X-native GeoFlow-SLAM front-end hot path (libgfs_hip.so).
 *
 * This is the drop-in boundary.  The reference has no FFI layer: the seams are four
 * ordinary C++ methods (sections 1-4), followed by the neighbouring rows of SURVEY.md §8(f) (sections 5-10).  Each entry point below names the reference interface it replaces
 * (file:line in HorizonRobotics/GeoFlowSlam).  Signatures are plain C: pointers, sizes, POD structs.
 * No torch / OpenCV / Eigen types cross this boundary.  INTEGRATION.md shows the reference-side
 * adaptor (what a maintainer adds to src/ORBextractor.cc etc. to call these).
 *
 * Conventions
 *   - every function returns GFS_OK (0) or a negative gfs_status unless documented otherwise;
 *     gfs_last_error() returns a thread-local human-readable message for the last failure.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point fails with
 *     GFS_ERR_NO_DEVICE.
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP device pointers on the
 *     handle's device.  `stream` is a hipStream_t passed as void* (NULL = the handle's own stream).
 *   - matrices are column-major (Eigen default), quaternions are (x, y, z, w).
 */
#ifndef GFS_ABI_H_
#define GFS_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFS_ABI_VERSION 1

typedef enum {
  GFS_OK = 0,
  GFS_ERR_INVALID_ARG = -1,
  GFS_ERR_NO_DEVICE = -2,   /* no gfx950 GPU / HIP runtime unusable */
  GFS_ERR_HIP = -3,         /* a HIP call failed; see gfs_last_error() */
  GFS_ERR_CAPACITY = -4,    /* caller buffer or handle capacity too small */
  GFS_ERR_UNSUPPORTED = -5, /* configuration outside what the kernels implement */
  GFS_ERR_STOPPED = -6      /* stop flag was raised (LBA) */
} gfs_status;

int gfs_abi_version(void);
const char* gfs_last_error(void);
/* number of usable gfx950 devices (0 if none / HIP unavailable) */
int gfs_device_count(void);

/* ============================================================================================
 * 1. ORB extraction — replaces ORB_SLAM3::ORBextractor
 *      ctor        include/ORBextractor.h:53-54, src/ORBextractor.cc:421-479
 *      operator()  include/ORBextractor.h:61-64, src/ORBextractor.cc:1145-1225
 *      getters     include/ORBextractor.h:66-80
 *    called from Frame::ExtractORB (src/Frame.cc:768-777).
 * ============================================================================================ */

/* Field order and types of cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id): 28 bytes. */
typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} gfs_keypoint;

typedef struct gfs_orb gfs_orb; /* opaque; re-entrant: concurrent calls on one handle serialise internally (F9) */

typedef struct {
  int32_t nfeatures;   /* ORBextractor.nFeatures   (1000) */
  float scale_factor;  /* ORBextractor.scaleFactor (1.2; must give non-integer level ratios) */
  int32_t nlevels;     /* ORBextractor.nLevels     (8)   */
  int32_t ini_th_fast; /* ORBextractor.iniThFAST   (20)  */
  int32_t min_th_fast; /* ORBextractor.minThFAST   (7)   */
  int32_t max_rows, max_cols; /* largest image the handle must accept */
  int32_t max_batch;   /* largest batch for the *_batch entry points */
  int32_t device;      /* HIP device ordinal */
  int32_t blur_taps_variant; /* 0: OpenCV >= 4.5.1 {18,34,48,56,48,34,18}; 1: 4.0-4.5.0 {18,34,49,55,49,34,18} */
} gfs_orb_config;

void gfs_orb_default_config(gfs_orb_config* cfg);
/* One handle per extractor.  nlevels = 1 is accepted (no pyramid is built; level 0 is the caller's image).
 *
 * WHICH IMAGES A HANDLE TAKES.  The workspace is sized once, from the geometry of max_rows x max_cols; a call with another size
 * rewrites the handle's tables (a device synchronisation and a dozen small uploads: not per-frame work) and is taken when
 *   - rows <= max_rows and cols <= max_cols                                          (else GFS_ERR_CAPACITY),
 *   - every pyramid level holds at least one 35 x 35 FAST cell inside its 16-pixel border, i.e. the top level is at least 67 x 67,
 *     and the image is smaller than 4096 x 4096                                      (else GFS_ERR_UNSUPPORTED),
 *   - the image's own geometry fits what the max size reserved: pyramid and blur bytes, FAST cells, candidate slots, and the
 *     key-point capacity kp_cap = sum over levels of (quota + 3 + 4 nIni), nIni = max(1, round(width / height)) of the level's
 *     border box (cols - 32, rows - 32) -- the handle holds kp_cap of max_rows x max_cols, + 8  (else GFS_ERR_CAPACITY).
 * The last rule is NOT "any smaller image": nIni is rounded per level, and the small top levels of a smaller image can round up where
 * those of the max size round down.  With the default configuration (1000 features, 8 levels, 640 x 480: kp_cap 1056, 1064 held)
 *   - 320 x 240, the same aspect ratio, needs 1068 -- its top three levels are 129 x 96, 107 x 80 and 89 x 67, nIni = 2 each -- and
 *   - 640 x 300 needs 1100 (nIni = 2 on levels 0..4, 3 above);
 * both are refused with GFS_ERR_CAPACITY, gfs_last_error() = "image 320x240 needs more workspace than the handle reserved".  A
 * refused call changes nothing: the handle keeps the geometry, the results and the device buffers of its last accepted call and
 * takes the next image as if the refused one had not been tried.  A caller that feeds several sizes creates one handle per size, or
 * creates the handle with the max_rows x max_cols whose kp_cap is the largest of its sizes (gfs_orb_max_keypoints reports
 * what a handle holds).  Resizing a handle's workspace is not implemented.
 * A level whose nIni exceeds 4, or whose quota + 4 nIni + 8 exceeds 768, is outside the device quadtree: such a call is taken, with
 * the same results, through the host quadtree (slower: one round trip of the candidates). */
int gfs_orb_create(const gfs_orb_config* cfg, gfs_orb** out);
void gfs_orb_destroy(gfs_orb* h);

/* GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:66-80) plus the per-level feature quota and the umax table. Any pointer may be NULL. */
int gfs_orb_get_tables(const gfs_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                       int32_t* features_per_level, int32_t* umax16);
/* upper bound of keypoints one image can produce: kp_cap of max_rows x max_cols + 8 (per level quota + 3 + 4 nIni: the octree may
 * overshoot its quota, and keeps the 4 nIni nodes of its first sweep whatever the quota; see gfs_orb_create). */
int gfs_orb_max_keypoints(const gfs_orb* h);

/* operator()(image, mask (ignored), keypoints, descriptors, vLappingArea): host image (CV_8UC1, `stride`
 * bytes per row) -> kps[cap], desc[cap*32], *n = number of keypoints.
 * RETURNS monoIndex (>= 0; == *n on the RGB-D path where lapping = {0,0}), -1 for an empty image
 * (src/ORBextractor.cc:1150), or a gfs_status < -1 ... NOTE: to keep -1 unambiguous, errors are
 * reported as (GFS_ERR_* - 100).  Do NOT test the return value with `< 0` (-1 is the reference's own answer for an empty image): use
 * the two macros below. */
#define GFS_ORB_EXTRACT_FAILED(rc) ((rc) < -1)                            /* an error of the library, not the reference's -1 */
#define GFS_ORB_EXTRACT_STATUS(rc) ((rc) < -1 ? (rc) + 100 : GFS_OK)      /* the gfs_status behind a failed call */
int gfs_orb_extract(gfs_orb* h, const uint8_t* img, int rows, int cols, int stride, int lap0, int lap1,
                    gfs_keypoint* kps, uint8_t* desc, int cap, int* n);

/* Batched operator() over B independent host images of identical size: image b at imgs[b].
 * kps: [B][cap], desc: [B][cap][32], n/mono_index: [B]. */
int gfs_orb_extract_batch(gfs_orb* h, const uint8_t* const* imgs, int B, int rows, int cols, int stride, int lap0,
                          int lap1, gfs_keypoint* kps, uint8_t* desc, int cap, int* n, int* mono_index);

/* Device-resident batch: dev_imgs is [B][rows][cols] dense u8 already in HBM.  Results stay in HBM in
 * handle-owned buffers (see gfs_orb_device_results) until the next call on this handle. */
int gfs_orb_extract_batch_device(gfs_orb* h, const void* dev_imgs, int B, int rows, int cols, int lap0, int lap1,
                                 void* stream);
/* Device result views of the last *_device call: kps [B][cap] gfs_keypoint, desc [B][cap][32] u8,
 * counts [B] int32 (n), mono [B] int32. */
int gfs_orb_device_results(gfs_orb* h, void** dev_kps, void** dev_desc, void** dev_counts, void** dev_mono, int* cap);
/* Copy the last device results of image b to host buffers. */
int gfs_orb_fetch(gfs_orb* h, int b, gfs_keypoint* kps, uint8_t* desc, int cap, int* n, int* mono_index);

/* Introspection used by the parity tests (mvImagePyramid is a public member of the reference class,
 * include/ORBextractor.h:82): copies level `level` of image b of the last call (un-padded, rows*cols). */
int gfs_orb_level_size(const gfs_orb* h, int level, int* rows, int* cols);
int gfs_orb_fetch_level(gfs_orb* h, int b, int level, int blurred, uint8_t* dst);
/* FAST candidates handed to the octree for (image b, level): x, y relative to (16,16), score. Returns count. */
int gfs_orb_fetch_candidates(gfs_orb* h, int b, int level, int32_t* x, int32_t* y, int32_t* score, int cap);
/* Host-logic test hook (no GPU needed): the library's DistributeOctTree (src/ORBextractor.cc:567-768) on caller
 * candidates (integer x, y < 4096 relative to (min_x, min_y); score 0..255). Returns the number kept;
 * out_idx[i] = input index of the i-th kept keypoint in the reference's std::list order. */
int gfs_orb_octree_host(const int32_t* x, const int32_t* y, const int32_t* score, int n, int min_x, int max_x,
                        int min_y, int max_y, int n_features, int32_t* out_idx, int cap);
/* GPU test hook: the device DistributeOctTree kernel on caller candidates (min_x = min_y = 16). Writes the kept
 * candidates (x, y, score) in list order; returns their number. */
int gfs_orb_octree_device(int device, const int32_t* x, const int32_t* y, const int32_t* score, int n, int min_x, int max_x,
                          int min_y, int max_y, int n_features, int32_t* out_x, int32_t* out_y, int32_t* out_score, int cap);
/* (the gfs_test_* hooks of the library's internal replicas -- sort, glibc math, traffic calibration -- are in gfs_abi_test.h) */

/* ============================================================================================
 * 2. Brute-force Hamming matching — replaces
 *      ORBmatcher::DescriptorDistance                       include/ORBmatcher.h:41, src/ORBmatcher.cc:2536-2550
 *      cv::BFMatcher(NORM_HAMMING).match(d1, d2, matches)   src/ORBmatcher.cc:755-756, 805-806, 888-889
 * ============================================================================================ */

/* 256-bit Hamming distance of two 32-byte descriptors (pure host helper, bit-identical to DescriptorDistance). */
int gfs_hamming256(const uint8_t* a, const uint8_t* b);

typedef struct gfs_matcher gfs_matcher;
int gfs_matcher_create(int device, int max_query, int max_train, int max_batch, gfs_matcher** out);
void gfs_matcher_destroy(gfs_matcher* h);

/* matcher.match(query, train): for every query row i the train row j of minimum Hamming distance, lowest j on
 * ties -> train_idx[i], dist[i] (DMatch{queryIdx=i, trainIdx=train_idx[i], imgIdx=0, distance=(float)dist[i]}).
 * Returns the number of matches written: nq, or 0 when the train set is empty (no matches, as OpenCV). */
int gfs_bf_match_hamming(gfs_matcher* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                         int32_t* train_idx, int32_t* dist);

/* Device-resident batch of B independent pairs.  dev_query/dev_train: [B][stride_rows][32] u8;
 * dev_nq/dev_nt: [B] int32 row counts (device memory); outputs dev_train_idx/dev_dist: [B][stride_rows] int32
 * (entries >= nq[b] untouched; train_idx = -1, dist = INT32_MAX when nt[b] == 0). */
int gfs_bf_match_hamming_batch_device(gfs_matcher* h, const void* dev_query, const void* dev_nq, const void* dev_train,
                                      const void* dev_nt, int B, int stride_rows, void* dev_train_idx, void* dev_dist,
                                      void* stream);

/* ============================================================================================
 * 3. GICP registration — replaces RegistrationGICP::RegisterPointClouds
 *      include/RegistrationGICP.h:25-28, src/RegistrationGICP.cc:5-20
 *    (small_gicp::align<float,4> with GICPFactor + LevenbergMarquardtOptimizer,
 *     Thirdparty/small_gicp/src/small_gicp/registration/registration_helper.cpp:57-122)
 *    called from Tracking::PredictStateICP (src/Tracking.cc:3380-3382).
 * ============================================================================================ */
typedef struct {
  int32_t num_threads;                /* kept for signature parity (src/RegistrationGICP.cc:10); ignored on GPU */
  double downsampling_resolution;     /* 0.02 */
  double max_correspondence_distance; /* 0.1  */
  double rotation_eps;                /* 0.1 * pi / 180 */
  double translation_eps;             /* 1e-3 */
  int32_t max_iterations;             /* 20 */
  int32_t num_neighbors;              /* 10 */
} gfs_gicp_config;

/* Field-for-field small_gicp::RegistrationResult (registration/registration_result.hpp:10-30). */
typedef struct {
  double T_target_source[16]; /* column-major 4x4 */
  int32_t converged;
  uint64_t iterations;
  uint64_t num_inliers;
  double H[36]; /* column-major 6x6 */
  double b[6];
  double error;
  /* extra diagnostics */
  int32_t n_target_downsampled, n_source_downsampled, n_linearize, n_error_evals;
} gfs_gicp_result;

typedef struct gfs_gicp gfs_gicp;
void gfs_gicp_default_config(gfs_gicp_config* cfg);
int gfs_gicp_create(int device, int max_points, int max_batch, gfs_gicp** out);
void gfs_gicp_destroy(gfs_gicp* h);

/* RegisterPointClouds(target_points, source_points, init_T_target_source): clouds are arrays of
 * Eigen::Vector4f (x, y, z, w; w ignored and forced to 1 like points/point_cloud.hpp:29). */
int gfs_gicp_align(gfs_gicp* h, const float* target_xyzw, int nt, const float* source_xyzw, int ns,
                   const double init_T_target_source[16], const gfs_gicp_config* cfg, gfs_gicp_result* out);

/* Device-resident batch of B independent (target, source) pairs.  dev_target/dev_source: [B][stride_pts][4] f32,
 * dev_nt/dev_ns: [B] int32 (device), init_T: host [B][16] (NULL = identity), out: host [B]. */
int gfs_gicp_align_batch_device(gfs_gicp* h, const void* dev_target, const void* dev_nt, const void* dev_source,
                                const void* dev_ns, int B, int stride_pts, const double* init_T,
                                const gfs_gicp_config* cfg, gfs_gicp_result* out, void* stream);

/* Streaming form (the gfs_gicp_cache of SURVEY.md 8b) for Tracking::PredictStateICP, where the target of every call is the
 * source of the previous one (src/Tracking.cc:3375-3382: target = mLastFrame.source_points, source = mCurrentFrame's): the
 * handle keeps the preprocessed clouds (voxel means, covariances, search grid) of its last call's SOURCES in HBM; these
 * calls register new source clouds against them and preprocess only the new clouds.  The result is bit-identical to
 * gfs_gicp_align*(previous sources, new sources) — preprocessing is deterministic, so reusing it changes nothing but the time.
 * GFS_ERR_INVALID_ARG unless the previous call on this handle had the same batch size, stride and preprocessing parameters. */
int gfs_gicp_align_next(gfs_gicp* h, const float* source_xyzw, int ns, const double init_T_target_source[16],
                        const gfs_gicp_config* cfg, gfs_gicp_result* out);
int gfs_gicp_align_next_batch_device(gfs_gicp* h, const void* dev_source, const void* dev_ns, int B, int stride_pts,
                                     const double* init_T, const gfs_gicp_config* cfg, gfs_gicp_result* out, void* stream);

/* Introspection for parity tests: preprocessing output (voxel means + covariances) of cloud `which`
 * (0 = target, 1 = source) of pair b of the last call. pts: [m][4] f64, covs: [m][9] f64 (3x3 col-major). */
int gfs_gicp_fetch_preprocessed(gfs_gicp* h, int b, int which, double* pts, double* covs, int cap, int* m);
/* Diagnostics: the handle's counter block of eight words since the last reset.  The library as built writes none of them; the
 * variant builds do (tools/variant.sh): -DGFS_KNN_UTIL counts in k_knn_cov out8[0] / [1] lanes at work / steps of the own-row walk,
 * [2] / [3] the same of the one loop over a lane's neighbouring rows, [4] / [5] queries / waves, [6] points of the own rows
 * (tools/probes/knn_util_probe.py); -DGFS_LIN_UTIL counts in the linearisation's 1-NN search [2] / [3] lanes / rounds of neighbouring
 * rows, [4] / [5] lanes / steps of the walk, [6] / [7] searches / waves (tools/probes/lin_util_probe.py).  Counted only by handles
 * created with GFS_GICP_TILE_STATS=1 in the environment (atomics of every wave on a few addresses are not free). */
int gfs_gicp_tile_stats(gfs_gicp* h, unsigned long long* out8, int reset);
/* Diagnostics (tools/knn_probe.py): out = {down-sampled points, queries deferred to the r = 2 pass, queries deferred to the
 * isolated-point pass} of cloud (b, which) of the last call; dk (may be NULL): the squared-distance bounds of the latter. */
int gfs_gicp_knn_stats(gfs_gicp* h, int b, int which, int out[3], double* dk, int cap);
/* Diagnostics: how the Levenberg-Marquardt loops of this handle's calls were driven.  out = {launches of the cooperative kernel
 * (the loop of a few pairs in ONE launch: a single live stream, a batch that fits the workgroup budget) so far, workgroups of the last such launch,
 * 1 if a launch ever failed to become resident and the handle fell back to a launch per step for good, the workgroup budget}. */
int gfs_gicp_coop_stats(gfs_gicp* h, int out[4]);

/* ============================================================================================
 * 4. Local bundle adjustment — replaces the numeric core of Optimizer::LocalBundleAdjustment
 *      include/Optimizer.h:62-65, src/Optimizer.cc:1588-2040 (graph build 1662-1953, optimize(10) 1958-1959,
 *      chi2 classification 1961-1999) with g2o BlockSolver<6,3> + Levenberg (Thirdparty/g2o).
 *    The pointer-graph gather / write-back (src/Optimizer.cc:1592-1660, 2003-2039) stays in the C++ adaptor.
 * ============================================================================================ */
typedef struct {
  int32_t n_poses, n_points, n_edges;
  const double* pose_q;      /* [n_poses][4] unit quaternion (x,y,z,w) of Tcw */
  const double* pose_t;      /* [n_poses][3] */
  const uint8_t* pose_fixed; /* [n_poses] 1 = fixed (setFixed(true), src/Optimizer.cc:1697,1715) */
  const double* points;      /* [n_points][3] world coordinates */
  const int32_t* edge_pose;  /* [n_edges] */
  const int32_t* edge_point; /* [n_edges]; several edges may join the same (pose, point) pair, as in g2o */
  const double* edge_obs;    /* [n_edges][3] (u, v, u_right); u_right ignored for mono edges */
  const double* edge_inv_sigma2; /* [n_edges] information = inv_sigma2 * I */
  const uint8_t* edge_stereo;    /* [n_edges] 1 = EdgeStereoSE3ProjectXYZ, 0 = EdgeSE3ProjectXYZ */
  double fx, fy, cx, cy, bf;
  double huber_mono, huber_stereo; /* sqrt(5.991), sqrt(7.815) (src/Optimizer.cc:1728-1729) */
  int32_t iterations;              /* 10 (src/Optimizer.cc:1959) */
} gfs_lba_problem;

typedef struct {
  double* pose_q;               /* [n_poses][4] */
  double* pose_t;               /* [n_poses][3] */
  double* points;               /* [n_points][3] */
  double* edge_chi2;            /* [n_edges] e->chi2() at the solution */
  uint8_t* edge_depth_positive; /* [n_edges] e->isDepthPositive() */
  int32_t iterations_run;
  double final_chi2, final_lambda;
} gfs_lba_solution;

typedef struct gfs_lba gfs_lba;
int gfs_lba_create(int device, int max_poses, int max_points, int max_edges, gfs_lba** out);
void gfs_lba_destroy(gfs_lba* h);
/* optimizer.optimize(iterations) with the stop flag polled like setForceStopFlag (src/Optimizer.cc:1679). */
int gfs_lba_solve(gfs_lba* h, const gfs_lba_problem* p, gfs_lba_solution* s, volatile const int* stop);
/* The same with the reference's own flag type: `stop` points at a C++ bool (one byte), e.g. pbStopFlag = &mbAbortBA of
 * LocalMapping (src/LocalMapping.cc: mbAbortBA is raised by the tracking thread while the adjustment runs).  It is read live,
 * at the top of every iteration and after every trial step, like g2o's setForceStopFlag (src/Optimizer.cc:1679). */
int gfs_lba_solve_bool(gfs_lba* h, const gfs_lba_problem* p, gfs_lba_solution* s, const volatile unsigned char* stop);
/* One BlockSolver::buildSystem (core/block_solver.hpp:502-558): Hpp [n_free][36] (col-major 6x6 diagonal blocks,
 * free poses in ascending index order), Hll [n_points][9], Hpl per edge [n_edges][18] (6x3 col-major, zero for
 * edges on fixed poses), bp [n_free][6], bl [n_points][3], edge_chi2 [n_edges]. Returns robust chi2 in *chi2. */
int gfs_lba_linearize(gfs_lba* h, const gfs_lba_problem* p, double* Hpp, double* Hll, double* Hpl, double* bp,
                      double* bl, double* edge_chi2, double* chi2);
/* n independent windows solved together (replicas: the LBA of one map does not shard; a server bundle-adjusting many maps, or
 * several candidate windows, fills the GPU this way).  Per window the result is bit-identical to gfs_lba_solve; the phase
 * kernels of all windows share their launches.  `stop` (may be NULL) is polled between LM trials: when raised, every window
 * closes its running iteration like SparseOptimizer::terminate() and returns what it has. */
typedef struct gfs_lba_batch gfs_lba_batch;
int gfs_lba_batch_create(int device, int max_windows, int max_poses, int max_points, int max_edges, gfs_lba_batch** out);
void gfs_lba_batch_destroy(gfs_lba_batch* h);
int gfs_lba_solve_batch(gfs_lba_batch* h, const gfs_lba_problem* problems, gfs_lba_solution* solutions, int n,
                        volatile const int* stop);

/* Optimizer::LocalVisualLidarBA (include/Optimizer.h:71, src/Optimizer.cc:1101-1587), called by LocalMapping::Run instead of
 * LocalBundleAdjustment when UsePointCloudObs and UseLidarLocalBA are both set (src/LocalMapping.cc:182-183, 231-240): the window
 * of gfs_lba_problem plus, for every local key-frame with mnMatchesInliers <= 75 (:1338) and a downsampled cloud of at least 50
 * points (GenerateLidarEdge, :8343-8345), the EdgeSE3LidarPoint2Plane edges GenerateLidarEdge builds (:1327-1362): 5-NN in the one
 * local map, float ColPivHouseholderQR plane, the 0.2 plane and s > 0.1 weight gates, as in section 11.  The association runs once,
 * before the optimisation, at the key-frame's stored pose: initPose = toMatrix4d(pKFi->GetPose().inverse()) (:1341) evaluated on
 * ((float) pose_q, (float) pose_t), which is exact for poses that come from Sophus::SE3f as the reference's do.  The edges stay fixed
 * for the 10 iterations.  Error s (n . (Twc p) + d), information 1e2 (:1348), Huber delta (float) sqrt(1.0) (:1328), g2o's numeric
 * Jacobian (central differences, delta 1e-9).  The edges of the fixed initial key-frame count in chi2, not in H / b.  Edge order
 * (g2o's sums): all lidar edges before the reprojection edges, key-frames in pose order (lLocalKeyFrames order), then cloud order.
 * The reprojection-edge outputs (chi2, depth, num_edges) are those of gfs_lba_solve; lidar edges only move the estimate.  Fixed
 * cameras (pose_local = 0) never get edges.  A window without lidar key-frames runs gfs_lba_solve's path: the same bits.
 * Refused: a map on another device or never set (GFS_ERR_INVALID_ARG), lidar key-frames' clouds beyond the capacity reserved with
 * gfs_lba_lidar_reserve (GFS_ERR_CAPACITY; nothing is truncated), two_camera != 0 (GFS_ERR_UNSUPPORTED).
 * DESIGN.md "Local BA with lidar edges". */
typedef struct {
  const struct gfs_lidar_map* map; /* laserCloudSurfFromMapDS (section 11), on the handle's device */
  const uint8_t* pose_local;      /* [n_poses] 1 = in lLocalKeyFrames (the fixed initial key-frame included), 0 = fixed camera */
  const int32_t* matches_inliers; /* [n_poses] KeyFrame::mnMatchesInliers */
  const int32_t* cloud_begin;     /* [n_poses + 1], cloud_begin[0] = 0 */
  const float* cloud;             /* [cloud_begin[n_poses]][3] mpPointCloudDownsampled, camera frame */
  int32_t two_camera;             /* some local key-frame has mpCamera2: refused */
} gfs_lba_lidar;
/* Capacity for the concatenated clouds of a window's lidar key-frames (call before the first lidar call; again to change it). */
int gfs_lba_lidar_reserve(gfs_lba* h, int max_cloud_points);
/* optimizer.optimize(10) with the lidar edges; stop flag as gfs_lba_solve.  pose_lidar_edges [n_poses] (may be NULL): edges of each pose. */
int gfs_lba_solve_lidar(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* lidar, gfs_lba_solution* s, int32_t* pose_lidar_edges,
                        volatile const int* stop);
/* The same with the reference's C++ bool flag (see gfs_lba_solve_bool). */
int gfs_lba_solve_lidar_bool(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* lidar, gfs_lba_solution* s,
                             int32_t* pose_lidar_edges, const volatile unsigned char* stop);
/* gfs_lba_linearize with the lidar edges: their terms in Hpp / bp and *chi2; lidar_edge_chi2 (up to cap) every lidar edge's chi2
 * in edge order; pose_lidar_edges [n_poses] (may be NULL). */
int gfs_lba_linearize_lidar(gfs_lba* h, const gfs_lba_problem* p, const gfs_lba_lidar* lidar, double* Hpp, double* Hll, double* Hpl,
                            double* bp, double* bl, double* edge_chi2, double* chi2, double* lidar_edge_chi2, int cap,
                            int32_t* pose_lidar_edges);
/* Diagnostic: the lidar edges of `pose` in the last lidar call on this handle (cloud index order): point index in the pose's cloud,
 * plane (pa, pb, pc, pd) and s.  Up to cap edges; *n = the pose's edge count. */
int gfs_lba_fetch_lidar_edges(gfs_lba* h, int pose, int32_t* index, float* plane /* [cap][4] */, float* s, int cap, int32_t* n);

/* Optimizer::GlobalBundleAdjustemnt -> Optimizer::BundleAdjustment (src/Optimizer.cc:47-363): optimizer.optimize(iterations) of the
 * full map after a loop closure or map merge (LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:2378: 10 iterations,
 * &mbStopGBA, bRobust = false) and of the monocular initial map (Tracking::CreateInitialMapMonocular, src/Tracking.cc:2963: 20
 * iterations).  The graph is LocalBundleAdjustment's (VertexSE3Expmap, marginalised VertexSBAPointXYZ, EdgeSE3ProjectXYZ /
 * EdgeStereoSE3ProjectXYZ, BlockSolver_6_3, Levenberg), so the problem and the solution are gfs_lba_problem / gfs_lba_solution; the
 * size is a map's: the reduced pose system is assembled from the pose pairs that share landmarks only and factored as a tiled dense
 * L D L^T over the whole device (DESIGN.md "Global bundle adjustment"), at every size.
 *  - No entry check: BundleAdjustment has no `if (*pbStopFlag) return` in front of optimize() (unlike src/Optimizer.cc:1955-1956).
 *    A flag that is already up gives GFS_OK, iterations_run = 0 and the caller's estimate bit for bit; never GFS_ERR_STOPPED.
 *    final_chi2 is then the robust chi2 of that estimate and final_lambda 0 (as gfs_lba_solve with iterations <= 0).
 *  - The flag (setForceStopFlag, src/Optimizer.cc:70-71) is read live where g2o reads it: at the top of every iteration
 *    (core/sparse_optimizer.cpp, `i < iterations && !terminate()`) -- the first look is the top of iteration 0 -- and after every
 *    rejected trial that would be retried (core/optimization_algorithm_levenberg.cpp).
 *  - bRobust = false (src/Optimizer.cc:171-176, 209-214: no setRobustKernel) is huber_mono = huber_stereo = +INFINITY:
 *    RobustKernelHuber::robustify then takes its `e <= dsqr` branch, rho = (e, 1, 0), and the multiplications by rho[1] = 1.0 are
 *    exact -- the kernel-free arithmetic.  A finite value is g2o with the kernel (thHuber2D / thHuber3D, :60-61).
 *  - gfs_gba_create fails cleanly (GFS_ERR_CAPACITY / GFS_ERR_HIP) when the reduced system and the workspaces of max_poses poses do
 *    not fit the device; gfs_gba_solve returns GFS_ERR_CAPACITY above the handle's limits.
 *  - edge_chi2 and edge_depth_positive are evaluated at the estimate that is returned.
 * Second-camera observations are the adaptor's to refuse, as for LocalBundleAdjustment. */
typedef struct gfs_gba gfs_gba;
typedef struct {
  int32_t n_free, panel_rows, panels; /* free poses; rows of a tile of the reduced system; tile rows */
  int64_t block_pairs, contributions; /* listed 6 x 6 blocks of the lower triangle; (edge, edge) terms in their lists */
  int64_t system_bytes;               /* bytes of the tiled reduced system */
  int32_t trials, launches;           /* Levenberg trials run; kernel launches of the call */
} gfs_gba_info;
int gfs_gba_create(int device, int max_poses, int max_points, int max_edges, gfs_gba** out);
void gfs_gba_destroy(gfs_gba* h);
int gfs_gba_solve(gfs_gba* h, const gfs_lba_problem* p, gfs_lba_solution* s, volatile const int* stop);
/* The same with the reference's own flag type (a C++ bool: &mbStopGBA). */
int gfs_gba_solve_bool(gfs_gba* h, const gfs_lba_problem* p, gfs_lba_solution* s, const volatile unsigned char* stop);
/* What the handle's last gfs_gba_solve did. */
int gfs_gba_last_info(const gfs_gba* h, gfs_gba_info* info);

/* ============================================================================================
 * 5. Frame helpers next to the hot path — keep GICP input and RGB-D "stereo" coordinates on device
 *      Frame::ConvertDepthToPointCloud(downSample, ...)   src/Frame.cc:590-623
 *      Frame::ComputeStereoFromRGBD(imDepth)              src/Frame.cc:1314-1332
 * ============================================================================================ */
typedef struct gfs_frame gfs_frame;
int gfs_frame_create(int device, int max_rows, int max_cols, int max_keypoints, gfs_frame** out);
void gfs_frame_destroy(gfs_frame* h);
/* depth: CV_32F metres, `stride_elems` floats per row.  Emits (x, y, z, 1) for every pixel of the `downsample` grid with
 * 0 < depth < 10 in raster order (the reference's push_back order): x = (u - cx) * depth / fx, y = (v - cy) * depth / fy.
 * An empty depth image yields *n = 0 (the reference logs an error and returns). */
int gfs_depth_to_cloud(gfs_frame* h, const float* depth, int rows, int cols, int stride_elems, int downsample, float fx,
                       float fy, float cx, float cy, float* out_xyzw, int cap, int* n);
/* dev_depth [B][rows][cols] f32 -> dev_out_xyzw [B][stride_pts][4] f32 + dev_counts [B] int32: exactly the cloud layout
 * gfs_gicp_align_batch_device consumes. */
int gfs_depth_to_cloud_batch_device(gfs_frame* h, const void* dev_depth, int B, int rows, int cols, int downsample, float fx,
                                    float fy, float cx, float cy, void* dev_out_xyzw, int stride_pts, void* dev_counts,
                                    void* stream);
/* imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) for a CV_16U sensor image (src/Tracking.cc:1622-1623), on the device: the
 * depth maps then cross PCIe as 2 bytes a pixel.  dev_depth_u16 [B][rows][cols] u16 (8-byte aligned) -> dev_depth_f32 (16-byte
 * aligned), float(raw) * factor in single precision like cv::Mat::convertTo. */
int gfs_depth_convert_u16_batch_device(gfs_frame* h, const void* dev_depth_u16, int B, int rows, int cols, float factor,
                                       void* dev_depth_f32, void* stream);
/* mvDepth[i] = d = imDepth.at<float>(kp.pt.y, kp.pt.x) (float -> int truncation), mvuRight[i] = kpUn.pt.x - bf / d when
 * d > 0, else both -1.  kps_un_x may be NULL (no distortion: mvKeysUn == mvKeys). */
int gfs_stereo_from_rgbd(gfs_frame* h, const gfs_keypoint* kps, const float* kps_un_x, int n, const float* depth, int rows,
                         int cols, int stride_elems, float bf, float* u_right, float* depth_out);
int gfs_stereo_from_rgbd_batch_device(gfs_frame* h, const void* dev_kps, const void* dev_kps_un_x, const void* dev_counts,
                                      int B, int kp_stride, const void* dev_depth, int rows, int cols, float bf,
                                      void* dev_u_right, void* dev_depth_out, void* stream);
/* The RGB-D tail of the Frame constructor in one call: ComputeStereoFromRGBD(imDepth) (src/Frame.cc:1314-1332) followed by
 * ConvertDepthToPointCloud (:590-623).  The depth map is uploaded once and the cloud stays on the device: *dev_cloud /
 * *dev_count / *cloud_stride are the arguments gfs_gicp_align_batch_device / gfs_gicp_align_next_batch_device take (valid until
 * the next call on this handle).  out_xyzw may be NULL (no host copy of the cloud); *n_cloud receives the point count.
 * depth == NULL: use the depth map the previous gfs_frame_rgbd call on this handle uploaded (same rows x cols); downsample <= 0:
 * no cloud in this call.  Together: the cloud first (n = 0), the registration, and the stereo coordinates when the key-points of
 * an ORB extraction that ran beside the registration have arrived -- one depth upload either way. */
int gfs_frame_rgbd(gfs_frame* h, const gfs_keypoint* kps, const float* kps_un_x, int n, const float* depth, int rows, int cols,
                   int stride_elems, float bf, int downsample, float fx, float fy, float cx, float cy, float* u_right,
                   float* depth_out, float* out_xyzw, int cap, int* n_cloud, void** dev_cloud, void** dev_count, int* cloud_stride);

/* ============================================================================================
 * 6. Optimizer::PoseOptimization — motion-only bundle adjustment of a frame
 *      int Optimizer::PoseOptimization(Frame*, bool, bool, int)      src/Optimizer.cc:763-1098
 *    conventional-SLAM branch (pFrame->mpCamera2 == nullptr): EdgeSE3ProjectXYZOnlyPose (src/OptimizableTypes.cpp:49-63) and
 *    g2o::EdgeStereoSE3ProjectXYZOnlyPose (Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:339-404), Huber kernels,
 *    4 rounds x optimize(10) with BlockSolver_6_3 + LinearSolverDense + OptimizationAlgorithmLevenberg.
 *    The two-camera rigid-body branch (:883-951, EdgeSE3ProjectXYZOnlyPoseToBody) is not implemented.
 *    Non-finite input is not rejected: a NaN / inf observation, point or information and a point at camera z = 0 go through the
 *    arithmetic as they do in g2o (a NaN chi2 is never above its gate, so the edge stays an inlier and no trial is accepted: the input
 *    pose comes back, avg_reproj_error is NaN; an inf chi2 leaves after round 0), the call returns, and the default sum order gives
 *    the sequential code's outputs for them too (tests/test_gpu_pose_step.py).
 * ============================================================================================ */
typedef struct {
  double q[4], t[3];          /* Tcw = pFrame->GetPose(): unit quaternion (x, y, z, w) and translation cast to double (:784-786) */
  int32_t n_obs;              /* key-points that have a MapPoint, in key-point index order (= edge creation order) */
  const double* xw;           /* [n_obs][3] pMP->GetWorldPos().cast<double>() */
  const double* obs;          /* [n_obs][3] kpUn.pt.x, kpUn.pt.y, mvuRight[i] (third value ignored for mono edges) */
  const float* inv_sigma2;    /* [n_obs] mvInvLevelSigma2[kpUn.octave] */
  const uint8_t* stereo;      /* [n_obs] mvuRight[i] >= 0 */
  double fx, fy, cx, cy, bf;  /* pFrame->fx ... mbf (floats widened to double, :865-869) */
  int32_t n_rounds;           /* 4 */
  int32_t its;                /* 10 (its[] = {10, 10, 10, 10}) */
} gfs_pose_problem;

typedef struct {
  uint8_t* outlier;       /* [n_obs] pFrame->mvbOutlier after the last round */
  double* chi2;           /* [n_obs] e->chi2() as read by the last classification */
  double q[4], t[3];      /* vSE3_recov->estimate(): the reference computes it and then drops it (SetPose is commented out, :1078-1097) */
  float avg_reproj_error; /* value of the last SetFrame2FrameReprojError / SetFrame2MapReprojError call */
  int32_t n_inliers;      /* return value: nInitialCorrespondences - nBad (0 when there are fewer than 3 correspondences) */
  int32_t rounds_run, iterations_run;
} gfs_pose_solution;

typedef struct gfs_pose gfs_pose;
int gfs_pose_create(int device, int max_obs, int max_batch, gfs_pose** out);
void gfs_pose_destroy(gfs_pose* h);
/* B independent frames (host pointers), one workgroup per frame. */
int gfs_pose_optimize(gfs_pose* h, const gfs_pose_problem* problems, int B, gfs_pose_solution* solutions);
/* How the sums over a frame's edges (activeRobustChi2, the 6x6 normal equations, the inliers' mean chi2) are added up.
 *   GFS_POSE_SUMS_EDGE_ORDER (default since round 6): g2o's order, edge after edge on one lane (core/sparse_optimizer.cpp:104-122,
 *     core/base_unary_edge.hpp:43-72): every double as the sequential code computes it -- mvbOutlier, the return value, the LM
 *     iteration counts and the pose are those of the reference's single-threaded solve, bit for bit against the oracle restatement.
 *   GFS_POSE_SUMS_TREE (opt-in): a tree of fixed shape -- deterministic, the same bits for a frame alone or inside any batch, about
 *     half the latency of a single frame; against g2o's edge-by-edge sums the last bits differ.  GUARANTEED (tests/test_gpu_pose.py):
 *     pose within 1e-7 relative; an outlier flag can differ only for an edge whose chi2 sits within 7.8e-6 of 5.991 / 7.815, the LM
 *     iteration count by at most 2.  A caller that needs the reference's flags exactly keeps the default. */
#define GFS_POSE_SUMS_TREE 0
#define GFS_POSE_SUMS_EDGE_ORDER 1
int gfs_pose_set_sum_order(gfs_pose* h, int order);

/* ============================================================================================
 * 7. ORBmatcher::SearchByProjection, frame to frame — the windowed matcher of TrackWithMotionModel
 *      int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool bMono)
 *                                                                             src/ORBmatcher.cc:1853-2063
 *    with Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (src/Frame.cc:734-761, 1073-1084, 1007-1071),
 *    ORBmatcher::DescriptorDistance (:2536-2550, TH_HIGH = 100) and ComputeThreeMaxima (:2500-2532, HISTO_LENGTH = 30).
 *    Single-camera frames only (Nleft == -1); the two-camera branch (:1951-2035) is not implemented.
 * ============================================================================================ */
typedef struct {
  /* LastFrame: the key-points i with mvpMapPoints[i] != NULL && !mvbOutlier[i], in index order (the loop of :1872-1875) */
  int32_t n_last;
  const float* last_xw;           /* [n_last][3] pMP->GetWorldPos() */
  const uint8_t* last_desc;       /* [n_last][32] pMP->GetDescriptor() */
  const int32_t* last_octave;     /* [n_last] LastFrame.mvKeys[i].octave */
  const float* last_angle;        /* [n_last] LastFrame.mvKeysUn[i].angle */
  const uint8_t* last_mp_has_obs; /* [n_last] pMP->Observations() > 0 */
  /* CurrentFrame */
  int32_t n_cur;
  const gfs_keypoint* cur_kps_un; /* [n_cur] mvKeysUn (cv::KeyPoint layout) */
  const float* cur_u_right;       /* [n_cur] mvuRight */
  const uint8_t* cur_desc;        /* [n_cur][32] mDescriptors */
  const uint8_t* cur_has_mp_obs;  /* [n_cur] mvpMapPoints[i] != NULL && ->Observations() > 0 on entry */
  float Tcw_q[4], Tcw_t[3];       /* CurrentFrame.GetPose(): Sophus::SE3f unit quaternion (x, y, z, w), translation */
  float Tlw_q[4], Tlw_t[3];       /* LastFrame.GetPose() */
  float fx, fy, cx, cy;           /* CurrentFrame.mpCamera (Pinhole) */
  float bf, b;                    /* CurrentFrame.mbf, mb */
  float min_x, max_x, min_y, max_y; /* Frame::mnMinX ... mnMaxY */
  float grid_w_inv, grid_h_inv;   /* Frame::mfGridElementWidthInv / HeightInv (64 x 48 grid) */
  const float* scale_factors;     /* CurrentFrame.mvScaleFactors */
  int32_t n_levels;               /* <= 16 */
  float th;                       /* window size factor (15 mono, 7 stereo in Tracking::TrackWithMotionModel) */
  int32_t mono;                   /* bMono */
  int32_t check_orientation;      /* ORBmatcher::mbCheckOrientation */
} gfs_sbp_problem;

typedef struct gfs_sbp gfs_sbp;
/* max_last <= 8192 map points, max_cur <= 4096 key-points per frame */
int gfs_sbp_create(int device, int max_last, int max_cur, int max_batch, gfs_sbp** out);
void gfs_sbp_destroy(gfs_sbp* h);
/* B independent frame pairs (host pointers).  cur_match[f][i] (n_cur entries): >= 0 = CurrentFrame.mvpMapPoints[i] now holds
 * the map point of last-list entry cur_match[f][i]; -1 = left as it was; -2 = reset to NULL by the rotation-consistency
 * check.  nmatches[f] = the function's return value (it counts overwritten assignments twice, like the reference). */
int gfs_search_by_projection(gfs_sbp* h, const gfs_sbp_problem* problems, int B, int32_t* const* cur_match, int32_t* nmatches);

/*      int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, float th, bool bFarPoints,
 *                                         float thFarPoints)                    src/ORBmatcher.cc:43-206
 *    (TrackLocalMap / relocalisation): the caller lists the map points that pass the filters of :53-58 (mbTrackInView, not
 *    beyond thFarPoints, !isBad()) with the projection Frame::isInFrustum left on them; the window depends on the viewing
 *    angle (RadiusByViewingCos :250-255), best / second-best ratio test (mfNNratio) when both sit on the same pyramid level. */
typedef struct {
  int32_t n_mp;
  const float* mp_proj;          /* [n_mp][3] pMP->mTrackProjX, mTrackProjY, mTrackProjXR */
  const int32_t* mp_level;       /* [n_mp] mnTrackScaleLevel */
  const float* mp_view_cos;      /* [n_mp] mTrackViewCos */
  const uint8_t* mp_desc;        /* [n_mp][32] GetDescriptor() */
  const uint8_t* mp_has_obs;     /* [n_mp] Observations() > 0 */
  int32_t n_cur;
  const gfs_keypoint* cur_kps_un; /* F.mvKeysUn */
  const float* cur_u_right;      /* F.mvuRight */
  const uint8_t* cur_desc;       /* F.mDescriptors */
  const uint8_t* cur_has_mp_obs; /* F.mvpMapPoints[i] != NULL && ->Observations() > 0 on entry */
  float min_x, min_y, grid_w_inv, grid_h_inv;
  const float* scale_factors;    /* F.mvScaleFactors */
  int32_t n_levels;
  float th;                      /* window factor (1, 3, 5 ... in Tracking::SearchLocalPoints) */
  float nn_ratio;                /* ORBmatcher::mfNNratio */
} gfs_sbp_map_problem;
/* cur_match[f][i]: >= 0 = F.mvpMapPoints[i] := map point of list entry cur_match[f][i]; -1 = left as it was. */
int gfs_search_by_projection_map(gfs_sbp* h, const gfs_sbp_map_problem* problems, int B, int32_t* const* cur_match,
                                 int32_t* nmatches);

/*      void Tracking::SearchLocalPoints()                                       src/Tracking.cc:4294-4359
 *    second loop onwards, in one call: Frame::isInFrustum (src/Frame.cc:876-931, Nleft == -1, Pinhole::project
 *    src/CameraModels/Pinhole.cpp:43-49) with MapPoint::PredictScale (src/MapPoint.cc:565-579: std::ceil(float) of glibc's logf)
 *    for every listed local map point, the filter of src/ORBmatcher.cc:53-58, and the search above over the survivors in list
 *    order.  The caller lists the points that pass `mnLastFrameSeen != F.mnId && !isBad()` (:4320-4321).  All arithmetic is
 *    float, every operation rounded once, sums left to right (DESIGN.md section 12 states the rule and its two chosen cases). */
typedef struct {
  int32_t n_mp;
  const float* mp_xw;            /* [n_mp][3] GetWorldPos() */
  const float* mp_normal;        /* [n_mp][3] GetNormal() */
  const float* mp_min_dist;      /* [n_mp] mfMinDistance (raw: the 0.8f of GetMinDistanceInvariance is applied here) */
  const float* mp_max_dist;      /* [n_mp] mfMaxDistance (raw: 1.2f likewise) */
  const uint8_t* mp_desc;        /* [n_mp][32] GetDescriptor() */
  const uint8_t* mp_has_obs;     /* [n_mp] Observations() > 0 */
  float Rcw[9], tcw[3], Ow[3];   /* F.mRcw (row-major), F.mtcw, F.mOw */
  float fx, fy, cx, cy, bf;      /* F.mpCamera (Pinhole), F.mbf */
  float min_x, max_x, min_y, max_y; /* F.mnMinX ... mnMaxY */
  float grid_w_inv, grid_h_inv;  /* F.mfGridElementWidthInv / HeightInv */
  const float* scale_factors;    /* F.mvScaleFactors */
  int32_t n_levels;              /* F.mnScaleLevels, <= 16 */
  float log_scale_factor;        /* F.mfLogScaleFactor */
  float view_cos_limit;          /* viewingCosLimit (0.5 in Tracking::SearchLocalPoints) */
  int32_t far_points;            /* mpLocalMapper->mbFarPoints */
  float th_far_points;           /* mpLocalMapper->mThFarPoints */
  float th;                      /* window factor */
  float nn_ratio;                /* ORBmatcher::mfNNratio (0.8) */
  int32_t n_cur;
  const gfs_keypoint* cur_kps_un; /* F.mvKeysUn */
  const float* cur_u_right;      /* F.mvuRight */
  const uint8_t* cur_desc;       /* F.mDescriptors */
  const uint8_t* cur_has_mp_obs; /* F.mvpMapPoints[i] != NULL && ->Observations() > 0 on entry */
} gfs_local_points_problem;

typedef struct {                 /* caller-owned arrays */
  uint8_t* in_view;              /* [n_mp] mbTrackInView */
  float* proj;                   /* [n_mp][3] mTrackProjX, mTrackProjY (-1, -1 until the image-bounds tests are passed), mTrackProjXR
                                  * (defined only where in_view) */
  float* depth;                  /* [n_mp] mTrackDepth   (defined where in_view, like the next two) */
  float* view_cos;               /* [n_mp] mTrackViewCos */
  int32_t* level;                /* [n_mp] mnTrackScaleLevel */
  int32_t* cur_match;            /* [n_cur] >= 0 = F.mvpMapPoints[i] := the caller's list entry cur_match[i]; -1 = left as it was */
  int32_t n_to_match;            /* nToMatch: the number of in_view points */
  int32_t n_searched;            /* size of the search set: in_view and not beyond th_far_points */
  int32_t nmatches;              /* return value of SearchByProjection */
} gfs_local_points_result;

/* Allocates the workspace of gfs_search_local_points for lists of up to max_local_points map points per frame (handles that
 * never call it are unchanged). */
int gfs_sbp_reserve_local(gfs_sbp* h, int max_local_points);
/* B independent frames (host pointers).  GFS_ERR_CAPACITY: a list longer than the reserve, or a search set larger than the handle's
 * max_last (nothing is truncated: the per-point outputs and counts are delivered, the search is skipped, nmatches = 0 and cur_match
 * all -1 for that frame).  GFS_ERR_INVALID_ARG: n_levels outside 1..16 or a NULL array.  The handle stays usable. */
int gfs_search_local_points(gfs_sbp* h, const gfs_local_points_problem* problems, int B, gfs_local_points_result* results);

/*      int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th, const bool bRight = false)
 *                                                                               src/ORBmatcher.cc:1378-1548
 *    the search of every listed map point in a key frame (:1424-1526), as LocalMapping::SearchInNeighbors
 *    (src/LocalMapping.cc:1129-1234) needs it: a point list is given once and searched in any number of key frames.  What the loop
 *    reads of its pointer state (isBad(), IsInKeyFrame, GetMapPoint, Observations()) and what it does with a match (:1529-1544) stay
 *    with the caller, in list order (gfs_host::Fuse, geoflowslam_amd/host/gfs_adaptors.hpp).  Single-camera pinhole key frames
 *    (NLeft == -1, bRight == false).  float, every operation rounded once, sums left to right: DESIGN.md section 13 states the rule. */
#define GFS_FUSE_NEG_DEPTH 0     /* p3Dc(2) < 0.0f (:1428) */
#define GFS_FUSE_NOT_IN_IMAGE 1  /* !pKF->IsInImage(u, v) (:1438; half-open bounds, NaN and inf fail it) */
#define GFS_FUSE_TOO_NEAR 2      /* dist3D < 0.8f * mfMinDistance (:1451) */
#define GFS_FUSE_TOO_FAR 3       /* dist3D > 1.2f * mfMaxDistance */
#define GFS_FUSE_VIEW_ANGLE 4    /* PO.dot(Pn) < 0.5 * dist3D (:1459) */
#define GFS_FUSE_EMPTY_WINDOW 5  /* GetFeaturesInArea returned nothing (:1472) */
#define GFS_FUSE_NO_CANDIDATE 6  /* bestDist > TH_LOW (:1529, :1543) */
#define GFS_FUSE_MATCHED 7       /* bestDist <= TH_LOW: the caller does :1530-1542 with best_idx */
typedef struct {
  int32_t n_mp;
  const float* mp_xw;            /* [n_mp][3] GetWorldPos() */
  const float* mp_normal;        /* [n_mp][3] GetNormal() */
  const float* mp_min_dist;      /* [n_mp] mfMinDistance (raw: the 0.8f of GetMinDistanceInvariance is applied inside) */
  const float* mp_max_dist;      /* [n_mp] mfMaxDistance (raw: 1.2f likewise) */
  const uint8_t* mp_desc;        /* [n_mp][32] GetDescriptor() */
} gfs_fuse_points;

typedef struct {
  float Tcw_q[4], Tcw_t[3];      /* pKF->GetPose(): Sophus::SE3f unit quaternion (x, y, z, w), translation */
  float Ow[3];                   /* pKF->GetCameraCenter() */
  float fx, fy, cx, cy, bf;      /* pKF->fx .. cy (Pinhole), mbf */
  float min_x, max_x, min_y, max_y; /* mnMinX ... mnMaxY */
  float grid_w_inv, grid_h_inv;  /* mfGridElementWidthInv / HeightInv (64 x 48 grid) */
  const float* scale_factors;    /* mvScaleFactors */
  const float* inv_level_sigma2; /* mvInvLevelSigma2 */
  int32_t n_levels;              /* mnScaleLevels, 1..16 */
  float log_scale_factor;        /* mfLogScaleFactor */
  float th;                      /* window factor (3.0 by default) */
  int32_t n_kp;                  /* N, <= the handle's max_cur */
  const gfs_keypoint* kps_un;    /* [n_kp] mvKeysUn (octave in [0, n_levels)) */
  const float* u_right;          /* [n_kp] mvuRight */
  const uint8_t* desc;           /* [n_kp][32] mDescriptors */
  int32_t list;                  /* which of the call's point lists is searched in this key frame */
} gfs_fuse_keyframe;

typedef struct {                 /* caller-owned arrays, [n_mp of the key frame's list] */
  uint8_t* exit;                 /* GFS_FUSE_* */
  int32_t* best_idx;             /* bestIdx; -1 where no candidate survived the level and chi2 filters (or the point left earlier) */
  int32_t* best_dist;            /* bestDist; 256 likewise */
  int32_t* level;                /* nPredictedLevel; defined where exit >= GFS_FUSE_EMPTY_WINDOW */
  int32_t n_matched;             /* the number of points with exit == GFS_FUSE_MATCHED */
} gfs_fuse_result;

/* Allocates the workspace of gfs_fuse_search: up to max_lists lists of up to max_points_per_list map points, searched in up to
 * max_keyframes key frames per call (handles that never call it are unchanged). */
int gfs_sbp_reserve_fuse(gfs_sbp* h, int max_lists, int max_points_per_list, int max_keyframes);
/* B (list, key frame) searches in one launch (host pointers); the lists are uploaded once.  GFS_ERR_CAPACITY: more lists, a longer
 * list, more key frames or more key-points than reserved.  GFS_ERR_INVALID_ARG: n_levels outside 1..16, a `list` index outside
 * [0, n_lists), a key-point octave outside [0, n_levels) or a NULL array.  Nothing is truncated; the handle stays usable. */
int gfs_fuse_search(gfs_sbp* h, const gfs_fuse_points* lists, int n_lists, const gfs_fuse_keyframe* kfs, int B, gfs_fuse_result* results);

/*      int ORBmatcher::Fuse(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints, float th,
 *                           vector<MapPoint*>& vpReplacePoint)                   src/ORBmatcher.cc:1550-1654
 *      int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
 *                           vector<MapPoint*>& vpMatched, int th, float ratioHamming)                  :432-529
 *      int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
 *                           const vector<KeyFrame*>& vpPointsKFs, vector<MapPoint*>& vpMatched,
 *                           vector<KeyFrame*>& vpMatchedKF, int th, float ratioHamming)                :531-636
 *    the three Sim3 searches of loop closing (src/LoopClosing.cc:811, :841, :1016, :2224-2302) under one rule, any number of
 *    (list, problem) pairs in one launch: projection with Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) and
 *    Ow = Tcw.inverse().translation(), which the CALLER forms (gfs_host::FuseSim3 / SearchAndFuse / SearchByProjectionSim3,
 *    geoflowslam_amd/host/gfs_adaptors.hpp); the gates of gfs_fuse_search without the chi2 gates and mvuRight; the window; the
 *    level filter; the Hamming minimum.  In the projection modes a match takes its key-point away from every later point of the
 *    list (vpMatched[bestIdx] = pMP): the results are those of the sequential loop.  Single-camera pinhole key frames.  float,
 *    every operation rounded once, sums left to right: DESIGN.md section 20 states the rule. */
#define GFS_SIM3_FUSE 0          /* Fuse: Pinhole::project; bestDist starts at INT_MAX; matched when bestDist <= TH_LOW */
#define GFS_SIM3_SBP 1           /* :432: Pinhole::project; key-points with kp_taken or taken by an earlier point are skipped;
                                    bestDist starts at 256; matched when bestDist <= TH_LOW * ratio_hamming */
#define GFS_SIM3_SBP_KFS 2       /* :531: as GFS_SIM3_SBP with u = fx * (Pc0 * (1 / Pc2)) + cx (:571-576) */
#define GFS_FUSE_SKIPPED 8       /* the point's mp_skip byte is set: pMP->isBad() || spAlreadyFound.count(pMP) at entry */
#define GFS_SIM3_SEARCH_LISTED 4 /* candidates the device lists per point in the projection modes; a point whose listed candidates
                                    are all taken by earlier points while more exist is searched again on the host */
typedef struct {
  int32_t mode;                  /* GFS_SIM3_* */
  float ratio_hamming;           /* ratioHamming (projection modes; not read in GFS_SIM3_FUSE) */
  float Tcw_q[4], Tcw_t[3];      /* Tcw: unit quaternion (x, y, z, w), translation */
  float Ow[3];                   /* Tcw.inverse().translation() */
  float fx, fy, cx, cy;          /* pKF->fx .. cy (Pinhole) */
  float min_x, max_x, min_y, max_y; /* mnMinX ... mnMaxY */
  float grid_w_inv, grid_h_inv;  /* mfGridElementWidthInv / HeightInv (64 x 48 grid) */
  const float* scale_factors;    /* mvScaleFactors */
  int32_t n_levels;              /* mnScaleLevels, 1..16 */
  float log_scale_factor;        /* mfLogScaleFactor */
  float th;                      /* window factor; the int th of the projection searches as the float it converts to */
  int32_t n_kp;                  /* N, <= the handle's max_cur */
  const gfs_keypoint* kps_un;    /* [n_kp] mvKeysUn (octave in [0, n_levels)) */
  const uint8_t* desc;           /* [n_kp][32] mDescriptors */
  const uint8_t* kp_taken;       /* [n_kp] vpMatched[idx] != NULL at entry, or NULL = none; must be NULL in GFS_SIM3_FUSE */
  const uint8_t* mp_skip;        /* [n_mp of the list] the point leaves at entry with GFS_FUSE_SKIPPED, or NULL = none */
  int32_t list;                  /* which of the call's point lists is searched in this problem */
} gfs_sim3_search_problem;

typedef struct {                 /* caller-owned arrays, [n_mp of the problem's list] */
  uint8_t* exit;                 /* GFS_FUSE_* 0..7, or GFS_FUSE_SKIPPED */
  int32_t* best_idx;             /* bestIdx when the point's candidate loop ended, after the dependency between points (projection
                                    modes); -1 where nothing survived or the point left earlier */
  int32_t* best_dist;            /* bestDist likewise; 256, or INT_MAX in GFS_SIM3_FUSE, where nothing survived or the point left earlier */
  int32_t* level;                /* nPredictedLevel; defined where exit is GFS_FUSE_EMPTY_WINDOW .. GFS_FUSE_MATCHED */
  int32_t n_matched;             /* the number of points with exit == GFS_FUSE_MATCHED */
} gfs_sim3_search_result;

/* Allocates the workspace of gfs_sim3_search: up to max_lists lists of up to max_points_per_list map points, searched in up to
 * max_problems problems per call (handles that never call it are unchanged). */
int gfs_sbp_reserve_sim3_search(gfs_sbp* h, int max_lists, int max_points_per_list, int max_problems);
/* B (list, problem) searches in one launch (host pointers); the lists are uploaded once.  Refused before anything is staged, the
 * handle left usable -- GFS_ERR_CAPACITY: more lists, a longer list, more problems or more key-points (the handle's max_cur) than
 * reserved.  GFS_ERR_INVALID_ARG: an unknown mode, n_levels outside 1..16, a key-point octave outside [0, n_levels), a `list` index
 * outside [0, n_lists), a NULL required array, kp_taken given in GFS_SIM3_FUSE, or in a projection mode a ratio_hamming that is
 * negative, NaN or has 50.0f * ratio_hamming >= 256.0f (the reference would then write vpMatched[-1]). */
int gfs_sim3_search(gfs_sbp* h, const gfs_fuse_points* lists, int n_lists, const gfs_sim3_search_problem* problems, int B,
                    gfs_sim3_search_result* results);

/*      void LocalMapping::CreateNewMapPoints()                                   src/LocalMapping.cc:803-1127
 *    for every neighbour key frame in order: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:1158-1376: Hamming search over the
 *    key-point pairs that share a vocabulary node, epipole and epipolar-line gates, optional rotation histogram) and the triangulation
 *    of every match with its gates (:904-1100).  A point created at neighbour i takes its idx1 out of the searches at the neighbours
 *    after i; that dependency is carried on the device.  What the loop does with a created point (:1103-1124) stays with the caller,
 *    neighbour by neighbour in ascending idx1 (gfs_host::CreateNewMapPoints, geoflowslam_amd/host/gfs_adaptors.hpp).  Single-camera
 *    pinhole key frames (NLeft == -1, mpCamera2 == nullptr).  DESIGN.md section 14 states the rule, with two written rules where the
 *    reference's arithmetic is a library's (the 4 x 4 null vector, the stereo parallax cosine). */
#define GFS_TRI_NO_MATCH 0          /* idx1 is in no pair of vMatchedIndices */
#define GFS_TRI_LOW_PARALLAX 1      /* "No stereo and very low parallax" (:1020) */
#define GFS_TRI_SVD_W_ZERO 2        /* GeometricTools::Triangulate returned false (:1010) */
#define GFS_TRI_UNPROJECT_FAILED 3  /* UnprojectStereo returned false (:1025) */
#define GFS_TRI_BEHIND_1 4          /* z1 <= 0 (:1029) */
#define GFS_TRI_BEHIND_2 5          /* z2 <= 0 (:1032) */
#define GFS_TRI_REPROJ_1 6          /* reprojection chi2 in the current key frame (:1045, :1054) */
#define GFS_TRI_REPROJ_2 7          /* ... in the neighbour (:1068, :1076) */
#define GFS_TRI_ZERO_DIST 8         /* dist1 == 0 || dist2 == 0 (:1088) */
#define GFS_TRI_FAR 9               /* mbFarPoints and a distance >= mThFarPoints (:1090) */
#define GFS_TRI_SCALE 10            /* scale consistency (:1098) */
#define GFS_TRI_CREATED 11          /* the caller does :1103-1124 with x3d */
typedef struct {
  float Tcw[12];                 /* GetPose().matrix3x4(), row-major */
  float Ow[3];                   /* GetCameraCenter() */
  float Rwc[9], twc[3];          /* mRwc (row-major) and mTwc.translation(), read by UnprojectStereo */
  float fx, fy, cx, cy, invfx, invfy, mbf, mb;
  const float* scale_factors;    /* mvScaleFactors */
  const float* level_sigma2;     /* mvLevelSigma2 */
  int32_t n_levels;              /* 1..16 */
  int32_t n_kp;                  /* N, <= the handle's max_cur */
  const gfs_keypoint* kps_un;    /* [n_kp] mvKeysUn: position, octave in [0, n_levels), angle */
  const gfs_keypoint* kps;       /* [n_kp] mvKeys (UnprojectStereo reads its position) */
  const float* u_right;          /* [n_kp] mvuRight */
  const float* depth;            /* [n_kp] mvDepth */
  const uint8_t* desc;           /* [n_kp][32] mDescriptors */
  const uint8_t* has_mp;         /* [n_kp] GetMapPoint(i) != nullptr at entry */
  int32_t n_nodes;               /* mFeatVec, flattened: */
  const int32_t* node_id;        /* [n_nodes] strictly ascending */
  const int32_t* node_start;     /* [n_nodes + 1] non-decreasing from 0 */
  const int32_t* feat_idx;       /* [node_start[n_nodes]] key-point indices in [0, n_kp), none twice */
} gfs_tri_keyframe;

typedef struct {
  gfs_tri_keyframe kf;           /* pKF2 */
  float ep[2];                   /* pKF2->mpCamera->project(T2w * Cw) (src/ORBmatcher.cc:1169-1171) */
  float F12[9];                  /* K1.transpose().inverse() * t12x * R12 * K2.inverse(), row-major (Pinhole.cpp:112) */
} gfs_tri_neighbour;

typedef struct {
  gfs_tri_keyframe cur;          /* mpCurrentKeyFrame */
  const gfs_tri_neighbour* neighbours; /* [n_neighbours] in the loop's order; short baselines (:860) already left out */
  int32_t n_neighbours;
  int32_t only_stereo, coarse, check_orientation; /* bOnlyStereo, bCoarse, the ORBmatcher's checkOri */
  int32_t inertial, far_points;  /* mbInertial, mbFarPoints */
  float th_far_points;           /* mThFarPoints */
  float ratio_factor;            /* 1.5f * mpCurrentKeyFrame->mfScaleFactor */
} gfs_tri_problem;

typedef struct {                 /* one per neighbour; caller-owned arrays of the current key frame's n_kp */
  int32_t* match12;              /* idx2 or -1, after the orientation check */
  uint8_t* exit;                 /* GFS_TRI_* */
  float* x3d;                    /* [n_kp][3] the point where exit >= GFS_TRI_BEHIND_1, zeros before */
  uint8_t* point_stereo;         /* bPointStereo */
  int32_t n_matches, n_created;
} gfs_tri_result;

/* Allocates the workspace of gfs_create_new_map_points: up to max_neighbours neighbours per problem and up to max_candidate_pairs
 * for the sum of n1 * n2 over the common nodes of all neighbours of one problem; max_batch problems of max_cur key-points per key
 * frame as the handle was created (handles that never call it are unchanged). */
int gfs_sbp_reserve_triangulation(gfs_sbp* h, int max_neighbours, int64_t max_candidate_pairs);
/* B independent current key frames in one call (host pointers); results[b] points to problems[b].n_neighbours results.
 * GFS_ERR_CAPACITY: above any reserve, or a handle that never reserved.  GFS_ERR_INVALID_ARG: a NULL array, n_levels outside 1..16,
 * an octave outside [0, n_levels), a feature index outside [0, n_kp) or listed twice, node ids not ascending.  Nothing is
 * truncated; the handle stays usable.  Two kernels (k_tri_candidates, k_tri_resolve), one synchronisation. */
int gfs_create_new_map_points(gfs_sbp* h, const gfs_tri_problem* problems, int B, gfs_tri_result* const* results);

/* ============================================================================================
 * 7a'. Loop detection's BoW-guided matching —
 *      int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)   src/ORBmatcher.cc:936-1053
 *    as LoopClosing::DetectCommonRegionsFromBoW calls it for every covisible of every candidate (src/LoopClosing.cc:706-715), for
 *    single-camera key frames (NLeft == -1).  One problem is one key frame 1 and any number of key frames 2; every (key frame 1,
 *    key frame 2) pair is independent.  Integer throughout but the ratio test; DESIGN.md section 22 states the rule. */
typedef struct {
  int32_t n_kp;                  /* N, <= the handle's max_cur */
  const float* angle;            /* [n_kp] mvKeysUn[i].angle */
  const uint8_t* desc;           /* [n_kp][32] mDescriptors */
  const uint8_t* has_mp;         /* [n_kp] GetMapPointMatches()[i] != nullptr && !isBad() */
  int32_t n_nodes;               /* mFeatVec, flattened as in gfs_tri_keyframe: */
  const int32_t* node_id;        /* [n_nodes] strictly ascending */
  const int32_t* node_start;     /* [n_nodes + 1] non-decreasing from 0 */
  const int32_t* feat_idx;       /* [node_start[n_nodes]] key-point indices in [0, n_kp), none twice */
} gfs_bow_keyframe;

typedef struct {
  gfs_bow_keyframe kf1;          /* pKF1 (mpCurrentKF), uploaded once */
  const gfs_bow_keyframe* kf2;   /* [n_kf2] pKF2 (vpCovKFi[j]) */
  int32_t n_kf2;
  float nn_ratio;                /* mfNNratio */
  int32_t check_orientation;     /* mbCheckOrientation */
} gfs_bow_problem;

typedef struct {                 /* one per key frame 2 */
  int32_t* match12;              /* [kf1.n_kp] caller-owned: idx2 or -1, after the orientation check */
  int32_t n_matches;             /* SearchByBoW's return value */
} gfs_bow_result;

/* Allocates the workspace of gfs_search_by_bow: up to max_problems key frames 1 and up to max_kf2_per_call key frames 2 (summed
 * over the problems) per call, each of up to the handle's max_cur key-points (handles that never call it are unchanged). */
int gfs_sbp_reserve_bow(gfs_sbp* h, int max_problems, int max_kf2_per_call);
/* B independent problems in one call (host pointers); results[b] points to problems[b].n_kf2 results.  GFS_ERR_CAPACITY: more
 * problems or more key frames 2 than reserved, or a handle that never reserved.  GFS_ERR_INVALID_ARG: a NULL array, node ids not
 * ascending, node_start not a prefix sum, a feature index outside [0, n_kp) or listed twice, n_kp or n_nodes above the handle's
 * max_cur.  Every refusal comes before anything is staged or written; nothing is truncated; the handle stays usable.  B == 0,
 * n_kf2 == 0 and n_nodes == 0 are valid.  One upload, one kernel (k_bow_search), one download, one synchronisation. */
int gfs_search_by_bow(gfs_sbp* h, const gfs_bow_problem* problems, int B, gfs_bow_result* const* results);

/* ============================================================================================
 * 7b. Map-point update — the numeric cores of
 *      void MapPoint::ComputeDistinctiveDescriptors()                            src/MapPoint.cc:376-448
 *      void MapPoint::UpdateNormalAndDepth()                                     src/MapPoint.cc:468-532
 *    for any number of map points in one call: the loops that end LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1219-1230),
 *    Optimizer::LocalBundleAdjustment's write-back and LocalMapping::ProcessNewKeyFrame (:439-454).  A point carries its observations
 *    in the iteration order of mObservations; the caller gathers them and writes the results back (gfs_host::UpdateMapPoints,
 *    geoflowslam_amd/host/gfs_adaptors.hpp).  Single-camera key frames (every observation is a left index).  Integer results equal the
 *    reference; float, every operation rounded once, sums left to right in list order: DESIGN.md section 15 states the rule.
 *    Where an operation yields a NaN (Pos == Ow gives 0 / 0, a list without an IN_NORMAL observation gives 0 / 0) the result is a NaN;
 *    its sign and payload are not part of the contract (IEEE 754 leaves them open, and the host's 0 / 0 is not the device's).
 * ============================================================================================ */
#define GFS_MAP_POINTS_FULL 0          /* descriptors and normals */
#define GFS_MAP_POINTS_NORMALS_ONLY 1  /* UpdateNormalAndDepth alone: obs_desc is not read (may be NULL), best_obs = best_median = -1 */
#define GFS_MAP_POINT_OBS_IN_NORMAL 1  /* obs_flags bit: leftIndex != -1 (:494) */
#define GFS_MAP_POINT_OBS_IN_DESC 2    /* obs_flags bit: key frame not null, not bad, leftIndex != -1 and < mDescriptors.rows (:396-403) */
#define GFS_MAP_POINT_NORMAL_SET 1     /* status bit: the list is not empty; normal, min_dist and max_dist are to be written */
#define GFS_MAP_POINT_DESC_SET 2       /* status bit: best_obs >= 0; the descriptor of that observation is to be written */
typedef struct {                 /* host pointers, caller-owned */
  int32_t n_points;
  int32_t mode;                  /* GFS_MAP_POINTS_FULL or GFS_MAP_POINTS_NORMALS_ONLY */
  const int32_t* obs_start;      /* [n_points + 1] non-decreasing from 0: point p owns the observations obs_start[p] .. obs_start[p+1]-1 */
  const float* obs_Ow;           /* [n_obs][3] the observing key frame's GetCameraCenter() (anything where IN_NORMAL is clear) */
  const uint8_t* obs_desc;       /* [n_obs][32] mDescriptors.row(leftIndex) (anything where IN_DESC is clear) */
  const uint8_t* obs_flags;      /* [n_obs] GFS_MAP_POINT_OBS_* */
  const float* pos;              /* [n_points][3] mWorldPos */
  const float* ref_Ow;           /* [n_points][3] mpRefKF->GetCameraCenter() */
  const float* level_scale;      /* [n_points] mpRefKF->mvScaleFactors[level of the point's observation in mpRefKF] */
  const float* max_scale;        /* [n_points] mpRefKF->mvScaleFactors[mnScaleLevels - 1] */
} gfs_map_points_problem;

typedef struct {                 /* caller-owned arrays, [n_points] */
  int32_t* best_obs;             /* BestIdx as an index into the point's own observation list; -1: no IN_DESC observation (or normals only) */
  int32_t* best_median;          /* BestMedian of that row; -1 likewise */
  float* normal;                 /* [n_points][3] mNormalVector; zeros where NORMAL_SET is clear */
  float* min_dist;               /* mfMinDistance; 0 likewise */
  float* max_dist;               /* mfMaxDistance; 0 likewise */
  uint8_t* status;               /* GFS_MAP_POINT_*_SET */
} gfs_map_points_result;

typedef struct gfs_map_points gfs_map_points;
/* Reserves room for max_points points and max_observations observations (over all points) per call. */
int gfs_map_points_create(int device, int max_points, int max_observations, gfs_map_points** out);
void gfs_map_points_destroy(gfs_map_points* h);
/* One upload, one launch, one download, one synchronisation.  GFS_ERR_CAPACITY: more points or more observations than reserved.
 * GFS_ERR_INVALID_ARG: a NULL array (obs_desc may be NULL in normals-only mode; the observation arrays when there is no observation),
 * obs_start[0] != 0, obs_start decreasing, an unknown mode.  Nothing is truncated; the handle stays usable.  n_points == 0 is no work. */
int gfs_map_points_update(gfs_map_points* h, const gfs_map_points_problem* problem, gfs_map_points_result* result);

/* ============================================================================================
 * 8. GMS filter of the brute-force matches (the second half of ORBmatcher::SearchWithGMS / SearchForInitializationWithGMS)
 *      gms_matcher gms(kp1, frameSize, kp2, frameSize, matches_all); nmatches = gms.GetInlierMask(vbInliers, false, false);
 *                                                                     src/ORBmatcher.cc:761-762, 812-813, 893-894
 *      Thirdparty/GMS/include/gms_matcher.h:43-60 (constructor), 289-301 (GetInlierMask), 356-455 (run, no scale / rotation)
 * ============================================================================================ */
typedef struct {
  int32_t n1, n2;
  const gfs_keypoint* kp1;   /* [n1] vkp1 (cv::KeyPoint layout; only pt is used) */
  const gfs_keypoint* kp2;   /* [n2] vkp2 */
  int32_t width1, height1, width2, height2; /* size1, size2 */
  int32_t n_matches;
  const int32_t* query_idx;  /* [n_matches] vDMatches[i].queryIdx */
  const int32_t* train_idx;  /* [n_matches] vDMatches[i].trainIdx */
} gfs_gms_problem;

typedef struct gfs_gms gfs_gms;
int gfs_gms_create(int device, int max_keypoints /* <= 8192 */, int max_batch, gfs_gms** out);
void gfs_gms_destroy(gfs_gms* h);
/* B pairs (host pointers): inlier[f][i] = vbInliers[i] (0 / 1), n_inliers[f] = the return value. */
int gfs_gms_inlier_mask(gfs_gms* h, const gfs_gms_problem* problems, int B, uint8_t* const* inlier, int32_t* n_inliers);
/* Device-resident chain ORB -> BF match -> GMS: dev_kps1 / dev_kps2 [B][kp_stride] gfs_keypoint and dev_n1 / dev_n2 [B] as
 * returned by gfs_orb_device_results, dev_train_idx [B][kp_stride] as written by gfs_bf_match_hamming_batch_device (match i
 * of pair b = (i, dev_train_idx[b][i]), i < n1[b]; no matches when n2[b] == 0).  dev_mask [B][kp_stride] u8, dev_counts [B]. */
int gfs_gms_inlier_mask_batch_device(gfs_gms* h, const void* dev_kps1, const void* dev_n1, const void* dev_kps2, const void* dev_n2,
                                     int B, int kp_stride, const void* dev_train_idx, int width, int height, void* dev_mask,
                                     void* dev_counts, void* stream);

/* ============================================================================================
 * 9. Optical-flow front end (the "GeoFlow" stream): replaces
 *      cv::buildOpticalFlowPyramid(image, mImGray, Size(w, w), 3)             src/Frame.cc:373, 505, 1415
 *      cv::calcOpticalFlowPyrLK(prevPyr, nextPyr, ...)                         src/ORBmatcher.cc:2224, 2271; src/Tracking.cc:3298, 3342
 *      ORBmatcher::fbKltTracking / Tracking::fbKltTracking                     src/ORBmatcher.cc:2186-2297; src/Tracking.cc:3262-3366
 *    (the projection of the priors, the mask bookkeeping and cv::findFundamentalMat of SearchByProjectionWithOF,
 *    src/ORBmatcher.cc:2304-2497, stay with the caller).  A gfs_klt_pyramid holds the pyramids of up to max_batch frames in HBM:
 *    level l of a frame is an image of (lw[l] + 2*win) x (lh[l] + 2*win) bytes at byte offset off[l] (BORDER_REFLECT_101 border
 *    of win pixels) plus as many short2 (Scharr dx, dy; zero border); a level is built while both sides exceed the window, as
 *    OpenCV does.  A frame's pyramid is built once and used as `cur` for one pair and as `prev` for the next.
 *    Sums of the 2x2 system are exact integer sums rounded once: bit-equal to oracle/klt_oracle.cpp.
 * ============================================================================================ */
#define GFS_KLT_MAX_LEVELS 8
#define GFS_KLT_USE_INITIAL_FLOW 4   /* cv::OPTFLOW_USE_INITIAL_FLOW */
#define GFS_KLT_GET_MIN_EIGENVALS 8  /* cv::OPTFLOW_LK_GET_MIN_EIGENVALS */
typedef struct gfs_klt gfs_klt;
typedef struct gfs_klt_pyramid gfs_klt_pyramid;
/* win = LKWindowSize (3 .. 63), max_level = the maxLevel given to buildOpticalFlowPyramid (the reference: 3). */
int gfs_klt_create(int device, int width, int height, int win, int max_level, int max_batch, int max_points, gfs_klt** out);
void gfs_klt_destroy(gfs_klt* h);
/* Number of levels held; lw / lh [levels] and off [levels + 1] may be NULL.  off[levels] = bytes of one frame's images. */
int gfs_klt_layout(const gfs_klt* h, int32_t* lw, int32_t* lh, int64_t* off);
int gfs_klt_pyramid_create(gfs_klt* h, gfs_klt_pyramid** out);
void gfs_klt_pyramid_destroy(gfs_klt_pyramid* p);
/* cv::buildOpticalFlowPyramid for B frames: images[f] = host pointer to height rows of `stride` bytes. */
int gfs_klt_build_pyramid(gfs_klt* h, gfs_klt_pyramid* pyr, const uint8_t* const* images, int stride, int B);
/* Same from device memory: dev_images = [B][height][stride] bytes; asynchronous on `stream` when it is not NULL. */
int gfs_klt_build_pyramid_device(gfs_klt* h, gfs_klt_pyramid* pyr, const void* dev_images, int stride, int B, void* stream);
/* Copies frame f's pyramid to the host: img [off[levels]] bytes, deriv [off[levels] * 2] int16 (parity tests). */
int gfs_klt_pyramid_download(gfs_klt* h, const gfs_klt_pyramid* pyr, int f, uint8_t* img, int16_t* deriv);
/* cv::calcOpticalFlowPyrLK(prev, next, prev_pts, next_pts, status, err, Size(win, win), max_level,
 * TermCriteria(COUNT + EPS, max_iter, eps), flags, min_eig_thr) for B pairs; n_points[f] <= max_points;
 * prev_pts[f] / next_pts[f]: n x 2 floats (next_pts is read when GFS_KLT_USE_INITIAL_FLOW is set). */
int gfs_klt_track(gfs_klt* h, const gfs_klt_pyramid* prev, const gfs_klt_pyramid* next, int B, const int32_t* n_points,
                  const float* const* prev_pts, float* const* next_pts, uint8_t* const* status, float* const* err, int max_level,
                  int max_iter, double eps, int flags, double min_eig_thr);
/* fbKltTracking(prev, cur, win, nbpyrlvl, ferr, fmax_fbklt_dist, kps, priors, kpstatus) for B pairs, both passes and the gates
 * in one kernel: priors[f] in/out (vpriorkps), kpstatus[f][i] 0 / 1, n_good[f] = points that survive both passes. */
int gfs_klt_fb_track(gfs_klt* h, const gfs_klt_pyramid* prev, const gfs_klt_pyramid* cur, int B, const int32_t* n_points,
                     const float* const* kps, float* const* priors, uint8_t* const* kpstatus, int32_t* n_good, int nbpyrlvl,
                     float ferr, float fmax_fbklt_dist);
/* Device-resident form: dev_kps / dev_priors [B][pt_stride][2] float, dev_n [B] int32, dev_kpstatus [B][pt_stride] u8,
 * dev_n_good [B] int32; asynchronous on `stream` when it is not NULL. */
int gfs_klt_fb_track_device(gfs_klt* h, const gfs_klt_pyramid* prev, const gfs_klt_pyramid* cur, int B, int pt_stride,
                            const void* dev_n, const void* dev_kps, void* dev_priors, void* dev_kpstatus, void* dev_n_good,
                            int nbpyrlvl, float ferr, float fmax_fbklt_dist, void* stream);

/* The bookkeeping around the F check of SearchByProjectionWithOF on the device (src/ORBmatcher.cc:2386-2406): the tracks that survived
 * fbKltTracking, in order, as the two point lists of the check plus their original indices (dev_out_a / dev_out_b
 * [B][pt_stride][2] float, dev_out_index [B][pt_stride] int32, dev_out_n [B] int32) ... */
int gfs_klt_compact_tracks_device(gfs_klt* h, int B, int pt_stride, const void* dev_n, const void* dev_kps, const void* dev_priors,
                                  const void* dev_kpstatus, void* dev_out_a, void* dev_out_b, void* dev_out_index, void* dev_out_n,
                                  void* stream);
/* ... and, after gfs_find_fundamental_ransac_device, kpstatus[index[j]] = 0 for every track j whose mask is 0. */
int gfs_klt_apply_mask_device(gfs_klt* h, int B, int pt_stride, const void* dev_m, const void* dev_index, const void* dev_mask,
                              void* dev_kpstatus, void* stream);

/* ============================================================================================
 * 10. cv::findFundamentalMat(points1, points2, cv::FM_RANSAC, threshold, confidence, mask) — the F check of the optical-flow
 *     matcher (src/ORBmatcher.cc:236, 2399-2405, 2463-2469) and of Tracking::EstimatePoseByOF (src/Tracking.cc:1973-1974):
 *     OpenCV's 7-point RANSAC (cv::RNG((uint64)-1), getSubset / checkSubset, symmetric epipolar distance against threshold^2,
 *     adaptive iteration budget, maxIters 1000) for n >= 15 points; for 8 .. 14 points the LMedS registrator the cv:: wrapper
 *     switches to (least median of the errors, inliers within 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median); `threshold` unused).
 *     Fewer than 8 points: GFS_ERR_UNSUPPORTED (the reference only calls it with more than 8).  The null space of the 7-point system and the roots
 *     of its cubic are computed with +, -, *, /, sqrt only (oracle/fmat_oracle.cpp): same inlier sets as the oracle
 *     bit for bit; against OpenCV the models agree to rounding noise, the order of the up to three models of a subset can differ.
 * ============================================================================================ */
typedef struct gfs_fmat gfs_fmat;
int gfs_fmat_create(int device, int max_points, int max_batch, gfs_fmat** out);
void gfs_fmat_destroy(gfs_fmat* h);
/* B independent problems (host pointers): pts1[b] / pts2[b] = n_points[b] x 2 floats (cv::Point2f), mask[b][i] = status[i] (0 / 1),
 * n_inliers[b] = size of the consensus set (0 = no model), F (may be NULL) = [B][9] row-major 3x3 of the best model.
 * threshold <= 0 -> 3, confidence outside (0, 1) -> 0.99, like the cv:: wrapper. */
int gfs_find_fundamental_ransac(gfs_fmat* h, int B, const int32_t* n_points, const float* const* pts1, const float* const* pts2,
                                double threshold, double confidence, int max_iters, uint8_t* const* mask, double* F,
                                int32_t* n_inliers);
/* Device-resident form: dev_pts1 / dev_pts2 [B][stride][2] float, dev_n [B] int32, dev_mask [B][stride] u8 (device); F and n_inliers
 * on the host.  Problems with 8 or fewer points are passed through (mask all ones, n_inliers = n): SearchByProjectionWithOF only runs
 * the check for more than 8 (src/ORBmatcher.cc:2397, 2461).  Synchronous (the acceptance rule is replayed on the host). */
int gfs_find_fundamental_ransac_device(gfs_fmat* h, int B, int stride, const void* dev_n, const void* dev_pts1, const void* dev_pts2,
                                       double threshold, double confidence, int max_iters, void* dev_mask, double* F,
                                       int32_t* n_inliers);

/* ============================================================================================
 * 11. Optimizer::PoseLidarVisualOptimization — motion-only BA of a frame with point-to-plane lidar edges
 *      int Optimizer::PoseLidarVisualOptimization(Frame*, PointCloud::Ptr laserCloudSurfFromMapDS, bool, bool,
 *                                                 int nIterations, int& nLidarInliers, float& residual)
 *                                                                             src/Optimizer.cc:7698-8059
 *    Replaces PoseOptimization when UsePointCloudObs: 1.  Visual edges as in section 6; per round, GenerateLidarEdge
 *    (:8339-8421: 5-NN of the frame's downsampled cloud in the local map, ColPivHouseholderQR plane fit, gates) adds
 *    EdgeSE3LidarPoint2Plane edges (include/G2oTypes.h:574-600, numeric Jacobian), optimize(its[it]) with its = {10, 5, 5, 5},
 *    the lidar edges are removed and the visual edges re-classified.  Conventional-SLAM branch only (two_camera != 0 is refused
 *    with GFS_ERR_UNSUPPORTED).  DESIGN.md "Pose with lidar edges" pins the two rules the reference leaves to Eigen / FLANN.
 * ============================================================================================ */
/* The local map (laserCloudSurfFromMapDS), uploaded once and reused by every frame until the next upload (the reference refreshes it
 * at key-frame rate).  gfs_lidar_map_set builds the search grid; n < 5 is refused (the reference reads sqdis[4]). */
typedef struct gfs_lidar_map gfs_lidar_map;
int gfs_lidar_map_create(int device, int max_points, gfs_lidar_map** out);
int gfs_lidar_map_set(gfs_lidar_map* map, const float* xyz /* [n][3] */, int n);
void gfs_lidar_map_destroy(gfs_lidar_map* map);

/* The local map built on the device -- LidarMapping::viewer's loop body (src/LidarMapping.cc:162-182): the key-frames that reach
 * transformPointCloud (:107-127), each cloud moved by toMatrix4d(Tcw.inverse()), concatenated, pcl::VoxelGrid at
 * LidarMapping.LocalResolution, and the search grid gfs_lidar_map_set would build -- straight into a gfs_lidar_map that
 * gfs_pose_lidar_optimize and gfs_lba_solve_lidar use unchanged.  DESIGN.md section 11 states the filter's rule (index, order,
 * float centroid).  In every refusal nothing is truncated and the map keeps its previous content:
 *   points beyond the mapper's capacity, map points beyond map->max_points or cap      GFS_ERR_CAPACITY
 *   map on another device; a transformed point not finite or not within 1e6 m; fewer than 5 map points (a build over zero points
 *   included); leaf not positive and finite                                            GFS_ERR_INVALID_ARG
 *   the filter's index range beyond int (where PCL's int arithmetic would overflow)    GFS_ERR_UNSUPPORTED */
typedef struct gfs_lidar_mapper gfs_lidar_mapper;
int gfs_lidar_mapper_create(int device, int max_points_in, int max_keyframes, gfs_lidar_mapper** out);
void gfs_lidar_mapper_destroy(gfs_lidar_mapper* h);

typedef struct {
  int32_t n_keyframes;        /* the key-frames that reach transformPointCloud, in mlNewKeyFrames order */
  const float* q;             /* [n_keyframes][4] Tcw as stored (x, y, z, w) */
  const float* t;             /* [n_keyframes][3] */
  const int32_t* cloud_begin; /* [n_keyframes + 1] */
  const float* cloud;         /* [cloud_begin[n_keyframes]][3] mpPointCloudDownsampled, camera frame */
  float leaf;                 /* (float) LidarMapping.LocalResolution */
} gfs_lidar_map_input;
typedef struct {
  int32_t n_in, n_out, passthrough; /* passthrough: the filter returned its input (PCL's "leaf size is too small") */
  int32_t div[3];                   /* the filter's grid (0 when passed through) */
} gfs_lidar_map_info;

int gfs_lidar_map_build(gfs_lidar_mapper* h, const gfs_lidar_map_input* in, gfs_lidar_map* map, gfs_lidar_map_info* info);
/* The map's points in map-index order (GetLocalMap); *n = the map's size; up to cap points are written. */
int gfs_lidar_map_fetch(const gfs_lidar_map* map, float* xyz /* [cap][3] */, int cap, int32_t* n);
/* pcl::VoxelGrid under the same rule on one host cloud (n >= 1) -> host points (the filters of src/Frame.cc:388-390 and
 * src/LidarProcess.cc are this filter). */
int gfs_voxel_grid_filter(gfs_lidar_mapper* h, const float* xyz /* [n][3] */, int n, float leaf, float* out_xyz /* [cap][3] */, int cap,
                          gfs_lidar_map_info* info);

typedef struct {
  float q[4], t[3];           /* Tcw = pFrame->GetPose(): Sophus::SE3f unit quaternion (x, y, z, w) and translation, as stored */
  int32_t n_obs;              /* the visual observations, exactly as gfs_pose_problem */
  const double* xw;           /* [n_obs][3] */
  const double* obs;          /* [n_obs][3] */
  const float* inv_sigma2;    /* [n_obs] */
  const uint8_t* stereo;      /* [n_obs] */
  double fx, fy, cx, cy, bf;
  int32_t n_cloud;            /* pFrame->mpPointCloudDownsampled->size() (0 = no cloud) */
  const float* cloud;         /* [n_cloud][3] camera frame */
  const gfs_lidar_map* map;   /* laserCloudSurfFromMapDS, on the handle's device */
  int32_t n_iterations;       /* nIterations, 1 .. 4 */
  int32_t two_camera;         /* pFrame->mpCamera2 != nullptr: refused */
} gfs_pose_lidar_problem;

typedef struct {
  uint8_t* outlier;           /* [n_obs] pFrame->mvbOutlier */
  double* chi2;               /* [n_obs] e->chi2() as read by the last classification */
  double q[4], t[3];          /* the g2o estimate after the last round */
  float qf[4], tf[3];         /* the pose given to pFrame->SetPose (the estimate through Sophus::SE3f; the input when < 3 obs) */
  float avg_reproj_error;     /* avgReprojectionError of the last classification (inf / NaN as the reference computes them) */
  int32_t n_inliers;          /* return value: nInitialCorrespondences - nBad */
  int32_t n_lidar_inliers;    /* in/out (int&): valid_edge of the last round that had lidar edges, else unchanged */
  float residual;             /* in/out (float&): chi2Lidar of the last round that had lidar edges, else unchanged */
  int32_t lidar_rounds;       /* rounds that had lidar edges (optimized and re-classified) */
  int32_t rounds_run;         /* rounds entered (a round without lidar edges `continue`s) */
  int32_t iterations_run;     /* LM iterations over all rounds */
  int32_t round_edges[4];     /* lidar edges of each round */
  float round_chi2[4];        /* chi2Lidar of each round (0 for a round without edges) */
  int32_t round_valid[4];     /* valid_edge of each round */
} gfs_pose_lidar_solution;

typedef struct gfs_pose_lidar gfs_pose_lidar;
int gfs_pose_lidar_create(int device, int max_obs, int max_cloud, int max_batch, gfs_pose_lidar** out);
void gfs_pose_lidar_destroy(gfs_pose_lidar* h);
/* GFS_POSE_SUMS_EDGE_ORDER (default): every sum in g2o's edge order, bit for bit the sequential restatement; GFS_POSE_SUMS_TREE:
 * a fixed-shape tree, pose within 1e-6 relative (an LM accept / stop decision can flip where the sums round differently; 3.4e-7
 * measured), flags equal up to chi2-threshold ties. */
int gfs_pose_lidar_set_sum_order(gfs_pose_lidar* h, int order);
/* B frames (host pointers; frames may share a map or use several maps on the handle's device). */
int gfs_pose_lidar_optimize(gfs_pose_lidar* h, const gfs_pose_lidar_problem* problems, int B, gfs_pose_lidar_solution* solutions);
/* Diagnostic: the lidar edges frame b of the last gfs_pose_lidar_optimize call generated in round `round` (cloud index order):
 * point index, plane (pa, pb, pc, pd) and s.  Up to cap edges; *n = the round's edge count. */
int gfs_pose_lidar_fetch_edges(gfs_pose_lidar* h, int b, int round, int32_t* index, float* plane /* [cap][4] */, float* s, int cap,
                               int32_t* n);

/* ============================================================================================
 * 12. cv::CLAHE on 8-bit single-channel images -- the equalisation of Frame::image in front of the optical-flow pyramid
 *      cv::Ptr<cv::CLAHE> clahe = cv::createCLAHE(3.0, cv::Size(8, 8)); clahe->apply(image, image);
 *                                                                              src/Frame.cc:366-369, 499-500 (UseClahe: 1)
 *    ORB keeps running on the un-equalised imGray; Tracking::EstimatePoseByOF (src/Tracking.cc:1961) reads the equalised image.
 *    The rule is DESIGN.md section 16 (a written restatement of OpenCV's imgproc/src/clahe.cpp): per-tile histogram of the image
 *    extended by BORDER_REFLECT_101, clip, redistribution, look-up table, bilinear blend of four tables per pixel in a fixed float
 *    order.  Bit-equal to tests/host/clahe_restatement.cpp.  residual_variant selects how the excess left after the even
 *    redistribution is spread: OpenCV >= 3.4 steps through the bins, OpenCV <= 3.3 fills the first bins.
 *    Refusals truncate nothing and leave the handle usable: a NULL pointer, a stride below the width, tiles outside 1 .. 16, an
 *    unknown variant (GFS_ERR_INVALID_ARG); more frames or a larger image than reserved (GFS_ERR_CAPACITY).
 * ============================================================================================ */
#define GFS_CLAHE_RESIDUAL_STEPPED 0    /* OpenCV >= 3.4: h[k * step] += 1, step = max(256 / residual, 1), k < residual */
#define GFS_CLAHE_RESIDUAL_CONTIGUOUS 1 /* OpenCV <= 3.3: h[i] += 1 for i < residual */
typedef struct {
  double clip_limit;        /* <= 0: no clipping (plain per-tile equalisation) */
  int32_t tiles_x, tiles_y; /* 1 .. 16 */
  int32_t residual_variant; /* GFS_CLAHE_RESIDUAL_* */
} gfs_clahe_config;
typedef struct gfs_clahe gfs_clahe;
void gfs_clahe_default_config(gfs_clahe_config* cfg); /* 3.0, 8 x 8, stepped */
/* Images up to max_width x max_height (<= 8192 per side), up to max_batch per call.  The handle has its own stream and lock. */
int gfs_clahe_create(int device, int max_width, int max_height, int max_batch, const gfs_clahe_config* cfg, gfs_clahe** out);
void gfs_clahe_destroy(gfs_clahe* h);
/* clahe->apply for B host images of any width, height >= 1 within the reserve: images[f] = height rows of `stride` bytes,
 * out[f] = height rows of `out_stride` bytes (may be images[f]). */
int gfs_clahe_apply(gfs_clahe* h, const uint8_t* const* images, int width, int height, int stride, int B, uint8_t* const* out,
                    int out_stride);
/* Same in device memory: dev_in [B][height][in_stride], dev_out [B][height][out_stride]; dev_out == dev_in with equal strides
 * equalises in place.  Asynchronous on `stream` when it is not NULL.  Calls on one handle share its table storage: calls issued on
 * different streams must be ordered by the caller. */
int gfs_clahe_apply_device(gfs_clahe* h, const void* dev_in, int width, int height, int in_stride, int B, void* dev_out, int out_stride,
                           void* stream);
/* The look-up tables of frame f of the last call, lut [tiles_y][tiles_x][256] (parity tests: tells which half is wrong).  Waits for
 * the whole device. */
int gfs_clahe_download_luts(gfs_clahe* h, int f, uint8_t* lut);
/* The Frame constructor's pair in one call on the tracker's stream: one upload, CLAHE, then gfs_klt_build_pyramid's launches
 * unchanged.  equalized_out (NULL, or B host pointers to height rows of eq_stride bytes) receives Frame::image.
 * GFS_ERR_INVALID_ARG: handles on different devices, a CLAHE reserve smaller than the tracker's image. */
int gfs_klt_build_pyramid_clahe(gfs_klt* h, gfs_clahe* clahe, gfs_klt_pyramid* pyr, const uint8_t* const* images, int stride, int B,
                                uint8_t* const* equalized_out, int eq_stride);
/* Same from device memory.  dev_equalized [B][height][eq_stride] receives the equalised images (it may be dev_images when the
 * strides are equal); with NULL they live in scratch owned by the CLAHE handle until its next call. */
int gfs_klt_build_pyramid_clahe_device(gfs_klt* h, gfs_clahe* clahe, gfs_klt_pyramid* pyr, const void* dev_images, int stride, int B,
                                       void* dev_equalized, int eq_stride, void* stream);

/* ============================================================================================
 * 14. The frame cloud -- the lidar-feature tail of the Frame constructor (UseICP / UsePointCloudObs)
 *      mpLidarProcess->featureExtraction(pointcloud_in, pointcloud_edge, pointcloud_surf);     src/LidarProcess.cc:20-204
 *      *mpPointCloud = *pointcloud_surf + *pointcloud_edge;  VoxelGrid at downsizeResolution()  src/Frame.cc:378-393
 *    on the camera-frame cloud of gfs_depth_to_cloud / gfs_frame_rgbd: scan split by atan2(y, z), padded scans, curvature, the
 *    std::sort pick of at most 10 edge points a scan, pcl::VoxelGrid (the rule of section 11) and RadiusOutlierRemoval on both
 *    feature clouds, surf ++ edge, the final VoxelGrid.  DESIGN.md section 17 states the rule, including what the reference
 *    leaves to libm, libstdc++ and PCL; the results are bit-equal to tests/host/frame_cloud_restatement.cpp for every input.
 *    The three comparisons that read atan2 are taken on the device only when they lie farther than angle_guard_deg from their
 *    threshold; otherwise the call redoes the scan table with the host's atan2 (info.host_scan_split = 1) -- same results.
 *    Refusals truncate nothing, leave the outputs untouched and the handle usable:
 *      GFS_ERR_INVALID_ARG  n == 0; a coordinate that is not finite or beyond 1e6 m, or a point whose float squared norm is 0
 *                           (the curvature divides by it); non-positive or non-finite resolutions (at creation)
 *      GFS_ERR_CAPACITY     n > max_points; a scan with more than 1024 candidates; cap / cap_down too small (info is filled)
 *      GFS_ERR_UNSUPPORTED  a voxel index range beyond int, as in section 11
 *    A cloud that yields no scan (a single row) is not an error: every output is empty.
 * ============================================================================================ */
typedef struct gfs_frame_cloud gfs_frame_cloud;
typedef struct {
  double horizontal_angle, max_distance, local_map_resolution; /* LidarParam: 70.0, 9.0, 0.05 */
  float downsize_resolution;                                   /* Frame: mpSettings->downsizeResolution() */
  double angle_guard_deg;                                      /* 1e-9 */
} gfs_frame_cloud_config;
typedef struct {
  int32_t n_in, n_scans, n_edge_raw, n_surf_raw, n_edge_voxel, n_surf_voxel, n_edge, n_surf, n_down;
  int32_t host_scan_split, passthrough[3]; /* edge, surf, final voxel filter returned its input */
} gfs_frame_cloud_info;
void gfs_frame_cloud_default_config(gfs_frame_cloud_config* cfg);
/* Clouds of up to max_points points.  The handle has its own stream and lock; all workspace is allocated here. */
int gfs_frame_cloud_create(int device, int max_points, const gfs_frame_cloud_config* cfg, gfs_frame_cloud** out);
void gfs_frame_cloud_destroy(gfs_frame_cloud* h);
/* xyzw [n][4]: the cloud in push_back order (w is not read).  cloud_xyz [cap][3] (may be NULL: not copied back) receives
 * mpPointCloud, the n_surf surf points then the n_edge edge points; down_xyz [cap_down][3] mpPointCloudDownsampled (n_down). */
int gfs_frame_cloud_extract(gfs_frame_cloud* h, const float* xyzw, int n, float* cloud_xyz, int cap, float* down_xyz, int cap_down,
                            gfs_frame_cloud_info* info);
/* Same on the cloud gfs_frame_rgbd left on the device (its *dev_cloud / *dev_count): nothing is uploaded. */
int gfs_frame_cloud_extract_device(gfs_frame_cloud* h, const void* dev_xyzw, const void* dev_count, float* cloud_xyz, int cap,
                                   float* down_xyz, int cap_down, gfs_frame_cloud_info* info);

/* ============================================================================================
 * 15. Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2042-2413) — the Sim3 pose graph of LoopClosing::CorrectLoop
 *     (src/LoopClosing.cc:1257), between SearchAndFuse (gfs_sim3_search in GFS_SIM3_FUSE mode) and gfs_gba_solve.
 *    The flattened graph: one VertexSim3Expmap per vertex (the estimate Siw = (q, t, s), `fixed` for the map's init key-frame,
 *    _fix_scale = fix_scale for all), one EdgeSim3 per edge with vertex 0 = i, vertex 1 = j, the measurement Sji (ICP edges: Sij, the
 *    vertices swapped) and information w I_7 (1; ICP edges 3), in the order the reference makes them: the sums run in this order.
 *    BlockSolver_7_3 + LinearSolverEigen + Levenberg with setUserLambdaInit(lambda_init = 1e-16), optimize(iterations = 20), no stop
 *    flag, no robust kernel, g2o's numeric Jacobians (central differences, delta 1e-9).  The pose system is factored as a tiled dense
 *    L D L^T over the whole device (the factorisation of gfs_gba_solve).  With fix_scale the scale column of every Jacobian is exactly
 *    zero and a vertex has 6 dimensions in the system; without, 7.  DESIGN.md "Essential graph".
 *    Then every map point goes through correctedSwr.map(Srw.map(P)) of its reference vertex (:2387-2409), in double, cast to float.
 *    The pointer-graph gather, the ICP registrations and the write-back stay in the C++ adaptor.
 *    Refused with GFS_ERR_INVALID_ARG before anything is queued: a vertex index outside the graph, an edge from a vertex to itself, a
 *    point reference >= n_vertices (negative: the point is left as it is), a scale or weight that is not positive and finite.
 *    GFS_ERR_CAPACITY above the handle's limits; gfs_essential_graph_create refuses with it when the tiles of 7 max_vertices rows do
 *    not fit the device.
 * ============================================================================================ */
typedef struct {
  int32_t n_vertices, n_edges, n_points;
  const double* vertex_q;      /* [n_vertices][4] (x, y, z, w) */
  const double* vertex_t;      /* [n_vertices][3] */
  const double* vertex_s;      /* [n_vertices] */
  const uint8_t* vertex_fixed; /* [n_vertices] */
  const int32_t* edge_i;       /* [n_edges] vertex 0 */
  const int32_t* edge_j;       /* [n_edges] vertex 1 */
  const double* edge_q;        /* [n_edges][4] the measurement */
  const double* edge_t;        /* [n_edges][3] */
  const double* edge_s;        /* [n_edges] */
  const double* edge_w;        /* [n_edges] information = w I_7 */
  int32_t fix_scale;           /* bFixScale */
  int32_t iterations;          /* 20 (src/Optimizer.cc:2362); <= 0: the estimate as it came and the chi2 at it */
  double lambda_init;          /* 1e-16 (src/Optimizer.cc:2059) */
  const float* points;         /* [n_points][3] world positions (may be NULL when n_points = 0) */
  const int32_t* point_ref;    /* [n_points] the reference vertex, or -1: leave the point as it is */
} gfs_essential_graph_problem;
typedef struct {
  double* vertex_q; /* [n_vertices][4] as g2o leaves it: not renormalised */
  double* vertex_t; /* [n_vertices][3] */
  double* vertex_s; /* [n_vertices] */
  float* points;    /* [n_points][3] (may be NULL) */
  double* edge_chi2; /* [n_edges] e->chi2() at the estimate that is returned (may be NULL) */
  int32_t iterations_run;
  double final_chi2, final_lambda;
} gfs_essential_graph_solution;
typedef struct {
  int32_t n_free, dimension, panels; /* free vertices; their dimension (6 or 7); tile rows of the system */
  int64_t blocks;                    /* listed blocks of the lower triangle */
  int32_t trials, launches;          /* Levenberg trials run; kernel launches of the call */
  int64_t system_bytes;              /* bytes of the tiled system */
} gfs_essential_graph_info;
typedef struct gfs_essential_graph gfs_essential_graph;
int gfs_essential_graph_create(int device, int max_vertices, int max_edges, int max_points, gfs_essential_graph** out);
void gfs_essential_graph_destroy(gfs_essential_graph* h);
int gfs_essential_graph_optimize(gfs_essential_graph* h, const gfs_essential_graph_problem* p, gfs_essential_graph_solution* s);
/* The point correction alone, on given Sim3s [n_vertices][8] = (q, t, s): `before` the reference vertices' Srw, `after` their
 * corrected Siw (inverted on the device).  LoopClosing::CorrectLoop maps the points of the corrected key-frames the same way. */
int gfs_essential_graph_correct_points(gfs_essential_graph* h, int n_vertices, const double* before, const double* after, int n_points,
                                       const float* points, const int32_t* point_ref, float* out);
/* What the handle's last gfs_essential_graph_optimize did. */
int gfs_essential_graph_last_info(const gfs_essential_graph* h, gfs_essential_graph_info* info);

/* ============================================================================================
 * 16. Optimizer::OptimizeSim3 (src/Optimizer.cc:2797-3054) — the Sim3 refinement of loop verification, between the two Sim3
 *     projection searches of LoopClosing::DetectCommonRegionsFromBoW (:811-841) and DetectAndReffineSim3FromLastKF (:579-616).
 *    One free VertexSim3Expmap (S12, _fix_scale = fix_scale); per pair, in this order, an EdgeSim3ProjectXYZ (obs1 - cam1.project(
 *    S12.map(x2c))) and an EdgeInverseSim3ProjectXYZ (obs2 - cam2.project(S12.inverse().map(x1c))) against fixed points, information
 *    inv_sigma2 I_2, g2o's numeric Jacobians (central differences through the vertex's oplus, delta 1e-9).  BlockSolverX +
 *    LinearSolverDense (Eigen::LDLT of the 7 x 7, also with fix_scale) + Levenberg.  The schedule: optimize(5) with Huber kernels of
 *    delta (float)sqrt(th2); a pair leaves when either chi2 -- as the solve's last computeActiveErrors left it, which after rejected
 *    trials is NOT the chi2 at the estimate -- is > th2; fewer than 10 pairs left: return 0, S12 untouched; else optimize(10 if a pair
 *    left else 5) without kernels, the errors recomputed, nIn counted.  Every sum over the edges runs in edge order (e12(0), e21(0),
 *    e12(1), ...).  B problems are one launch, one workgroup each.  DESIGN.md section 21.
 *    Refused before anything is staged, the handle left usable -- GFS_ERR_CAPACITY: B above max_batch or n_pairs above max_pairs;
 *    GFS_ERR_INVALID_ARG: a NULL required array, n_pairs < 0, th2 not finite or <= 0.  n_pairs == 0 is valid (the early return).
 * ============================================================================================ */
#define GFS_SIM3_OPT_EARLY_RETURN 0 /* status: nCorrespondences - nBad < 10 after the first phase; s12 is the input */
#define GFS_SIM3_OPT_BOTH_PHASES 1  /* status: both phases ran */
#define GFS_SIM3_PAIR_INLIER 0        /* pair_state: counted in n_in (after an early return: not removed by the first check) */
#define GFS_SIM3_PAIR_REMOVED_FIRST 1 /* removed by the first check (vpMatches1[idx] = NULL, edges removed) */
#define GFS_SIM3_PAIR_REMOVED_FINAL 2 /* failed the final check (vpMatches1[idx] = NULL) */
typedef struct {
  double s12[8];            /* g2oS12: quaternion (x, y, z, w), translation, scale */
  double cam1[4], cam2[4];  /* fx, fy, cx, cy of pKF1->mpCamera / pKF2->mpCamera (pinhole) */
  float th2;
  int32_t fix_scale;
  int32_t n_pairs;          /* the pairs that got edges, in the order of the reference's loop */
  const double* x1c;        /* [n_pairs][3] P3D1c.cast<double>() */
  const double* x2c;        /* [n_pairs][3] P3D2c.cast<double>() */
  const double* obs1;       /* [n_pairs][2] kpUn1.pt */
  const double* obs2;       /* [n_pairs][2] kpUn2.pt, or the float x / z, y / z of the i2 < 0 branch */
  const float* inv_sigma2_1; /* [n_pairs] pKF1->mvInvLevelSigma2[kpUn1.octave] */
  const float* inv_sigma2_2; /* [n_pairs] pKF2->mvInvLevelSigma2[kpUn2.octave] */
} gfs_sim3_opt_problem;
typedef struct {
  double s12[8];                  /* vSim3_recov->estimate(); the input after an early return */
  int32_t n_in, n_bad, status;    /* the return value (0 after an early return); nBad of the first check; GFS_SIM3_OPT_* */
  int32_t iterations_run[2];      /* outer Levenberg iterations of the two optimize() calls */
  uint8_t* pair_state;            /* [n_pairs] GFS_SIM3_PAIR_* */
  double* chi2;                   /* [n_pairs][2] (may be NULL) e12 / e21 chi2 as last read by a check: the final one for a pair that
                                     reached it, else the first one's */
} gfs_sim3_opt_solution;
typedef struct gfs_sim3_opt gfs_sim3_opt;
int gfs_sim3_opt_create(int device, int max_batch, int max_pairs, gfs_sim3_opt** out);
void gfs_sim3_opt_destroy(gfs_sim3_opt* h);
int gfs_sim3_optimize(gfs_sim3_opt* h, const gfs_sim3_opt_problem* problems, int B, gfs_sim3_opt_solution* solutions);

/* ============================================================================================
 * 17. Sim3Solver (src/Sim3Solver.cc) — the RANSAC step of LoopClosing::DetectCommonRegionsFromBoW (:742-759), between
 *     gfs_search_by_bow and the first gfs_sim3_search: every hypothesis of a candidate, and every candidate, in one call.
 *    A problem is what the constructor (:43-116) leaves: N pairs of camera-frame points, their thresholds, two pinhole cameras, and
 *    the draws of DUtils::Random::RandomInt for every iteration (an input: the reference reads the process-global rand()).  Each of
 *    the n_iterations hypotheses is the closed-form Horn solve of the three drawn pairs, scored by projecting all N pairs both ways
 *    (csrc/sim3_ransac_rule.hpp, DESIGN.md section 23: three written rules stand for Eigen::EigenSolver, Sophus::SO3f::exp and
 *    Eigen's reductions).  The solution is what the sequential loop of iterate() would have returned after running to its end:
 *    the FIRST hypothesis with more than min_inliers inliers (status CONVERGED, iterations = its index + 1), else the LAST of those
 *    with the most inliers (NO_MORE, iterations = n_iterations).  n_pairs < min_inliers or n_pairs < 3 (where the reference would
 *    index out of range) is TOO_FEW: nothing is iterated, T12 and R12 are the identity, t12 = 0, s12 = 1, the mask is cleared.
 *    Refused before anything is staged, the handle left usable, nothing truncated -- GFS_ERR_CAPACITY: B above max_batch, n_pairs
 *    above max_pairs, n_iterations above max_iterations; GFS_ERR_INVALID_ARG: a NULL required array, n_pairs < 0, n_iterations < 1
 *    or a draw outside its range [0, N-1], [0, N-2], [0, N-3] in a problem that iterates.
 * ============================================================================================ */
#define GFS_SIM3_RANSAC_CONVERGED 0 /* bConverge */
#define GFS_SIM3_RANSAC_NO_MORE 1   /* bNoMore after mRansacMaxIts iterations: the best hypothesis, not good enough */
#define GFS_SIM3_RANSAC_TOO_FEW 2   /* bNoMore at once (:215-218) */
typedef struct {
  int32_t n_pairs;                 /* N: pairs that passed the constructor's filter (:73-111) */
  const float* x3d_c1;             /* [N][3] mvX3Dc1 */
  const float* x3d_c2;             /* [N][3] mvX3Dc2 */
  const float* max_err1;           /* [N] mvnMaxError1 as the comparison reads it: (float)(size_t)(9.210 * sigma2) of kp1's level
                                      (the member is a vector<size_t>, include/Sim3Solver.h:85) */
  const float* max_err2;           /* [N] the same for kp2 */
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
  int32_t fix_scale, min_inliers, n_iterations;   /* n_iterations = mRansacMaxIts after SetRansacParameters */
  const int32_t* draws;            /* [n_iterations][3] r0, r1, r2 as RandomInt returned them */
} gfs_sim3_ransac_problem;
typedef struct {
  float T12[16], R12[9], t12[3], s12;  /* mBestT12 (row-major), mBestRotation (row-major), mBestTranslation, mBestScale */
  int32_t n_inliers, iterations, status;   /* GFS_SIM3_RANSAC_CONVERGED / _NO_MORE / _TOO_FEW */
  uint8_t* inlier;                 /* [N] mask of the returned hypothesis */
  int32_t* counts;                 /* [n_iterations] (may be NULL) every hypothesis's count, for tests */
} gfs_sim3_ransac_solution;
typedef struct gfs_sim3_ransac gfs_sim3_ransac;
/* SetRansacParameters (:119-143): mRansacMaxIts for n_pairs correspondences, with the host's libm */
int gfs_sim3_ransac_iterations(int n_pairs, double probability, int min_inliers, int max_iterations);
int gfs_sim3_ransac_create(int device, int max_batch, int max_pairs, int max_iterations, gfs_sim3_ransac** out);
int gfs_sim3_ransac_solve(gfs_sim3_ransac* h, const gfs_sim3_ransac_problem* problems, int B, gfs_sim3_ransac_solution* solutions);
void gfs_sim3_ransac_destroy(gfs_sim3_ransac* h);

/* ============================================================================================
 * 18. ComputeBoW and the BoW database query — the head of loop detection, and the one piece of it the tracking thread runs too:
 *      DBoW2::TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)   TemplatedVocabulary.h:1119-1259
 *        as KeyFrame::ComputeBoW (src/KeyFrame.cc:219-227) and Frame::ComputeBoW (src/Frame.cc:1086-1091) call it, and
 *      the numeric core of KeyFrameDatabase::DetectNBestCandidates (src/KeyFrameDatabase.cc:583-718): the common-word count of the
 *        query against every key frame of the database and L1Scoring::score (ScoringObject.cpp:23-68).
 *    csrc/bow_vocab_rule.hpp and DESIGN.md section 24 state the rule: the descent by strict `<` in `children` order, the
 *    accumulation in feature order, the L1 norm summed in ascending word id, the score's terms added in ascending word id.  Every
 *    output is the reference's byte for byte.  Only TF_IDF weighting with L1_NORM scoring is accepted: the header `10 6 0 0` of
 *    ORBvoc.txt, scoring = 0 (L1_NORM), weighting = 0 (TF_IDF).
 *
 *    gfs_bow_create validates the tree on the host before anything is uploaded (GFS_ERR_INVALID_ARG): 1 <= k <= 20, 1 <= L <= 10,
 *    scoring == 0 and weighting == 0, the root an inner node, every non-root node listed once and under its `parent` only, no
 *    cycles, every index in range, an inner node (word_id == -1) with 1..k children, a leaf (word_id >= 0) with none, the word ids
 *    a permutation of 0..n_words-1, depth <= L, weights finite.  It uploads a repacked table in which the children of a node are
 *    contiguous and in `children` order.  max_features <= 4096 (else GFS_ERR_UNSUPPORTED: one workgroup sorts a frame in LDS).
 * ============================================================================================ */
typedef struct {
  int32_t k, L, scoring, weighting;  /* header of the vocabulary */
  int32_t n_nodes;                   /* node 0 is the root */
  const int32_t* parent;             /* [n_nodes], parent[0] ignored */
  const int32_t* child_start;        /* [n_nodes + 1] prefix sum */
  const int32_t* children;           /* [child_start[n_nodes]] in the order of m_nodes[n].children */
  const uint8_t* desc;               /* [n_nodes][32] */
  const double*  weight;             /* [n_nodes] */
  const int32_t* word_id;            /* [n_nodes] >= 0 for a leaf, -1 for an inner node */
} gfs_bow_vocabulary;
typedef struct gfs_bow_vocab gfs_bow_vocab;  /* (not gfs_bow: that names the rule of section 7a' inside the library) */
int  gfs_bow_create(int device, const gfs_bow_vocabulary* v, int max_batch, int max_features, gfs_bow_vocab** out);
void gfs_bow_destroy(gfs_bow_vocab* h);

typedef struct {           /* caller-owned, capacities = max_features of the handle (node_start: max_features + 1) */
  int32_t n_words;  int32_t* word_id; double* word_value;          /* BowVector, ascending id */
  int32_t n_nodes;  int32_t* node_id; int32_t* node_start; int32_t* feat_idx; /* FeatureVector in the layout of gfs_bow_keyframe */
  int32_t* word_of_feature;  /* [n] (may be NULL) word id of every feature, -1 when stopped: for tests */
} gfs_bow_vectors;
/* B frames in one call: desc[b] is [n[b]][32] (host pointers), out[b] the vectors of frame b.  feat_idx is ascending within a node,
 * node_id strictly ascending, node_start a prefix sum: gfs_search_by_bow and gfs_create_new_map_points accept the output unchanged.
 * Refused before anything is staged, nothing truncated, the handle left usable -- GFS_ERR_CAPACITY: B > max_batch or
 * n[b] > max_features; GFS_ERR_INVALID_ARG: a NULL array, n[b] < 0, levelsup < 0, or a vocabulary with a leaf shallower than level
 * L - levelsup (where the reference leaves *nid uninitialised).  B == 0 and n[b] == 0 are valid: an empty frame yields empty vectors.
 * One upload, two kernels (k_bow_descend, k_bow_vectors), one download, one synchronisation. */
int gfs_bow_transform(gfs_bow_vocab* h, const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out);
/* The same on descriptors as gfs_orb_device_results leaves them: dev_desc [B][stride][32] u8 (16-byte aligned), dev_counts [B]
 * int32, both in HBM; no upload.  The counts are only known on the device: a frame with more than max_features or more than `stride`
 * key-points is found by the kernel, which writes nothing for it, and the call returns GFS_ERR_CAPACITY after the synchronisation. */
int gfs_bow_transform_device(gfs_bow_vocab* h, const void* dev_desc, const void* dev_counts, int stride, int B, int levelsup,
                             gfs_bow_vectors* out);

/* The database: a fixed-stride store of BowVectors, one slot per key frame.  The caller owns the mapping from key frame to slot and
 * the `add` sequence numbers.  add to an occupied slot replaces its contents; erase of an empty slot is valid and does nothing.
 * query fills, for every slot (each array [max_entries]): n_common = mnPlaceRecognitionWords (0 for an empty slot), first_word =
 * the lowest common word id or -1 (the sharing list of :596-614 is ordered by (first_word, add sequence)), score =
 * (float)L1Scoring::score(query, entry) where n_common > 0, else 0: the score of every sharing entry, since the `> minCommonWords`
 * filter needs the maximum over the non-connected entries, which only the caller knows.
 * Refused before anything is staged, the handle left usable -- GFS_ERR_INVALID_ARG: a NULL array, ids not strictly ascending or
 * negative, a non-finite value, a slot outside [0, max_entries); GFS_ERR_CAPACITY: n_words > max_words.  max_words <= 4096 (else
 * GFS_ERR_UNSUPPORTED at creation: the query lives in LDS).  query: one upload, one kernel (k_bow_score), one download, one
 * synchronisation. */
typedef struct gfs_bow_db gfs_bow_db;
int  gfs_bow_db_create(int device, int max_entries, int max_words, gfs_bow_db** out);
void gfs_bow_db_destroy(gfs_bow_db* h);
int  gfs_bow_db_add(gfs_bow_db* h, int slot, int n_words, const int32_t* word_id, const double* word_value);
int  gfs_bow_db_erase(gfs_bow_db* h, int slot);
int  gfs_bow_db_query(gfs_bow_db* h, int n_words, const int32_t* word_id, const double* word_value,
                      int32_t* n_common, int32_t* first_word, float* score);   /* each [max_entries] */

/* ============================================================================================
 * 19. PoseInertialOptimization — the IMU pose step that ends Tracking::TrackLocalMap once the IMU is initialised
 *     (src/Tracking.cc:3763-3798): Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:5899-6283, mode
 *     GFS_POSE_INERTIAL_LAST_KEYFRAME: the other end of the inertial edge is the last key frame, fixed, 15 unknowns) and
 *     ...LastFrame (:6762-7171, mode GFS_POSE_INERTIAL_LAST_FRAME: the previous frame, free, 30 unknowns, with its prior).
 *    One graph with two settings, one kernel: n_rounds <= 4 rounds of ten Gauss-Newton iterations over the dense 15 x 15 / 30 x 30
 *    system, the re-classification of the visual edges after each, the recovery pass and the Hessian of the new prior, B problems
 *    a call with the modes mixed freely, one workgroup a problem, no host round trip.  csrc/pose_inertial_rule.hpp and DESIGN.md
 *    section 25 state the rule, the quirks kept and the written rules N / E / L / S; every output is the sequential restatement's
 *    (tests/host/pose_inertial_restatement.cpp) byte for byte, alone or inside any batch.
 *    A problem carries what the reference's constructors leave: no matrix inverse and no eigen-solver runs here.  Matrices are
 *    row-major.  Only Nleft == -1 and the pinhole camera (uncertainty2 == 1).
 *    Refused before anything is staged, the handle left usable, nothing truncated -- GFS_ERR_CAPACITY: B above max_batch, n_obs
 *    above max_obs; GFS_ERR_INVALID_ARG: a NULL required array (xw, obs, inv_sigma2, stereo, close, outlier when n_obs > 0), n_obs < 0,
 *    n_rounds outside 1..4, an unknown mode.
 * ============================================================================================ */
#define GFS_POSE_INERTIAL_LAST_KEYFRAME 0
#define GFS_POSE_INERTIAL_LAST_FRAME 1
typedef struct {  /* one end of the inertial edge as ImuCamPose(Frame*) / (KeyFrame*) and the Vertex* constructors leave it */
  double Rwb[9], twb[3], Rcw[9], tcw[3];   /* src/G2oTypes.cc:28-119 */
  double v[3], bg[3], ba[3];               /* VertexVelocity, VertexGyroBias, VertexAccBias */
} gfs_imu_state;
typedef struct {
  int32_t mode;                    /* GFS_POSE_INERTIAL_LAST_KEYFRAME / _LAST_FRAME */
  int32_t n_obs;                   /* visual edges, in the reference's index order (mono and stereo interleaved) */
  int32_t n_rounds;                /* nIterations, 1..4 */
  int32_t rec_init;                /* bRecInit */
  const double* xw;                /* [n][3] pMP->GetWorldPos(), doubles from floats */
  const double* obs;               /* [n][3] kpUn.pt.x, kpUn.pt.y, mvuRight (ignored for a mono edge), doubles from floats */
  const float* inv_sigma2;         /* [n] mvInvLevelSigma2[octave] / uncertainty2 */
  const uint8_t* stereo;           /* [n] 1: EdgeStereoOnlyPose, 0: EdgeMonoOnlyPose */
  const uint8_t* close;            /* [n] bClose = mTrackDepth < 10.f (read for mono edges) */
  double fx, fy, cx, cy, bf;       /* the pinhole's float parameters and mbf as doubles */
  double Rcb[9], tcb[3], Rbc[9], tbc[3];
  gfs_imu_state cur;               /* pFrame: vertices 0..3 */
  gfs_imu_state other;             /* pFrame->mpLastKeyFrame (fixed) or pFrame->mpPrevFrame (free): vertices 4..7 */
  /* the preintegration of the inertial edge: mpImuPreintegrated (key-frame mode) or mpImuPreintegratedFrame (frame mode) */
  float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
  float preint_bg[3], preint_ba[3];  /* its bias b: bwx bwy bwz, bax bay baz */
  float dT;
  double info_inertial[81];        /* EdgeInertial's information after the constructor's inverse and eigenvalue clamp (:485-492) */
  double info_gyro_rw[9];          /* mpImuPreintegrated->C.block<3,3>(9,9).cast<double>().inverse(), in both modes (:6961) */
  double info_acc_rw[9];           /* ... block<3,3>(12,12) ... (:6968) */
  /* frame mode only: pFp->mpcpi */
  double prior_Rwb[9], prior_twb[3], prior_vwb[3], prior_bg[3], prior_ba[3], prior_H[225];
} gfs_pose_inertial_problem;
typedef struct {  /* the estimates as doubles: the caller casts, as SetImuPoseVelocity and IMU::Bias do */
  double Rwb[9], twb[3], v[3], bg[3], ba[3];
} gfs_imu_estimate;
typedef struct {
  gfs_imu_estimate cur;            /* VP, VV, VG, VA */
  gfs_imu_estimate other;          /* frame mode: the previous frame's (for tests); key-frame mode: the key frame's, unchanged */
  uint8_t* outlier;                /* [n] mvbOutlier */
  int32_t n_good;                  /* the return value: nInitialCorrespondences - nBad */
  int32_t n_inliers;               /* nInliers of the last round */
  int32_t rounds_run;
  float avg_reproj;                /* avgReprojectionError of the last round */
  double H[900];                   /* row-major 15 x 15 (key-frame mode: VP, VV, VG, VA) or 30 x 30 (frame mode: the previous
                                      frame's 15, then the current frame's), BEFORE Optimizer::Marginalize and ConstraintPoseImu */
} gfs_pose_inertial_solution;
typedef struct gfs_pose_inertial gfs_pose_inertial;
int gfs_pose_inertial_create(int device, int max_obs, int max_batch, gfs_pose_inertial** out);
void gfs_pose_inertial_destroy(gfs_pose_inertial* h);
int gfs_pose_inertial_optimize(gfs_pose_inertial* h, const gfs_pose_inertial_problem* problems, int B, gfs_pose_inertial_solution* solutions);

/* ============================================================================================
 * 20. LocalInertialBA — the inertial local bundle adjustment of LocalMapping::Run once the IMU is initialised
 *     (src/LocalMapping.cc:186-228, Optimizer::LocalInertialBA src/Optimizer.cc:3056-3702): the numeric core from
 *     optimizer.initializeOptimization() (:3589) to the end of the two classification loops (:3626).  The pointer-graph gather and
 *     the write-back are gfs_host::LocalInertialBA's (geoflowslam_amd/host/gfs_adaptors.hpp).
 *    One optimize(iterations) of the fork's OptimizationAlgorithmLevenberg over n_opt window key frames of 15 unknowns (pose,
 *    velocity, gyro bias, accelerometer bias), marginalised map points and the chain of inertial edges; the whole solve is queued at
 *    once, the trial decisions are made on the device, the host waits once.  csrc/lba_inertial_rule.hpp and DESIGN.md section 26
 *    state the rule, the quirks kept and the written rules; every output is the sequential restatement's
 *    (tests/host/lba_inertial_restatement.cpp) byte for byte.  There is no stop flag: the reference polls none (:3594).
 *    Key-frame indices of edge_kf: 0 .. n_opt - 1 the window, newest first; n_opt the fixed key frame in front of the window (prev);
 *    n_opt + 1 + k the k-th other fixed key frame.  The visual edges come point by point (point_edge_begin), within a point in
 *    observation order.  One camera and one IMU calibration for the whole window; matrices row-major.
 *    Refused before anything is staged, the handle left usable -- GFS_ERR_CAPACITY: n_opt, n_fixed, n_points, n_edges or the number
 *    of Schur pairs above what the handle was created for; GFS_ERR_INVALID_ARG: a NULL required array, n_opt < 1, iterations < 0,
 *    a negative count, point_edge_begin not ascending from 0 to n_edges, an edge_kf out of range; GFS_ERR_UNSUPPORTED: a window key
 *    frame without IMU (window_imu[i] == 0), n_cameras != 1.
 * ============================================================================================ */
typedef struct {  /* EdgeInertial, EdgeGyroRW, EdgeAccRW onto window key frame i: pKFi->mpImuPreintegrated as the constructors leave it */
  float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
  float preint_bg[3], preint_ba[3];
  float dT;
  double info_inertial[81];        /* after the constructor's inverse and eigenvalue clamp; the library applies the 1e-2 of i = N - 1 */
  double info_gyro_rw[9];          /* C.block<3,3>(9,9).cast<double>().inverse() (:3384) */
  double info_acc_rw[9];           /* C.block<3,3>(12,12)... (:3393) */
} gfs_lba_inertial_edge;
typedef struct {
  int32_t n_opt;                   /* N: optimisable temporal key frames, newest first */
  int32_t n_fixed;                 /* other fixed key frames (lFixedKeyFrames without the window's predecessor), at most 200 */
  int32_t n_points, n_edges;
  int32_t iterations;              /* opt_it: 8, or 4 with bLarge */
  int32_t n_cameras;               /* 1; anything else is refused */
  double lambda_init;              /* setUserLambdaInit: 1e0, or 1e-2 with bLarge */
  double fx, fy, cx, cy, bf;
  double Rcb[9], tcb[3], Rbc[9], tbc[3];
  const gfs_imu_state* window;     /* [n_opt] */
  const uint8_t* window_imu;       /* [n_opt] pKFi->bImu */
  gfs_imu_state prev;              /* the fixed key frame in front of the window: all four vertices fixed */
  const double* fixed_Rcw;         /* [n_fixed][9] */
  const double* fixed_tcw;         /* [n_fixed][3] */
  const gfs_lba_inertial_edge* inertial;  /* [n_opt]: set i joins key frame i + 1 (or prev) to key frame i */
  const double* points;            /* [n_points][3] pMP->GetWorldPos(), doubles from floats */
  const int32_t* point_edge_begin; /* [n_points + 1] */
  const int32_t* edge_kf;          /* [n_edges] */
  const double* obs;               /* [n_edges][3] kpUn.pt.x, kpUn.pt.y, mvuRight (ignored for a mono edge) */
  const float* inv_sigma2;         /* [n_edges] */
  const uint8_t* stereo;           /* [n_edges] 1: EdgeStereo, 0: EdgeMono */
  const uint8_t* close;            /* [n_edges] pMP->mTrackDepth < 10.f (read for mono edges) */
} gfs_lba_inertial_problem;
typedef struct {
  gfs_imu_state* window;           /* [n_opt] Rwb, twb, Rcw, tcw, v, bg, ba as doubles */
  double* points;                  /* [n_points][3] */
  double* edge_chi2;               /* [n_edges] e->chi2() as the edges hold it after optimize */
  uint8_t* edge_depth_positive;    /* [n_edges] isDepthPositive() at the returned estimate */
  uint8_t* edge_erase;             /* [n_edges] the classification loops' verdict (:3601-3626) */
  float err, err_end;              /* the fail gate (2 * err < err_end || isnan ...) && !bLarge is the caller's */
  int32_t iterations_run, trials_run;
  double final_lambda;
} gfs_lba_inertial_solution;
typedef struct gfs_lba_inertial gfs_lba_inertial;
int gfs_lba_inertial_create(int device, int max_opt, int max_fixed, int max_points, int max_edges, gfs_lba_inertial** out);
void gfs_lba_inertial_destroy(gfs_lba_inertial* h);
int gfs_lba_inertial_solve(gfs_lba_inertial* h, const gfs_lba_inertial_problem* problem, gfs_lba_inertial_solution* solution);

/* ============================================================================================
 * 21. PoseLidarVisualInertialOptimization — the pose step that ends Tracking::TrackLocalMap for IMU_RGBD with point-cloud
 *     observations (src/Tracking.cc:3763-3798): Optimizer::PoseLidarVisualInertialOptimizationLastKeyFrame (src/Optimizer.cc:6285-6760)
 *     and ...LastFrame (:7173-7678).  The graph of section 19 plus, in every round, the point-to-plane edges GenerateLidarEdge builds
 *     from the frame's downsampled cloud and the local map (the association of section 11: 5-NN, float QR plane, gates, weight),
 *     differentiated numerically as g2o does.  Per round an association launch over all problems and a round launch (one workgroup a
 *     problem), then one final launch; everything is queued at once and the host waits once.  csrc/pose_lidar_inertial_rule.hpp and
 *     DESIGN.md section 27 state the rule and the quirks kept; every output is the sequential restatement's
 *     (tests/host/pose_lidar_inertial_restatement.cpp) byte for byte, alone or inside any batch.
 *    Refused before anything is staged, the handle left usable -- GFS_ERR_CAPACITY: B above max_batch, n_obs above max_obs, n_cloud
 *    above max_cloud; GFS_ERR_INVALID_ARG: a NULL required array (those of section 19; cloud when n_cloud > 0), a negative count,
 *    n_rounds outside 1..4, an unknown mode, n_cloud > 0 with a NULL map or a map of fewer than 5 points, a map on another device.
 * ============================================================================================ */
typedef struct {
  gfs_pose_inertial_problem vi;    /* every field of section 19, with its meaning there */
  float q[4], t[3];                /* pFrame->GetPose(): the stored Sophus::SE3f Tcw, quaternion (x, y, z, w) */
  float tcb_q[4], tcb_t[3];        /* pFrame->mImuCalib.mTcb as stored, beside the doubles vi.Rcb / vi.tcb */
  double kf_time_gap;              /* pFrame->mTimeStamp - pKF->mTimeStamp, signed (read in key-frame mode) */
  int32_t n_cloud;                 /* mpPointCloudDownsampled->size(); 0 for a null cloud */
  const float* cloud;              /* [n_cloud][3] camera frame */
  const struct gfs_lidar_map* map; /* laserCloudSurfFromMapDS (section 11), on the handle's device; may be NULL when n_cloud == 0 */
} gfs_pose_lidar_inertial_problem;
typedef struct {
  gfs_pose_inertial_solution vi;   /* every field of section 19; H includes the lidar edges of the last entered round */
  int32_t n_lidar_inliers;         /* nInliersLidar */
  float residual;                  /* residual */
  int32_t round_edges[4];          /* lidar edges generated in each round that ran */
  float round_chi2[4];             /* chi2Lidar of the round */
  int32_t round_valid[4];          /* valid_edge of the round */
} gfs_pose_lidar_inertial_solution;
typedef struct gfs_pose_lidar_inertial gfs_pose_lidar_inertial;
int gfs_pose_lidar_inertial_create(int device, int max_obs, int max_cloud, int max_batch, gfs_pose_lidar_inertial** out);
void gfs_pose_lidar_inertial_destroy(gfs_pose_lidar_inertial* h);
int gfs_pose_lidar_inertial_optimize(gfs_pose_lidar_inertial* h, const gfs_pose_lidar_inertial_problem* problems, int B,
                                     gfs_pose_lidar_inertial_solution* solutions);
/* Diagnostic: the lidar edges problem b of the last call generated in `round`, in cloud-index order.  *n is their number; at most
 * cap are written to index [cap], plane [cap][4], s [cap]. */
int gfs_pose_lidar_inertial_fetch_edges(gfs_pose_lidar_inertial* h, int b, int round, int32_t* index, float* plane, float* s, int cap,
                                        int32_t* n);

/* ============================================================================================
 * Timing helper for the harness: HIP events on a given stream (bench.py measures the dominant kernel
 * with these rather than torch events, which only see torch's current stream).
 * ============================================================================================ */
typedef struct gfs_timer gfs_timer;
int gfs_timer_create(int device, gfs_timer** out);
void gfs_timer_destroy(gfs_timer* t);
int gfs_timer_start(gfs_timer* t, void* stream);
int gfs_timer_stop(gfs_timer* t, void* stream);
/* blocks until the stop event completed; milliseconds between start and stop */
int gfs_timer_elapsed_ms(gfs_timer* t, float* ms);

/* Per-kernel accumulated device time (HIP events around each launch) — enable for profiling runs only. */
int gfs_profile_enable(int on);
/* Fills up to cap entries; returns number of distinct kernels. name buffers are 64 bytes each. */
int gfs_profile_report(char (*names)[64], double* total_ms, int64_t* launches, int cap);
int gfs_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GFS_ABI_H_ */
