// C++ host-side mirror of the reference's four seams on top of the C ABI (include/gfs_abi.h).
//
// The reference is C++17 (OpenCV / Eigen types in its signatures).  Neither library exists in this image, so there are TWO layers:
//   1. this header, namespace gfs_host: the same classes with plain std:: containers (always compiled; used by the examples, the
//      tests and by anything that does not want OpenCV / Eigen);
//   2. gfs_reference_dropins.hpp beside it, namespace gfs_dropin: the code a maintainer adds to the reference tree, written against
//      the reference's own types --
//        GfsORBextractor : ORB_SLAM3::ORBextractor, operator()(cv::InputArray, cv::InputArray, std::vector<cv::KeyPoint>&,
//                                                              cv::OutputArray, std::vector<int>&)   include/ORBextractor.h:61-64
//        bf_match(d1, d2, std::vector<cv::DMatch>&), gms_inlier_mask(...)                            src/ORBmatcher.cc:755-762
//        RegisterPointClouds(...) -> small_gicp::RegistrationResult                                  include/RegistrationGICP.h:25-28
//        LbaAccess<KeyFrame, MapPoint> for gfs_host::LocalBundleAdjustment                           src/Optimizer.cc:1588-2040
//      compile-checked against the reference's real headers over declaration-only OpenCV / Eigen / Sophus stand-ins
//      (tests/test_host_logic.py::test_reference_dropins_compile).  INTEGRATION.md shows where they are swapped in.
// Error behaviour follows the reference: operator() returns -1 on an empty image, asserts CV_8UC1; GICP never throws.
// Anything the GPU library reports as an error is raised as std::runtime_error (there is no CPU fallback).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gfs_abi.h"
#include "../csrc/bow_vocab_rule.hpp"
#include "../csrc/fuse_rule.hpp"
#include "../csrc/lba_inertial_rule.hpp"
#include "../csrc/sim3_search_rule.hpp"
#include "../csrc/map_point_rule.hpp"
#include "../csrc/sim3_dev.hpp"
#include "../csrc/sim3_ransac_rule.hpp"
#include "../csrc/triangulate_rule.hpp"

namespace gfs_host {

inline void check(int rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + gfs_last_error());
}

// ORB_SLAM3::ORBextractor (reference include/ORBextractor.h:46-118)
class ORBextractor {
 public:
  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int max_rows = 720,
               int max_cols = 1280, int device = 0)
      : nlevels_(nlevels) {
    gfs_orb_config c;
    gfs_orb_default_config(&c);
    c.nfeatures = nfeatures;
    c.scale_factor = scaleFactor;
    c.nlevels = nlevels;
    c.ini_th_fast = iniThFAST;
    c.min_th_fast = minThFAST;
    c.max_rows = max_rows;
    c.max_cols = max_cols;
    c.device = device;
    check(gfs_orb_create(&c, &h_), "gfs_orb_create");
    cap_ = gfs_orb_max_keypoints(h_);
  }
  ~ORBextractor() { gfs_orb_destroy(h_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // operator()(image, mask, keypoints, descriptors, vLappingArea): returns monoIndex, or -1 for an empty image
  int operator()(const uint8_t* image, int rows, int cols, int stride, std::vector<gfs_keypoint>& keypoints,
                 std::vector<uint8_t>& descriptors, const std::vector<int>& vLappingArea) {
    keypoints.assign(cap_, gfs_keypoint{});
    descriptors.assign((size_t)cap_ * 32, 0);
    int n = 0;
    const int lap0 = vLappingArea.size() > 0 ? vLappingArea[0] : 0, lap1 = vLappingArea.size() > 1 ? vLappingArea[1] : 0;
    const int r = gfs_orb_extract(h_, image, rows, cols, stride, lap0, lap1, keypoints.data(), descriptors.data(), cap_, &n);
    if (r < -1) check(r + 100, "gfs_orb_extract");
    keypoints.resize(n);
    descriptors.resize((size_t)n * 32);
    return r;
  }
  int GetLevels() const { return nlevels_; }
  std::vector<float> GetScaleFactors() const { return table(0); }
  std::vector<float> GetInverseScaleFactors() const { return table(1); }
  std::vector<float> GetScaleSigmaSquares() const { return table(2); }
  std::vector<float> GetInverseScaleSigmaSquares() const { return table(3); }
  gfs_orb* handle() { return h_; }

 private:
  std::vector<float> table(int which) const {
    std::vector<float> t[4];
    for (auto& v : t) v.resize(nlevels_);
    gfs_orb_get_tables(h_, t[0].data(), t[1].data(), t[2].data(), t[3].data(), nullptr, nullptr);
    return t[which];
  }
  gfs_orb* h_ = nullptr;
  int nlevels_, cap_ = 0;
};

struct DMatch {  // cv::DMatch
  int queryIdx, trainIdx, imgIdx;
  float distance;
};

// the brute-force part of ORB_SLAM3::ORBmatcher (reference src/ORBmatcher.cc:744-778, 2536-2550)
class ORBmatcher {
 public:
  explicit ORBmatcher(int max_rows = 8192, int device = 0) { check(gfs_matcher_create(device, max_rows, max_rows, 1, &h_), "gfs_matcher_create"); }
  ~ORBmatcher() { gfs_matcher_destroy(h_); }
  static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return gfs_hamming256(a, b); }
  // cv::BFMatcher(cv::NORM_HAMMING).match(query, train, matches)
  void match(const uint8_t* query, int nq, const uint8_t* train, int nt, std::vector<DMatch>& matches) {
    std::vector<int32_t> idx(nq > 0 ? nq : 1), dist(nq > 0 ? nq : 1);
    const int n = gfs_bf_match_hamming(h_, query, nq, train, nt, idx.data(), dist.data());
    check(n, "gfs_bf_match_hamming");
    matches.resize(n);
    for (int i = 0; i < n; i++) matches[i] = DMatch{i, idx[i], 0, (float)dist[i]};
  }

 private:
  gfs_matcher* h_ = nullptr;
};

// RegistrationGICP (reference include/RegistrationGICP.h:19-31); result = small_gicp::RegistrationResult
class RegistrationGICP {
 public:
  explicit RegistrationGICP(int max_points = 65536, int device = 0) { check(gfs_gicp_create(device, max_points, 1, &h_), "gfs_gicp_create"); }
  ~RegistrationGICP() { gfs_gicp_destroy(h_); }
  // target / source: arrays of (x, y, z, w) floats like std::vector<Eigen::Vector4f>; init: column-major 4x4
  gfs_gicp_result RegisterPointClouds(const float* target_points, int nt, const float* source_points, int ns,
                                      const double init_T_target_source[16]) {
    gfs_gicp_config cfg;
    gfs_gicp_default_config(&cfg);  // threads 4, voxel 0.02, max-corr 0.1, GICP (src/RegistrationGICP.cc:9-15)
    gfs_gicp_result r;
    check(gfs_gicp_align(h_, target_points, nt, source_points, ns, init_T_target_source, &cfg, &r), "gfs_gicp_align");
    return r;
  }
  // Streaming form for Tracking::PredictStateICP: the target is the source cloud of the previous call on this object, kept
  // preprocessed in HBM (bit-identical to RegisterPointClouds(previous source, source_points)).
  gfs_gicp_result RegisterNext(const float* source_points, int ns, const double init_T_target_source[16]) {
    gfs_gicp_config cfg;
    gfs_gicp_default_config(&cfg);
    gfs_gicp_result r;
    check(gfs_gicp_align_next(h_, source_points, ns, init_T_target_source, &cfg, &r), "gfs_gicp_align_next");
    return r;
  }

 private:
  gfs_gicp* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// LidarMapping::viewer's loop body (reference src/LidarMapping.cc:162-182): localMap is cleared, every key-frame of lNewKeyFrames
// (mlNewKeyFrames, at most 30: insertKeyFrame :72-80) that is not bad and has an mpPointCloudDownsampled is transformed by
// toMatrix4d(GetPoseInverse()) and appended, and voxel_local filters the sum at LidarMapping.LocalResolution.  The gather is host code;
// transform, filter and search grid run on the device (gfs_lidar_map_build) and land in a gfs_lidar_map the optimizers use as it is.
// The key-frames are read through an access type (no PCL / Sophus here) with static members
//     bool is_bad(const KeyFrame*);                          // pKF->isBad()
//     const float* cloud(const KeyFrame*, int* n);           // mpPointCloudDownsampled packed to [n][3] floats; nullptr = no cloud
//     void get_pose(const KeyFrame*, float q[4], float t[3]);   // GetPose(): unit_quaternion() (x, y, z, w), translation()
// ------------------------------------------------------------------------------------------------------------------------
struct LidarMapFlat {  // the key-frames that reach transformPointCloud, in list order
  std::vector<float> q, t, cloud;
  std::vector<int32_t> cloud_begin;
  int n_keyframes() const { return (int)cloud_begin.size() - 1; }
};

template <class Access, class It>
void GatherLidarKeyFrames(It first, It last, LidarMapFlat& f) {
  f.q.clear();
  f.t.clear();
  f.cloud.clear();
  f.cloud_begin.assign(1, 0);
  for (It it = first; it != last; ++it) {
    const auto* pKF = &**it;
    if (Access::is_bad(pKF)) continue;  // :164
    int n = 0;
    const float* c = Access::cloud(pKF, &n);
    if (!c) continue;  // :165
    if (n < 0) n = 0;
    float q[4], t[3];
    Access::get_pose(pKF, q, t);
    f.q.insert(f.q.end(), q, q + 4);
    f.t.insert(f.t.end(), t, t + 3);
    f.cloud.insert(f.cloud.end(), c, c + 3 * (size_t)n);
    f.cloud_begin.push_back(f.cloud_begin.back() + n);
  }
}

class LidarLocalMapper {
 public:
  LidarLocalMapper(int max_points_in = 262144, int max_keyframes = 30, int device = 0) {
    check(gfs_lidar_mapper_create(device, max_points_in, max_keyframes, &h_), "gfs_lidar_mapper_create");
  }
  ~LidarLocalMapper() { gfs_lidar_mapper_destroy(h_); }
  LidarLocalMapper(const LidarLocalMapper&) = delete;
  LidarLocalMapper& operator=(const LidarLocalMapper&) = delete;
  // [first, last): lNewKeyFrames (iterators to KeyFrame*); resolution: LidarMapping.LocalResolution.  Throws on a refusal (the map
  // then keeps what it held).
  template <class Access, class It>
  gfs_lidar_map_info Update(It first, It last, float resolution, gfs_lidar_map* map) {
    GatherLidarKeyFrames<Access>(first, last, flat_);
    gfs_lidar_map_input in{};
    in.n_keyframes = flat_.n_keyframes();
    in.q = flat_.q.data();
    in.t = flat_.t.data();
    in.cloud_begin = flat_.cloud_begin.data();
    in.cloud = flat_.cloud.data();
    in.leaf = resolution;
    gfs_lidar_map_info info{};
    check(gfs_lidar_map_build(h_, &in, map, &info), "gfs_lidar_map_build");
    return info;
  }
  // pcl::VoxelGrid (default settings) with leaf size `leaf` on one cloud -> out ([n][3] at most; resized to the result)
  gfs_lidar_map_info VoxelFilter(const float* xyz, int n, float leaf, std::vector<float>& out) {
    out.resize(3 * (size_t)n);
    gfs_lidar_map_info info{};
    check(gfs_voxel_grid_filter(h_, xyz, n, leaf, out.data(), n, &info), "gfs_voxel_grid_filter");
    out.resize(3 * (size_t)info.n_out);
    return info;
  }
  const LidarMapFlat& gathered() const { return flat_; }

 private:
  gfs_lidar_mapper* h_ = nullptr;
  LidarMapFlat flat_;
};

// ------------------------------------------------------------------------------------------------------------------------
// Frame::Frame, the lidar-feature tail                                                      reference src/Frame.cc:378-393
//     mpLidarProcess->featureExtraction(pointcloud_in, pointcloud_edge, pointcloud_surf);
//     *mpPointCloud = *pointcloud_surf + *pointcloud_edge;
//     downSizeFilter.setLeafSize(res, res, res); ... downSizeFilter.filter(*mpPointCloudDownsampled);
// on plain arrays around gfs_frame_cloud_extract.  `LidarParam` is the reference's own class, read through
// getHorizontalAngle(), getMaxDistance() and getLocalMapResolution() (src/Lidar.cc:100-128); downsize_resolution is
// mpSettings->downsizeResolution().  Both clouds come back as [n][3] floats (colour is not carried).  The warning the constructor
// prints when the downsampled cloud is empty stays with the caller.  A refusal throws.
// ------------------------------------------------------------------------------------------------------------------------
template <class LidarParam>
inline gfs_frame_cloud_config FrameCloudConfigFrom(const LidarParam& lp, float downsize_resolution) {
  gfs_frame_cloud_config cfg;
  gfs_frame_cloud_default_config(&cfg);
  cfg.horizontal_angle = lp.getHorizontalAngle();
  cfg.max_distance = lp.getMaxDistance();
  cfg.local_map_resolution = lp.getLocalMapResolution();
  cfg.downsize_resolution = downsize_resolution;
  return cfg;
}

class FrameCloudExtractor {
 public:
  template <class LidarParam>
  FrameCloudExtractor(const LidarParam& lp, float downsize_resolution, int max_points = 131072, int device = 0) {
    const gfs_frame_cloud_config cfg = FrameCloudConfigFrom(lp, downsize_resolution);
    check(gfs_frame_cloud_create(device, max_points, &cfg, &h_), "gfs_frame_cloud_create");
  }
  ~FrameCloudExtractor() { gfs_frame_cloud_destroy(h_); }
  FrameCloudExtractor(const FrameCloudExtractor&) = delete;
  FrameCloudExtractor& operator=(const FrameCloudExtractor&) = delete;
  // xyzw [n][4]: ConvertDepthToPointCloud's cloud in push_back order -> mpPointCloud (surf then edge) and mpPointCloudDownsampled
  gfs_frame_cloud_info Extract(const float* xyzw, int n, std::vector<float>& cloud, std::vector<float>& down) {
    cloud.resize(3 * (size_t)n);
    down.resize(3 * (size_t)n);
    gfs_frame_cloud_info info{};
    check(gfs_frame_cloud_extract(h_, xyzw, n, cloud.data(), n, down.data(), n, &info), "gfs_frame_cloud_extract");
    cloud.resize(3 * (size_t)(info.n_surf + info.n_edge));
    down.resize(3 * (size_t)info.n_down);
    return info;
  }
  // the same on the cloud gfs_frame_rgbd left on the device (n: its *n_cloud)
  gfs_frame_cloud_info ExtractDevice(const void* dev_xyzw, const void* dev_count, int n, std::vector<float>& cloud, std::vector<float>& down) {
    cloud.resize(3 * (size_t)n);
    down.resize(3 * (size_t)n);
    gfs_frame_cloud_info info{};
    check(gfs_frame_cloud_extract_device(h_, dev_xyzw, dev_count, cloud.data(), n, down.data(), n, &info), "gfs_frame_cloud_extract_device");
    cloud.resize(3 * (size_t)(info.n_surf + info.n_edge));
    down.resize(3 * (size_t)info.n_down);
    return info;
  }

 private:
  gfs_frame_cloud* h_ = nullptr;
};

// numeric core of Optimizer::LocalBundleAdjustment (reference include/Optimizer.h:62-65)
class LocalBundleAdjuster {
 public:
  LocalBundleAdjuster(int max_poses = 64, int max_points = 16384, int max_edges = 262144, int device = 0) : device_(device) {
    check(gfs_lba_create(device, max_poses, max_points, max_edges, &h_), "gfs_lba_create");
  }
  ~LocalBundleAdjuster() {
    gfs_lba_destroy(h_);
    gfs_lidar_map_destroy(map_);
  }
  LocalBundleAdjuster(const LocalBundleAdjuster&) = delete;
  LocalBundleAdjuster& operator=(const LocalBundleAdjuster&) = delete;
  // returns false when *pbStopFlag was already set (the reference returns early, src/Optimizer.cc:1955-1956)
  bool solve(const gfs_lba_problem& p, gfs_lba_solution& s, const bool* pbStopFlag) {
    // the caller's flag itself goes down (a C++ bool is one byte): the solver reads it live, at the top of every iteration and
    // after every trial step, so an mbAbortBA raised by the tracking thread WHILE the adjustment runs ends it (setForceStopFlag)
    static_assert(sizeof(bool) == 1, "gfs_lba_solve_bool reads the flag as one byte");
    const int rc = gfs_lba_solve_bool(h_, &p, &s, reinterpret_cast<const volatile unsigned char*>(pbStopFlag));
    if (rc == GFS_ERR_STOPPED) return false;
    check(rc, "gfs_lba_solve");
    return true;
  }
  // Optimizer::LocalBundleAdjustment on the reference's own KeyFrame / MapPoint / Map classes (see LocalBundleAdjustment below)
  template <class Access, class KeyFrame, class Map>
  void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs,
                             int& num_edges);
  // ... with the write-back's UpdateNormalAndDepth loop as one call of `update_points` (MapPointUpdater::solver())
  template <class Access, class KeyFrame, class Map, class UpdatePoints>
  void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs,
                             int& num_edges, UpdatePoints&& update_points);
  // LocalVisualLidarBA's numeric core on the handle's owned local map (gfs_lba_solve_lidar_bool); false when *pbStopFlag was set
  bool solve_lidar(const gfs_lba_problem& p, gfs_lba_lidar lidar, gfs_lba_solution& s, const bool* pbStopFlag,
                   int32_t* pose_lidar_edges = nullptr) {
    lidar.map = map_;
    const int n = lidar.cloud_begin ? lidar.cloud_begin[p.n_poses] : 0;
    if (n > lidar_cap_) {  // the library refuses a window beyond the reserve (it never truncates): grow it first
      check(gfs_lba_lidar_reserve(h_, n), "gfs_lba_lidar_reserve");
      lidar_cap_ = n;
    }
    static_assert(sizeof(bool) == 1, "gfs_lba_solve_lidar_bool reads the flag as one byte");
    const int rc = gfs_lba_solve_lidar_bool(h_, &p, &lidar, &s, pose_lidar_edges, reinterpret_cast<const volatile unsigned char*>(pbStopFlag));
    if (rc == GFS_ERR_STOPPED) return false;
    check(rc, "gfs_lba_solve_lidar");
    return true;
  }
  // Optimizer::LocalVisualLidarBA(pKF, laserCloudSurfFromMapDS, pbStopFlag, pMap, ...) (include/Optimizer.h:71) with the local map as
  // packed xyz floats ([n_map][3]; pcl::PointXYZRGBA is 32 bytes), uploaded into the owned map (see LocalVisualLidarBA below)
  template <class Access, class KeyFrame, class Map>
  void LocalVisualLidarBA(KeyFrame* pKF, const float* map_xyz, int n_map, bool* pbStopFlag, Map* pMap, int& num_fixedKF,
                          int& num_OptKF, int& num_MPs, int& num_edges);
  // The owned local map built on the device from lNewKeyFrames (LidarLocalMapper::Update) instead of uploaded: what
  // mpLidarMapping->GetLocalMap() would have returned (src/LocalMapping.cc:216, 235).  max_map_points: the map's capacity.
  template <class Access, class It>
  gfs_lidar_map_info BuildLocalMap(It first, It last, float resolution, int max_map_points = 262144) {
    if (!map_ || max_map_points > map_cap_) {
      gfs_lidar_map_destroy(map_);
      map_ = nullptr;
      map_cap_ = std::max(max_map_points, 5);
      check(gfs_lidar_map_create(device_, map_cap_, &map_), "gfs_lidar_map_create");
    }
    if (!mapper_) mapper_.reset(new LidarLocalMapper(map_cap_, 30, device_));
    return mapper_->template Update<Access>(first, last, resolution, map_);
  }
  // LocalVisualLidarBA on the map BuildLocalMap left
  template <class Access, class KeyFrame, class Map>
  void LocalVisualLidarBA(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges);

 private:
  gfs_lba* h_ = nullptr;
  int device_ = 0;
  std::unique_ptr<LidarLocalMapper> mapper_;  // created at the first BuildLocalMap
  gfs_lidar_map* map_ = nullptr;  // created at the first LocalVisualLidarBA
  int map_cap_ = 0, lidar_cap_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------------
// void MapPoint::ComputeDistinctiveDescriptors()                                           reference src/MapPoint.cc:376-448
// void MapPoint::UpdateNormalAndDepth()                                                    reference src/MapPoint.cc:468-532
// void LocalMapping::ProcessNewKeyFrame(), its map-point loop                              reference src/LocalMapping.cc:439-454
// as real code around gfs_map_points_update, for a whole list of map points at once.  A point's update reads
// its own observation list, its position and reference key frame, and of the key frames only what the loops around it never write
// (camera centre, descriptors, isBad, the level tables); the two functions write disjoint fields (mDescriptor; mNormalVector,
// mfMinDistance, mfMaxDistance) that neither reads.  So the points of a loop are independent, and one call serves the loop:
//   gather:  per point, GetObservations() in map order.  A null or bad point uploads an empty list (both functions return at once).
//            IN_NORMAL is leftIndex != -1 (:494); IN_DESC is a key frame that is not null and not bad with leftIndex != -1 and
//            < its descriptor rows (:396-403).  The reference key frame's level is read at observations[pRefKF], which is index 0
//            when the reference key frame is not among the observations (std::map::operator[] inserts a zero tuple, :511).
//   solve:   `solve(problem, result)`: MapPointUpdater::solve below (the GPU), or map_points_update_host (the same rule on the host).
//   write:   set_normal_and_depth where the status says NORMAL_SET, set_descriptor with the chosen observation's row where DESC_SET.
// In normals-only mode IN_DESC is never set and descriptor_rows / descriptors / set_descriptor are not called.
// Single-camera key frames only: a right index, NLeft != -1, or a null key frame that UpdateNormalAndDepth would dereference throws.
// Compile with -ffp-contract=off when map_points_update_host is used (the host rule is the device's arithmetic).
//
// MapPoint / KeyFrame are the reference's own classes, used through pMP->isBad(), GetObservations(), IsInKeyFrame, AddObservation;
// pKF->isBad(), NLeft, mvScaleFactors, mnScaleLevels, GetMapPointMatches.  `Access` (world_pos, keys_un, descriptors as for Fuse) plus:
//     static int descriptor_rows(const KeyFrame&);                                   // mDescriptors.rows
//     static void camera_center(const KeyFrame&, float Ow[3]);                       // GetCameraCenter()
//     static KeyFrame* reference_keyframe(const MapPoint*);                          // GetReferenceKeyFrame()
//     static void set_descriptor(MapPoint*, const uint8_t row[32]);                  // mDescriptor = row.clone() under mMutexFeatures
//     static void set_normal_and_depth(MapPoint*, const float normal[3], float min_distance, float max_distance);  // under mMutexPos
// ------------------------------------------------------------------------------------------------------------------------
struct PerPointUpdate {};  // in place of a map-point solver: the adaptor calls the reference's own per-point functions

// gfs_map_points_update on the host: one thread, the rule of csrc/map_point_rule.hpp, the library's refusals
inline int map_points_update_host(const gfs_map_points_problem* pr, gfs_map_points_result* res) {
  if (!pr || !res || pr->n_points < 0 || !pr->obs_start || pr->obs_start[0] != 0) return GFS_ERR_INVALID_ARG;
  if (pr->mode != GFS_MAP_POINTS_FULL && pr->mode != GFS_MAP_POINTS_NORMALS_ONLY) return GFS_ERR_INVALID_ARG;
  const bool with_desc = pr->mode == GFS_MAP_POINTS_FULL;
  for (int p = 0; p < pr->n_points; p++)
    if (pr->obs_start[p + 1] < pr->obs_start[p]) return GFS_ERR_INVALID_ARG;
  if (pr->n_points == 0) return GFS_OK;
  const int O = pr->obs_start[pr->n_points];
  if (!pr->pos || !pr->ref_Ow || !pr->level_scale || !pr->max_scale) return GFS_ERR_INVALID_ARG;
  if (O > 0 && (!pr->obs_Ow || !pr->obs_flags || (with_desc && !pr->obs_desc))) return GFS_ERR_INVALID_ARG;
  if (!res->best_obs || !res->best_median || !res->normal || !res->min_dist || !res->max_dist || !res->status) return GFS_ERR_INVALID_ARG;
  for (int p = 0; p < pr->n_points; p++) {
    const size_t a = (size_t)pr->obs_start[p];
    const int n = pr->obs_start[p + 1] - pr->obs_start[p];
    const gfs_mp::PointResult r = gfs_mp::update_point(n, n ? pr->obs_Ow + 3 * a : nullptr, with_desc && n ? pr->obs_desc + 32 * a : nullptr,
                                                       n ? pr->obs_flags + a : nullptr, pr->pos + 3 * (size_t)p, pr->ref_Ow + 3 * (size_t)p,
                                                       pr->level_scale[p], pr->max_scale[p], with_desc);
    res->best_obs[p] = r.best_obs;
    res->best_median[p] = r.best_median;
    for (int c = 0; c < 3; c++) res->normal[3 * (size_t)p + c] = r.normal[c];
    res->min_dist[p] = r.min_dist;
    res->max_dist[p] = r.max_dist;
    res->status[p] = (uint8_t)r.status;
  }
  return GFS_OK;
}

template <class Access, class MapPoint, class Solve>
void UpdateMapPoints(Solve&& solve, const std::vector<MapPoint*>& points, int mode = GFS_MAP_POINTS_FULL) {
  const size_t n = points.size();
  if (n == 0) return;
  const bool with_desc = mode == GFS_MAP_POINTS_FULL;
  std::vector<int32_t> obs_start(n + 1, 0);
  std::vector<float> obs_Ow, pos(3 * n, 0.0f), ref_Ow(3 * n, 0.0f), level_scale(n, 1.0f), max_scale(n, 1.0f);
  std::vector<uint8_t> obs_flags, obs_desc;
  std::vector<const uint8_t*> obs_row;  // the key frame's own row of every IN_DESC observation
  for (size_t p = 0; p < n; p++) {
    const MapPoint* pMP = points[p];
    obs_start[p + 1] = obs_start[p];
    if (!pMP || pMP->isBad()) continue;  // if (mbBad) return; (:384, :475)
    const auto observations = pMP->GetObservations();
    if (observations.empty()) continue;  // (:388, :481)
    for (const auto& mit : observations) {
      const auto* pKF = mit.first;
      const int leftIndex = std::get<0>(mit.second), rightIndex = std::get<1>(mit.second);
      if (rightIndex != -1 || (pKF && pKF->NLeft != -1)) throw std::invalid_argument("UpdateMapPoints: single-camera key frames only");
      uint8_t flags = 0;
      float Ow[3] = {0.0f, 0.0f, 0.0f};
      const uint8_t* row = nullptr;
      if (leftIndex != -1) {
        if (!pKF) throw std::invalid_argument("UpdateMapPoints: an observation with an index and no key frame");
        flags |= GFS_MAP_POINT_OBS_IN_NORMAL;
        Access::camera_center(*pKF, Ow);
      }
      if (with_desc && pKF && !pKF->isBad() && leftIndex != -1 && leftIndex < Access::descriptor_rows(*pKF)) {  // (normals only: not asked)
        flags |= GFS_MAP_POINT_OBS_IN_DESC;
        row = Access::descriptors(*pKF) + 32 * (size_t)leftIndex;
      }
      obs_flags.push_back(flags);
      obs_Ow.insert(obs_Ow.end(), Ow, Ow + 3);
      obs_row.push_back(row);
      if (with_desc) {
        obs_desc.resize(obs_desc.size() + 32, 0);
        if (row) std::memcpy(&obs_desc[obs_desc.size() - 32], row, 32);
      }
      obs_start[p + 1]++;
    }
    Access::world_pos(pMP, &pos[3 * p]);
    auto* pRefKF = Access::reference_keyframe(pMP);
    if (!pRefKF || pRefKF->NLeft != -1) throw std::invalid_argument("UpdateMapPoints: a single-camera reference key frame is needed");
    Access::camera_center(*pRefKF, &ref_Ow[3 * p]);
    const auto at = observations.find(pRefKF);
    const int refIndex = at == observations.end() ? 0 : std::get<0>(at->second);  // observations[pRefKF] (:511)
    if (refIndex < 0) throw std::invalid_argument("UpdateMapPoints: the reference key frame observes the point without an index");
    const int level = Access::keys_un(*pRefKF)[refIndex].octave;
    level_scale[p] = pRefKF->mvScaleFactors[level];
    max_scale[p] = pRefKF->mvScaleFactors[pRefKF->mnScaleLevels - 1];
  }
  // (one spare element each: a vector's data() may be null when it is empty)
  obs_Ow.resize(obs_Ow.size() + 3, 0.0f);
  obs_flags.push_back(0);
  obs_desc.resize(obs_desc.size() + 32, 0);
  gfs_map_points_problem pr{};
  pr.n_points = (int32_t)n;
  pr.mode = mode;
  pr.obs_start = obs_start.data();
  pr.obs_Ow = obs_Ow.data();
  pr.obs_desc = with_desc ? obs_desc.data() : nullptr;
  pr.obs_flags = obs_flags.data();
  pr.pos = pos.data();
  pr.ref_Ow = ref_Ow.data();
  pr.level_scale = level_scale.data();
  pr.max_scale = max_scale.data();
  std::vector<int32_t> best_obs(n, -1), best_median(n, -1);
  std::vector<float> normal(3 * n, 0.0f), min_dist(n, 0.0f), max_dist(n, 0.0f);
  std::vector<uint8_t> status(n, 0);
  gfs_map_points_result res{best_obs.data(), best_median.data(), normal.data(), min_dist.data(), max_dist.data(), status.data()};
  check(solve(&pr, &res), "gfs_map_points_update");
  for (size_t p = 0; p < n; p++) {
    MapPoint* pMP = points[p];
    if (status[p] & GFS_MAP_POINT_DESC_SET) Access::set_descriptor(pMP, obs_row[(size_t)obs_start[p] + (size_t)best_obs[p]]);
    if (status[p] & GFS_MAP_POINT_NORMAL_SET) Access::set_normal_and_depth(pMP, &normal[3 * p], min_dist[p], max_dist[p]);
  }
}

// The map-point loop of LocalMapping::ProcessNewKeyFrame (:439-454): the first pass adds the observations and fills
// mlpRecentAddedMapPoints exactly as the loop does; the points that took the first branch are then updated in one call (a point
// listed twice takes the else branch the second time, so no point is updated before its last AddObservation of this loop).
// ComputeBoW, UpdateConnections and Atlas::AddKeyFrame stay with the caller.  If the gather of the second step throws (a two-camera
// observation, a point without a reference key frame), the first pass has already happened: the observations are added and
// mlpRecentAddedMapPoints is filled, and no point has been updated; the caller is left with a half-processed key frame.
template <class Access, class KeyFrame, class MapPoint, class Solve>
void ProcessNewKeyFrame(Solve&& solve, KeyFrame* pCurrentKF, std::list<MapPoint*>& mlpRecentAddedMapPoints) {
  const std::vector<MapPoint*> vpMapPointMatches = pCurrentKF->GetMapPointMatches();
  std::vector<MapPoint*> added;
  for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (pMP) {
      if (!pMP->isBad()) {
        if (!pMP->IsInKeyFrame(pCurrentKF)) {
          pMP->AddObservation(pCurrentKF, (int)i);
          added.push_back(pMP);
        } else {  // this can only happen for new stereo points inserted by the Tracking
          mlpRecentAddedMapPoints.push_back(pMP);
        }
      }
    }
  }
  UpdateMapPoints<Access>(solve, added, GFS_MAP_POINTS_FULL);
}

// the numeric core of the map-point update on the GPU: one handle, its reserve grown to the largest call seen
class MapPointUpdater {
 public:
  explicit MapPointUpdater(int max_points = 4096, int max_observations = 65536, int device = 0)
      : device_(device), points_(max_points), obs_(max_observations) {
    check(gfs_map_points_create(device_, points_, obs_, &h_), "gfs_map_points_create");
  }
  ~MapPointUpdater() { gfs_map_points_destroy(h_); }
  MapPointUpdater(const MapPointUpdater&) = delete;
  MapPointUpdater& operator=(const MapPointUpdater&) = delete;
  int solve(const gfs_map_points_problem* p, gfs_map_points_result* r) {
    const int n_obs = (p && p->obs_start && p->n_points > 0) ? p->obs_start[p->n_points] : 0;
    if (p && (p->n_points > points_ || n_obs > obs_)) {  // the library refuses what exceeds the reserve (it never truncates): grow it first
      const int np = std::max(p->n_points, points_), no = std::max(n_obs, obs_);
      gfs_map_points* bigger = nullptr;
      check(gfs_map_points_create(device_, np, no, &bigger), "gfs_map_points_create");
      gfs_map_points_destroy(h_);
      h_ = bigger;
      points_ = np;
      obs_ = no;
    }
    return gfs_map_points_update(h_, p, r);
  }
  auto solver() {
    return [this](const gfs_map_points_problem* p, gfs_map_points_result* r) { return solve(p, r); };
  }

 private:
  gfs_map_points* h_ = nullptr;
  int device_ = 0, points_ = 0, obs_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------------
// Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, bool pbICPFlag, Map* pMap, int& num_fixedKF,
//                                  int& num_OptKF, int& num_MPs, int& num_edges)          reference src/Optimizer.cc:1588-2040
// as real code around the flat solver: the pointer-graph gather (:1592-1660), the vertices and edges of the g2o graph flattened
// into a gfs_lba_problem in the reference's creation order (:1686-1721, 1816-1952), the stop-flag checks (:1679, 1955-1956),
// the chi2 / depth classification (:1961-1999) and the write-back under mMutexMapUpdate (:2003-2039).
//
// It is a template over the reference's own classes: KeyFrame, MapPoint and Map are used through exactly the members the
// reference function uses (mnId, mnBALocalForKF, mnBAFixedForKF, isBad(), GetMap(), GetVectorCovisibleKeyFrames(),
// GetMapPointMatches(), GetObservations(), mvKeysUn[i].pt / .octave, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf, mpCamera2,
// EraseMapPointMatch(), EraseObservation(), UpdateNormalAndDepth(), GetInitKFid(), mMutexMapUpdate, IncreaseChangeIndex(),
// msOptKFs / msFixedKFs).  The four places that touch Sophus / Eigen value types go through `Access`:
//     static void pose(const KeyFrame*, float q_xyzw[4], float t[3]);        // GetPose(): unit_quaternion(), translation()
//     static void set_pose(KeyFrame*, const float q_xyzw[4], const float t[3]);   // SetPose(Sophus::SE3f(q, t))
//     static void world_pos(const MapPoint*, float p[3]);                    // GetWorldPos()
//     static void set_world_pos(MapPoint*, const float p[3]);                // SetWorldPos()
// (INTEGRATION.md section 4 gives the Access for the reference's types; tests/host/lba_adaptor_test.cpp one for plain structs.)
// `solve(problem, solution, stop)` is the numeric core: LocalBundleAdjuster::solve below (gfs_lba_solve on the GPU).
//
// Arithmetic the reference performs on the way in and out, reproduced here:
//   * poses: Sophus::SE3<float> -> g2o::SE3Quat(q.cast<double>(), t.cast<double>()) (the constructor's normalizeRotation() is
//     part of gfs_lba_solve), back through .cast<float>();
//   * points: Eigen::Vector3f -> cast<double>() and back;
//   * observations: kpUn.pt.x, kpUn.pt.y, mvuRight[idx] are floats assigned to doubles;
//   * information: Identity * invSigma2 with `const float& invSigma2` -> the float value as a double;
//   * Huber deltas: `const float thHuberMono = sqrt(5.991)` -> (double)(float)sqrt(5.991), same for sqrt(7.815).
// Not supported (GFS_ERR_UNSUPPORTED is raised): key-frames with a second camera (mpCamera2, EdgeSE3ProjectXYZToBody
// :1906-1949).  The ICP block :1762-1814 is dead code in the reference and has no counterpart.
// ------------------------------------------------------------------------------------------------------------------------
struct LbaFlat {  // the flattened graph, in the reference's vertex / edge creation order
  std::vector<double> pose_q, pose_t, points, edge_obs, edge_inv_sigma2;
  std::vector<uint8_t> pose_fixed, edge_stereo;
  std::vector<int32_t> edge_pose, edge_point;
  gfs_lba_problem problem{};
  void finish(double fx, double fy, double cx, double cy, double bf) {
    problem.n_poses = (int32_t)pose_fixed.size();
    problem.n_points = (int32_t)(points.size() / 3);
    problem.n_edges = (int32_t)edge_pose.size();
    problem.pose_q = pose_q.data();
    problem.pose_t = pose_t.data();
    problem.pose_fixed = pose_fixed.data();
    problem.points = points.data();
    problem.edge_pose = edge_pose.data();
    problem.edge_point = edge_point.data();
    problem.edge_obs = edge_obs.data();
    problem.edge_inv_sigma2 = edge_inv_sigma2.data();
    problem.edge_stereo = edge_stereo.data();
    problem.fx = fx;
    problem.fy = fy;
    problem.cx = cx;
    problem.cy = cy;
    problem.bf = bf;
    const float thHuberMono = (float)std::sqrt(5.991), thHuberStereo = (float)std::sqrt(7.815);  // src/Optimizer.cc:1728-1729
    problem.huber_mono = thHuberMono;
    problem.huber_stereo = thHuberStereo;
    problem.iterations = 10;  // optimizer.optimize(10), :1959
  }
};

// `solve` is called as solve(problem, solution, pbStopFlag), or -- when it takes them -- with two more arguments: the key-frame of
// every pose in the problem's pose order (lLocalKeyFrames in list order, then lFixedCameras) and the number of local key-frames.
// LocalVisualLidarBA (below) gathers its per-key-frame data through them.
// `update_points`, when given, is a map-point solver (MapPointUpdater::solver(), or map_points_update_host): the write-back then runs
// UpdateNormalAndDepth for all local map points in one normals-only call after the poses and positions are set (exact: a point's
// update reads its own position and the camera centres, and writes what no other point's update reads); `Access` then needs the
// members of UpdateMapPoints too.
template <class Access, class KeyFrame, class MapPoint, class Map, class Solve, class UpdatePoints = PerPointUpdate>
void LocalBundleAdjustment(Solve&& solve, KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF,
                           int& /*num_MPs: never written by the reference either*/, int& num_edges,
                           UpdatePoints&& update_points = UpdatePoints()) {
  constexpr bool kPerPoint = std::is_same<typename std::decay<UpdatePoints>::type, PerPointUpdate>::value;
  // ---- Local KeyFrames: first breadth search from the current key-frame (:1592-1607)
  std::list<KeyFrame*> lLocalKeyFrames;
  lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  Map* pCurrentMap = pKF->GetMap();
  const std::vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (int i = 0, iend = (int)vNeighKFs.size(); i < iend; i++) {
    KeyFrame* pKFi = vNeighKFs[i];
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lLocalKeyFrames.push_back(pKFi);
  }
  // ---- Local MapPoints seen in local key-frames (:1609-1634)
  num_fixedKF = 0;
  std::list<MapPoint*> lLocalMapPoints;
  for (KeyFrame* pKFi : lLocalKeyFrames) {
    if (pKFi->mnId == pMap->GetInitKFid()) num_fixedKF = 1;
    std::vector<MapPoint*> vpMPs = pKFi->GetMapPointMatches();
    for (MapPoint* pMP : vpMPs)
      if (pMP)
        if (!pMP->isBad() && pMP->GetMap() == pCurrentMap)
          if (pMP->mnBALocalForKF != pKF->mnId) {
            lLocalMapPoints.push_back(pMP);
            pMP->mnBALocalForKF = pKF->mnId;
          }
  }
  // ---- Fixed key-frames: see local MapPoints but are not local (:1636-1660)
  std::list<KeyFrame*> lFixedCameras;
  for (MapPoint* pMP : lLocalMapPoints) {
    auto observations = pMP->GetObservations();  // std::map<KeyFrame*, std::tuple<int, int>>
    for (auto mit = observations.begin(), mend = observations.end(); mit != mend; ++mit) {
      KeyFrame* pKFi = mit->first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
      }
    }
  }
  num_fixedKF = (int)lFixedCameras.size() + num_fixedKF;
  if (num_fixedKF == 0) return;  // "LM-LBA: There are 0 fixed KF in the optimizations, LBA aborted" (:1662-1667)

  // ---- vertices (:1686-1721): pose index = creation order, local key-frames first
  LbaFlat F;
  std::map<const KeyFrame*, int32_t> pose_index;  // == optimizer.vertex(pKFi->mnId) != NULL
  std::vector<KeyFrame*> pose_kf;                  // the key-frame of every pose, in pose order
  pCurrentMap->msOptKFs.clear();
  pCurrentMap->msFixedKFs.clear();
  auto add_pose = [&](KeyFrame* pKFi, bool fixed) {
    float q[4], t[3];
    Access::pose(pKFi, q, t);
    pose_index[pKFi] = (int32_t)F.pose_fixed.size();
    pose_kf.push_back(pKFi);
    for (int k = 0; k < 4; k++) F.pose_q.push_back((double)q[k]);  // .cast<double>()
    for (int k = 0; k < 3; k++) F.pose_t.push_back((double)t[k]);
    F.pose_fixed.push_back(fixed ? 1 : 0);
  };
  for (KeyFrame* pKFi : lLocalKeyFrames) {
    add_pose(pKFi, pKFi->mnId == pMap->GetInitKFid());  // vSE3->setFixed(pKFi->mnId == pMap->GetInitKFid())
    pCurrentMap->msOptKFs.insert(pKFi->mnId);
  }
  num_OptKF = (int)lLocalKeyFrames.size();
  for (KeyFrame* pKFi : lFixedCameras) {
    add_pose(pKFi, true);
    pCurrentMap->msFixedKFs.insert(pKFi->mnId);
  }
  // ---- MapPoint vertices and edges (:1816-1952).  The mono, body and stereo edges live in three vectors in the reference and
  //      are classified in that order afterwards; here every edge records its kind and (key-frame, point).
  struct EdgeRef {
    KeyFrame* kf;
    MapPoint* mp;
  };
  std::vector<EdgeRef> vpEdgesMono, vpEdgesStereo;
  std::vector<int32_t> mono_edge, stereo_edge;  // flat edge index of the k-th mono / stereo edge
  int nEdges = 0;
  int32_t point_index = 0;
  for (MapPoint* pMP : lLocalMapPoints) {
    float X[3];
    Access::world_pos(pMP, X);
    for (int k = 0; k < 3; k++) F.points.push_back((double)X[k]);
    const auto observations = pMP->GetObservations();
    for (auto mit = observations.begin(), mend = observations.end(); mit != mend; ++mit) {
      KeyFrame* pKFi = mit->first;
      if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) {
        const int leftIndex = std::get<0>(mit->second);
        const auto pit = pose_index.find(pKFi);
        if (leftIndex != -1) {
          const bool stereo = pKFi->mvuRight[leftIndex] >= 0;
          if (pit != pose_index.end()) {  // optimizer.vertex(pKFi->mnId) == NULL -> continue
            const auto& kpUn = pKFi->mvKeysUn[leftIndex];
            F.edge_pose.push_back(pit->second);
            F.edge_point.push_back(point_index);
            F.edge_obs.push_back((double)kpUn.pt.x);
            F.edge_obs.push_back((double)kpUn.pt.y);
            F.edge_obs.push_back(stereo ? (double)pKFi->mvuRight[leftIndex] : 0.0);
            const float& invSigma2 = pKFi->mvInvLevelSigma2[kpUn.octave];
            F.edge_inv_sigma2.push_back((double)invSigma2);
            F.edge_stereo.push_back(stereo ? 1 : 0);
            (stereo ? vpEdgesStereo : vpEdgesMono).push_back(EdgeRef{pKFi, pMP});
            (stereo ? stereo_edge : mono_edge).push_back((int32_t)F.edge_pose.size() - 1);
            nEdges++;
          } else {
            continue;  // (the reference's `continue` also skips the second-camera block of this observation)
          }
        }
        if (pKFi->mpCamera2 && std::get<1>(mit->second) != -1)
          throw std::runtime_error("LocalBundleAdjustment: second-camera observations (EdgeSE3ProjectXYZToBody) are not supported");
      }
    }
    point_index++;
  }
  num_edges = nEdges;
  if (pbStopFlag)
    if (*pbStopFlag) return;  // :1955-1956
  F.finish(pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf);

  // ---- optimizer.initializeOptimization(); optimizer.optimize(10);
  std::vector<double> out_q(F.pose_q.size()), out_t(F.pose_t.size()), out_p(F.points.size()), chi2((size_t)std::max(nEdges, 1));
  std::vector<uint8_t> depth_pos((size_t)std::max(nEdges, 1));
  gfs_lba_solution S{};
  S.pose_q = out_q.data();
  S.pose_t = out_t.data();
  S.points = out_p.data();
  S.edge_chi2 = chi2.data();
  S.edge_depth_positive = depth_pos.data();
  if constexpr (std::is_invocable_v<Solve&, const gfs_lba_problem&, gfs_lba_solution&, const bool*, const std::vector<KeyFrame*>&, int>) {
    if (!solve(F.problem, S, pbStopFlag, static_cast<const std::vector<KeyFrame*>&>(pose_kf), num_OptKF)) return;
  } else {
    if (!solve(F.problem, S, pbStopFlag)) return;
  }

  // ---- check inlier observations (:1961-1999): mono edges first, then stereo, each in creation order
  std::vector<std::pair<KeyFrame*, MapPoint*>> vToErase;
  vToErase.reserve(vpEdgesMono.size() + vpEdgesStereo.size());
  for (size_t i = 0; i < vpEdgesMono.size(); i++) {
    MapPoint* pMP = vpEdgesMono[i].mp;
    if (pMP->isBad()) continue;
    const int32_t e = mono_edge[i];
    if (chi2[e] > 5.991 || !depth_pos[e]) vToErase.push_back(std::make_pair(vpEdgesMono[i].kf, pMP));
  }
  for (size_t i = 0; i < vpEdgesStereo.size(); i++) {
    MapPoint* pMP = vpEdgesStereo[i].mp;
    if (pMP->isBad()) continue;
    const int32_t e = stereo_edge[i];
    if (chi2[e] > 7.815 || !depth_pos[e]) vToErase.push_back(std::make_pair(vpEdgesStereo[i].kf, pMP));
  }
  // ---- write-back under the map mutex (:2001-2039)
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  for (size_t i = 0; i < vToErase.size(); i++) {
    KeyFrame* pKFi = vToErase[i].first;
    MapPoint* pMPi = vToErase[i].second;
    pKFi->EraseMapPointMatch(pMPi);
    pMPi->EraseObservation(pKFi);
  }
  {
    int32_t k = 0;
    for (KeyFrame* pKFi : lLocalKeyFrames) {  // SE3quat.rotation().cast<float>(), translation().cast<float>()
      float q[4], t[3];
      for (int c = 0; c < 4; c++) q[c] = (float)out_q[4 * (size_t)k + c];
      for (int c = 0; c < 3; c++) t[c] = (float)out_t[3 * (size_t)k + c];
      Access::set_pose(pKFi, q, t);
      k++;
    }
  }
  {
    int32_t k = 0;
    for (MapPoint* pMP : lLocalMapPoints) {
      float X[3];
      for (int c = 0; c < 3; c++) X[c] = (float)out_p[3 * (size_t)k + c];
      Access::set_world_pos(pMP, X);
      if constexpr (kPerPoint) pMP->UpdateNormalAndDepth();
      k++;
    }
    if constexpr (!kPerPoint) {
      const std::vector<MapPoint*> vpLocal(lLocalMapPoints.begin(), lLocalMapPoints.end());
      UpdateMapPoints<Access>(update_points, vpLocal, GFS_MAP_POINTS_NORMALS_ONLY);
    }
  }
  pMap->IncreaseChangeIndex();
}

template <class Access, class KeyFrame, class Map>
void LocalBundleAdjuster::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF,
                                                int& num_MPs, int& num_edges) {
  using MapPoint = typename std::remove_pointer<typename decltype(pKF->GetMapPointMatches())::value_type>::type;
  gfs_host::LocalBundleAdjustment<Access, KeyFrame, MapPoint, Map>(
      [this](const gfs_lba_problem& p, gfs_lba_solution& s, const bool* stop) { return this->solve(p, s, stop); }, pKF, pbStopFlag,
      pMap, num_fixedKF, num_OptKF, num_MPs, num_edges);
}

template <class Access, class KeyFrame, class Map, class UpdatePoints>
void LocalBundleAdjuster::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF,
                                                int& num_MPs, int& num_edges, UpdatePoints&& update_points) {
  using MapPoint = typename std::remove_pointer<typename decltype(pKF->GetMapPointMatches())::value_type>::type;
  gfs_host::LocalBundleAdjustment<Access, KeyFrame, MapPoint, Map>(
      [this](const gfs_lba_problem& p, gfs_lba_solution& s, const bool* stop) { return this->solve(p, s, stop); }, pKF, pbStopFlag,
      pMap, num_fixedKF, num_OptKF, num_MPs, num_edges, update_points);
}

// ------------------------------------------------------------------------------------------------------------------------
// Optimizer::LocalVisualLidarBA(KeyFrame* pKF, PointCloud::Ptr laserCloudSurfFromMapDS, bool* pbStopFlag, Map* pMap, int& num_fixedKF,
//                               int& num_OptKF, int& num_MPs, int& num_edges)                   reference src/Optimizer.cc:1101-1587
// LocalBundleAdjustment line for line (the gather, the stop flag, the classification and the write-back above are reused as they
// are) plus the lidar edges of :1327-1362.  Per pose, in pose order, it hands the numeric core what those need: pose_local (1 for the
// lLocalKeyFrames, 0 for lFixedCameras), pKFi->mnMatchesInliers and pKFi->mpPointCloudDownsampled, the clouds concatenated in
// lLocalKeyFrames order (a fixed camera never gets edges, so its cloud is not read).  The library applies the 75-inlier and 50-point
// gates.  `Access` adds to LocalBundleAdjustment's four functions
//     static int matches_inliers(const KeyFrame*);                          // pKFi->mnMatchesInliers
//     static const float* cloud(const KeyFrame*, int* n);                   // mpPointCloudDownsampled packed to [n][3] floats
// `solve(problem, lidar, solution, pbStopFlag)`: LocalBundleAdjuster::solve_lidar on the GPU (lidar.map is set there).
// num_edges counts the reprojection edges only (the lidar edges increment the reference's unused edge_num).
// ------------------------------------------------------------------------------------------------------------------------
struct LbaLidarFlat {  // the lidar half of the window, in pose order
  std::vector<uint8_t> pose_local;
  std::vector<int32_t> matches_inliers, cloud_begin;
  std::vector<float> cloud;
  gfs_lba_lidar lidar{};
};

template <class Access, class KeyFrame, class MapPoint, class Map, class SolveLidar>
void LocalVisualLidarBA(SolveLidar&& solve, KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs,
                        int& num_edges) {
  LbaLidarFlat L;
  LocalBundleAdjustment<Access, KeyFrame, MapPoint, Map>(
      [&](const gfs_lba_problem& p, gfs_lba_solution& s, const bool* stop, const std::vector<KeyFrame*>& pose_kf, int n_local) {
        L.cloud_begin.assign(1, 0);
        for (size_t i = 0; i < pose_kf.size(); i++) {
          const bool local = (int)i < n_local;
          int n = 0;
          const float* c = local ? Access::cloud(pose_kf[i], &n) : nullptr;
          if (!c || n < 0) n = 0;
          L.pose_local.push_back(local ? 1 : 0);
          L.matches_inliers.push_back(local ? (int32_t)Access::matches_inliers(pose_kf[i]) : 0);
          L.cloud.insert(L.cloud.end(), c, c + 3 * (size_t)n);
          L.cloud_begin.push_back(L.cloud_begin.back() + n);
        }
        L.lidar.pose_local = L.pose_local.data();
        L.lidar.matches_inliers = L.matches_inliers.data();
        L.lidar.cloud_begin = L.cloud_begin.data();
        L.lidar.cloud = L.cloud.data();
        L.lidar.two_camera = 0;  // (observations of a second camera are refused by the gather, as in LocalBundleAdjustment)
        return solve(p, static_cast<const gfs_lba_lidar&>(L.lidar), s, stop);
      },
      pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges);
}

template <class Access, class KeyFrame, class Map>
void LocalBundleAdjuster::LocalVisualLidarBA(KeyFrame* pKF, const float* map_xyz, int n_map, bool* pbStopFlag, Map* pMap, int& num_fixedKF,
                                             int& num_OptKF, int& num_MPs, int& num_edges) {
  using MapPoint = typename std::remove_pointer<typename decltype(pKF->GetMapPointMatches())::value_type>::type;
  if (!map_ || n_map > map_cap_) {
    gfs_lidar_map_destroy(map_);
    map_ = nullptr;
    map_cap_ = std::max(n_map, 5);
    check(gfs_lidar_map_create(device_, map_cap_, &map_), "gfs_lidar_map_create");
  }
  check(gfs_lidar_map_set(map_, map_xyz, n_map), "gfs_lidar_map_set");
  gfs_host::LocalVisualLidarBA<Access, KeyFrame, MapPoint, Map>(
      [this](const gfs_lba_problem& p, const gfs_lba_lidar& lidar, gfs_lba_solution& s, const bool* stop) {
        return this->solve_lidar(p, lidar, s, stop);
      },
      pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges);
}

template <class Access, class KeyFrame, class Map>
void LocalBundleAdjuster::LocalVisualLidarBA(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs,
                                             int& num_edges) {
  using MapPoint = typename std::remove_pointer<typename decltype(pKF->GetMapPointMatches())::value_type>::type;
  if (!map_) throw std::runtime_error("LocalVisualLidarBA: no local map (BuildLocalMap first)");
  gfs_host::LocalVisualLidarBA<Access, KeyFrame, MapPoint, Map>(
      [this](const gfs_lba_problem& p, const gfs_lba_lidar& lidar, gfs_lba_solution& s, const bool* stop) {
        return this->solve_lidar(p, lidar, s, stop);
      },
      pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges);
}

// gms_matcher(kp1, size1, kp2, size2, matches).GetInlierMask(mask, false, false) (reference Thirdparty/GMS/include/gms_matcher.h;
// the filter SearchWithGMS applies to the brute-force matches, src/ORBmatcher.cc:761-762)
class GmsMatcher {
 public:
  explicit GmsMatcher(int max_keypoints = 8192, int device = 0) { check(gfs_gms_create(device, max_keypoints, 1, &h_), "gfs_gms_create"); }
  ~GmsMatcher() { gfs_gms_destroy(h_); }
  // matches[i] = (queryIdx, trainIdx); returns the number of inliers, mask[i] = vbInliers[i]
  int GetInlierMask(const gfs_keypoint* kp1, int n1, int w1, int h1, const gfs_keypoint* kp2, int n2, int w2, int h2,
                    const std::vector<int32_t>& query_idx, const std::vector<int32_t>& train_idx, std::vector<uint8_t>& mask) {
    const int n = (int)query_idx.size();
    mask.assign((size_t)std::max(n, 1), 0);
    gfs_gms_problem p{n1, n2, kp1, kp2, w1, h1, w2, h2, n, query_idx.data(), train_idx.data()};
    uint8_t* mp = mask.data();
    int32_t nin = 0;
    check(gfs_gms_inlier_mask(h_, &p, 1, &mp, &nin), "gfs_gms_inlier_mask");
    mask.resize((size_t)n);
    return nin;
  }

 private:
  gfs_gms* h_ = nullptr;
};

// The optical-flow front end: cv::buildOpticalFlowPyramid (reference src/Frame.cc:373), ORBmatcher::fbKltTracking
// (src/ORBmatcher.cc:2186-2297 == Tracking::fbKltTracking, src/Tracking.cc:3262-3366).  A Pyramid is what Frame::mImGray holds in
// the reference (a std::vector<cv::Mat>), kept in HBM; build it once per frame, use it as `cur` and then as `prev`.
// cv::CLAHE on 8-bit single-channel images (cv::createCLAHE(3.0, cv::Size(8, 8)), reference src/Frame.cc:366-369, 499-500).
// residual_variant: GFS_CLAHE_RESIDUAL_STEPPED (OpenCV >= 3.4) or GFS_CLAHE_RESIDUAL_CONTIGUOUS (OpenCV <= 3.3).
class Clahe {
 public:
  Clahe(int max_width, int max_height, double clip_limit = 3.0, int tiles_x = 8, int tiles_y = 8,
        int residual_variant = GFS_CLAHE_RESIDUAL_STEPPED, int device = 0) {
    gfs_clahe_config cfg;
    gfs_clahe_default_config(&cfg);
    cfg.clip_limit = clip_limit;
    cfg.tiles_x = tiles_x;
    cfg.tiles_y = tiles_y;
    cfg.residual_variant = residual_variant;
    check(gfs_clahe_create(device, max_width, max_height, 1, &cfg, &h_), "gfs_clahe_create");
  }
  ~Clahe() { gfs_clahe_destroy(h_); }
  Clahe(const Clahe&) = delete;
  Clahe& operator=(const Clahe&) = delete;
  // clahe->apply(src, dst); dst may be src
  void apply(const uint8_t* src, int width, int height, int stride, uint8_t* dst, int dst_stride) {
    check(gfs_clahe_apply(h_, &src, width, height, stride, 1, &dst, dst_stride), "gfs_clahe_apply");
  }
  gfs_clahe* handle() const { return h_; }

 private:
  gfs_clahe* h_ = nullptr;
};

class KltTracker {
 public:
  class Pyramid {
   public:
    explicit Pyramid(KltTracker& t) : t_(t) { check(gfs_klt_pyramid_create(t.h_, &p_), "gfs_klt_pyramid_create"); }
    ~Pyramid() { gfs_klt_pyramid_destroy(p_); }
    Pyramid(const Pyramid&) = delete;
    Pyramid& operator=(const Pyramid&) = delete;
    // cv::buildOpticalFlowPyramid(image, pyr, Size(win, win), max_level)
    void build(const uint8_t* image, int stride) { check(gfs_klt_build_pyramid(t_.h_, p_, &image, stride, 1), "gfs_klt_build_pyramid"); }
    // clahe->apply(image, image); cv::buildOpticalFlowPyramid(image, pyr, ...) in one device pass (src/Frame.cc:366-373): `image`
    // itself is left alone; equalized_out (rows of `stride` bytes, may be `image`) receives Frame::image when it is not null
    void build(const uint8_t* image, int stride, Clahe& clahe, uint8_t* equalized_out = nullptr) {
      check(gfs_klt_build_pyramid_clahe(t_.h_, clahe.handle(), p_, &image, stride, 1, equalized_out ? &equalized_out : nullptr, stride),
            "gfs_klt_build_pyramid_clahe");
    }
    gfs_klt_pyramid* get() const { return p_; }

   private:
    KltTracker& t_;
    gfs_klt_pyramid* p_ = nullptr;
  };

  KltTracker(int width, int height, int nwinsize, int max_level = 3, int max_points = 8192, int device = 0) {
    check(gfs_klt_create(device, width, height, nwinsize, max_level, 1, max_points, &h_), "gfs_klt_create");
  }
  ~KltTracker() { gfs_klt_destroy(h_); }
  gfs_klt* handle() const { return h_; }
  // fbKltTracking(vprevpyr, vcurpyr, nwinsize, nbpyrlvl, ferr, fmax_fbklt_dist, vkps, vpriorkps, vkpstatus): points are
  // (x, y) float pairs as cv::Point2f; vpriorkps is updated in place, vkpstatus is resized to vkps.size() / 2.
  void fbKltTracking(const Pyramid& vprevpyr, const Pyramid& vcurpyr, int nbpyrlvl, float ferr, float fmax_fbklt_dist,
                     const std::vector<float>& vkps, std::vector<float>& vpriorkps, std::vector<uint8_t>& vkpstatus) {
    const int32_t n = (int32_t)(vkps.size() / 2);
    vkpstatus.assign((size_t)std::max(n, 1), 0);
    if (n == 0) {  // src/ORBmatcher.cc:2197-2199: nothing is touched
      vkpstatus.clear();
      return;
    }
    const float* kp = vkps.data();
    float* pr = vpriorkps.data();
    uint8_t* st = vkpstatus.data();
    int32_t good = 0;
    check(gfs_klt_fb_track(h_, vprevpyr.get(), vcurpyr.get(), 1, &n, &kp, &pr, &st, &good, nbpyrlvl, ferr, fmax_fbklt_dist), "gfs_klt_fb_track");
    vkpstatus.resize((size_t)n);
  }

 private:
  gfs_klt* h_ = nullptr;
};

// cv::findFundamentalMat(points1, points2, cv::FM_RANSAC, threshold, confidence, status), 8 or more points (reference call
// sites src/ORBmatcher.cc:236, 2399, 2463; src/Tracking.cc:1974)
class FundamentalMatcher {
 public:
  explicit FundamentalMatcher(int max_points = 8192, int device = 0) { check(gfs_fmat_create(device, max_points, 1, &h_), "gfs_fmat_create"); }
  ~FundamentalMatcher() { gfs_fmat_destroy(h_); }
  // points: (x, y) float pairs as cv::Point2f; returns the consensus size, status[i] = 0 / 1, F = row-major 3x3 (zeros: no model)
  int findFundamentalMat(const std::vector<float>& points1, const std::vector<float>& points2, double threshold, double confidence,
                         std::vector<uint8_t>& status, double F[9] = nullptr) {
    const int32_t n = (int32_t)(points1.size() / 2);
    status.assign((size_t)std::max(n, 1), 0);
    const float* a = points1.data();
    const float* b = points2.data();
    uint8_t* st = status.data();
    int32_t n_in = 0;
    check(gfs_find_fundamental_ransac(h_, 1, &n, &a, &b, threshold, confidence, 1000, &st, F, &n_in), "gfs_find_fundamental_ransac");
    status.resize((size_t)n);
    return n_in;
  }

 private:
  gfs_fmat* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByProjectionWithOF(CurrentFrame, LastFrame, mask, th, winsize, F_THRESHOLD, DIST_THRESHOLD, bMono)
// (reference src/ORBmatcher.cc:2303-2497): the bookkeeping around the two forward-backward KLT passes and their F checks —
// prior projection of the last frame's map points into the current frame (:2320-2373), the occupancy mask (cv::circle filled
// discs, :2296-2302, 2326-2332), the hand-over of failed 3-D tracks to the 2-D pass (:2434-2442), the tracked key-point lists
// that the caller passes to Frame::AddPts (:2444, 2492) — on plain arrays.  The numeric parts run on the GPU through KltTracker
// and FundamentalMatcher above.  What stays with the caller (it touches Frame / MapPoint members only): mnLastFrameSeen of the
// tracked map points, track_feature_pts_, the two AddPts calls and AssignFeaturesToGrid.
// ------------------------------------------------------------------------------------------------------------------------
struct OfFrames {
  int n_last = 0;                         // LastFrame.mvpMapPoints.size() == LastFrame.mvKeys.size()
  const gfs_keypoint* last_keys = nullptr;  // LastFrame.mvKeys (cv::KeyPoint layout)
  const uint8_t* last_has_mp = nullptr;   // mvpMapPoints[i] != nullptr
  const uint8_t* last_mp_bad = nullptr;   // mp->isBad()
  const uint8_t* last_outlier = nullptr;  // LastFrame.mvbOutlier[i]
  const float* last_mp_xw = nullptr;      // [n_last][3] mp->GetWorldPos()
  int n_cur = 0;
  const gfs_keypoint* cur_keys = nullptr;  // CurrentFrame.mvKeys
  float Tcw_q[4] = {0, 0, 0, 1}, Tcw_t[3] = {0, 0, 0};  // CurrentFrame.GetPose(): unit quaternion (x, y, z, w), translation
  float fx = 0, fy = 0, cx = 0, cy = 0, min_x = 0, max_x = 0, min_y = 0, max_y = 0;  // CurrentFrame.fx ... mnMaxY
  int img_w = 0, img_h = 0;               // CurrentFrame.image.cols / rows
};
struct OfTracked {                         // one AddPts call: tracked_kps[i] continues LastFrame key-point last_index[i]
  std::vector<gfs_keypoint> kps;
  std::vector<int32_t> last_index;
};

// cv::circle(mask, pt, radius, Scalar(255), FILLED) on CV_8UC1 (OpenCV 4.5.4 imgproc/src/drawing.cpp Circle(): the midpoint
// recurrence, filled with horizontal spans, clipped to the image; the float centre converts with cvRound like Point2f -> Point)
inline void fill_circle_u8(uint8_t* img, int rows, int cols, int stride, float fx_, float fy_, int radius) {
  const int cx = (int)std::lrint(fx_), cy = (int)std::lrint(fy_);  // saturate_cast<int>(float): round half to even
  auto hline = [&](int y, int x0, int x1) {
    if (y < 0 || y >= rows) return;
    x0 = std::max(x0, 0);
    x1 = std::min(x1, cols - 1);
    for (int x = x0; x <= x1; x++) img[(size_t)y * stride + x] = 255;
  };
  int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
  while (dx >= dy) {
    hline(cy - dy, cx - dx, cx + dx);
    hline(cy + dy, cx - dx, cx + dx);
    hline(cy - dx, cx - dy, cx + dy);
    hline(cy + dx, cx - dy, cx + dy);
    dy++;
    err += plus;
    plus += 2;
    const int m = (err <= 0) - 1;
    err -= minus & m;
    dx += m;
    minus -= m & 2;
  }
}

// returns nbgood; mask: img_h x img_w bytes (stride img_w), updated like the reference's cv::Mat& mask
inline int SearchByProjectionWithOF(KltTracker& klt, FundamentalMatcher& fmat, const KltTracker::Pyramid& last_pyr,
                                    const KltTracker::Pyramid& cur_pyr, const OfFrames& in, uint8_t* mask, float F_THRESHOLD,
                                    int DIST_THRESHOLD, OfTracked& tracked3d, OfTracked& tracked2d) {
  int nbgood = 0;
  std::vector<int32_t> v3dkpids, v2dkpids;
  std::vector<float> v3dkps, v3dpriors, v2dkps, v2dpriors;  // (x, y) pairs
  tracked3d.kps.clear();
  tracked3d.last_index.clear();
  tracked2d.kps.clear();
  tracked2d.last_index.clear();
  const int W = in.img_w, H = in.img_h;
  for (int i = 0; i < in.n_cur; i++) {  // mask of the key points already extracted in the current frame (:2326-2332)
    const float x = in.cur_keys[i].x, y = in.cur_keys[i].y;
    if (x > 0 && x < W && y > 0 && y < H) mask[(size_t)(int)y * W + (int)x] = 255;  // Mat::at<uchar>(float, float) truncates
  }
  auto push2d = [&](int cnt) {
    const float u = in.last_keys[cnt].x, v = in.last_keys[cnt].y;
    v2dkps.push_back(u);
    v2dkps.push_back(v);
    v2dpriors.push_back(u);
    v2dpriors.push_back(v);
    v2dkpids.push_back(cnt);
  };
  const float qx = in.Tcw_q[0], qy = in.Tcw_q[1], qz = in.Tcw_q[2], qw = in.Tcw_q[3];
  for (int cnt = 0; cnt < in.n_last; cnt++) {
    if (!in.last_has_mp[cnt]) {  // key points without a map point are tracked in the image only
      push2d(cnt);
      continue;
    }
    if (in.last_mp_bad[cnt] || in.last_outlier[cnt]) continue;
    // x3Dc = Tcw * x3Dw (Sophus: unit_quaternion()._transformVector in float: v + w t + q x t, t = 2 q x v)
    const float* X = in.last_mp_xw + 3 * (size_t)cnt;
    const float tx = 2.f * (qy * X[2] - qz * X[1]), ty = 2.f * (qz * X[0] - qx * X[2]), tz = 2.f * (qx * X[1] - qy * X[0]);
    const float xc = X[0] + qw * tx + (qy * tz - qz * ty) + in.Tcw_t[0];
    const float yc = X[1] + qw * ty + (qz * tx - qx * tz) + in.Tcw_t[1];
    const float zc = X[2] + qw * tz + (qx * ty - qy * tx) + in.Tcw_t[2];
    const float invzc = (float)(1.0 / (double)zc);  // `const float invzc = 1.0 / x3Dc(2)`
    const float u = in.fx * xc * invzc + in.cx, v = in.fy * yc * invzc + in.cy;
    if (invzc < 0 || u < in.min_x || u > in.max_x || v < in.min_y || v > in.max_y) {
      push2d(cnt);
      continue;
    }
    v3dkps.push_back(in.last_keys[cnt].x);
    v3dkps.push_back(in.last_keys[cnt].y);
    v3dpriors.push_back(u);
    v3dpriors.push_back(v);
    v3dkpids.push_back(cnt);
  }
  const float nklt_err = 15.f, max_fbklt_dist = 0.5f;
  auto track_and_check = [&](int nbpyrlvl, const std::vector<float>& kps, std::vector<float>& priors, float f_thr,
                             std::vector<uint8_t>& vkpstatus) {
    klt.fbKltTracking(last_pyr, cur_pyr, nbpyrlvl, nklt_err, max_fbklt_dist, kps, priors, vkpstatus);
    std::vector<int32_t> index;
    std::vector<float> un_cur, un_forw;
    for (size_t i = 0; i < vkpstatus.size(); i++)
      if (vkpstatus[i]) {
        index.push_back((int32_t)i);
        un_cur.push_back(kps[2 * i]);
        un_cur.push_back(kps[2 * i + 1]);
        un_forw.push_back(priors[2 * i]);
        un_forw.push_back(priors[2 * i + 1]);
      }
    if (index.size() > 8) {  // cv::findFundamentalMat(un_cur_pts, un_forw_pts, FM_RANSAC, f_thr, 0.99, status)
      std::vector<uint8_t> status;
      fmat.findFundamentalMat(un_cur, un_forw, (double)f_thr, 0.99, status);
      for (size_t i = 0; i < status.size(); i++)
        if (!status[i]) vkpstatus[(size_t)index[i]] = 0;
    }
  };
  // cv::Point(pt.x, pt.y): truncation.  A track that left the image cannot sit next to a key point of the mask: it is not "nearby"
  // (the reference reads mask.at<uchar>() unchecked behind cv's own in-image filtering; here nothing is read outside the buffer).
  auto is_nearby = [&](float x, float y) {
    const int xi = (int)x, yi = (int)y;
    return xi >= 0 && xi < W && yi >= 0 && yi < H && mask[(size_t)yi * W + xi] == 255;
  };
  if (!v3dkpids.empty()) {  // 1st: key points with a map point, prior = projection (3 pyramid levels)
    std::vector<uint8_t> vkpstatus;
    track_and_check(3, v3dkps, v3dpriors, F_THRESHOLD, vkpstatus);
    for (size_t i = 0; i < v3dkpids.size(); i++) {
      if (vkpstatus[i]) {
        gfs_keypoint pt = in.last_keys[v3dkpids[i]];
        pt.x = v3dpriors[2 * i];
        pt.y = v3dpriors[2 * i + 1];
        if (is_nearby(pt.x, pt.y)) continue;
        tracked3d.kps.push_back(pt);
        tracked3d.last_index.push_back(v3dkpids[i]);
        nbgood++;
        fill_circle_u8(mask, H, W, W, pt.x, pt.y, DIST_THRESHOLD);
      } else {
        push2d(v3dkpids[i]);  // not tracked: tried again as a 2-D point
      }
    }
  }
  if (!v2dkpids.empty()) {  // 2nd: image-only tracking (6 pyramid levels requested), F threshold halved
    std::vector<uint8_t> vkpstatus;
    track_and_check(6, v2dkps, v2dpriors, F_THRESHOLD * 0.5f, vkpstatus);
    for (size_t i = 0; i < v2dkpids.size(); i++)
      if (vkpstatus[i]) {
        gfs_keypoint pt = in.last_keys[v2dkpids[i]];
        pt.x = v2dpriors[2 * i];
        pt.y = v2dpriors[2 * i + 1];
        if (is_nearby(pt.x, pt.y)) continue;
        tracked2d.kps.push_back(pt);
        tracked2d.last_index.push_back(v2dkpids[i]);
        fill_circle_u8(mask, H, W, W, pt.x, pt.y, DIST_THRESHOLD);
        nbgood++;
      }
  }
  return nbgood;
}

// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) on flattened frames (reference src/ORBmatcher.cc:1853-2063;
// see INTEGRATION.md §6 for the flattening of Frame / MapPoint)
class ProjectionMatcher {
 public:
  ProjectionMatcher(int max_last = 8192, int max_cur = 4096, int device = 0) { check(gfs_sbp_create(device, max_last, max_cur, 1, &h_), "gfs_sbp_create"); }
  ~ProjectionMatcher() { gfs_sbp_destroy(h_); }
  // cur_match: p.n_cur entries (>= 0 new map point = last-list entry, -1 untouched, -2 reset to NULL); returns nmatches
  int SearchByProjection(const gfs_sbp_problem& p, std::vector<int32_t>& cur_match) {
    cur_match.assign((size_t)std::max(p.n_cur, 1), -1);
    int32_t* ptr = cur_match.data();
    int32_t n = 0;
    check(gfs_search_by_projection(h_, &p, 1, &ptr, &n), "gfs_search_by_projection");
    cur_match.resize((size_t)p.n_cur);
    return n;
  }

 private:
  gfs_sbp* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// void Tracking::SearchLocalPoints()                                                       reference src/Tracking.cc:4294-4359
// as real code around one device call: the first loop (:4296-4310: bad matches dropped, the others marked seen), the gather of
// the local map points that pass `mnLastFrameSeen != F.mnId && !isBad()` (:4320-4321), gfs_search_local_points (Frame::isInFrustum,
// MapPoint::PredictScale, the far-points filter and ORBmatcher::SearchByProjection, src/ORBmatcher.cc:43-206), and the write-back
// of what isInFrustum leaves on a map point (mbTrackInView, mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos, mTrackDepth),
// IncreaseVisible (:4324), mmProjectPoints (:4327-4330) and F.mvpMapPoints[idx] (ORBmatcher.cc:122).  The choice of th (:4335-4353)
// stays with the caller.  Single-camera pinhole frames only: a frame with Nleft != -1 or another camera model throws.
//
// Frame and MapPoint are the reference's own classes, used through the members the reference function uses (F.mvpMapPoints, mnId,
// Nleft, N, mvuRight, mbf, mnMinX .. mnMaxY, mfGridElementWidthInv / HeightInv, mvScaleFactors, mnScaleLevels, mfLogScaleFactor;
// isBad(), IncreaseVisible(), Observations(), mnId, mnLastFrameSeen, mbTrackInView, mbTrackInViewR and the mTrack* fields).  What
// touches Eigen / OpenCV value types or protected members goes through `Access` (INTEGRATION.md section 14 gives it for the
// reference's types; tests/host/local_points_adaptor_test.cpp one for plain structs):
//     static bool is_pinhole(const Frame&);                                    // mpCamera->GetType() == CAM_PINHOLE
//     static void pose(const Frame&, float Rcw[9], float tcw[3], float Ow[3]); // mRcw (row-major), mtcw, mOw
//     static void intrinsics(const Frame&, float k[4]);                        // fx, fy, cx, cy of mpCamera
//     static const gfs_keypoint* keys_un(const Frame&);                        // mvKeysUn.data() (cv::KeyPoint layout)
//     static const uint8_t* descriptors(const Frame&);                         // mDescriptors.data ([N][32], continuous)
//     static void set_project_point(Frame&, unsigned long id, float x, float y);   // mmProjectPoints[id] = cv::Point2f(x, y)
//     static void world_pos(const MapPoint*, float p[3]);                      // GetWorldPos()
//     static void normal(const MapPoint*, float n[3]);                         // GetNormal()
//     static void distances(const MapPoint*, float* min_d, float* max_d);      // mfMinDistance, mfMaxDistance (raw)
//     static void descriptor(const MapPoint*, uint8_t d[32]);                  // GetDescriptor()
// `solve(problem, result)` is the numeric core: LocalPointsSearcher::solve below (gfs_search_local_points on the GPU).  Returns the
// matcher's return value (the reference drops it).
// ------------------------------------------------------------------------------------------------------------------------
constexpr float kSearchLocalPointsViewCosLimit = 0.5f;  // isInFrustum(pMP, 0.5) (:4323)
constexpr float kSearchLocalPointsNNRatio = 0.8f;       // ORBmatcher matcher(0.8) (:4334)

template <class Access, class Frame, class MapPoint, class Solve>
int SearchLocalPoints(Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, float th, bool bFarPoints, float thFarPoints, Solve&& solve) {
  if (F.Nleft != -1 || !Access::is_pinhole(F)) throw std::invalid_argument("SearchLocalPoints: single-camera pinhole frames only");
  // Do not search map points already matched (:4296-4310)
  for (auto vit = F.mvpMapPoints.begin(), vend = F.mvpMapPoints.end(); vit != vend; ++vit) {
    MapPoint* pMP = *vit;
    if (!pMP) continue;
    if (pMP->isBad()) {
      *vit = static_cast<MapPoint*>(nullptr);
    } else {
      pMP->IncreaseVisible();
      pMP->mnLastFrameSeen = F.mnId;
      pMP->mbTrackInView = false;
      pMP->mbTrackInViewR = false;
    }
  }
  // the points isInFrustum is called on (:4320-4321), in list order
  std::vector<MapPoint*> listed;
  listed.reserve(vpLocalMapPoints.size());
  for (MapPoint* pMP : vpLocalMapPoints) {
    if (pMP->mnLastFrameSeen == F.mnId) continue;
    if (pMP->isBad()) continue;
    listed.push_back(pMP);
  }
  const size_t n = listed.size(), nc = (size_t)F.N;
  std::vector<float> xw(3 * n + 3), nrm(3 * n + 3), dmin(n + 1), dmax(n + 1), proj(3 * n + 3), depth(n + 1), vcos(n + 1);
  std::vector<uint8_t> desc(32 * n + 32), has_obs(n + 1), in_view(n + 1), cur_obs(nc + 1);
  std::vector<int32_t> level(n + 1), cur_match(nc + 1, -1);
  for (size_t i = 0; i < n; i++) {
    Access::world_pos(listed[i], &xw[3 * i]);
    Access::normal(listed[i], &nrm[3 * i]);
    Access::distances(listed[i], &dmin[i], &dmax[i]);
    Access::descriptor(listed[i], &desc[32 * i]);
    has_obs[i] = listed[i]->Observations() > 0;
  }
  for (size_t i = 0; i < nc; i++) cur_obs[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0;
  gfs_local_points_problem p{};
  p.n_mp = (int32_t)n;
  p.mp_xw = xw.data();
  p.mp_normal = nrm.data();
  p.mp_min_dist = dmin.data();
  p.mp_max_dist = dmax.data();
  p.mp_desc = desc.data();
  p.mp_has_obs = has_obs.data();
  Access::pose(F, p.Rcw, p.tcw, p.Ow);
  float k[4];
  Access::intrinsics(F, k);
  p.fx = k[0];
  p.fy = k[1];
  p.cx = k[2];
  p.cy = k[3];
  p.bf = F.mbf;
  p.min_x = F.mnMinX;
  p.max_x = F.mnMaxX;
  p.min_y = F.mnMinY;
  p.max_y = F.mnMaxY;
  p.grid_w_inv = F.mfGridElementWidthInv;
  p.grid_h_inv = F.mfGridElementHeightInv;
  p.scale_factors = F.mvScaleFactors.data();
  p.n_levels = F.mnScaleLevels;
  p.log_scale_factor = F.mfLogScaleFactor;
  p.view_cos_limit = kSearchLocalPointsViewCosLimit;
  p.far_points = bFarPoints ? 1 : 0;
  p.th_far_points = thFarPoints;
  p.th = th;
  p.nn_ratio = kSearchLocalPointsNNRatio;
  p.n_cur = (int32_t)nc;
  p.cur_kps_un = Access::keys_un(F);
  p.cur_u_right = F.mvuRight.data();
  p.cur_desc = Access::descriptors(F);
  p.cur_has_mp_obs = cur_obs.data();
  gfs_local_points_result r{};
  r.in_view = in_view.data();
  r.proj = proj.data();
  r.depth = depth.data();
  r.view_cos = vcos.data();
  r.level = level.data();
  r.cur_match = cur_match.data();
  check(solve(p, r), "gfs_search_local_points");
  for (size_t i = 0; i < n; i++) {  // what isInFrustum leaves on the point, then :4324-4330
    MapPoint* pMP = listed[i];
    pMP->mbTrackInView = in_view[i] != 0;
    pMP->mTrackProjX = proj[3 * i];
    pMP->mTrackProjY = proj[3 * i + 1];
    if (!in_view[i]) continue;
    pMP->mTrackProjXR = proj[3 * i + 2];
    pMP->mTrackDepth = depth[i];
    pMP->mnTrackScaleLevel = level[i];
    pMP->mTrackViewCos = vcos[i];
    pMP->IncreaseVisible();
    Access::set_project_point(F, pMP->mnId, pMP->mTrackProjX, pMP->mTrackProjY);
  }
  for (size_t i = 0; i < nc; i++)
    if (cur_match[i] >= 0) F.mvpMapPoints[i] = listed[(size_t)cur_match[i]];
  return r.nmatches;
}

// the numeric core of SearchLocalPoints on the GPU: one handle, its reserve grown to the longest list seen
class LocalPointsSearcher {
 public:
  LocalPointsSearcher(int max_search = 8192, int max_cur = 4096, int device = 0) { check(gfs_sbp_create(device, max_search, max_cur, 1, &h_), "gfs_sbp_create"); }
  ~LocalPointsSearcher() { gfs_sbp_destroy(h_); }
  LocalPointsSearcher(const LocalPointsSearcher&) = delete;
  LocalPointsSearcher& operator=(const LocalPointsSearcher&) = delete;
  int solve(const gfs_local_points_problem& p, gfs_local_points_result& r) {
    if (p.n_mp > reserve_) {  // the library refuses a list beyond the reserve (it never truncates): grow it first
      const int want = std::max(p.n_mp, 2 * reserve_);
      check(gfs_sbp_reserve_local(h_, want), "gfs_sbp_reserve_local");
      reserve_ = want;
    }
    return gfs_search_local_points(h_, &p, 1, &r);
  }
  template <class Access, class Frame, class MapPoint>
  int SearchLocalPoints(Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, float th, bool bFarPoints, float thFarPoints) {
    return gfs_host::SearchLocalPoints<Access>(F, vpLocalMapPoints, th, bFarPoints, thFarPoints,
                                               [this](const gfs_local_points_problem& p, gfs_local_points_result& r) { return solve(p, r); });
  }

 private:
  gfs_sbp* h_ = nullptr;
  int reserve_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------------
// int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th, const bool bRight = false)
//                                                                                          reference src/ORBmatcher.cc:1378-1548
// void LocalMapping::SearchInNeighbors(), from `ORBmatcher matcher;` on                    reference src/LocalMapping.cc:1179-1234
// as real code around gfs_fuse_search.  Inside one Fuse call the per-point search (:1424-1526) reads only data the loop never
// changes (the point's position, normal, distances and descriptor; the key frame's pose, intrinsics, key-points, mvuRight,
// descriptors and level tables), and the loop changes only pointer state, which it reads before the search (:1411-1422) and after it
// (:1529-1544).  So the search of every listed point is done on the device from the entry state, and the decisions are replayed
// here in list order against the live pointer state:
//   gather:  every non-null slot uploads GetWorldPos / GetNormal / mfMinDistance / mfMaxDistance / GetDescriptor; a null slot is
//            flagged.  isBad() and IsInKeyFrame are NOT evaluated here.
//   replay:  per key frame in the reference's order, per point in list order: skip if null, isBad() or IsInKeyFrame(pKF), all live;
//            if the point's descriptor is no longer the uploaded one (pMPinKF->Replace(pMP) ends in
//            pMP->ComputeDistinctiveDescriptors(), src/MapPoint.cc:303-351 -- it happens between the Fuse calls of
//            SearchInNeighbors) this one (point, key frame) search is recomputed on the host with the same rule
//            (gfs_fuse::search_point, csrc/fuse_rule.hpp); then the Replace / AddObservation / AddMapPoint block of :1529-1544.
// Compile the translation unit that includes this with -ffp-contract=off (the host rule is the device's arithmetic).
// Single-camera pinhole key frames only: NLeft != -1 or another camera model throws.
//
// KeyFrame and MapPoint are the reference's own classes, used through the members the reference functions use (pKF->NLeft, N, fx,
// fy, cx, cy, mbf, mnMinX .. mnMaxY, mfGridElementWidthInv / HeightInv, mvScaleFactors, mvInvLevelSigma2, mnScaleLevels,
// mfLogScaleFactor, mvuRight, mnId, GetMapPoint, AddMapPoint, GetMapPointMatches, UpdateConnections; pMP->isBad, IsInKeyFrame,
// Observations, Replace, AddObservation, mnFuseCandidateForKF, ComputeDistinctiveDescriptors, UpdateNormalAndDepth).  `Access` as for
// SearchLocalPoints (world_pos, normal, distances, descriptor of a MapPoint), plus for a key frame:
//     static bool is_pinhole(const KeyFrame&);                                       // mpCamera->GetType() == CAM_PINHOLE
//     static void pose(const KeyFrame&, float q[4], float t[3], float Ow[3]);        // GetPose(): unit_quaternion() (x, y, z, w),
//                                                                                    // translation(); GetCameraCenter()
//     static const gfs_keypoint* keys_un(const KeyFrame&);                           // mvKeysUn.data()
//     static const uint8_t* descriptors(const KeyFrame&);                            // mDescriptors.data
// `solve(lists, n_lists, kfs, B, results)` is the numeric core: FuseSearcher::solve below (gfs_fuse_search on the GPU).
// ------------------------------------------------------------------------------------------------------------------------
struct FuseList {  // one gathered point list
  std::vector<uint8_t> present, desc;
  std::vector<float> xw, nrm, dmin, dmax;
  gfs_fuse_points view() const {
    gfs_fuse_points p{};
    p.n_mp = (int32_t)present.size();
    p.mp_xw = xw.data();
    p.mp_normal = nrm.data();
    p.mp_min_dist = dmin.data();
    p.mp_max_dist = dmax.data();
    p.mp_desc = desc.data();
    return p;
  }
};

struct FuseOutputs {  // the result arrays of one (list, key frame) search
  std::vector<uint8_t> exit;
  std::vector<int32_t> best_idx, best_dist, level;
  gfs_fuse_result view(size_t n) {
    exit.assign(n + 1, 0);
    best_idx.assign(n + 1, -1);
    best_dist.assign(n + 1, 256);
    level.assign(n + 1, 0);
    gfs_fuse_result r{};
    r.exit = exit.data();
    r.best_idx = best_idx.data();
    r.best_dist = best_dist.data();
    r.level = level.data();
    return r;
  }
};

template <class Access, class MapPoint>
void fuse_gather(const std::vector<MapPoint*>& vpMapPoints, FuseList& L) {
  const size_t n = vpMapPoints.size();
  L.present.assign(n, 0);
  L.xw.assign(3 * n + 3, 0.0f);
  L.nrm.assign(3 * n + 3, 0.0f);
  L.dmin.assign(n + 1, 0.0f);
  L.dmax.assign(n + 1, 0.0f);
  L.desc.assign(32 * n + 32, 0);
  for (size_t i = 0; i < n; i++) {
    const MapPoint* pMP = vpMapPoints[i];
    if (!pMP) continue;  // (its slot is searched with zeros and skipped on replay)
    L.present[i] = 1;
    Access::world_pos(pMP, &L.xw[3 * i]);
    Access::normal(pMP, &L.nrm[3 * i]);
    Access::distances(pMP, &L.dmin[i], &L.dmax[i]);
    Access::descriptor(pMP, &L.desc[32 * i]);
  }
}

template <class Access, class KeyFrame>
gfs_fuse_keyframe fuse_keyframe(const KeyFrame& KF, float th, int list) {
  if (KF.NLeft != -1 || !Access::is_pinhole(KF)) throw std::invalid_argument("Fuse: single-camera pinhole key frames only");
  gfs_fuse_keyframe k{};
  Access::pose(KF, k.Tcw_q, k.Tcw_t, k.Ow);
  k.fx = KF.fx;
  k.fy = KF.fy;
  k.cx = KF.cx;
  k.cy = KF.cy;
  k.bf = KF.mbf;
  k.min_x = KF.mnMinX;
  k.max_x = KF.mnMaxX;
  k.min_y = KF.mnMinY;
  k.max_y = KF.mnMaxY;
  k.grid_w_inv = KF.mfGridElementWidthInv;
  k.grid_h_inv = KF.mfGridElementHeightInv;
  k.scale_factors = KF.mvScaleFactors.data();
  k.inv_level_sigma2 = KF.mvInvLevelSigma2.data();
  k.n_levels = KF.mnScaleLevels;
  k.log_scale_factor = KF.mfLogScaleFactor;
  k.th = th;
  k.n_kp = KF.N;
  k.kps_un = Access::keys_un(KF);
  k.u_right = KF.mvuRight.data();
  k.desc = Access::descriptors(KF);
  k.list = list;
  return k;
}

// one (point, key frame) search on the host from the point's CURRENT descriptor (the replay's recompute path)
inline gfs_fuse::PointResult fuse_search_point_host(const gfs_fuse_keyframe& k, const float* P, const float* Pn, float min_d, float max_d,
                                                    const uint8_t* desc) {
  if (k.n_levels < 1 || k.n_levels > 16) throw std::invalid_argument("Fuse: 1..16 pyramid levels");
  gfs_fuse::KeyFrame K{};
  for (int c = 0; c < 4; c++) K.q[c] = k.Tcw_q[c];
  for (int c = 0; c < 3; c++) {
    K.t[c] = k.Tcw_t[c];
    K.Ow[c] = k.Ow[c];
  }
  K.fx = k.fx;
  K.fy = k.fy;
  K.cx = k.cx;
  K.cy = k.cy;
  K.bf = k.bf;
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
  for (int c = 0; c < k.n_levels; c++) {
    K.scale[c] = k.scale_factors[c];
    K.inv_sigma2[c] = k.inv_level_sigma2[c];
  }
  std::vector<float> kx((size_t)k.n_kp + 1), ky((size_t)k.n_kp + 1);
  std::vector<int32_t> oct((size_t)k.n_kp + 1);
  for (int i = 0; i < k.n_kp; i++) {
    kx[i] = k.kps_un[i].x;
    ky[i] = k.kps_un[i].y;
    oct[i] = k.kps_un[i].octave;
    if (oct[i] < 0 || oct[i] >= k.n_levels) throw std::invalid_argument("Fuse: key-point octave outside the pyramid");
  }
  return gfs_fuse::search_point(K, P, Pn, min_d, max_d, desc, kx.data(), ky.data(), k.u_right, oct.data(), k.desc);
}

// The loop of :1408-1545 around the device's search results of (L, k).  recomputed: incremented per host recompute.
template <class Access, class KeyFrame, class MapPoint>
int fuse_replay(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const FuseList& L, const gfs_fuse_keyframe& k, const FuseOutputs& r,
                int* recomputed = nullptr) {
  int nFused = 0;
  for (size_t i = 0; i < vpMapPoints.size(); i++) {
    MapPoint* pMP = vpMapPoints[i];
    if (!L.present[i]) continue;
    if (pMP->isBad()) continue;
    if (pMP->IsInKeyFrame(pKF)) continue;
    int exit = r.exit[i], bestIdx = r.best_idx[i];
    uint8_t now[32];
    Access::descriptor(pMP, now);
    if (std::memcmp(now, &L.desc[32 * i], 32) != 0) {  // the descriptor changed after the upload: this pair again, on the host
      const gfs_fuse::PointResult o = fuse_search_point_host(k, &L.xw[3 * i], &L.nrm[3 * i], L.dmin[i], L.dmax[i], now);
      exit = o.exit;
      bestIdx = o.best_idx;
      if (recomputed) ++*recomputed;
    }
    if (exit != GFS_FUSE_MATCHED) continue;
    // If there is already a MapPoint replace otherwise add new measurement (:1529-1542)
    MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) {
        if (pMPinKF->Observations() > pMP->Observations())
          pMP->Replace(pMPinKF);
        else
          pMPinKF->Replace(pMP);
      }
    } else {
      pMP->AddObservation(pKF, bestIdx);
      pKF->AddMapPoint(pMP, bestIdx);
    }
    nFused++;
  }
  return nFused;
}

// ORBmatcher::Fuse(pKF, vpMapPoints, th): one list, one key frame
template <class Access, class KeyFrame, class MapPoint, class Solve>
int Fuse(Solve&& solve, KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, float th = 3.0f, int* recomputed = nullptr) {
  const gfs_fuse_keyframe k = fuse_keyframe<Access>(*pKF, th, 0);
  FuseList L;
  fuse_gather<Access>(vpMapPoints, L);
  const gfs_fuse_points lp = L.view();
  FuseOutputs out;
  gfs_fuse_result r = out.view(vpMapPoints.size());
  check(solve(&lp, 1, &k, 1, &r), "gfs_fuse_search");
  return fuse_replay<Access>(pKF, vpMapPoints, L, k, out, recomputed);
}

struct SearchInNeighborsCounts {
  int fused_in_targets = 0, fused_in_current = 0, recomputed = 0;
  bool aborted = false;
};

// LocalMapping::SearchInNeighbors from `ORBmatcher matcher;` (:1180) to its end: the current key frame's points in every target (ONE
// device call: list 0 against all targets), the targets' points in the current key frame (a second call: one list, one key frame),
// then the update of the current key frame's points and connections.  The caller keeps the target selection (:1131-1177);
// pbAbortBA is mbAbortBA, looked at where the reference looks (:1191).
// `update_points`, when given, is a map-point solver (MapPointUpdater::solver(), or map_points_update_host): the update of the current
// key frame's points is then one UpdateMapPoints call; `Access` then needs its members too.
template <class Access, class KeyFrame, class Solve, class UpdatePoints = PerPointUpdate>
SearchInNeighborsCounts SearchInNeighborsFuse(Solve&& solve, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpTargetKFs,
                                              const bool* pbAbortBA = nullptr, float th = 3.0f, UpdatePoints&& update_points = UpdatePoints()) {
  using MapPoint = std::remove_pointer_t<typename decltype(pCurrentKF->GetMapPointMatches())::value_type>;
  SearchInNeighborsCounts c;
  if (pCurrentKF->NLeft != -1 || !Access::is_pinhole(*pCurrentKF)) throw std::invalid_argument("Fuse: single-camera pinhole key frames only");
  // Search matches by projection from current KF in target KFs
  std::vector<MapPoint*> vpMapPointMatches = pCurrentKF->GetMapPointMatches();
  if (!vpTargetKFs.empty()) {
    std::vector<gfs_fuse_keyframe> kfs;
    for (KeyFrame* pKFi : vpTargetKFs) kfs.push_back(fuse_keyframe<Access>(*pKFi, th, 0));
    FuseList L;
    fuse_gather<Access>(vpMapPointMatches, L);
    const gfs_fuse_points lp = L.view();
    std::vector<FuseOutputs> outs(kfs.size());
    std::vector<gfs_fuse_result> rs;
    for (FuseOutputs& o : outs) rs.push_back(o.view(vpMapPointMatches.size()));
    check(solve(&lp, 1, kfs.data(), (int)kfs.size(), rs.data()), "gfs_fuse_search");
    for (size_t f = 0; f < kfs.size(); f++)
      c.fused_in_targets += fuse_replay<Access>(vpTargetKFs[f], vpMapPointMatches, L, kfs[f], outs[f], &c.recomputed);
  }
  if (pbAbortBA && *pbAbortBA) {
    c.aborted = true;
    return c;
  }
  // Search matches by projection from target KFs in current KF
  std::vector<MapPoint*> vpFuseCandidates;
  vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
  for (KeyFrame* pKFi : vpTargetKFs) {
    const std::vector<MapPoint*> vpMapPointsKFi = pKFi->GetMapPointMatches();
    for (MapPoint* pMP : vpMapPointsKFi) {
      if (!pMP) continue;
      if (pMP->isBad() || pMP->mnFuseCandidateForKF == pCurrentKF->mnId) continue;
      pMP->mnFuseCandidateForKF = pCurrentKF->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }
  c.fused_in_current = Fuse<Access>(solve, pCurrentKF, vpFuseCandidates, th, &c.recomputed);
  // Update points
  vpMapPointMatches = pCurrentKF->GetMapPointMatches();
  if constexpr (std::is_same<typename std::decay<UpdatePoints>::type, PerPointUpdate>::value) {
    for (MapPoint* pMP : vpMapPointMatches) {
      if (pMP && !pMP->isBad()) {
        pMP->ComputeDistinctiveDescriptors();
        pMP->UpdateNormalAndDepth();
      }
    }
  } else {
    UpdateMapPoints<Access>(update_points, vpMapPointMatches, GFS_MAP_POINTS_FULL);  // (null and bad entries upload empty lists)
  }
  // Update connections in covisibility graph
  pCurrentKF->UpdateConnections();
  return c;
}

// the numeric core of Fuse on the GPU: one handle, its reserve grown to the largest call seen
class FuseSearcher {
 public:
  FuseSearcher(int max_kp = 4096, int device = 0) { check(gfs_sbp_create(device, 64, max_kp, 1, &h_), "gfs_sbp_create"); }
  ~FuseSearcher() { gfs_sbp_destroy(h_); }
  FuseSearcher(const FuseSearcher&) = delete;
  FuseSearcher& operator=(const FuseSearcher&) = delete;
  int solve(const gfs_fuse_points* lists, int n_lists, const gfs_fuse_keyframe* kfs, int B, gfs_fuse_result* results) {
    int n = 0;
    for (int l = 0; l < n_lists; l++) n = std::max(n, lists[l].n_mp);
    if (n_lists > lists_ || n > points_ || B > kfs_) {  // the library refuses what exceeds the reserve (it never truncates): grow it first
      const int nl = std::max(n_lists, lists_), np = std::max(std::max(n, 64), points_), nk = std::max(B, kfs_);
      check(gfs_sbp_reserve_fuse(h_, nl, np, nk), "gfs_sbp_reserve_fuse");
      lists_ = nl;
      points_ = np;
      kfs_ = nk;
    }
    return gfs_fuse_search(h_, lists, n_lists, kfs, B, results);
  }
  auto solver() {
    return [this](const gfs_fuse_points* l, int nl, const gfs_fuse_keyframe* k, int B, gfs_fuse_result* r) { return solve(l, nl, k, B, r); };
  }

 private:
  gfs_sbp* h_ = nullptr;
  int lists_ = 0, points_ = 0, kfs_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------------
// int ORBmatcher::Fuse(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints, float th,
//                      vector<MapPoint*>& vpReplacePoint)                                  reference src/ORBmatcher.cc:1550-1654
// void LoopClosing::SearchAndFuse(const KeyFrameAndPose& CorrectedPosesMap, vector<MapPoint*>& vpMapPoints)
// void LoopClosing::SearchAndFuse(const vector<KeyFrame*>& vConectedKFs, vector<MapPoint*>& vpMapPoints)
//                                                                                          reference src/LoopClosing.cc:2224-2302
// int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
//                      vector<MapPoint*>& vpMatched, int th, float ratioHamming)           reference src/ORBmatcher.cc:432-529
// int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
//                      const vector<KeyFrame*>& vpPointsKFs, vector<MapPoint*>& vpMatched, vector<KeyFrame*>& vpMatchedKF, int th,
//                      float ratioHamming)                                                 reference src/ORBmatcher.cc:531-636
// as real code around gfs_sim3_search.
//   The projection searches change nothing but vpMatched (and vpMatchedKF), and the entry resolves that dependency itself: the
//   adaptor uploads isBad() || spAlreadyFound.count(pMP) as mp_skip and vpMatched[idx] != NULL as kp_taken, and writes the matches.
//   Fuse reads pointer state before the search (isBad(), the GetMapPoints() set taken at entry) and after it (GetMapPoint(bestIdx),
//   isBad() of the point there), and SearchAndFuse changes it between two key frames (pRep->Replace(vpMapPoints[i]), which ends in
//   vpMapPoints[i]->ComputeDistinctiveDescriptors()).  So SearchAndFuse searches every (key frame, point) pair in ONE device call
//   from the entry state and replays key frame by key frame in the reference's order against the live state; a point whose
//   descriptor is no longer the uploaded one is searched again on the host with the same rule (gfs_sim3::search_point,
//   csrc/sim3_search_rule.hpp), as in Fuse above.
// Compile the translation unit that includes this with -ffp-contract=off.  Single-camera pinhole key frames only: NLeft != -1 or
// another camera model throws.
//
// KeyFrame and MapPoint members used: pKF->NLeft, N, fx, fy, cx, cy, mnMinX .. mnMaxY, mfGridElementWidthInv / HeightInv,
// mvScaleFactors, mnScaleLevels, mfLogScaleFactor, GetMapPoints, GetMapPoint, AddMapPoint, GetPose (through Access); pMP->isBad,
// AddObservation, Replace.  `Access` as for Fuse (is_pinhole, keys_un, descriptors; world_pos, normal, distances, descriptor), plus:
//     template <class Sim3> static void sim3_pose(const Sim3& Scw, float q[4], float t[3], float Ow[3]);
//         // the caller's own Sophus, as :442-444 / :1560-1562: Sophus::SE3f Tcw(Scw.rotationMatrix(), Scw.translation() / Scw.scale());
//         // q = Tcw.unit_quaternion() (x, y, z, w), t = Tcw.translation(), Ow = Tcw.inverse().translation().  For a g2o::Sim3 (the
//         // values of KeyFrameAndPose) Converter::toSophus first (:2241).
//     static void pose_as_sim3(const KeyFrame&, float q[4], float t[3], float Ow[3]);
//         // :2277-2279: Sophus::Sim3f Scw(Tcw.unit_quaternion(), Tcw.translation()); Scw.setScale(1.f); then as sim3_pose
//     static Guard lock_map_update(KeyFrame*);   // unique_lock<mutex>(pKF->GetMap()->mMutexMapUpdate), held over the Replace loop
// `solve(lists, n_lists, problems, B, results)` is the numeric core: Sim3Searcher::solve below (gfs_sim3_search on the GPU).
// ------------------------------------------------------------------------------------------------------------------------
struct Sim3SearchOutputs {  // the result arrays of one (list, problem) search
  std::vector<uint8_t> exit;
  std::vector<int32_t> best_idx, best_dist, level;
  gfs_sim3_search_result view(size_t n) {
    exit.assign(n + 1, 0);
    best_idx.assign(n + 1, -1);
    best_dist.assign(n + 1, 256);
    level.assign(n + 1, 0);
    gfs_sim3_search_result r{};
    r.exit = exit.data();
    r.best_idx = best_idx.data();
    r.best_dist = best_dist.data();
    r.level = level.data();
    return r;
  }
};

// the problem of one key frame; Tcw_q / Tcw_t / Ow are the caller's to fill
template <class Access, class KeyFrame>
gfs_sim3_search_problem sim3_search_keyframe(const KeyFrame& KF, int mode, float th, float ratio_hamming, int list) {
  if (KF.NLeft != -1 || !Access::is_pinhole(KF)) throw std::invalid_argument("Sim3 search: single-camera pinhole key frames only");
  gfs_sim3_search_problem k{};
  k.mode = mode;
  k.ratio_hamming = ratio_hamming;
  k.fx = KF.fx;
  k.fy = KF.fy;
  k.cx = KF.cx;
  k.cy = KF.cy;
  k.min_x = KF.mnMinX;
  k.max_x = KF.mnMaxX;
  k.min_y = KF.mnMinY;
  k.max_y = KF.mnMaxY;
  k.grid_w_inv = KF.mfGridElementWidthInv;
  k.grid_h_inv = KF.mfGridElementHeightInv;
  k.scale_factors = KF.mvScaleFactors.data();
  k.n_levels = KF.mnScaleLevels;
  k.log_scale_factor = KF.mfLogScaleFactor;
  k.th = th;
  k.n_kp = KF.N;
  k.kps_un = Access::keys_un(KF);
  k.desc = Access::descriptors(KF);
  k.list = list;
  return k;
}

// one (point, problem) search on the host from the point's CURRENT descriptor (the replay's recompute path); taken may be NULL
inline gfs_sim3::PointResult sim3_search_point_host(const gfs_sim3_search_problem& k, const float* P, const float* Pn, float min_d, float max_d,
                                                    const uint8_t* desc, const uint8_t* taken = nullptr) {
  if (k.n_levels < 1 || k.n_levels > 16) throw std::invalid_argument("Sim3 search: 1..16 pyramid levels");
  gfs_fuse::KeyFrame K{};
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
  for (int i = 0; i < k.n_kp; i++)
    if (k.kps_un[i].octave < 0 || k.kps_un[i].octave >= k.n_levels) throw std::invalid_argument("Sim3 search: key-point octave outside the pyramid");
  return gfs_sim3::search_point(
      K, k.mode, k.ratio_hamming, P, Pn, min_d, max_d, desc,
      [&](int j, float* x, float* y, int* oct) {
        *x = k.kps_un[j].x;
        *y = k.kps_un[j].y;
        *oct = k.kps_un[j].octave;
      },
      k.desc, taken);
}

// The loop of :1572-1651 around the device's search results of (L, k), which were computed WITHOUT mp_skip: the skip test and the
// replace / add block run here against the live state.  recomputed: incremented per host recompute.
template <class Access, class KeyFrame, class MapPoint>
int fuse_sim3_replay(KeyFrame* pKF, const std::vector<MapPoint*>& vpPoints, const FuseList& L, const gfs_sim3_search_problem& k,
                     const Sim3SearchOutputs& r, std::vector<MapPoint*>& vpReplacePoint, int* recomputed = nullptr) {
  // Set of MapPoints already found in the KeyFrame
  const auto spAlreadyFound = pKF->GetMapPoints();
  int nFused = 0;
  for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
    MapPoint* pMP = vpPoints[iMP];
    if (!L.present[iMP]) continue;
    // Discard Bad MapPoints and already found
    if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
    int exit = r.exit[iMP], bestIdx = r.best_idx[iMP];
    uint8_t now[32];
    Access::descriptor(pMP, now);
    if (std::memcmp(now, &L.desc[32 * iMP], 32) != 0) {  // the descriptor changed after the upload: this pair again, on the host
      const gfs_sim3::PointResult o = sim3_search_point_host(k, &L.xw[3 * iMP], &L.nrm[3 * iMP], L.dmin[iMP], L.dmax[iMP], now);
      exit = o.exit;
      bestIdx = o.best_idx;
      if (recomputed) ++*recomputed;
    }
    if (exit != GFS_FUSE_MATCHED) continue;
    // If there is already a MapPoint replace otherwise add new measurement (:1641-1649)
    MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
    if (pMPinKF) {
      if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
    } else {
      pMP->AddObservation(pKF, bestIdx);
      pKF->AddMapPoint(pMP, bestIdx);
    }
    nFused++;
  }
  return nFused;
}

// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): one list, one key frame
template <class Access, class KeyFrame, class MapPoint, class Sim3, class Solve>
int FuseSim3(Solve&& solve, KeyFrame* pKF, const Sim3& Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint,
             int* recomputed = nullptr) {
  gfs_sim3_search_problem k = sim3_search_keyframe<Access>(*pKF, GFS_SIM3_FUSE, th, 1.0f, 0);
  Access::sim3_pose(Scw, k.Tcw_q, k.Tcw_t, k.Ow);
  FuseList L;
  fuse_gather<Access>(vpPoints, L);
  const gfs_fuse_points lp = L.view();
  Sim3SearchOutputs out;
  gfs_sim3_search_result r = out.view(vpPoints.size());
  check(solve(&lp, 1, &k, 1, &r), "gfs_sim3_search");
  return fuse_sim3_replay<Access>(pKF, vpPoints, L, k, out, vpReplacePoint, recomputed);
}

struct SearchAndFuseCounts {
  int fused = 0, replaced = 0, recomputed = 0;
};

// both SearchAndFuse overloads from `ORBmatcher matcher(0.8);` on: problems[f] is key frame vpKFs[f]'s, its pose filled
template <class Access, class KeyFrame, class MapPoint, class Solve>
SearchAndFuseCounts search_and_fuse(Solve&& solve, const std::vector<KeyFrame*>& vpKFs, std::vector<gfs_sim3_search_problem>& problems,
                                    std::vector<MapPoint*>& vpMapPoints) {
  SearchAndFuseCounts c;
  if (vpKFs.empty()) return c;
  FuseList L;
  fuse_gather<Access>(vpMapPoints, L);
  const gfs_fuse_points lp = L.view();
  std::vector<Sim3SearchOutputs> outs(vpKFs.size());
  std::vector<gfs_sim3_search_result> rs;
  for (Sim3SearchOutputs& o : outs) rs.push_back(o.view(vpMapPoints.size()));
  check(solve(&lp, 1, problems.data(), (int)problems.size(), rs.data()), "gfs_sim3_search");
  for (size_t f = 0; f < vpKFs.size(); f++) {
    KeyFrame* pKFi = vpKFs[f];
    std::vector<MapPoint*> vpReplacePoints(vpMapPoints.size(), static_cast<MapPoint*>(nullptr));
    c.fused += fuse_sim3_replay<Access>(pKFi, vpMapPoints, L, problems[f], outs[f], vpReplacePoints, &c.recomputed);
    // Get Map Mutex
    auto lock = Access::lock_map_update(pKFi);
    (void)lock;
    const int nLP = (int)vpMapPoints.size();
    for (int i = 0; i < nLP; i++) {
      MapPoint* pRep = vpReplacePoints[i];
      if (pRep) {
        c.replaced += 1;
        pRep->Replace(vpMapPoints[i]);
      }
    }
  }
  return c;
}

// LoopClosing::SearchAndFuse(CorrectedPosesMap, vpMapPoints): a map from KeyFrame* to the corrected Sim3, walked in its own order
template <class Access, class PosesMap, class MapPoint, class Solve>
SearchAndFuseCounts SearchAndFuse(Solve&& solve, const PosesMap& CorrectedPosesMap, std::vector<MapPoint*>& vpMapPoints, float th = 4.0f) {
  using KeyFrame = std::remove_pointer_t<typename PosesMap::key_type>;
  std::vector<KeyFrame*> kfs;
  std::vector<gfs_sim3_search_problem> problems;
  for (auto mit = CorrectedPosesMap.begin(), mend = CorrectedPosesMap.end(); mit != mend; mit++) {
    KeyFrame* pKFi = mit->first;
    problems.push_back(sim3_search_keyframe<Access>(*pKFi, GFS_SIM3_FUSE, th, 1.0f, 0));
    Access::sim3_pose(mit->second, problems.back().Tcw_q, problems.back().Tcw_t, problems.back().Ow);
    kfs.push_back(pKFi);
  }
  return search_and_fuse<Access>(solve, kfs, problems, vpMapPoints);
}

// LoopClosing::SearchAndFuse(vConectedKFs, vpMapPoints): every key frame under its own pose as a Sim3 of scale 1
template <class Access, class KeyFrame, class MapPoint, class Solve>
SearchAndFuseCounts SearchAndFuse(Solve&& solve, const std::vector<KeyFrame*>& vConectedKFs, std::vector<MapPoint*>& vpMapPoints, float th = 4.0f) {
  std::vector<gfs_sim3_search_problem> problems;
  for (KeyFrame* pKF : vConectedKFs) {
    problems.push_back(sim3_search_keyframe<Access>(*pKF, GFS_SIM3_FUSE, th, 1.0f, 0));
    Access::pose_as_sim3(*pKF, problems.back().Tcw_q, problems.back().Tcw_t, problems.back().Ow);
  }
  return search_and_fuse<Access>(solve, vConectedKFs, problems, vpMapPoints);
}

// both SearchByProjection(pKF, Scw, ...) overloads: vpPointsKFs / vpMatchedKF are NULL for the first
template <class Access, class KeyFrame, class MapPoint, class Sim3, class Solve>
int search_by_projection_sim3(Solve&& solve, KeyFrame* pKF, const Sim3& Scw, const std::vector<MapPoint*>& vpPoints,
                              const std::vector<KeyFrame*>* vpPointsKFs, std::vector<MapPoint*>& vpMatched, std::vector<KeyFrame*>* vpMatchedKF,
                              int th, float ratioHamming) {
  gfs_sim3_search_problem k = sim3_search_keyframe<Access>(*pKF, vpPointsKFs ? GFS_SIM3_SBP_KFS : GFS_SIM3_SBP, (float)th, ratioHamming, 0);
  Access::sim3_pose(Scw, k.Tcw_q, k.Tcw_t, k.Ow);
  if ((int)vpMatched.size() < k.n_kp || (vpMatchedKF && (int)vpMatchedKF->size() < k.n_kp) || (vpPointsKFs && vpPointsKFs->size() < vpPoints.size()))
    throw std::invalid_argument("SearchByProjection: vpMatched / vpMatchedKF / vpPointsKFs are too short");
  // Set of MapPoints already found in the KeyFrame
  std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
  spAlreadyFound.erase(static_cast<MapPoint*>(nullptr));
  FuseList L;
  fuse_gather<Access>(vpPoints, L);
  std::vector<uint8_t> skip(vpPoints.size() + 1, 0), taken((size_t)k.n_kp + 1, 0);
  for (size_t i = 0; i < vpPoints.size(); i++) skip[i] = !L.present[i] || vpPoints[i]->isBad() || spAlreadyFound.count(vpPoints[i]);
  for (int j = 0; j < k.n_kp; j++) taken[j] = vpMatched[j] != nullptr;
  k.mp_skip = skip.data();
  k.kp_taken = taken.data();
  const gfs_fuse_points lp = L.view();
  Sim3SearchOutputs out;
  gfs_sim3_search_result r = out.view(vpPoints.size());
  check(solve(&lp, 1, &k, 1, &r), "gfs_sim3_search");
  int nmatches = 0;
  for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
    if (out.exit[iMP] != GFS_FUSE_MATCHED) continue;
    vpMatched[out.best_idx[iMP]] = vpPoints[iMP];
    if (vpMatchedKF) (*vpMatchedKF)[out.best_idx[iMP]] = (*vpPointsKFs)[iMP];
    nmatches++;
  }
  return nmatches;
}

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming)
template <class Access, class KeyFrame, class MapPoint, class Sim3, class Solve>
int SearchByProjectionSim3(Solve&& solve, KeyFrame* pKF, const Sim3& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched,
                           int th, float ratioHamming = 1.0f) {
  return search_by_projection_sim3<Access, KeyFrame, MapPoint>(solve, pKF, Scw, vpPoints, nullptr, vpMatched, nullptr, th, ratioHamming);
}

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming)
template <class Access, class KeyFrame, class MapPoint, class Sim3, class Solve>
int SearchByProjectionSim3(Solve&& solve, KeyFrame* pKF, const Sim3& Scw, const std::vector<MapPoint*>& vpPoints,
                           const std::vector<KeyFrame*>& vpPointsKFs, std::vector<MapPoint*>& vpMatched, std::vector<KeyFrame*>& vpMatchedKF, int th,
                           float ratioHamming = 1.0f) {
  return search_by_projection_sim3<Access, KeyFrame, MapPoint>(solve, pKF, Scw, vpPoints, &vpPointsKFs, vpMatched, &vpMatchedKF, th, ratioHamming);
}

// the numeric core of the Sim3 searches on the GPU: one handle, its reserve grown to the largest call seen
class Sim3Searcher {
 public:
  Sim3Searcher(int max_kp = 4096, int device = 0) { check(gfs_sbp_create(device, 64, max_kp, 1, &h_), "gfs_sbp_create"); }
  ~Sim3Searcher() { gfs_sbp_destroy(h_); }
  Sim3Searcher(const Sim3Searcher&) = delete;
  Sim3Searcher& operator=(const Sim3Searcher&) = delete;
  int solve(const gfs_fuse_points* lists, int n_lists, const gfs_sim3_search_problem* problems, int B, gfs_sim3_search_result* results) {
    int n = 0;
    for (int l = 0; l < n_lists; l++) n = std::max(n, lists[l].n_mp);
    if (n_lists > lists_ || n > points_ || B > problems_) {  // the library refuses what exceeds the reserve (it never truncates): grow it first
      const int nl = std::max(n_lists, lists_), np = std::max(std::max(n, 64), points_), nk = std::max(B, problems_);
      check(gfs_sbp_reserve_sim3_search(h_, nl, np, nk), "gfs_sbp_reserve_sim3_search");
      lists_ = nl;
      points_ = np;
      problems_ = nk;
    }
    return gfs_sim3_search(h_, lists, n_lists, problems, B, results);
  }
  auto solver() {
    return [this](const gfs_fuse_points* l, int nl, const gfs_sim3_search_problem* k, int B, gfs_sim3_search_result* r) {
      return solve(l, nl, k, B, r);
    };
  }

 private:
  gfs_sbp* h_ = nullptr;
  int lists_ = 0, points_ = 0, problems_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------------
// void LocalMapping::CreateNewMapPoints()                                                  reference src/LocalMapping.cc:803-1127
// as real code around gfs_create_new_map_points.  The numeric result at neighbour i (SearchForTriangulation's pairs, each pair's
// triangulation and gates) depends only on the entry state and on which idx1 of the current key frame received a point at the
// neighbours before i; the device carries exactly that, so ONE call serves the whole neighbour loop and every prefix of it is exact.
//   gather:  the neighbour list (:805-819); neighbours with a short baseline (:859-866) are not uploaded; every key frame's
//            mFeatVec is flattened; `Access` computes ep and F12 with the reference's own Sophus / Eigen expressions.
//   solve:   `solve(problems, 1, results)`: MapPointCreator::solve below (the GPU), or tri_solve_host (the same rule on the host).
//   replay:  per neighbour of the ORIGINAL list in order: `if (i > 0 && check_new_key_frames()) return` (:847) -- exact, because the
//            results of the neighbours before i do not depend on those after; then for ascending idx1 with GFS_TRI_CREATED the block
//            :1103-1124 (new MapPoint, AddObservation x 2, the optical-flow feature's pointer, AddMapPoint x 2,
//            ComputeDistinctiveDescriptors, UpdateNormalAndDepth, Atlas::AddMapPoint, mlpRecentAddedMapPoints).
// What other threads change in the map during the call is not seen: has_mp is read at entry (as for Fuse).
// Single-camera pinhole key frames only: NLeft != -1 or another camera model throws.  Compile with -ffp-contract=off when
// tri_solve_host is used (the host rule is the device's arithmetic).
//
// KeyFrame / MapPoint / Atlas are the reference's own classes, used through the members the reference function uses (pKF->NLeft, N,
// fx .. invfy, mbf, mb, mfScaleFactor, mnScaleLevels, mvScaleFactors, mvLevelSigma2, mvuRight, mvDepth, mPrevKF,
// GetBestCovisibilityKeyFrames, GetMapPoint, AddMapPoint, ComputeSceneMedianDepth; pMP->AddObservation, ComputeDistinctiveDescriptors,
// UpdateNormalAndDepth; atlas->AddMapPoint).  `Access` as for Fuse (is_pinhole, keys_un, descriptors), plus:
//     static void pose3x4(const KeyFrame&, float Tcw[12], float Ow[3], float Rwc[9], float twc[3]);  // GetPose().matrix3x4() row-major,
//                                                                       // GetCameraCenter(), mRwc row-major, mTwc.translation()
//     static const gfs_keypoint* keys(const KeyFrame&);                 // mvKeys.data()
//     template <class F> static void for_each_node(const KeyFrame&, F&& f);  // f(node id, const std::vector<unsigned>&) over mFeatVec
//     static void epipolar(const KeyFrame& kf1, const KeyFrame& kf2, float ep[2], float F12[9]);  // src/ORBmatcher.cc:1165-1171 and
//                                                                       // Pinhole.cpp:109-112 (F12 row-major), in float as written
//     static MapPoint* new_map_point(const float x3D[3], KeyFrame* pRefKF, Atlas* atlas);  // new MapPoint(x3D, pKF, GetCurrentMap())
//     static void set_tracked_feature(KeyFrame* pKF, int idx1, MapPoint* pMP);             // track_feature_pts_.at(idx1): mp, is_3d
// ------------------------------------------------------------------------------------------------------------------------
struct CreateNewMapPointsParams {
  bool monocular = false, inertial = false, coarse = false, far_points = false, use_optical_flow = false;  // mbMonocular, mbInertial,
  float th_far_points = 0.0f;  // bCoarse (:870), mbFarPoints, mpTracker->GetUseOpticalFlow(); mThFarPoints
};

struct TriKeyFrameFlat {  // one gathered key frame
  std::vector<int32_t> node_id, node_start, feat_idx;
  std::vector<uint8_t> has_mp;
  gfs_tri_keyframe k{};
};

template <class Access, class KeyFrame>
void tri_gather(KeyFrame* pKF, TriKeyFrameFlat& F) {
  const KeyFrame& KF = *pKF;
  if (KF.NLeft != -1 || !Access::is_pinhole(KF)) throw std::invalid_argument("CreateNewMapPoints: single-camera pinhole key frames only");
  gfs_tri_keyframe& k = F.k;
  Access::pose3x4(KF, k.Tcw, k.Ow, k.Rwc, k.twc);
  k.fx = KF.fx;
  k.fy = KF.fy;
  k.cx = KF.cx;
  k.cy = KF.cy;
  k.invfx = KF.invfx;
  k.invfy = KF.invfy;
  k.mbf = KF.mbf;
  k.mb = KF.mb;
  k.scale_factors = KF.mvScaleFactors.data();
  k.level_sigma2 = KF.mvLevelSigma2.data();
  k.n_levels = KF.mnScaleLevels;
  k.n_kp = KF.N;
  k.kps_un = Access::keys_un(KF);
  k.kps = Access::keys(KF);
  k.u_right = KF.mvuRight.data();
  k.depth = KF.mvDepth.data();
  k.desc = Access::descriptors(KF);
  F.has_mp.assign((size_t)KF.N + 1, 0);
  for (int i = 0; i < KF.N; i++) F.has_mp[i] = pKF->GetMapPoint(i) != nullptr;
  F.node_id.clear();
  F.feat_idx.clear();
  F.node_start.assign(1, 0);
  Access::for_each_node(KF, [&](unsigned id, const std::vector<unsigned>& idx) {
    F.node_id.push_back((int32_t)id);
    for (unsigned i : idx) F.feat_idx.push_back((int32_t)i);
    F.node_start.push_back((int32_t)F.feat_idx.size());
  });
  F.node_id.push_back(0);   // (never NULL)
  F.feat_idx.push_back(0);
  k.has_mp = F.has_mp.data();
  k.n_nodes = (int32_t)F.node_start.size() - 1;
  k.node_id = F.node_id.data();
  k.node_start = F.node_start.data();
  k.feat_idx = F.feat_idx.data();
}

struct TriOutputs {  // the result arrays of one neighbour
  std::vector<int32_t> match12;
  std::vector<uint8_t> exit, point_stereo;
  std::vector<float> x3d;
  gfs_tri_result view(size_t n) {
    match12.assign(n + 1, -1);
    exit.assign(n + 1, 0);
    point_stereo.assign(n + 1, 0);
    x3d.assign(3 * n + 3, 0.0f);
    gfs_tri_result r{};
    r.match12 = match12.data();
    r.exit = exit.data();
    r.point_stereo = point_stereo.data();
    r.x3d = x3d.data();
    return r;
  }
};

// gfs_create_new_map_points on the host with the device's rule (csrc/triangulate_rule.hpp): per neighbour, per common node, every idx1
// in list order takes the candidate of minimum distance, last list position among equals, that no earlier idx1 of the node took.
inline int tri_solve_host(const gfs_tri_problem* problems, int B, gfs_tri_result* const* results) {
  auto cam = [](const gfs_tri_keyframe& k) {
    gfs_tri::Cam C{};
    std::memcpy(C.Tcw, k.Tcw, sizeof(k.Tcw));
    std::memcpy(C.Ow, k.Ow, sizeof(k.Ow));
    std::memcpy(C.Rwc, k.Rwc, sizeof(k.Rwc));
    std::memcpy(C.twc, k.twc, sizeof(k.twc));
    C.fx = k.fx, C.fy = k.fy, C.cx = k.cx, C.cy = k.cy, C.invfx = k.invfx, C.invfy = k.invfy, C.mbf = k.mbf, C.mb = k.mb;
    if (k.n_levels < 1 || k.n_levels > 16) throw std::invalid_argument("CreateNewMapPoints: 1..16 pyramid levels");
    C.n_levels = k.n_levels;
    for (int l = 0; l < k.n_levels; l++) C.scale[l] = k.scale_factors[l], C.sigma2[l] = k.level_sigma2[l];
    return C;
  };
  auto kp = [](const gfs_tri_keyframe& k, int i) {
    if (k.kps_un[i].octave < 0 || k.kps_un[i].octave >= k.n_levels) throw std::invalid_argument("CreateNewMapPoints: key-point octave outside the pyramid");
    return gfs_tri::Kp{k.kps_un[i].x, k.kps_un[i].y, k.kps_un[i].angle, k.kps[i].x, k.kps[i].y, k.u_right[i], k.depth[i], k.kps_un[i].octave};
  };
  for (int b = 0; b < B; b++) {
    const gfs_tri_problem& Q = problems[b];
    const gfs_tri_keyframe& K1 = Q.cur;
    const gfs_tri::Cam C1 = cam(K1);
    std::vector<uint8_t> has1(K1.has_mp, K1.has_mp + K1.n_kp);
    for (int i = 0; i < Q.n_neighbours; i++) {
      const gfs_tri_neighbour& NB = Q.neighbours[i];
      const gfs_tri_keyframe& K2 = NB.kf;
      const gfs_tri::Cam C2 = cam(K2);
      gfs_tri_result& R = results[b][i];
      for (int p = 0; p < K1.n_kp; p++) {
        R.match12[p] = -1;
        R.exit[p] = GFS_TRI_NO_MATCH;
        R.point_stereo[p] = 0;
        R.x3d[3 * p] = R.x3d[3 * p + 1] = R.x3d[3 * p + 2] = 0.0f;
      }
      std::vector<uint8_t> taken;
      for (int n1 = 0; n1 < K1.n_nodes; n1++) {
        const int32_t* e = std::lower_bound(K2.node_id, K2.node_id + K2.n_nodes, K1.node_id[n1]);
        if (e == K2.node_id + K2.n_nodes || *e != K1.node_id[n1]) continue;
        const int n2 = (int)(e - K2.node_id), b2 = K2.node_start[n2], c2 = K2.node_start[n2 + 1] - b2;
        taken.assign((size_t)c2, 0);
        for (int a = K1.node_start[n1]; a < K1.node_start[n1 + 1]; a++) {
          const int idx1 = K1.feat_idx[a];
          const bool st1 = K1.u_right[idx1] >= 0;
          if (has1[idx1] || (Q.only_stereo && !st1)) continue;
          const gfs_tri::Line line = gfs_tri::epipolar_line(NB.F12, K1.kps_un[idx1].x, K1.kps_un[idx1].y);
          int best = 256, at = -1;
          for (int c = 0; c < c2; c++) {
            const int idx2 = K2.feat_idx[b2 + c];
            const bool st2 = K2.u_right[idx2] >= 0;
            if (taken[c] || K2.has_mp[idx2] || (Q.only_stereo && !st2)) continue;
            int d = 0;
            for (int w = 0; w < 32; w++) d += __builtin_popcount((unsigned)(K1.desc[32 * (size_t)idx1 + w] ^ K2.desc[32 * (size_t)idx2 + w]));
            if (d > gfs_tri::kThLow || d > best) continue;
            const int o2 = K2.kps_un[idx2].octave;
            if (o2 < 0 || o2 >= K2.n_levels) throw std::invalid_argument("CreateNewMapPoints: key-point octave outside the pyramid");
            if (!gfs_tri::candidate_ok(line, NB.ep, st1, st2, K2.kps_un[idx2].x, K2.kps_un[idx2].y, K2.scale_factors[o2], K2.level_sigma2[o2], Q.coarse != 0))
              continue;
            best = d;
            at = c;
          }
          if (at >= 0) {
            taken[at] = 1;
            R.match12[idx1] = K2.feat_idx[b2 + at];
          }
        }
      }
      if (Q.check_orientation) {
        int hist[gfs_tri::kHisto] = {0}, ind1, ind2, ind3;
        for (int p = 0; p < K1.n_kp; p++)
          if (R.match12[p] >= 0) hist[gfs_tri::rot_bin(K1.kps_un[p].angle, K2.kps_un[R.match12[p]].angle)]++;
        gfs_tri::three_maxima(hist, ind1, ind2, ind3);
        for (int p = 0; p < K1.n_kp; p++) {
          if (R.match12[p] < 0) continue;
          const int bin = gfs_tri::rot_bin(K1.kps_un[p].angle, K2.kps_un[R.match12[p]].angle);
          if (bin != ind1 && bin != ind2 && bin != ind3) R.match12[p] = -1;
        }
      }
      R.n_matches = R.n_created = 0;
      for (int p = 0; p < K1.n_kp; p++) {
        if (R.match12[p] < 0) continue;
        int ps = 0;
        const int ex = gfs_tri::triangulate_match(C1, C2, kp(K1, p), kp(K2, R.match12[p]), Q.inertial != 0, Q.far_points != 0, Q.th_far_points,
                                                  Q.ratio_factor, R.x3d + 3 * p, &ps);
        R.exit[p] = (uint8_t)ex;
        R.point_stereo[p] = (uint8_t)ps;
        R.n_matches++;
        if (ex == GFS_TRI_CREATED) {
          has1[p] = 1;
          R.n_created++;
        }
      }
    }
  }
  return GFS_OK;
}

// LocalMapping::CreateNewMapPoints.  recent: mlpRecentAddedMapPoints.  -> the number of map points created.
template <class Access, class KeyFrame, class MapPoint, class Atlas, class Solve, class CheckNewKeyFrames>
int CreateNewMapPoints(Solve&& solve, KeyFrame* pCurrentKF, Atlas* atlas, std::list<MapPoint*>& recent, const CreateNewMapPointsParams& prm,
                       CheckNewKeyFrames&& check_new_key_frames) {
  // Retrieve neighbor keyframes in covisibility graph (:805-819)
  int nn = gfs_tri::kNeighbours;
  if (prm.monocular) nn = gfs_tri::kNeighboursMono;
  std::vector<KeyFrame*> vpNeighKFs = pCurrentKF->GetBestCovisibilityKeyFrames(nn);
  {
    KeyFrame* pKF = pCurrentKF;
    int count = 0;
    while (((int)vpNeighKFs.size() <= nn) && (pKF->mPrevKF) && (count++ < nn)) {
      if (std::find(vpNeighKFs.begin(), vpNeighKFs.end(), pKF->mPrevKF) == vpNeighKFs.end()) vpNeighKFs.push_back(pKF->mPrevKF);
      pKF = pKF->mPrevKF;
    }
  }
  std::vector<TriKeyFrameFlat> flat(vpNeighKFs.size() + 1);
  tri_gather<Access>(pCurrentKF, flat[0]);
  std::vector<gfs_tri_neighbour> nbs;
  std::vector<int> slot_of(vpNeighKFs.size(), -1);  // which uploaded neighbour an entry of the list is, -1 = short baseline
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    KeyFrame* pKF2 = vpNeighKFs[i];
    tri_gather<Access>(pKF2, flat[i + 1]);
    const float* Ow1 = flat[0].k.Ow;
    const float* Ow2 = flat[i + 1].k.Ow;
    const float v[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
    const float baseline = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);  // vBaseline.norm()
    if (!prm.monocular) {
      if (baseline < pKF2->mb) continue;
    } else {
      const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
      const float ratioBaselineDepth = baseline / medianDepthKF2;
      if (ratioBaselineDepth < 0.01) continue;
    }
    gfs_tri_neighbour nb{};
    nb.kf = flat[i + 1].k;
    Access::epipolar(*pCurrentKF, *pKF2, nb.ep, nb.F12);
    slot_of[i] = (int)nbs.size();
    nbs.push_back(nb);
  }
  gfs_tri_problem P{};
  P.cur = flat[0].k;
  P.neighbours = nbs.data();
  P.n_neighbours = (int32_t)nbs.size();
  P.only_stereo = 0;  // SearchForTriangulation(..., false, bCoarse) (:872)
  P.coarse = prm.coarse;
  P.check_orientation = 0;  // ORBmatcher matcher(th, false) (:824)
  P.inertial = prm.inertial;
  P.far_points = prm.far_points;
  P.th_far_points = prm.th_far_points;
  P.ratio_factor = gfs_tri::kRatioFactor * pCurrentKF->mfScaleFactor;
  std::vector<TriOutputs> outs(nbs.size());
  std::vector<gfs_tri_result> rs;
  for (TriOutputs& o : outs) rs.push_back(o.view((size_t)P.cur.n_kp));
  if (!nbs.empty()) {
    gfs_tri_result* rp = rs.data();
    check(solve(&P, 1, &rp), "gfs_create_new_map_points");
  }
  int created = 0;
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    if (i > 0 && check_new_key_frames()) return created;
    if (slot_of[i] < 0) continue;
    KeyFrame* pKF2 = vpNeighKFs[i];
    const TriOutputs& o = outs[(size_t)slot_of[i]];
    for (int idx1 = 0; idx1 < P.cur.n_kp; idx1++) {
      if (o.exit[idx1] != GFS_TRI_CREATED) continue;
      const int idx2 = o.match12[idx1];
      // Triangulation is succesfull (:1103-1124)
      MapPoint* pMP = Access::new_map_point(&o.x3d[3 * (size_t)idx1], pCurrentKF, atlas);
      pMP->AddObservation(pCurrentKF, idx1);
      pMP->AddObservation(pKF2, idx2);
      if (prm.use_optical_flow) Access::set_tracked_feature(pCurrentKF, idx1, pMP);
      pCurrentKF->AddMapPoint(pMP, idx1);
      pKF2->AddMapPoint(pMP, idx2);
      pMP->ComputeDistinctiveDescriptors();
      pMP->UpdateNormalAndDepth();
      atlas->AddMapPoint(pMP);
      recent.push_back(pMP);
      created++;
    }
  }
  return created;
}

// the numeric core of CreateNewMapPoints on the GPU: one handle, its reserve grown to the largest call seen
class MapPointCreator {
 public:
  MapPointCreator(int max_kp = 4096, int device = 0) { check(gfs_sbp_create(device, 64, max_kp, 1, &h_), "gfs_sbp_create"); }
  ~MapPointCreator() { gfs_sbp_destroy(h_); }
  MapPointCreator(const MapPointCreator&) = delete;
  MapPointCreator& operator=(const MapPointCreator&) = delete;
  int solve(const gfs_tri_problem* problems, int B, gfs_tri_result* const* results) {
    int nb = 1;
    int64_t pairs = 1;
    for (int b = 0; b < B; b++) {
      const gfs_tri_problem& Q = problems[b];
      nb = std::max(nb, (int)Q.n_neighbours);
      int64_t sum = 0;
      for (int i = 0; i < Q.n_neighbours; i++) {
        const gfs_tri_keyframe& K2 = Q.neighbours[i].kf;
        for (int n1 = 0, n2 = 0; n1 < Q.cur.n_nodes && n2 < K2.n_nodes;) {
          if (Q.cur.node_id[n1] < K2.node_id[n2]) n1++;
          else if (Q.cur.node_id[n1] > K2.node_id[n2]) n2++;
          else {
            sum += (int64_t)(Q.cur.node_start[n1 + 1] - Q.cur.node_start[n1]) * (K2.node_start[n2 + 1] - K2.node_start[n2]);
            n1++, n2++;
          }
        }
      }
      pairs = std::max(pairs, sum);
    }
    if (nb > neighbours_ || pairs > pairs_) {  // the library refuses what exceeds the reserve (it never truncates): grow it first
      const int n = std::max(nb, neighbours_);
      const int64_t p = std::max(pairs, pairs_);
      check(gfs_sbp_reserve_triangulation(h_, n, p), "gfs_sbp_reserve_triangulation");
      neighbours_ = n;
      pairs_ = p;
    }
    return gfs_create_new_map_points(h_, problems, B, results);
  }
  auto solver() {
    return [this](const gfs_tri_problem* p, int B, gfs_tri_result* const* r) { return solve(p, B, r); };
  }

 private:
  gfs_sbp* h_ = nullptr;
  int neighbours_ = 0;
  int64_t pairs_ = 0;
};

// Optimizer::PoseOptimization on a flattened frame (reference src/Optimizer.cc:763-1098)
class PoseOptimizer {
 public:
  PoseOptimizer(int max_obs = 8192, int device = 0) { check(gfs_pose_create(device, max_obs, 1, &h_), "gfs_pose_create"); }
  ~PoseOptimizer() { gfs_pose_destroy(h_); }
  // returns nInitialCorrespondences - nBad; s.outlier / s.chi2 must point to p.n_obs entries
  int PoseOptimization(const gfs_pose_problem& p, gfs_pose_solution& s) {
    check(gfs_pose_optimize(h_, &p, 1, &s), "gfs_pose_optimize");
    return s.n_inliers;
  }

 private:
  gfs_pose* h_ = nullptr;
};

// Optimizer::PoseLidarVisualOptimization (src/Optimizer.cc:7698-8059), conventional-SLAM branch.  The frame is read through an
// access type (no PCL / Sophus / OpenCV here), with static members:
//   int N(const F&); bool has_map_point(const F&, int i); void world_pos(const F&, int i, float xyz[3]);
//   void key_point(const F&, int i, float* x, float* y, int* octave); float u_right(const F&, int i); float inv_level_sigma2(const F&, int o);
//   void intrinsics(const F&, float* fx, float* fy, float* cx, float* cy, float* bf); bool two_camera(const F&);
//   void get_pose(const F&, float q[4], float t[3]); void set_pose(F&, const float q[4], const float t[3]); void set_outlier(F&, int i, bool);
// The local map (laserCloudSurfFromMapDS) is uploaded with SetLocalMap whenever the caller refreshes it; the frame's downsampled cloud
// (mpPointCloudDownsampled) is passed as xyz floats.  Writes back mvbOutlier, the pose (SetPose) and the two out-parameters.
class PoseLidarOptimizer {
 public:
  PoseLidarOptimizer(int max_obs = 8192, int max_cloud = 16384, int max_map = 262144, int device = 0) : max_map_(max_map), device_(device) {
    check(gfs_pose_lidar_create(device, max_obs, max_cloud, 1, &h_), "gfs_pose_lidar_create");
    const int rc = gfs_lidar_map_create(device, max_map, &map_);
    if (rc) {
      gfs_pose_lidar_destroy(h_);
      check(rc, "gfs_lidar_map_create");
    }
  }
  ~PoseLidarOptimizer() {
    gfs_pose_lidar_destroy(h_);
    gfs_lidar_map_destroy(map_);
  }
  PoseLidarOptimizer(const PoseLidarOptimizer&) = delete;
  PoseLidarOptimizer& operator=(const PoseLidarOptimizer&) = delete;
  void SetLocalMap(const float* xyz, int n) { check(gfs_lidar_map_set(map_, xyz, n), "gfs_lidar_map_set"); }
  // The local map built on the device from lNewKeyFrames (LidarLocalMapper::Update) instead of uploaded
  template <class Access, class It>
  gfs_lidar_map_info BuildLocalMap(It first, It last, float resolution) {
    if (!mapper_) mapper_.reset(new LidarLocalMapper(max_map_, 30, device_));
    return mapper_->template Update<Access>(first, last, resolution, map_);
  }

  template <class Access, class F>
  int PoseLidarVisualOptimization(F* frame, const float* cloud_xyz, int n_cloud, int nIterations, int& nLidarInliers, float& residual) {
    gfs_pose_lidar_problem p{};
    Access::get_pose(*frame, p.q, p.t);
    float fx, fy, cx, cy, bf;
    Access::intrinsics(*frame, &fx, &fy, &cx, &cy, &bf);
    p.fx = fx;
    p.fy = fy;
    p.cx = cx;
    p.cy = cy;
    p.bf = bf;
    p.two_camera = Access::two_camera(*frame) ? 1 : 0;
    idx_.clear();
    xw_.clear();
    obs_.clear();
    w_.clear();
    st_.clear();
    const int N = Access::N(*frame);
    for (int i = 0; i < N; i++) {  // key-point index order = the reference's edge creation order
      if (!Access::has_map_point(*frame, i)) continue;
      float X[3], x, y, ur = Access::u_right(*frame, i);
      int octave;
      Access::world_pos(*frame, i, X);
      Access::key_point(*frame, i, &x, &y, &octave);
      idx_.push_back(i);
      for (int k = 0; k < 3; k++) xw_.push_back((double)X[k]);
      obs_.push_back((double)x);
      obs_.push_back((double)y);
      obs_.push_back((double)ur);
      w_.push_back(Access::inv_level_sigma2(*frame, octave));
      st_.push_back(ur < 0 ? 0 : 1);
    }
    const int n = (int)idx_.size();
    outlier_.assign(std::max(n, 1), 0);
    chi2_.assign(std::max(n, 1), 0.0);
    p.n_obs = n;
    p.xw = xw_.data();
    p.obs = obs_.data();
    p.inv_sigma2 = w_.data();
    p.stereo = st_.data();
    p.n_cloud = n_cloud;
    p.cloud = cloud_xyz;
    p.map = map_;
    p.n_iterations = nIterations;
    gfs_pose_lidar_solution s{};
    s.outlier = outlier_.data();
    s.chi2 = chi2_.data();
    s.n_lidar_inliers = nLidarInliers;
    s.residual = residual;
    check(gfs_pose_lidar_optimize(h_, &p, 1, &s), "gfs_pose_lidar_optimize");
    for (int k = 0; k < n; k++) Access::set_outlier(*frame, idx_[k], outlier_[k] != 0);  // all false when n < 3 (:7754, :7782)
    if (n < 3) return 0;  // nInitialCorrespondences < 3: return 0 before SetPose
    Access::set_pose(*frame, s.qf, s.tf);
    nLidarInliers = s.n_lidar_inliers;
    residual = s.residual;
    return s.n_inliers;
  }

 private:
  gfs_pose_lidar* h_ = nullptr;
  gfs_lidar_map* map_ = nullptr;
  int max_map_ = 0, device_ = 0;
  std::unique_ptr<LidarLocalMapper> mapper_;  // created at the first BuildLocalMap
  std::vector<int> idx_;
  std::vector<double> xw_, obs_, chi2_;
  std::vector<float> w_;
  std::vector<uint8_t> st_, outlier_;
};

// ------------------------------------------------------------------------------------------------------------------------
// Optimizer::BundleAdjustment(const vector<KeyFrame*>& vpKFs, const vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag,
//                             const unsigned long nLoopKF, const bool bRobust)                  reference src/Optimizer.cc:56-363
// and Optimizer::GlobalBundleAdjustemnt(Map*, ...) (:47-54) as real code around the flat solver, line for line: bad key-frames
// skipped and maxKFid (:113-124), the init key-frame fixed (:121), per map point the `pKF->isBad() || pKF->mnId > maxKFid` and
// null-vertex filters (:148-150), mono against stereo decided by mvuRight (:155, :185-186), a point with nEdges == 0 dropped and
// vbNotIncludedMP set (:263-268), optimize(nIterations) with the caller's flag handed down (:78, :274), and both write-back
// branches (:279-362): nLoopKF == pMap->GetOriginKF()->mnId -> SetPose / SetWorldPos + UpdateNormalAndDepth, otherwise mTcwGBA,
// mPosGBA and mnBAGlobalForKF.  There is no stop-flag check in front of optimize() and no chi2 classification behind it.
//
// The block under `dist > 1` (:298-341) only counts inliers and outliers into locals that nothing reads: it is left out.
//
// Classes as for LocalBundleAdjustment, plus Map::GetOriginKF(), KeyFrame::mnBAGlobalForKF, MapPoint::mnBAGlobalForKF and two more
// functions of `Access`:
//     static void set_pose_gba(KeyFrame*, const double q_xyzw[4], const double t[3]);  // mTcwGBA = Sophus::SE3d(q, t).cast<float>()
//     static void set_pos_gba(MapPoint*, const float p[3]);                            // mPosGBA
// Arithmetic on the way in and out as in LocalBundleAdjustment; the Huber deltas here are `const float thHuber2D = sqrt(5.99)`
// (5.99, not 5.991: :126) and `thHuber3D = sqrt(7.815)`; bRobust = false (no setRobustKernel, :172, :205) is +infinity for both
// (include/gfs_abi.h).  Second-camera observations (EdgeSE3ProjectXYZToBody, :224-260) are refused.
// `solve(problem, solution, pbStopFlag)` is the numeric core: GlobalBundleAdjuster::solve (gfs_gba_solve on the GPU).
// ------------------------------------------------------------------------------------------------------------------------
template <class Access, class KeyFrame, class MapPoint, class Solve>
void BundleAdjustment(Solve&& solve, const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations = 5,
                      bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0, const bool bRobust = true) {
  std::vector<bool> vbNotIncludedMP;
  vbNotIncludedMP.resize(vpMP.size());
  auto* pMap = vpKFs[0]->GetMap();
  unsigned long maxKFid = 0;
  // ---- key-frame vertices (:113-124): pose index = creation order
  LbaFlat F;
  std::map<const KeyFrame*, int32_t> pose_index;  // == optimizer.vertex(pKF->mnId) != NULL
  for (size_t i = 0; i < vpKFs.size(); i++) {
    KeyFrame* pKF = vpKFs[i];
    if (pKF->isBad()) continue;
    float q[4], t[3];
    Access::pose(pKF, q, t);
    pose_index[pKF] = (int32_t)F.pose_fixed.size();
    for (int k = 0; k < 4; k++) F.pose_q.push_back((double)q[k]);
    for (int k = 0; k < 3; k++) F.pose_t.push_back((double)t[k]);
    F.pose_fixed.push_back(pKF->mnId == pMap->GetInitKFid() ? 1 : 0);
    if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
  }
  // ---- map-point vertices and their edges (:130-269)
  std::vector<int32_t> point_of(vpMP.size(), -1);  // flat point of vpMP[i]; -1: bad or without an edge
  for (size_t i = 0; i < vpMP.size(); i++) {
    MapPoint* pMP = vpMP[i];
    if (pMP->isBad()) continue;
    float X[3];
    Access::world_pos(pMP, X);
    const int32_t point_index = (int32_t)(F.points.size() / 3);
    const size_t edges_before = F.edge_pose.size();
    const auto observations = pMP->GetObservations();
    int nEdges = 0;
    for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
      KeyFrame* pKF = mit->first;
      if (pKF->isBad() || pKF->mnId > maxKFid) continue;
      const auto pit = pose_index.find(pKF);
      if (pit == pose_index.end()) continue;  // optimizer.vertex(pKF->mnId) == NULL
      nEdges++;
      const int leftIndex = std::get<0>(mit->second);
      if (leftIndex != -1) {
        const bool stereo = pKF->mvuRight[leftIndex] >= 0;
        const auto& kpUn = pKF->mvKeysUn[leftIndex];
        F.edge_pose.push_back(pit->second);
        F.edge_point.push_back(point_index);
        F.edge_obs.push_back((double)kpUn.pt.x);
        F.edge_obs.push_back((double)kpUn.pt.y);
        F.edge_obs.push_back(stereo ? (double)pKF->mvuRight[leftIndex] : 0.0);
        const float& invSigma2 = pKF->mvInvLevelSigma2[kpUn.octave];
        F.edge_inv_sigma2.push_back((double)invSigma2);
        F.edge_stereo.push_back(stereo ? 1 : 0);
      }
      if (pKF->mpCamera2 && std::get<1>(mit->second) != -1)
        throw std::runtime_error("BundleAdjustment: second-camera observations (EdgeSE3ProjectXYZToBody) are not supported");
    }
    if (nEdges == 0) {  // optimizer.removeVertex(vPoint)
      vbNotIncludedMP[i] = true;
    } else {
      vbNotIncludedMP[i] = false;
      if (F.edge_pose.size() == edges_before)  // (counted observations, none of them in the left image: a vertex without an edge)
        throw std::runtime_error("BundleAdjustment: a map point seen by second cameras only is not supported");
      for (int k = 0; k < 3; k++) F.points.push_back((double)X[k]);
      point_of[i] = point_index;
    }
  }
  KeyFrame* first = nullptr;
  for (KeyFrame* pKF : vpKFs)
    if (!pKF->isBad()) {
      first = pKF;
      break;
    }
  if (!first) return;  // (the reference would optimise an empty graph and write nothing back)
  F.finish(first->fx, first->fy, first->cx, first->cy, first->mbf);
  const float thHuber2D = (float)std::sqrt(5.99), thHuber3D = (float)std::sqrt(7.815);  // :126-127
  F.problem.huber_mono = bRobust ? (double)thHuber2D : (double)INFINITY;
  F.problem.huber_stereo = bRobust ? (double)thHuber3D : (double)INFINITY;
  F.problem.iterations = nIterations;
  // ---- optimizer.initializeOptimization(); optimizer.optimize(nIterations);  (no entry check)
  std::vector<double> out_q(F.pose_q.size()), out_t(F.pose_t.size()), out_p(F.points.size());
  gfs_lba_solution S{};
  S.pose_q = out_q.data();
  S.pose_t = out_t.data();
  S.points = out_p.data();
  solve(F.problem, S, pbStopFlag);
  // ---- recover optimised data: key-frames (:279-343)
  const bool in_place = nLoopKF == pMap->GetOriginKF()->mnId;
  for (size_t i = 0; i < vpKFs.size(); i++) {
    KeyFrame* pKF = vpKFs[i];
    if (pKF->isBad()) continue;
    const size_t k = (size_t)pose_index[pKF];
    if (in_place) {
      float q[4], t[3];
      for (int c = 0; c < 4; c++) q[c] = (float)out_q[4 * k + c];
      for (int c = 0; c < 3; c++) t[c] = (float)out_t[3 * k + c];
      Access::set_pose(pKF, q, t);
    } else {
      Access::set_pose_gba(pKF, &out_q[4 * k], &out_t[3 * k]);
      pKF->mnBAGlobalForKF = nLoopKF;
    }
  }
  // ---- points (:346-362)
  for (size_t i = 0; i < vpMP.size(); i++) {
    if (vbNotIncludedMP[i]) continue;
    MapPoint* pMP = vpMP[i];
    if (pMP->isBad()) continue;
    float X[3];
    for (int c = 0; c < 3; c++) X[c] = (float)out_p[3 * (size_t)point_of[i] + c];
    if (in_place) {
      Access::set_world_pos(pMP, X);
      pMP->UpdateNormalAndDepth();
    } else {
      Access::set_pos_gba(pMP, X);
      pMP->mnBAGlobalForKF = nLoopKF;
    }
  }
}

// Optimizer::GlobalBundleAdjustemnt (src/Optimizer.cc:47-54)
template <class Access, class Map, class Solve>
void GlobalBundleAdjustemnt(Solve&& solve, Map* pMap, int nIterations = 5, bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0,
                            const bool bRobust = true) {
  auto vpKFs = pMap->GetAllKeyFrames();
  auto vpMP = pMap->GetAllMapPoints();
  using KeyFrame = typename std::remove_pointer<typename decltype(vpKFs)::value_type>::type;
  using MapPoint = typename std::remove_pointer<typename decltype(vpMP)::value_type>::type;
  BundleAdjustment<Access, KeyFrame, MapPoint>(solve, vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

// numeric core of Optimizer::BundleAdjustment: the full map on the device (gfs_gba_solve)
class GlobalBundleAdjuster {
 public:
  GlobalBundleAdjuster(int max_poses = 2048, int max_points = 262144, int max_edges = 4194304, int device = 0) {
    check(gfs_gba_create(device, max_poses, max_points, max_edges, &h_), "gfs_gba_create");
  }
  ~GlobalBundleAdjuster() { gfs_gba_destroy(h_); }
  GlobalBundleAdjuster(const GlobalBundleAdjuster&) = delete;
  GlobalBundleAdjuster& operator=(const GlobalBundleAdjuster&) = delete;
  // the caller's flag itself goes down (&mbStopGBA): read live at the top of every iteration and after every rejected trial
  void solve(const gfs_lba_problem& p, gfs_lba_solution& s, const bool* pbStopFlag) {
    static_assert(sizeof(bool) == 1, "gfs_gba_solve_bool reads the flag as one byte");
    check(gfs_gba_solve_bool(h_, &p, &s, reinterpret_cast<const volatile unsigned char*>(pbStopFlag)), "gfs_gba_solve");
  }
  template <class Access, class Map>
  void GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0,
                              const bool bRobust = true) {
    gfs_host::GlobalBundleAdjustemnt<Access>([this](const gfs_lba_problem& p, gfs_lba_solution& s, const bool* stop) { this->solve(p, s, stop); },
                                             pMap, nIterations, pbStopFlag, nLoopKF, bRobust);
  }

 private:
  gfs_gba* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph(Map*, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale,
//                                   bUseICPConstraint)                                       reference src/Optimizer.cc:2042-2413
// as real code around the flat solver, line for line.  Vertices (:2099-2136): one per key-frame that is not bad, the estimate from
// CorrectedSim3 or GetPose().cast<double>() with scale 1, the init key-frame fixed.  Edges in creation order: the loop connections
// (:2147-2186; the weight test spares the (pCurKF, pLoopKF) pair; a missing vertex skips the edge, :2170), then per key-frame --
// bad ones too, this loop has no isBad() test -- the spanning-tree edge (a missing vertex ends the KEY-FRAME, the `continue` of
// :2224-2225 sits in the key-frame loop), the loop edges to older key-frames (:2236-2290; a missing vertex skips the edge, :2254)
// each followed, with bUseICPConstraint, by a registration whose accepted result becomes an edge of information 3 I, the
// covisibility edges of weight >= 100 that are neither parent nor child nor already inserted (:2294-2331; :2319 skips one edge), and
// the inertial edge to mPrevKF (:2334-2355; a missing vertex ends the key-frame there too, :2345-2347).  Every measurement is
// Sjw * Swi with NonCorrectedSim3 where it has the key-frame, vScw else.  Then optimize(20), and under mMutexMapUpdate the poses
// (:2369-2383) and every map point that is not bad through its reference key-frame (:2387-2409), UpdateNormalAndDepth, and
// IncreaseChangeIndex.  A reference key-frame without a vertex has default Sim3s in vScw and vCorrectedSwc: the point keeps its
// position (reference -1).
//
// Classes as for BundleAdjustment, plus KeyFrame::GetParent(), GetLoopEdges(), GetCovisiblesByWeight(int), hasChild(), GetWeight(),
// bImu, mPrevKF; MapPoint::mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame(); Map::GetAllKeyFrames(), GetAllMapPoints();
// the two KeyFrameAndPose maps and LoopConnections as the reference passes them; and of `Access`:
//     static void pose_d(const KeyFrame*, double q_xyzw[4], double t[3]);  // GetPose().cast<double>(): unit_quaternion(), translation()
//     static void sim3(const Sim3&, double S[8]);          // g2o::Sim3 -> rotation().coeffs() (x, y, z, w), translation(), scale()
//     static void set_pose(KeyFrame*, const float q_xyzw[4], const float t[3]);   // SetPose(Sophus::SE3f(q, t))
//     static void world_pos / set_world_pos                                       // as above
// `solve(problem, solution)` is the numeric core (EssentialGraphOptimizer::solve: gfs_essential_graph_optimize on the GPU);
// `reg(pLKF, pKF, init_T_target_source[16]) -> gfs_gicp_result` is mpRegistration->RegisterPointClouds(*pLKF->source_points,
// *pKF->source_points, init_T).
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kEssentialGraphMinFeat = 100;            // :2075
constexpr int kEssentialGraphIterations = 20;          // :2362
constexpr double kEssentialGraphLambdaInit = 1e-16;    // :2058
constexpr double kEssentialGraphIcpInformation = 3.0;  // :2285
constexpr uint64_t kEssentialGraphIcpMinInliers = 100;  // :2277
constexpr double kEssentialGraphIcpMaxError = 0.1;     // :2278

struct EssentialGraphFlat {
  std::vector<double> vq, vt, vs, eq, et, es, ew;
  std::vector<uint8_t> vfixed;
  std::vector<int32_t> ei, ej, pref;
  std::vector<float> points;
  void add_edge(int32_t i, int32_t j, const double S[8], double w) {
    ei.push_back(i);
    ej.push_back(j);
    eq.insert(eq.end(), S, S + 4);
    et.insert(et.end(), S + 4, S + 7);
    es.push_back(S[7]);
    ew.push_back(w);
  }
};

template <class Access, class Map, class KeyFrame, class KeyFrameAndPose, class LoopConnectionsT, class Solve, class Register>
void OptimizeEssentialGraph(Solve&& solve, Register&& reg, Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
                            const KeyFrameAndPose& CorrectedSim3, const LoopConnectionsT& LoopConnections, const bool& bFixScale,
                            const bool& bUseICPConstraint) {
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMPs = pMap->GetAllMapPoints();
  const int minFeat = kEssentialGraphMinFeat;
  EssentialGraphFlat F;
  std::map<unsigned long, int32_t> vertex;  // mnId -> flat vertex: optimizer.vertex(id) != NULL
  std::vector<double> vScw;                 // [vertex][8]
  auto has = [&](unsigned long id) { return vertex.find(id) != vertex.end(); };
  auto scw = [&](unsigned long id) { return &vScw[8 * (size_t)vertex.find(id)->second]; };
  // ---- key-frame vertices (:2099-2136)
  for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
    KeyFrame* pKF = vpKFs[i];
    if (pKF->isBad()) continue;
    double S[8];
    auto it = CorrectedSim3.find(pKF);
    if (it != CorrectedSim3.end()) {
      Access::sim3(it->second, S);
    } else {
      Access::pose_d(pKF, S, S + 4);
      S[7] = 1.0;
    }
    vertex[pKF->mnId] = (int32_t)F.vs.size();
    vScw.insert(vScw.end(), S, S + 8);
    F.vq.insert(F.vq.end(), S, S + 4);
    F.vt.insert(F.vt.end(), S + 4, S + 7);
    F.vs.push_back(S[7]);
    F.vfixed.push_back(pKF->mnId == pMap->GetInitKFid() ? 1 : 0);
  }
  std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
  // the Sim3 an edge is measured on: NonCorrectedSim3 where it has the key-frame, vScw else (a default Sim3 without a vertex)
  auto measured = [&](KeyFrame* pKF, double S[8]) {
    auto it = NonCorrectedSim3.find(pKF);
    if (it != NonCorrectedSim3.end()) {
      Access::sim3(it->second, S);
    } else if (has(pKF->mnId)) {
      std::memcpy(S, scw(pKF->mnId), 8 * sizeof(double));
    } else {
      const double I[8] = {0, 0, 0, 1, 0, 0, 0, 1};
      std::memcpy(S, I, sizeof(I));
    }
  };
  // ---- loop edges (:2147-2186)
  for (auto mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
    KeyFrame* pKF = mit->first;
    const unsigned long nIDi = pKF->mnId;
    const auto& spConnections = mit->second;
    for (auto sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
      const unsigned long nIDj = (*sit)->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
      if (!has(nIDj) || !has(nIDi)) continue;
      double Swi[8], Sji[8];
      gfs_sim3::sim3_inverse(scw(nIDi), Swi);
      gfs_sim3::sim3_mul(scw(nIDj), Swi, Sji);
      F.add_edge(vertex[nIDi], vertex[nIDj], Sji, 1.0);
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // ---- normal edges (:2190-2356)
  for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
    KeyFrame* pKF = vpKFs[i];
    const unsigned long nIDi = pKF->mnId;
    double Siw[8], Swi[8];
    measured(pKF, Siw);
    gfs_sim3::sim3_inverse(Siw, Swi);
    KeyFrame* pParentKF = pKF->GetParent();
    // spanning tree edge
    if (pParentKF) {
      const unsigned long nIDj = pParentKF->mnId;
      double Sjw[8], Sji[8];
      measured(pParentKF, Sjw);
      gfs_sim3::sim3_mul(Sjw, Swi, Sji);
      if (!has(nIDj) || !has(nIDi)) continue;  // (the rest of this key-frame goes with it)
      F.add_edge(vertex[nIDi], vertex[nIDj], Sji, 1.0);
    }
    // loop edges
    const auto sLoopEdges = pKF->GetLoopEdges();
    for (auto sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
      KeyFrame* pLKF = *sit;
      if (pLKF->mnId < pKF->mnId) {
        double Slw[8], Sli[8];
        measured(pLKF, Slw);
        gfs_sim3::sim3_mul(Slw, Swi, Sli);
        if (!has(pLKF->mnId) || !has(nIDi)) continue;
        F.add_edge(vertex[nIDi], vertex[pLKF->mnId], Sli, 1.0);
        if (bUseICPConstraint) {
          double R[9], init_T[16] = {0};  // column-major: linear() = Sli.rotation().toRotationMatrix(), translation() = t / s
          gfs_sim3::quat_to_R(Sli, R);
          for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) init_T[4 * c + r] = R[3 * r + c];
          for (int r = 0; r < 3; r++) init_T[12 + r] = Sli[4 + r] / Sli[7];
          init_T[15] = 1.0;
          const gfs_gicp_result result = reg(pLKF, pKF, init_T);
          double icp[8], Ricp[9];
          for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Ricp[3 * r + c] = result.T_target_source[4 * c + r];
          gfs_sim3::R_to_quat(Ricp, icp);
          for (int r = 0; r < 3; r++) icp[4 + r] = result.T_target_source[12 + r];
          icp[7] = 1.0;
          if (result.converged && result.num_inliers > kEssentialGraphIcpMinInliers &&
              (result.error / result.num_inliers) < kEssentialGraphIcpMaxError)
            F.add_edge(vertex[nIDi], vertex[pLKF->mnId], icp, kEssentialGraphIcpInformation);
        }
      }
    }
    // covisibility graph edges
    const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
      KeyFrame* pKFn = *vit;
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          double Snw[8], Sni[8];
          measured(pKFn, Snw);
          gfs_sim3::sim3_mul(Snw, Swi, Sni);
          if (!has(pKFn->mnId) || !has(nIDi)) continue;
          F.add_edge(vertex[nIDi], vertex[pKFn->mnId], Sni, 1.0);
        }
      }
    }
    // inertial edges if inertial
    if (pKF->bImu && pKF->mPrevKF) {
      double Spw[8], Spi[8];
      measured(pKF->mPrevKF, Spw);
      gfs_sim3::sim3_mul(Spw, Swi, Spi);
      if (!has(pKF->mPrevKF->mnId) || !has(nIDi)) continue;
      F.add_edge(vertex[nIDi], vertex[pKF->mPrevKF->mnId], Spi, 1.0);
    }
  }
  // ---- the map points and their reference vertices (:2387-2401)
  F.points.resize(3 * vpMPs.size());
  F.pref.assign(vpMPs.size(), -1);
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    unsigned long nIDr;
    if (pMP->mnCorrectedByKF == pCurKF->mnId)
      nIDr = pMP->mnCorrectedReference;
    else
      nIDr = pMP->GetReferenceKeyFrame()->mnId;
    Access::world_pos(pMP, &F.points[3 * i]);
    if (has(nIDr)) F.pref[i] = vertex[nIDr];
  }
  if (F.vs.empty()) return;  // (the reference would optimise an empty graph and move nothing)
  // ---- optimizer.initializeOptimization(); optimizer.optimize(20)
  gfs_essential_graph_problem P{};
  P.n_vertices = (int32_t)F.vs.size();
  P.n_edges = (int32_t)F.ei.size();
  P.n_points = (int32_t)F.pref.size();
  P.vertex_q = F.vq.data();
  P.vertex_t = F.vt.data();
  P.vertex_s = F.vs.data();
  P.vertex_fixed = F.vfixed.data();
  P.edge_i = F.ei.data();
  P.edge_j = F.ej.data();
  P.edge_q = F.eq.data();
  P.edge_t = F.et.data();
  P.edge_s = F.es.data();
  P.edge_w = F.ew.data();
  P.fix_scale = bFixScale ? 1 : 0;
  P.iterations = kEssentialGraphIterations;
  P.lambda_init = kEssentialGraphLambdaInit;
  P.points = F.points.data();
  P.point_ref = F.pref.data();
  std::vector<double> oq(F.vq.size()), ot(F.vt.size()), os(F.vs.size());
  std::vector<float> op(F.points.size());
  gfs_essential_graph_solution S{};
  S.vertex_q = oq.data();
  S.vertex_t = ot.data();
  S.vertex_s = os.data();
  S.points = op.data();
  solve(P, S);
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  // SE3 pose recovering.  Sim3: [sR t; 0 1] -> SE3: [R t/s; 0 1]  (:2369-2383)
  for (size_t i = 0; i < vpKFs.size(); i++) {
    KeyFrame* pKFi = vpKFs[i];
    if (!pKFi) continue;
    if (!has(pKFi->mnId)) continue;
    const size_t k = (size_t)vertex[pKFi->mnId];
    float q[4], t[3];
    for (int c = 0; c < 4; c++) q[c] = (float)oq[4 * k + c];
    for (int c = 0; c < 3; c++) t[c] = (float)ot[3 * k + c] / (float)os[k];  // translation().cast<float>() / s
    Access::set_pose(pKFi, q, t);
  }
  // correct points (:2387-2409)
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    Access::set_world_pos(pMP, &op[3 * i]);
    pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}

// numeric core of Optimizer::OptimizeEssentialGraph: the pose graph on the device (gfs_essential_graph_optimize).  The ICP edges come
// from RegistrationGICP above, with `static const float* source_points(const KeyFrame*, int* n)` of Access ([n][4] floats).
class EssentialGraphOptimizer {
 public:
  EssentialGraphOptimizer(int max_vertices = 4096, int max_edges = 65536, int max_points = 1048576, int device = 0) : device_(device) {
    check(gfs_essential_graph_create(device, max_vertices, max_edges, max_points, &h_), "gfs_essential_graph_create");
  }
  ~EssentialGraphOptimizer() { gfs_essential_graph_destroy(h_); }
  EssentialGraphOptimizer(const EssentialGraphOptimizer&) = delete;
  EssentialGraphOptimizer& operator=(const EssentialGraphOptimizer&) = delete;
  void solve(const gfs_essential_graph_problem& p, gfs_essential_graph_solution& s) {
    check(gfs_essential_graph_optimize(h_, &p, &s), "gfs_essential_graph_optimize");
  }
  template <class Access, class Map, class KeyFrame, class KeyFrameAndPose, class LoopConnectionsT>
  void OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
                              const KeyFrameAndPose& CorrectedSim3, const LoopConnectionsT& LoopConnections, const bool& bFixScale,
                              const bool& bUseICPConstraint = false) {
    auto reg = [this](const KeyFrame* pLKF, const KeyFrame* pKF, const double init_T[16]) {
      if (!gicp_) gicp_.reset(new RegistrationGICP(65536, device_));
      int nt = 0, ns = 0;
      const float* target = Access::source_points(pLKF, &nt);
      const float* source = Access::source_points(pKF, &ns);
      return gicp_->RegisterPointClouds(target, nt, source, ns, init_T);
    };
    gfs_host::OptimizeEssentialGraph<Access>([this](const gfs_essential_graph_problem& p, gfs_essential_graph_solution& s) { this->solve(p, s); },
                                             reg, pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale,
                                             bUseICPConstraint);
  }

 private:
  gfs_essential_graph* h_ = nullptr;
  std::unique_ptr<RegistrationGICP> gicp_;
  int device_;
};

// ------------------------------------------------------------------------------------------------------------------------
// int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
//                             const bool bFixScale, Eigen::Matrix<double, 7, 7>& mAcumHessian, const bool bAllPoints)
//                                                                                          reference src/Optimizer.cc:2797-3054
// as real code around the flat solver.  Everything of :2815-2984 that touches pointers runs here, with the
// caller's own Eigen as the reference writes it: P3D1c = R1w * P3D1w + t1w in float, cast to double; the skips (no match; a bad point:
// nBadMPs; no pMP1: nMatchWithoutMP; i2 < 0 && !bAllPoints; P3D2c(2) < 0) in the reference's order; the i2 < 0 branch's float
// invz, x, y.  The pairs that get edges are compacted, vnIndexEdge kept.  After the solve vpMatches1[idx] is nulled for the pairs the
// first check removed (also when the early return follows) and for those the final check rejects; g2oS12 is written and mAcumHessian
// zeroed (:3031: it is never filled) only when both optimizations ran; the return value is nIn, or 0 after the early return.
// One thing reads differently from what its text suggests: cv::KeyPoint(cv::Point2f(x, y), pMP2->mnTrackScaleLevel) (:2957) passes
// the level as the key-point's SIZE; its octave stays 0, so the i2 < 0 branch weighs its edge with pKF2->mvInvLevelSigma2[0].
// Single-camera pinhole key frames only (NLeft == -1, Access::is_pinhole): anything else throws.
// Classes as for the Sim3 searches, plus KeyFrame::GetRotation(), GetTranslation() (Eigen floats), mvKeysUn, mvInvLevelSigma2, fx, fy,
// cx, cy; MapPoint::GetWorldPos(), GetIndexInKeyFrame(), isBad(); and of `Access`:
//     static void sim3(const Sim3&, double S[8]);      // g2o::Sim3 -> rotation().coeffs() (x, y, z, w), translation(), scale()
//     static void set_sim3(Sim3&, const double S[8]);  // g2oS12 = g2o::Sim3(Quaterniond(w, x, y, z), t, s): as they are, not renormalised
// `solve(problem, solution)` is the numeric core: Sim3Optimizer::solve below (gfs_sim3_optimize on the GPU).
// ------------------------------------------------------------------------------------------------------------------------
struct Sim3OptCounters {  // the reference's local counters (:2845-2849, :2991-2992), for whoever wants to log them
  int nCorrespondences = 0, nBadMPs = 0, nInKF2 = 0, nOutKF2 = 0, nMatchWithoutMP = 0, nBad = 0, nBadOutKF2 = 0;
};

template <class Access, class KeyFrame, class MapPoint, class Sim3, class Hessian, class Solve>
int OptimizeSim3(Solve&& solve, KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, Sim3& g2oS12, const float th2,
                 const bool bFixScale, Hessian& mAcumHessian, const bool bAllPoints, Sim3OptCounters* counters = nullptr) {
  if (pKF1->NLeft != -1 || pKF2->NLeft != -1 || !Access::is_pinhole(*pKF1) || !Access::is_pinhole(*pKF2))
    throw std::invalid_argument("OptimizeSim3: single-camera pinhole key frames only");
  // Camera poses
  const auto R1w = pKF1->GetRotation();
  const auto t1w = pKF1->GetTranslation();
  const auto R2w = pKF2->GetRotation();
  const auto t2w = pKF2->GetTranslation();
  using Vector3f = typename std::decay<decltype(t1w)>::type;

  const int N = vpMatches1.size();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  std::vector<size_t> vnIndexEdge;
  std::vector<bool> vbIsInKF2;
  std::vector<double> x1c, x2c, obs1, obs2;
  std::vector<float> w1, w2;
  Sim3OptCounters c;

  for (int i = 0; i < N; i++) {
    if (!vpMatches1[i]) continue;

    MapPoint* pMP1 = vpMapPoints1[i];
    MapPoint* pMP2 = vpMatches1[i];

    const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));

    Vector3f P3D1c;
    Vector3f P3D2c;

    if (pMP1 && pMP2) {
      if (!pMP1->isBad() && !pMP2->isBad()) {
        Vector3f P3D1w = pMP1->GetWorldPos();
        P3D1c = R1w * P3D1w + t1w;
        Vector3f P3D2w = pMP2->GetWorldPos();
        P3D2c = R2w * P3D2w + t2w;
      } else {
        c.nBadMPs++;
        continue;
      }
    } else {
      c.nMatchWithoutMP++;
      continue;  // (the reference adds a lone vertex for pMP2 here: no edge ever uses it)
    }

    if (i2 < 0 && !bAllPoints) continue;

    if (P3D2c(2) < 0) continue;

    c.nCorrespondences++;

    // Set edge x1 = S12*X2
    const auto& kpUn1 = pKF1->mvKeysUn[i];
    obs1.push_back(kpUn1.pt.x);
    obs1.push_back(kpUn1.pt.y);
    w1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);

    // Set edge x2 = S21*X1
    if (i2 >= 0) {
      const auto& kpUn2 = pKF2->mvKeysUn[i2];
      obs2.push_back(kpUn2.pt.x);
      obs2.push_back(kpUn2.pt.y);
      w2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
      c.nInKF2++;
    } else {
      float invz = 1 / P3D2c(2);
      float x = P3D2c(0) * invz;
      float y = P3D2c(1) * invz;
      obs2.push_back(x);
      obs2.push_back(y);
      w2.push_back(pKF2->mvInvLevelSigma2[0]);  // cv::KeyPoint(pt, size = mnTrackScaleLevel): octave 0
      c.nOutKF2++;
    }
    for (int k = 0; k < 3; k++) {
      x1c.push_back((double)P3D1c(k));
      x2c.push_back((double)P3D2c(k));
    }
    vnIndexEdge.push_back(i);
    vbIsInKF2.push_back(i2 >= 0);
  }

  const int n = (int)vnIndexEdge.size();
  gfs_sim3_opt_problem p{};
  Access::sim3(g2oS12, p.s12);
  p.cam1[0] = pKF1->fx, p.cam1[1] = pKF1->fy, p.cam1[2] = pKF1->cx, p.cam1[3] = pKF1->cy;
  p.cam2[0] = pKF2->fx, p.cam2[1] = pKF2->fy, p.cam2[2] = pKF2->cx, p.cam2[3] = pKF2->cy;
  p.th2 = th2;
  p.fix_scale = bFixScale ? 1 : 0;
  p.n_pairs = n;
  p.x1c = x1c.data();
  p.x2c = x2c.data();
  p.obs1 = obs1.data();
  p.obs2 = obs2.data();
  p.inv_sigma2_1 = w1.data();
  p.inv_sigma2_2 = w2.data();
  std::vector<uint8_t> state(n + 1, 0);
  gfs_sim3_opt_solution s{};
  s.pair_state = state.data();
  solve(p, s);

  for (int i = 0; i < n; i++) {
    if (state[i] == GFS_SIM3_PAIR_INLIER) continue;
    vpMatches1[vnIndexEdge[i]] = static_cast<MapPoint*>(NULL);
    if (state[i] == GFS_SIM3_PAIR_REMOVED_FIRST && !vbIsInKF2[i]) c.nBadOutKF2++;
  }
  c.nBad = s.n_bad;
  if (counters) *counters = c;
  if (s.status != GFS_SIM3_OPT_BOTH_PHASES) return 0;  // nCorrespondences - nBad < 10 (:3024)
  mAcumHessian.setZero();
  Access::set_sim3(g2oS12, s.s12);
  return s.n_in;
}

// numeric core of Optimizer::OptimizeSim3 on the device (gfs_sim3_optimize)
class Sim3Optimizer {
 public:
  explicit Sim3Optimizer(int max_batch = 16, int max_pairs = 4096, int device = 0) {
    check(gfs_sim3_opt_create(device, max_batch, max_pairs, &h_), "gfs_sim3_opt_create");
  }
  ~Sim3Optimizer() { gfs_sim3_opt_destroy(h_); }
  Sim3Optimizer(const Sim3Optimizer&) = delete;
  Sim3Optimizer& operator=(const Sim3Optimizer&) = delete;
  void solve(const gfs_sim3_opt_problem& p, gfs_sim3_opt_solution& s) { check(gfs_sim3_optimize(h_, &p, 1, &s), "gfs_sim3_optimize"); }
  template <class Access, class KeyFrame, class MapPoint, class Sim3, class Hessian>
  int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, Sim3& g2oS12, const float th2, const bool bFixScale,
                   Hessian& mAcumHessian, const bool bAllPoints = false, Sim3OptCounters* counters = nullptr) {
    return gfs_host::OptimizeSim3<Access>([this](const gfs_sim3_opt_problem& p, gfs_sim3_opt_solution& s) { this->solve(p, s); }, pKF1, pKF2,
                                          vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints, counters);
  }

 private:
  gfs_sim3_opt* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// class Sim3Solver                                                     reference include/Sim3Solver.h, src/Sim3Solver.cc
// with the interface its one live call site uses (src/LoopClosing.cc:742-759, :796-798), so that the call site changes only the type
// name: the constructor, SetRansacParameters, the five-argument iterate, GetEstimatedRotation / Translation / Scale  (DESIGN.md
// section 23).  The constructor runs :43-116 on the caller's classes.  Kept as the reference has them:
//   - an empty vpKeyFrameMatchedMP (the default) means every pMP2 is looked up in pKF2 (:44-47);
//   - every X3Dc2 goes through pKF2's pose (Rcw2, tcw2) and is projected with pKF2's camera also when the point was matched in a
//     covisible key frame pKFm, while its key-point, and so its threshold, come from pKFm's mvKeysUn / mvLevelSigma2 (:82-106);
//   - mvnIndices1: vbInliers is indexed by the position in vpMatched12, not by the pair (:100, :263);
//   - mvnMaxError1 / 2 are vector<size_t> (include/Sim3Solver.h:85-86): 9.210 * sigma2 is truncated to an integer before the float
//     comparison reads it.
// The first iterate() draws all 3 * mRansacMaxIts values through Access::random_int (the reference draws them as it goes: when it
// converges early this uses more of the global rand() stream, whose position other threads move anyway), makes ONE solve call and
// answers itself and every later call by replaying the result in steps of nIterations: bConverge in the step that contains the
// converging iteration, bNoMore when the count reaches mRansacMaxIts.  The matrix a step returns is the result's T12 when the step
// converges or ends the run, the identity otherwise (the reference returns its best so far there, or an uninitialised matrix when
// the step found none; the call site reads it only after bConverge).  After bConverge or bNoMore a further call answers bNoMore.
// Single-camera pinhole key frames only (NLeft == -1, Access::is_pinhole): anything else throws.
// KeyFrame: NLeft, fx, fy, cx, cy, GetRotation(), GetTranslation(), GetMapPointMatches(), mvKeysUn, mvLevelSigma2; MapPoint: isBad(),
// GetWorldPos(), GetIndexInKeyFrame(); and of `Access`:
//     static int random_int(int min, int max);                          // DUtils::Random::RandomInt
//     static void sim3_ransac_solve(const gfs_sim3_ransac_problem&, gfs_sim3_ransac_solution&);   // Sim3RansacDevice::solve below
//     static Matrix4f matrix4f(const float T[16]); static Matrix3f matrix3f(const float R[9]);    // row-major -> Eigen
//     static Vector3f vector3f(const float t[3]);
// ------------------------------------------------------------------------------------------------------------------------
constexpr double kSim3RansacProbability = 0.99;  // the call site's SetRansacParameters(0.99, nBoWInliers, 300) (src/LoopClosing.cc:745)
constexpr int kSim3RansacMaxIterations = 300, kSim3RansacStep = 20, kSim3RansacBoWInliers = 15;  // :745, :754 iterate(20, ...), :632

template <class Access>
class Sim3RansacSolver {
 public:
  using Matrix4f = decltype(Access::matrix4f(static_cast<const float*>(nullptr)));
  using Matrix3f = decltype(Access::matrix3f(static_cast<const float*>(nullptr)));
  using Vector3f = decltype(Access::vector3f(static_cast<const float*>(nullptr)));

  template <class KeyFrame, class MapPoint>
  Sim3RansacSolver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true,
                   std::vector<KeyFrame*> vpKeyFrameMatchedMP = std::vector<KeyFrame*>())
      : mbFixScale(bFixScale) {
    auto single_pinhole = [](const KeyFrame& k) { return k.NLeft == -1 && Access::is_pinhole(k); };
    if (!single_pinhole(*pKF1) || !single_pinhole(*pKF2)) throw std::invalid_argument("Sim3Solver: single-camera pinhole key frames only");
    bool bDifferentKFs = true;
    if (vpKeyFrameMatchedMP.empty()) {
      bDifferentKFs = false;
      vpKeyFrameMatchedMP = std::vector<KeyFrame*>(vpMatched12.size(), pKF2);
    }
    const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    const auto Rcw1 = pKF1->GetRotation();
    const auto tcw1 = pKF1->GetTranslation();
    const auto Rcw2 = pKF2->GetRotation();
    const auto tcw2 = pKF2->GetTranslation();
    KeyFrame* pKFm = pKF2;  // Default variable
    for (int i1 = 0; i1 < mN1; i1++) {
      if (vpMatched12[i1]) {
        MapPoint* pMP1 = vpKeyFrameMP1[i1];
        MapPoint* pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
        if (!single_pinhole(*pKFm)) throw std::invalid_argument("Sim3Solver: single-camera pinhole key frames only");
        const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
        const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const auto& kp1 = pKF1->mvKeysUn[indexKF1];
        const auto& kp2 = pKFm->mvKeysUn[indexKF2];
        const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
        const float sigmaSquare2 = pKFm->mvLevelSigma2[kp2.octave];
        mvnMaxError1.push_back((float)(size_t)(gfs_s3r::kChi2 * sigmaSquare1));  // (a vector<size_t> in the reference)
        mvnMaxError2.push_back((float)(size_t)(gfs_s3r::kChi2 * sigmaSquare2));
        mvnIndices1.push_back(i1);
        const auto X3D1c = Rcw1 * pMP1->GetWorldPos() + tcw1;
        const auto X3D2c = Rcw2 * pMP2->GetWorldPos() + tcw2;  // pKF2's pose also when pKFm is another key frame
        for (int k = 0; k < 3; k++) {
          mvX3Dc1.push_back(X3D1c(k));
          mvX3Dc2.push_back(X3D2c(k));
        }
      }
    }
    cam1_[0] = pKF1->fx, cam1_[1] = pKF1->fy, cam1_[2] = pKF1->cx, cam1_[3] = pKF1->cy;
    cam2_[0] = pKF2->fx, cam2_[1] = pKF2->fy, cam2_[2] = pKF2->cx, cam2_[3] = pKF2->cy;
    SetRansacParameters();
  }

  void SetRansacParameters(double probability = gfs_s3r::kDefaultProbability, int minInliers = gfs_s3r::kDefaultMinInliers,
                           int maxIterations = gfs_s3r::kDefaultMaxIterations) {
    mRansacMinInliers = minInliers;
    N = (int)mvnIndices1.size();
    mRansacMaxIts = gfs_s3r::ransac_iterations(N, probability, minInliers, maxIterations);
    mnIterations = 0;
    solved_ = finished_ = false;
  }

  Matrix4f iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
    bNoMore = false;
    bConverge = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (N < mRansacMinInliers || N < 3 || finished_) {  // (N < 3: the reference would index out of range)
      bNoMore = true;
      return Access::matrix4f(identity);
    }
    if (!solved_) solve();
    const int end = std::min(mRansacMaxIts, mnIterations + std::max(nIterations, 0));
    if (sol_.status == GFS_SIM3_RANSAC_CONVERGED && sol_.iterations <= end) {
      mnIterations = sol_.iterations;
      nInliers = sol_.n_inliers;
      for (int i = 0; i < N; i++)
        if (inlier_[i]) vbInliers[mvnIndices1[i]] = true;
      bConverge = true;
      finished_ = true;
      return Access::matrix4f(sol_.T12);
    }
    mnIterations = end;
    if (mnIterations >= mRansacMaxIts) {
      bNoMore = true;
      finished_ = true;
      return Access::matrix4f(sol_.T12);
    }
    return Access::matrix4f(identity);
  }

  Matrix3f GetEstimatedRotation() { return Access::matrix3f(sol_.R12); }
  Vector3f GetEstimatedTranslation() { return Access::vector3f(sol_.t12); }
  float GetEstimatedScale() { return sol_.s12; }

  // what the solve call was given and what the run used, for whoever wants to log it
  int pairs() const { return N; }
  int max_iterations() const { return mRansacMaxIts; }
  int iterations() const { return mnIterations; }
  const std::vector<float>& X3Dc1() const { return mvX3Dc1; }
  const std::vector<float>& X3Dc2() const { return mvX3Dc2; }
  const std::vector<float>& MaxError1() const { return mvnMaxError1; }
  const std::vector<float>& MaxError2() const { return mvnMaxError2; }
  const std::vector<size_t>& Indices1() const { return mvnIndices1; }

 private:
  void solve() {
    draws_.resize(3 * (size_t)mRansacMaxIts);
    for (int it = 0; it < mRansacMaxIts; it++)
      for (int k = 0; k < 3; k++) draws_[3 * it + k] = Access::random_int(0, N - k - 1);  // RandomInt(0, vAvailableIndices.size() - 1)
    inlier_.assign(N, 0);
    gfs_sim3_ransac_problem p{};
    p.n_pairs = N;
    p.x3d_c1 = mvX3Dc1.data();
    p.x3d_c2 = mvX3Dc2.data();
    p.max_err1 = mvnMaxError1.data();
    p.max_err2 = mvnMaxError2.data();
    p.fx1 = cam1_[0], p.fy1 = cam1_[1], p.cx1 = cam1_[2], p.cy1 = cam1_[3];
    p.fx2 = cam2_[0], p.fy2 = cam2_[1], p.cx2 = cam2_[2], p.cy2 = cam2_[3];
    p.fix_scale = mbFixScale ? 1 : 0;
    p.min_inliers = mRansacMinInliers;
    p.n_iterations = mRansacMaxIts;
    p.draws = draws_.data();
    sol_ = gfs_sim3_ransac_solution{};
    sol_.inlier = inlier_.data();
    Access::sim3_ransac_solve(p, sol_);
    solved_ = true;
  }

  bool mbFixScale;
  int mN1 = 0, N = 0, mRansacMinInliers = 0, mRansacMaxIts = 0, mnIterations = 0;
  bool solved_ = false, finished_ = false;
  float cam1_[4], cam2_[4];
  std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
  std::vector<size_t> mvnIndices1;
  std::vector<int32_t> draws_;
  std::vector<uint8_t> inlier_;
  gfs_sim3_ransac_solution sol_{};
};

// numeric core of Sim3Solver on the device (gfs_sim3_ransac_solve): one handle, sized for the call site's 300 iterations
class Sim3RansacDevice {
 public:
  explicit Sim3RansacDevice(int max_batch = 4, int max_pairs = 4096, int max_iterations = kSim3RansacMaxIterations, int device = 0) {
    check(gfs_sim3_ransac_create(device, max_batch, max_pairs, max_iterations, &h_), "gfs_sim3_ransac_create");
  }
  ~Sim3RansacDevice() { gfs_sim3_ransac_destroy(h_); }
  Sim3RansacDevice(const Sim3RansacDevice&) = delete;
  Sim3RansacDevice& operator=(const Sim3RansacDevice&) = delete;
  void solve(const gfs_sim3_ransac_problem& p, gfs_sim3_ransac_solution& s) { check(gfs_sim3_ransac_solve(h_, &p, 1, &s), "gfs_sim3_ransac_solve"); }
  void solve(const gfs_sim3_ransac_problem* p, int B, gfs_sim3_ransac_solution* s) { check(gfs_sim3_ransac_solve(h_, p, B, s), "gfs_sim3_ransac_solve"); }

 private:
  gfs_sim3_ransac* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)  reference src/ORBmatcher.cc:936-1053
// for ONE key frame 1 against a list of key frames 2 in one device call, as LoopClosing::DetectCommonRegionsFromBoW needs it
// (src/LoopClosing.cc:706-715), and the merge of the per-key-frame lists behind it (:717-730)  (DESIGN.md section 22).
//   gather:  per key frame mvKeysUn's angles, mDescriptors, GetMapPointMatches() folded into has_mp (pMP && !pMP->isBad()), mFeatVec
//            flattened.  A null or bad key frame 2 is not uploaded.
//   solve:   `solve(problems, 1, results)`: BowSearcher::solve below (gfs_search_by_bow on the GPU).
//   scatter: vvpMatches12[j][idx1] = GetMapPointMatches()[idx2] of key frame 2 j, vnMatches[j] = SearchByBoW's return value; for a key
//            frame 2 that was skipped the list stays EMPTY and the count 0, as :707 leaves vvpMatchedMPs[j].
// What other threads change in the map during the call is not seen: the map points are read once, at the gather.
// Single-camera key frames only: NLeft != -1 throws.  `Access` as for Fuse: keys_un, descriptors, for_each_node.  KeyFrame: NLeft, N,
// isBad(), GetMapPointMatches(); MapPoint: isBad().
// ------------------------------------------------------------------------------------------------------------------------
struct BowKeyFrameFlat {  // one gathered key frame
  std::vector<float> angle;
  std::vector<uint8_t> has_mp;
  std::vector<int32_t> node_id, node_start, feat_idx;
  gfs_bow_keyframe k{};
};

template <class Access, class KeyFrame, class MapPoint>
void bow_gather(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, BowKeyFrameFlat& F) {
  const KeyFrame& KF = *pKF;
  if (KF.NLeft != -1) throw std::invalid_argument("SearchByBoW: single-camera key frames only");
  const size_t N = vpMapPoints.size();
  const gfs_keypoint* kps = Access::keys_un(KF);
  F.angle.assign(N + 1, 0.0f);
  F.has_mp.assign(N + 1, 0);
  for (size_t i = 0; i < N; i++) {
    F.angle[i] = kps[i].angle;
    MapPoint* pMP = vpMapPoints[i];
    F.has_mp[i] = pMP && !pMP->isBad();
  }
  F.node_id.clear();
  F.feat_idx.clear();
  F.node_start.assign(1, 0);
  Access::for_each_node(KF, [&](unsigned id, const std::vector<unsigned>& idx) {
    F.node_id.push_back((int32_t)id);
    for (unsigned i : idx) F.feat_idx.push_back((int32_t)i);
    F.node_start.push_back((int32_t)F.feat_idx.size());
  });
  F.node_id.push_back(0);  // (never NULL)
  F.feat_idx.push_back(0);
  gfs_bow_keyframe& k = F.k;
  k.n_kp = (int32_t)N;
  k.angle = F.angle.data();
  k.desc = Access::descriptors(KF);
  k.has_mp = F.has_mp.data();
  k.n_nodes = (int32_t)F.node_start.size() - 1;
  k.node_id = F.node_id.data();
  k.node_start = F.node_start.data();
  k.feat_idx = F.feat_idx.data();
}

template <class Access, class KeyFrame, class MapPoint, class Solve>
void SearchByBoW(Solve&& solve, KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, const float nnratio, const bool checkOri,
                 std::vector<std::vector<MapPoint*>>& vvpMatches12, std::vector<int>& vnMatches) {
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  const size_t N = vpMapPoints1.size();
  vvpMatches12.assign(vpKF2.size(), std::vector<MapPoint*>());
  vnMatches.assign(vpKF2.size(), 0);
  BowKeyFrameFlat F1;
  bow_gather<Access>(pKF1, vpMapPoints1, F1);
  std::vector<size_t> used;  // the entries of vpKF2 that are searched
  for (size_t j = 0; j < vpKF2.size(); j++)
    if (vpKF2[j] && !vpKF2[j]->isBad()) used.push_back(j);
  if (used.empty()) return;
  std::vector<BowKeyFrameFlat> F2(used.size());
  std::vector<std::vector<MapPoint*>> vpMapPoints2(used.size());
  std::vector<gfs_bow_keyframe> k2(used.size());
  std::vector<std::vector<int32_t>> match12(used.size());
  std::vector<gfs_bow_result> res(used.size());
  for (size_t u = 0; u < used.size(); u++) {
    vpMapPoints2[u] = vpKF2[used[u]]->GetMapPointMatches();
    bow_gather<Access>(vpKF2[used[u]], vpMapPoints2[u], F2[u]);
    k2[u] = F2[u].k;
    match12[u].assign(N + 1, -1);
    res[u].match12 = match12[u].data();
    res[u].n_matches = 0;
  }
  gfs_bow_problem p{};
  p.kf1 = F1.k;
  p.kf2 = k2.data();
  p.n_kf2 = (int32_t)used.size();
  p.nn_ratio = nnratio;
  p.check_orientation = checkOri ? 1 : 0;
  gfs_bow_result* rp = res.data();
  check(solve(&p, 1, &rp), "SearchByBoW");
  for (size_t u = 0; u < used.size(); u++) {
    std::vector<MapPoint*>& vpMatches12 = vvpMatches12[used[u]];
    vpMatches12.assign(N, static_cast<MapPoint*>(NULL));
    for (size_t i = 0; i < N; i++)
      if (match12[u][i] >= 0) vpMatches12[i] = vpMapPoints2[u][match12[u][i]];
    vnMatches[used[u]] = res[u].n_matches;
  }
}

// src/LoopClosing.cc:692-730 for one candidate: SearchByBoW against every covisible of the candidate (a null or bad one is skipped and
// its list stays empty), then the merge: in the order of vpCovKFi, a point that an earlier key frame already gave is not taken again.
// nIndexMostBoWMatchesKF is computed as the reference computes it; the reference never reads it (the line that would assign
// pMostBoWMatchesKF from it, :732, is commented out), so pMostBoWMatchesKF stays the candidate itself at the caller.
template <class KeyFrame, class MapPoint>
struct BowCandidateMatches {
  std::vector<MapPoint*> vpMatchedPoints;
  std::vector<KeyFrame*> vpKeyFrameMatchedMP;
  std::vector<std::vector<MapPoint*>> vvpMatchedMPs;
  int numBoWMatches = 0, nIndexMostBoWMatchesKF = 0, nMostBoWNumMatches = 0;
};

template <class Access, class MapPoint, class KeyFrame, class Solve>
BowCandidateMatches<KeyFrame, MapPoint> BowMatchesOfCandidate(Solve&& solve, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpCovKFi,
                                                              const float nnratio = 0.9f, const bool checkOri = true) {
  BowCandidateMatches<KeyFrame, MapPoint> out;
  std::vector<int> vnMatches;
  SearchByBoW<Access>(solve, pCurrentKF, vpCovKFi, nnratio, checkOri, out.vvpMatchedMPs, vnMatches);
  for (size_t j = 0; j < vpCovKFi.size(); ++j) {
    if (!vpCovKFi[j] || vpCovKFi[j]->isBad()) continue;
    if (vnMatches[j] > out.nMostBoWNumMatches) {
      out.nMostBoWNumMatches = vnMatches[j];
      out.nIndexMostBoWMatchesKF = (int)j;
    }
  }
  const size_t N = pCurrentKF->GetMapPointMatches().size();
  out.vpMatchedPoints.assign(N, static_cast<MapPoint*>(NULL));
  out.vpKeyFrameMatchedMP.assign(N, static_cast<KeyFrame*>(NULL));
  std::set<MapPoint*> spMatchedMPi;
  for (size_t j = 0; j < vpCovKFi.size(); ++j) {
    for (size_t k = 0; k < out.vvpMatchedMPs[j].size(); ++k) {
      MapPoint* pMPi_j = out.vvpMatchedMPs[j][k];
      if (!pMPi_j || pMPi_j->isBad()) continue;
      if (spMatchedMPi.find(pMPi_j) == spMatchedMPi.end()) {
        spMatchedMPi.insert(pMPi_j);
        out.numBoWMatches++;
        out.vpMatchedPoints[k] = pMPi_j;
        out.vpKeyFrameMatchedMP[k] = vpCovKFi[j];
      }
    }
  }
  return out;
}

// the numeric core of SearchByBoW on the GPU: one handle, its reserve grown to the largest call seen
class BowSearcher {
 public:
  BowSearcher(int max_kp = 4096, int device = 0) { check(gfs_sbp_create(device, 64, max_kp, 1, &h_), "gfs_sbp_create"); }
  ~BowSearcher() { gfs_sbp_destroy(h_); }
  BowSearcher(const BowSearcher&) = delete;
  BowSearcher& operator=(const BowSearcher&) = delete;
  int solve(const gfs_bow_problem* problems, int B, gfs_bow_result* const* results) {
    int n2 = 1;
    for (int b = 0, sum = 0; b < B; b++) n2 = std::max(n2, sum += problems[b].n_kf2);
    if (B > problems_ || n2 > kf2_) {  // the library refuses what exceeds the reserve (it never truncates): grow it first
      const int p = std::max(std::max(B, 1), problems_), k = std::max(n2, kf2_);
      check(gfs_sbp_reserve_bow(h_, p, k), "gfs_sbp_reserve_bow");
      problems_ = p;
      kf2_ = k;
    }
    return gfs_search_by_bow(h_, problems, B, results);
  }
  auto solver() {
    return [this](const gfs_bow_problem* p, int B, gfs_bow_result* const* r) { return solve(p, B, r); };
  }

 private:
  gfs_sbp* h_ = nullptr;
  int problems_ = 0, kf2_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------------
// ComputeBoW and the place-recognition query:
//   bool TemplatedVocabulary::loadFromTextFile(filename)                    Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424
//   void KeyFrame::ComputeBoW() / void Frame::ComputeBoW()                   src/KeyFrame.cc:219-227, src/Frame.cc:1086-1091
//   void KeyFrameDatabase::DetectNBestCandidates(pKF, loop, merge, n)        src/KeyFrameDatabase.cc:583-718
// LoadVocabularyText fills a gfs_bow_vocabulary as the loader fills m_nodes: node id = line order (the root is node 0 and has no
// line), children in line order, word ids in leaf line order, the 32 descriptor bytes as decimal tokens.  Empty lines are skipped: the
// reference builds a node with an uninitialised parent from the empty line that getline returns after a trailing newline.
// ComputeBoW fills mBowVec and mFeatVec from one `transform` call under the reference's empty() guards.  DetectNBestCandidates takes the
// three arrays of `query` (gfs_bow_db_query's) and replays the rest of :587-717 in the reference's order.  `transform` and `query` are
// callables, as `solve` is in the other adaptors: BowTransformer::transformer() and BowDatabaseDevice::querier() below on the GPU.
// ------------------------------------------------------------------------------------------------------------------------
struct BowVocabularyFlat {  // a vocabulary backed by vectors
  std::vector<int32_t> parent, child_start, children, word_id;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
  gfs_bow_vocabulary v{};
};

inline bool LoadVocabularyText(const std::string& path, BowVocabularyFlat& F) {
  std::ifstream f(path.c_str());
  if (!f.is_open()) return false;
  std::string s;
  std::getline(f, s);
  std::stringstream ss;
  ss << s;
  int k = -1, L = -1, n1 = -1, n2 = -1;
  ss >> k >> L >> n1 >> n2;
  if (ss.fail() || k < 0 || k > gfs_bowv::kMaxK || L < 1 || L > gfs_bowv::kMaxL || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) return false;
  F = BowVocabularyFlat{};
  std::vector<std::vector<int32_t>> kids(1);
  F.parent.assign(1, 0);
  F.word_id.assign(1, -1);
  F.weight.assign(1, 0.0);
  F.desc.assign(32, 0);
  int n_words = 0;
  while (std::getline(f, s)) {
    if (s.find_first_not_of(" \t\r\n") == std::string::npos) continue;
    std::stringstream ssnode;
    ssnode << s;
    const int nid = (int)F.parent.size();
    int pid = -1, nIsLeaf = 0;
    ssnode >> pid >> nIsLeaf;
    if (ssnode.fail() || pid < 0 || pid >= nid) return false;
    F.parent.push_back(pid);
    kids[(size_t)pid].push_back(nid);
    kids.emplace_back();
    for (int iD = 0; iD < 32; iD++) {
      int e = 0;
      ssnode >> e;  // FORB::fromString: `ss >> n` into an int, stored as a byte
      F.desc.push_back((uint8_t)e);
    }
    double w = 0;
    ssnode >> w;
    if (ssnode.fail()) return false;
    F.weight.push_back(w);
    F.word_id.push_back(nIsLeaf > 0 ? n_words++ : -1);
  }
  F.child_start.assign(1, 0);
  for (const std::vector<int32_t>& c : kids) {
    F.children.insert(F.children.end(), c.begin(), c.end());
    F.child_start.push_back((int32_t)F.children.size());
  }
  F.children.push_back(0);  // (never NULL)
  F.v.k = k;
  F.v.L = L;
  F.v.scoring = n1;
  F.v.weighting = n2;
  F.v.n_nodes = (int32_t)F.parent.size();
  F.v.parent = F.parent.data();
  F.v.child_start = F.child_start.data();
  F.v.children = F.children.data();
  F.v.desc = F.desc.data();
  F.v.weight = F.weight.data();
  F.v.word_id = F.word_id.data();
  return true;
}

// Access: n_descriptors(kf), descriptors(kf) ([n][32] bytes, mDescriptors' rows); kf.mBowVec is a map<unsigned, double>, kf.mFeatVec a
// map<unsigned, vector<unsigned>>.  KeyFrameGuard: `mBowVec.empty() || mFeatVec.empty()` (KeyFrame), else `mBowVec.empty()` (Frame).
template <class Access, bool KeyFrameGuard, class KeyFrameOrFrame, class Transform>
void ComputeBoW(Transform&& transform, KeyFrameOrFrame& kf) {
  if (!(kf.mBowVec.empty() || (KeyFrameGuard && kf.mFeatVec.empty()))) return;
  const int32_t n = (int32_t)Access::n_descriptors(kf);
  const uint8_t* desc = Access::descriptors(kf);
  std::vector<int32_t> word_id((size_t)n + 1), node_id((size_t)n + 1), node_start((size_t)n + 2), feat_idx((size_t)n + 1);
  std::vector<double> word_value((size_t)n + 1);
  gfs_bow_vectors o{};
  o.word_id = word_id.data();
  o.word_value = word_value.data();
  o.node_id = node_id.data();
  o.node_start = node_start.data();
  o.feat_idx = feat_idx.data();
  check(transform(&desc, &n, 1, gfs_bowv::kLevelsUp, &o), "ComputeBoW");
  kf.mBowVec.clear();
  kf.mFeatVec.clear();
  for (int i = 0; i < o.n_words; i++) kf.mBowVec.insert(kf.mBowVec.end(), std::make_pair((unsigned)word_id[i], word_value[i]));
  for (int q = 0; q < o.n_nodes; q++)
    kf.mFeatVec.insert(kf.mFeatVec.end(), std::make_pair((unsigned)node_id[q], std::vector<unsigned>(feat_idx.begin() + node_start[q],
                                                                                                      feat_idx.begin() + node_start[q + 1])));
}

// The caller's half of the database: which key frame sits in which slot, and the order in which they were added (the order of an
// inverted file's lists).  add() of a key frame that has a slot moves it to the end of that order, as erase + add does.
template <class KeyFrame>
struct BowDatabaseIndex {
  std::vector<KeyFrame*> kf;       // [max_entries] or nullptr
  std::vector<long long> seq;      // [max_entries] add sequence number
  std::map<KeyFrame*, int> slot_of;
  long long next = 0;
  explicit BowDatabaseIndex(int max_entries) : kf((size_t)max_entries, nullptr), seq((size_t)max_entries, 0) {}
  int add(KeyFrame* p) {  // -> the slot, -1 when full
    int s = -1;
    auto it = slot_of.find(p);
    if (it != slot_of.end()) s = it->second;
    for (size_t i = 0; s < 0 && i < kf.size(); i++)
      if (!kf[i]) s = (int)i;
    if (s < 0) return -1;
    kf[(size_t)s] = p;
    seq[(size_t)s] = next++;
    slot_of[p] = s;
    return s;
  }
  int erase(KeyFrame* p) {  // -> the slot it had, -1 when it had none
    auto it = slot_of.find(p);
    if (it == slot_of.end()) return -1;
    const int s = it->second;
    kf[(size_t)s] = nullptr;
    slot_of.erase(it);
    return s;
  }
};

// KeyFrame: mnId, mBowVec, GetConnectedKeyFrames(), GetBestCovisibilityKeyFrames(int), isBad(), GetMap() (-> a Map with IsBad()), and
// the three members the reference writes: mnPlaceRecognitionQuery, mnPlaceRecognitionWords, mPlaceRecognitionScore.
// query(n_words, word_id, word_value, n_common, first_word, score) -> gfs_status, the arrays [index.kf.size()].
template <class KeyFrame, class Query>
void DetectNBestCandidates(Query&& query, const BowDatabaseIndex<KeyFrame>& index, KeyFrame* pKF, std::vector<KeyFrame*>& vpLoopCand,
                           std::vector<KeyFrame*>& vpMergeCand, int nNumCandidates = gfs_bowv::kLoopNumCandidates) {
  const std::set<KeyFrame*> spConnectedKF = pKF->GetConnectedKeyFrames();
  std::vector<int32_t> ids;
  std::vector<double> vals;
  for (const auto& w : pKF->mBowVec) {
    ids.push_back((int32_t)w.first);
    vals.push_back(w.second);
  }
  const size_t E = index.kf.size();
  std::vector<int32_t> n_common(E + 1, 0), first_word(E + 1, -1);
  std::vector<float> score(E + 1, 0.0f);
  ids.push_back(0), vals.push_back(0.0);  // (never NULL)
  check(query((int)ids.size() - 1, ids.data(), vals.data(), n_common.data(), first_word.data(), score.data()), "DetectNBestCandidates");
  // lKFsSharingWords (:596-614): the query's words ascending, a word's list in insertion order -> (lowest common word, add sequence)
  std::vector<size_t> sharing;
  for (size_t s = 0; s < E; s++) {
    KeyFrame* pKFi = index.kf[s];
    if (!pKFi || n_common[s] <= 0) continue;
    if (pKFi->mnPlaceRecognitionQuery == pKF->mnId) {  // (already this query's: :605 only counts on)
      pKFi->mnPlaceRecognitionWords += n_common[s];
      continue;
    }
    if (spConnectedKF.count(pKFi)) {
      pKFi->mnPlaceRecognitionWords = 1;  // reset and incremented at every shared word, never marked
      continue;
    }
    pKFi->mnPlaceRecognitionQuery = pKF->mnId;
    pKFi->mnPlaceRecognitionWords = n_common[s];
    sharing.push_back(s);
  }
  std::sort(sharing.begin(), sharing.end(), [&](size_t a, size_t b) {
    return first_word[a] != first_word[b] ? first_word[a] < first_word[b] : index.seq[a] < index.seq[b];
  });
  if (sharing.empty()) return;
  int maxCommonWords = 0;
  for (size_t s : sharing)
    if (index.kf[s]->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = index.kf[s]->mnPlaceRecognitionWords;
  int minCommonWords = maxCommonWords * gfs_bowv::kMinCommonShare;
  std::vector<std::pair<float, KeyFrame*>> lScoreAndMatch;
  for (size_t s : sharing) {
    KeyFrame* pKFi = index.kf[s];
    if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
      float si = score[s];
      pKFi->mPlaceRecognitionScore = si;
      lScoreAndMatch.push_back(std::make_pair(si, pKFi));
    }
  }
  if (lScoreAndMatch.empty()) return;
  std::vector<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
  for (const auto& sm : lScoreAndMatch) {
    KeyFrame* pKFi = sm.second;
    std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(gfs_bowv::kCovisibles);
    float bestScore = sm.first;
    float accScore = bestScore;
    KeyFrame* pBestKF = pKFi;
    for (KeyFrame* pKF2 : vpNeighs) {
      if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;
      accScore += pKF2->mPlaceRecognitionScore;
      if (pKF2->mPlaceRecognitionScore > bestScore) {
        pBestKF = pKF2;
        bestScore = pKF2->mPlaceRecognitionScore;
      }
    }
    lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
  }
  // list::sort(compFirst) is stable: equal accumulated scores keep list order
  std::stable_sort(lAccScoreAndMatch.begin(), lAccScoreAndMatch.end(),
                   [](const std::pair<float, KeyFrame*>& a, const std::pair<float, KeyFrame*>& b) { return a.first > b.first; });
  vpLoopCand.reserve((size_t)nNumCandidates);
  vpMergeCand.reserve((size_t)nNumCandidates);
  std::set<KeyFrame*> spAlreadyAddedKF;
  for (size_t i = 0; i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates); i++) {
    KeyFrame* pKFi = lAccScoreAndMatch[i].second;
    if (pKFi->isBad()) continue;
    if (spAlreadyAddedKF.count(pKFi)) continue;
    if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) {
      vpLoopCand.push_back(pKFi);
    } else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) {
      vpMergeCand.push_back(pKFi);
    }
    spAlreadyAddedKF.insert(pKFi);
  }
}

// the vocabulary transform on the GPU
class BowTransformer {
 public:
  BowTransformer(const gfs_bow_vocabulary& v, int max_batch = 1, int max_features = 4096, int device = 0) {
    check(gfs_bow_create(device, &v, max_batch, max_features, &h_), "gfs_bow_create");
  }
  ~BowTransformer() { gfs_bow_destroy(h_); }
  BowTransformer(const BowTransformer&) = delete;
  BowTransformer& operator=(const BowTransformer&) = delete;
  auto transformer() {
    return [this](const uint8_t* const* desc, const int32_t* n, int B, int levelsup, gfs_bow_vectors* out) {
      return gfs_bow_transform(h_, desc, n, B, levelsup, out);
    };
  }

 private:
  gfs_bow_vocab* h_ = nullptr;
};

// the database's store on the GPU; the BowDatabaseIndex beside it says which key frame a slot holds
class BowDatabaseDevice {
 public:
  BowDatabaseDevice(int max_entries, int max_words, int device = 0) { check(gfs_bow_db_create(device, max_entries, max_words, &h_), "gfs_bow_db_create"); }
  ~BowDatabaseDevice() { gfs_bow_db_destroy(h_); }
  BowDatabaseDevice(const BowDatabaseDevice&) = delete;
  BowDatabaseDevice& operator=(const BowDatabaseDevice&) = delete;
  template <class BowVector>
  void add(int slot, const BowVector& v) {  // KeyFrameDatabase::add: pKF->mBowVec into the key frame's slot
    std::vector<int32_t> ids;
    std::vector<double> vals;
    for (const auto& w : v) ids.push_back((int32_t)w.first), vals.push_back(w.second);
    const int n = (int)ids.size();
    ids.push_back(0), vals.push_back(0.0);
    check(gfs_bow_db_add(h_, slot, n, ids.data(), vals.data()), "gfs_bow_db_add");
  }
  void erase(int slot) { check(gfs_bow_db_erase(h_, slot), "gfs_bow_db_erase"); }
  auto querier() {
    return [this](int n, const int32_t* id, const double* value, int32_t* n_common, int32_t* first_word, float* score) {
      return gfs_bow_db_query(h_, n, id, value, n_common, first_word, score);
    };
  }

 private:
  gfs_bow_db* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame* pFrame, bool bRecInit, const bool bFrame2FrameReprojError,
//                                                     const bool bFrame2MapReprojError, const int nIterations)   src/Optimizer.cc:5899-6283
// int Optimizer::PoseInertialOptimizationLastFrame(...same...)                                                   :6762-7171
// the two calls that end Tracking::TrackLocalMap once the IMU is initialised (src/Tracking.cc:3763-3798), around one flat solve
// (include/gfs_abi.h section 19).
//   gather:     the visual edges in the index order of mvpMapPoints (every non-NULL pMP; mvbOutlier[i] = false): GetWorldPos, mvKeysUn,
//               mvuRight, mvInvLevelSigma2[octave], stereo = mvuRight[i] >= 0, close = mTrackDepth < 10.f; both ends of the inertial
//               edge, the calibration, the preintegration, the information matrices and (frame mode) pFp->mpcpi through `Access`, which
//               runs the reference's own constructors on the reference's own types (Eigen is not restated here).
//   solve:      `solve(problem, solution)`: PoseInertialDevice::solve below (gfs_pose_inertial_optimize on the GPU).
//   write back: mvbOutlier, SetImuPoseVelocity and mImuBias (the casts are Access's), the reprojection error under the two flags, the
//               new pFrame->mpcpi from the returned H with the reference's own Optimizer::Marginalize and ConstraintPoseImu
//               (Access::new_constraint), and in frame mode `delete pFp->mpcpi; pFp->mpcpi = NULL`.
// Refused (std::runtime_error, nothing touched): Nleft != -1, a camera that is not the pinhole, and in frame mode a missing
// pFp->mpcpi, which the reference would dereference.
// Frame: N, Nleft, mvpMapPoints, mvbOutlier, mvKeysUn, mvuRight, mvInvLevelSigma2, mpLastKeyFrame, mpPrevFrame, mpImuPreintegrated,
// mpImuPreintegratedFrame, mpcpi, SetFrame2FrameReprojError, SetFrame2MapReprojError; MapPoint: mTrackDepth; and of `Access`:
//     static bool is_pinhole(const Frame*);
//     static void world_pos(const MapPoint*, float X[3]);
//     static void calibration(const Frame*, gfs_pose_inertial_problem&);                 // fx fy cx cy bf Rcb tcb Rbc tbc
//     static void state(const Frame*, gfs_imu_state&); static void state(const KeyFrame*, gfs_imu_state&);  // ImuCamPose + Vertex* ctors
//     static void preintegration(const Preintegrated*, gfs_pose_inertial_problem&);      // dR .. dT and info_inertial (EdgeInertial's ctor)
//     static void random_walk_information(const Preintegrated*, double info_gyro[9], double info_acc[9]);
//     static void prior(const Constraint*, gfs_pose_inertial_problem&);                  // prior_Rwb .. prior_H
//     static void set_imu_pose_velocity_bias(Frame*, const gfs_imu_estimate&);
//     static Constraint* new_constraint(const gfs_imu_estimate&, const double* H, int mode);  // mode 1: Marginalize(H, 0, 14) first
// ------------------------------------------------------------------------------------------------------------------------
template <class Access, class Frame, class Solve>
int PoseInertialOptimization(Solve&& solve, int mode, Frame* pFrame, bool bRecInit, const bool bFrame2FrameReprojError,
                             const bool bFrame2MapReprojError, const int nIterations) {
  const bool frame_mode = mode == GFS_POSE_INERTIAL_LAST_FRAME;
  if (pFrame->Nleft != -1) throw std::runtime_error("PoseInertialOptimization: two-camera frames (Nleft != -1) are not supported");
  if (!Access::is_pinhole(pFrame)) throw std::runtime_error("PoseInertialOptimization: only the pinhole camera is supported");
  if (frame_mode && !pFrame->mpPrevFrame->mpcpi) throw std::runtime_error("PoseInertialOptimization: pFp->mpcpi does not exist");
  const int N = pFrame->N;
  std::vector<int> idx;
  std::vector<double> xw, obs;
  std::vector<float> w;
  std::vector<uint8_t> st, close;
  for (int i = 0; i < N; i++) {
    auto* pMP = pFrame->mvpMapPoints[i];
    if (!pMP) continue;
    pFrame->mvbOutlier[i] = false;
    const auto& kpUn = pFrame->mvKeysUn[i];
    const bool stereo = !(pFrame->mvuRight[i] < 0);  // (!bRight && mvuRight[i] < 0) is the mono branch (:5963)
    float X[3];
    Access::world_pos(pMP, X);
    for (int k = 0; k < 3; k++) xw.push_back((double)X[k]);
    obs.push_back((double)kpUn.pt.x);
    obs.push_back((double)kpUn.pt.y);
    obs.push_back((double)pFrame->mvuRight[i]);
    w.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);  // / uncertainty2 == 1 for the pinhole
    st.push_back(stereo ? 1 : 0);
    close.push_back(pMP->mTrackDepth < 10.f ? 1 : 0);
    idx.push_back(i);
  }
  const int n = (int)idx.size();
  gfs_pose_inertial_problem P{};
  P.mode = mode;
  P.n_obs = n;
  P.n_rounds = nIterations;
  P.rec_init = bRecInit ? 1 : 0;
  P.xw = xw.data(), P.obs = obs.data(), P.inv_sigma2 = w.data(), P.stereo = st.data(), P.close = close.data();
  Access::calibration(pFrame, P);
  Access::state(pFrame, P.cur);
  if (frame_mode) {
    Access::state(pFrame->mpPrevFrame, P.other);
    Access::preintegration(pFrame->mpImuPreintegratedFrame, P);
    Access::prior(pFrame->mpPrevFrame->mpcpi, P);
  } else {
    Access::state(pFrame->mpLastKeyFrame, P.other);
    Access::preintegration(pFrame->mpImuPreintegrated, P);
  }
  Access::random_walk_information(pFrame->mpImuPreintegrated, P.info_gyro_rw, P.info_acc_rw);  // mpImuPreintegrated in BOTH modes (:6961)
  std::vector<uint8_t> outlier((size_t)std::max(n, 1));
  gfs_pose_inertial_solution S{};
  S.outlier = outlier.data();
  solve(P, S);
  for (int k = 0; k < n; k++) pFrame->mvbOutlier[idx[k]] = outlier[k] != 0;
  if (bFrame2FrameReprojError) pFrame->SetFrame2FrameReprojError(S.avg_reproj);
  if (bFrame2MapReprojError) pFrame->SetFrame2MapReprojError(S.avg_reproj);
  Access::set_imu_pose_velocity_bias(pFrame, S.cur);
  pFrame->mpcpi = Access::new_constraint(S.cur, S.H, mode);
  if (frame_mode) {
    delete pFrame->mpPrevFrame->mpcpi;
    pFrame->mpPrevFrame->mpcpi = nullptr;
  }
  return S.n_good;
}
template <class Access, class Frame, class Solve>
int PoseInertialOptimizationLastKeyFrame(Solve&& solve, Frame* pFrame, bool bRecInit = false, const bool bFrame2FrameReprojError = false,
                                         const bool bFrame2MapReprojError = false, const int nIterations = 4) {
  return PoseInertialOptimization<Access>(solve, GFS_POSE_INERTIAL_LAST_KEYFRAME, pFrame, bRecInit, bFrame2FrameReprojError, bFrame2MapReprojError,
                                          nIterations);
}
template <class Access, class Frame, class Solve>
int PoseInertialOptimizationLastFrame(Solve&& solve, Frame* pFrame, bool bRecInit = false, const bool bFrame2FrameReprojError = false,
                                      const bool bFrame2MapReprojError = false, const int nIterations = 4) {
  return PoseInertialOptimization<Access>(solve, GFS_POSE_INERTIAL_LAST_FRAME, pFrame, bRecInit, bFrame2FrameReprojError, bFrame2MapReprojError,
                                          nIterations);
}

// numeric core of both: one problem (or a batch) on the device
class PoseInertialDevice {
 public:
  explicit PoseInertialDevice(int max_obs = 4096, int max_batch = 1, int device = 0) {
    check(gfs_pose_inertial_create(device, max_obs, max_batch, &h_), "gfs_pose_inertial_create");
  }
  ~PoseInertialDevice() { gfs_pose_inertial_destroy(h_); }
  PoseInertialDevice(const PoseInertialDevice&) = delete;
  PoseInertialDevice& operator=(const PoseInertialDevice&) = delete;
  void solve(const gfs_pose_inertial_problem& p, gfs_pose_inertial_solution& s) { check(gfs_pose_inertial_optimize(h_, &p, 1, &s), "gfs_pose_inertial_optimize"); }
  void solve(const gfs_pose_inertial_problem* p, int B, gfs_pose_inertial_solution* s) { check(gfs_pose_inertial_optimize(h_, p, B, s), "gfs_pose_inertial_optimize"); }

 private:
  gfs_pose_inertial* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// int Optimizer::PoseLidarVisualInertialOptimizationLastKeyFrame(Frame* pFrame, pcl::PointCloud<PointType>::Ptr laserCloudSurfFromMapDS,
//     bool bRecInit, const bool bFrame2FrameReprojError, const bool bFrame2MapReprojError, const int nIterations,
//     int& nInliersLidar, float& residual)                                                                     src/Optimizer.cc:6285-6760
// int Optimizer::PoseLidarVisualInertialOptimizationLastFrame(...same...)                                      :7173-7678
// the two calls that end Tracking::TrackLocalMap for IMU_RGBD with useLidarObs() (src/Tracking.cc:3763-3798), around one flat solve
// (include/gfs_abi.h section 21).  The gather and the write-back are those of PoseInertialOptimization above,
// which runs underneath; on top of them:
//   gather:     the stored Tcw and mTcb as float quaternion (x, y, z, w) and translation, the signed time gap to the last key frame
//               (key-frame mode), the downsampled cloud in the camera frame (a null mpPointCloudDownsampled gives n_cloud = 0), the map
//               handle in place of laserCloudSurfFromMapDS (gfs_lidar_map_build or gfs_lidar_map_set made it).
//   write back: nInliersLidar and residual, by reference.
// Marginalize and ConstraintPoseImu stay the reference's own (Access::new_constraint).
// Frame, beyond the list above: mTimeStamp, mpPointCloudDownsampled; KeyFrame: mTimeStamp; and of `Access`, beyond the list above:
//     static void stored_pose(const Frame*, float q[4], float t[3]);       // pFrame->GetPose(): unit_quaternion().coeffs(), translation()
//     static void stored_tcb(const Frame*, float q[4], float t[3]);        // pFrame->mImuCalib.mTcb
//     static void cloud(const Cloud&, std::vector<float>& xyz);            // the points of *mpPointCloudDownsampled, [n][3]
// ------------------------------------------------------------------------------------------------------------------------
template <class Access, class Frame, class Solve>
int PoseLidarVisualInertialOptimization(Solve&& solve, int mode, Frame* pFrame, const gfs_lidar_map* map, bool bRecInit,
                                        const bool bFrame2FrameReprojError, const bool bFrame2MapReprojError, const int nIterations,
                                        int& nInliersLidar, float& residual) {
  auto with_lidar = [&](const gfs_pose_inertial_problem& p, gfs_pose_inertial_solution& s) {
    gfs_pose_lidar_inertial_problem P{};
    P.vi = p;
    Access::stored_pose(pFrame, P.q, P.t);
    Access::stored_tcb(pFrame, P.tcb_q, P.tcb_t);
    P.kf_time_gap = mode == GFS_POSE_INERTIAL_LAST_KEYFRAME ? pFrame->mTimeStamp - pFrame->mpLastKeyFrame->mTimeStamp : 0.0;
    std::vector<float> cloud;
    if (pFrame->mpPointCloudDownsampled) Access::cloud(*pFrame->mpPointCloudDownsampled, cloud);
    P.n_cloud = (int)(cloud.size() / 3);
    P.cloud = cloud.data();
    P.map = map;
    gfs_pose_lidar_inertial_solution S{};
    S.vi.outlier = s.outlier;
    solve(P, S);
    s = S.vi;
    nInliersLidar = S.n_lidar_inliers;
    residual = S.residual;
  };
  return PoseInertialOptimization<Access>(with_lidar, mode, pFrame, bRecInit, bFrame2FrameReprojError, bFrame2MapReprojError, nIterations);
}
template <class Access, class Frame, class Solve>
int PoseLidarVisualInertialOptimizationLastKeyFrame(Solve&& solve, Frame* pFrame, const gfs_lidar_map* map, bool bRecInit,
                                                    const bool bFrame2FrameReprojError, const bool bFrame2MapReprojError, const int nIterations,
                                                    int& nInliersLidar, float& residual) {
  return PoseLidarVisualInertialOptimization<Access>(solve, GFS_POSE_INERTIAL_LAST_KEYFRAME, pFrame, map, bRecInit, bFrame2FrameReprojError,
                                                     bFrame2MapReprojError, nIterations, nInliersLidar, residual);
}
template <class Access, class Frame, class Solve>
int PoseLidarVisualInertialOptimizationLastFrame(Solve&& solve, Frame* pFrame, const gfs_lidar_map* map, bool bRecInit,
                                                 const bool bFrame2FrameReprojError, const bool bFrame2MapReprojError, const int nIterations,
                                                 int& nInliersLidar, float& residual) {
  return PoseLidarVisualInertialOptimization<Access>(solve, GFS_POSE_INERTIAL_LAST_FRAME, pFrame, map, bRecInit, bFrame2FrameReprojError,
                                                     bFrame2MapReprojError, nIterations, nInliersLidar, residual);
}

// numeric core of both: one problem (or a batch) on the device
class PoseLidarInertialDevice {
 public:
  explicit PoseLidarInertialDevice(int max_obs = 4096, int max_cloud = 8192, int max_batch = 1, int device = 0) {
    check(gfs_pose_lidar_inertial_create(device, max_obs, max_cloud, max_batch, &h_), "gfs_pose_lidar_inertial_create");
  }
  ~PoseLidarInertialDevice() { gfs_pose_lidar_inertial_destroy(h_); }
  PoseLidarInertialDevice(const PoseLidarInertialDevice&) = delete;
  PoseLidarInertialDevice& operator=(const PoseLidarInertialDevice&) = delete;
  void solve(const gfs_pose_lidar_inertial_problem& p, gfs_pose_lidar_inertial_solution& s) {
    check(gfs_pose_lidar_inertial_optimize(h_, &p, 1, &s), "gfs_pose_lidar_inertial_optimize");
  }
  void solve(const gfs_pose_lidar_inertial_problem* p, int B, gfs_pose_lidar_inertial_solution* s) {
    check(gfs_pose_lidar_inertial_optimize(h_, p, B, s), "gfs_pose_lidar_inertial_optimize");
  }

 private:
  gfs_pose_lidar_inertial* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------------------
// void Optimizer::LocalInertialBA(KeyFrame* pKF, bool* pbStopFlag, bool pbICPFlag, Map* pMap, int& num_fixedKF, int& num_OptKF,
//                                 int& num_MPs, int& num_edges, bool bLarge, bool bRecInit)                  src/Optimizer.cc:3056-3702
// the local BA LocalMapping::Run calls for every new key frame once the IMU is initialised (src/LocalMapping.cc:186-228), around one
// flat solve (include/gfs_abi.h section 20).
//   gather:     exactly :3060-3166 -- the window along the mPrevKF chain (at most 10, or 20 with bLarge; Nd from KeyFramesInMap() - 2),
//               its map points in match order, the fixed predecessor or, without one, the oldest key frame popped and fixed, no
//               "optimisable visual" key frames (maxCovKF is 0), the other fixed key frames from the observations until the list holds
//               gfs_li::kMaxFixKF, with the mnBALocalForKF / mnBAFixedForKF marks; SetNewBias on every preintegration (:3336); the
//               visual edges point by point in the order of GetObservations() (:3446-3578).  The reference's constructors run on the
//               reference's own types inside `Access`.
//   solve:      `solve(problem, solution)`: LocalInertialBADevice::solve below (gfs_lba_inertial_solve on the GPU).
//   write back: the fail gate (:3632; the marks are left as they are there, as the reference leaves them), EraseMapPointMatch /
//               EraseObservation of the flagged observations whose point is not bad, the marks' reset, SetPose / SetVelocity /
//               SetNewBias (the casts are Access's), SetWorldPos + UpdateNormalAndDepth, IncreaseChangeIndex, under mMutexMapUpdate.
// pbICPFlag == true goes to `reference(...)`, the reference's own function: the EdgeICP block registers a GICP per key frame, and no
// shipped configuration enables it.  pbStopFlag is never polled by the reference (:3594) and is not read; num_* are never written by
// it; bRecInit is unused by it.
// Refused (std::runtime_error, every mark put back, nothing else touched): a window key frame or the predecessor without IMU or without
// a preintegration, a key frame with a second camera, a camera that is not the pinhole.  Returns false when the fail gate fired.
// Of `Access`:
//     static bool is_pinhole(const KeyFrame*);
//     static void calibration(const KeyFrame*, gfs_lba_inertial_problem&);          // fx fy cx cy bf Rcb tcb Rbc tbc
//     static void state(const KeyFrame*, gfs_imu_state&);                            // ImuCamPose(KeyFrame*) + the Vertex* constructors
//     static void preintegration(const Preintegrated*, gfs_lba_inertial_edge&);      // dR .. dT, info_inertial, info_gyro_rw, info_acc_rw
//     static void world_pos(const MapPoint*, float X[3]); static void set_world_pos(MapPoint*, const double X[3]);
//     static void set_pose_velocity_bias(KeyFrame*, const gfs_imu_state&);           // SetPose(Tcw), SetVelocity, SetNewBias(IMU::Bias)
// ------------------------------------------------------------------------------------------------------------------------
template <class Access, class KeyFrame, class Map, class Solve, class Reference>
bool LocalInertialBA(Solve&& solve, Reference&& reference, KeyFrame* pKF, bool* pbStopFlag, bool pbICPFlag, Map* pMap, int& num_fixedKF,
                     int& num_OptKF, int& num_MPs, int& num_edges, bool bLarge = false, bool bRecInit = false) {
  if (pbICPFlag) {
    reference(pKF, pbStopFlag, pbICPFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges, bLarge, bRecInit);
    return true;
  }
  using MapPoint = std::remove_pointer_t<std::decay_t<decltype(pKF->GetMapPointMatches()[0])>>;
  auto* pCurrentMap = pKF->GetMap();
  const int maxOpt = bLarge ? gfs_li::kMaxWindowLarge : gfs_li::kMaxWindow;
  const int Nd = std::min((int)pCurrentMap->KeyFramesInMap() - 2, maxOpt);
  std::vector<std::function<void()>> undo;  // every mark the gather sets, for a refusal
  auto mark = [&](auto& field, auto value) {
    const auto old = field;
    undo.push_back([&field, old] { field = old; });
    field = value;
  };
  auto refuse = [&](const char* what) {
    for (auto it = undo.rbegin(); it != undo.rend(); ++it) (*it)();
    throw std::runtime_error(what);
  };
  std::vector<KeyFrame*> vpOptimizableKFs;
  vpOptimizableKFs.push_back(pKF);
  mark(pKF->mnBALocalForKF, pKF->mnId);
  for (int i = 1; i < Nd; i++) {
    if (!vpOptimizableKFs.back()->mPrevKF) break;
    vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
    mark(vpOptimizableKFs.back()->mnBALocalForKF, pKF->mnId);
  }
  int N = (int)vpOptimizableKFs.size();
  std::list<MapPoint*> lLocalMapPoints;
  for (int i = 0; i < N; i++)
    for (MapPoint* pMP : vpOptimizableKFs[i]->GetMapPointMatches())
      if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
        lLocalMapPoints.push_back(pMP);
        mark(pMP->mnBALocalForKF, pKF->mnId);
      }
  std::list<KeyFrame*> lFixedKeyFrames;
  if (vpOptimizableKFs.back()->mPrevKF) {
    lFixedKeyFrames.push_back(vpOptimizableKFs.back()->mPrevKF);
    mark(vpOptimizableKFs.back()->mPrevKF->mnBAFixedForKF, pKF->mnId);
  } else {
    mark(vpOptimizableKFs.back()->mnBALocalForKF, decltype(pKF->mnId)(0));
    mark(vpOptimizableKFs.back()->mnBAFixedForKF, pKF->mnId);
    lFixedKeyFrames.push_back(vpOptimizableKFs.back());
    vpOptimizableKFs.pop_back();
  }
  N = (int)vpOptimizableKFs.size();
  for (MapPoint* pMP : lLocalMapPoints) {
    const auto observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrame* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        mark(pKFi->mnBAFixedForKF, pKF->mnId);
        if (!pKFi->isBad()) {
          lFixedKeyFrames.push_back(pKFi);
          break;
        }
      }
    }
    if ((int)lFixedKeyFrames.size() >= gfs_li::kMaxFixKF) break;
  }
  if (N < 1) refuse("LocalInertialBA: no optimisable key frame");
  // key-frame indices: the window, the predecessor, the other fixed ones in list order
  std::map<KeyFrame*, int> index;
  for (int i = 0; i < N; i++) index[vpOptimizableKFs[i]] = i;
  KeyFrame* prev = lFixedKeyFrames.front();
  if (vpOptimizableKFs.back()->mPrevKF != prev) refuse("LocalInertialBA: the window has no fixed predecessor");
  std::vector<KeyFrame*> fixed(std::next(lFixedKeyFrames.begin()), lFixedKeyFrames.end());
  index[prev] = N;
  for (size_t k = 0; k < fixed.size(); k++) index[fixed[k]] = N + 1 + (int)k;
  for (const auto& kv : index) {
    if (kv.first->mpCamera2) refuse("LocalInertialBA: key frames with a second camera are not supported");
    if (!Access::is_pinhole(kv.first)) refuse("LocalInertialBA: only the pinhole camera is supported");
  }
  if (!prev->bImu) refuse("LocalInertialBA: the key frame in front of the window has no IMU");
  for (int i = 0; i < N; i++)
    if (!vpOptimizableKFs[i]->bImu || !vpOptimizableKFs[i]->mpImuPreintegrated) refuse("LocalInertialBA: a window key frame has no IMU preintegration");
  gfs_lba_inertial_problem P{};
  P.n_opt = N, P.n_fixed = (int)fixed.size(), P.n_cameras = 1;
  P.iterations = bLarge ? gfs_li::kOptItLarge : gfs_li::kOptIt;
  P.lambda_init = bLarge ? gfs_li::kLambdaInitLarge : gfs_li::kLambdaInit;
  Access::calibration(pKF, P);
  std::vector<gfs_imu_state> window((size_t)N), window_out((size_t)N);
  std::vector<uint8_t> window_imu((size_t)N, 1);
  std::vector<gfs_lba_inertial_edge> inertial((size_t)N);
  for (int i = 0; i < N; i++) {
    KeyFrame* pKFi = vpOptimizableKFs[i];
    Access::state(pKFi, window[(size_t)i]);
    pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());
    Access::preintegration(pKFi->mpImuPreintegrated, inertial[(size_t)i]);
  }
  Access::state(prev, P.prev);
  std::vector<double> fixed_Rcw(9 * fixed.size() + 1), fixed_tcw(3 * fixed.size() + 1);
  for (size_t k = 0; k < fixed.size(); k++) {
    gfs_imu_state s{};
    Access::state(fixed[k], s);
    memcpy(&fixed_Rcw[9 * k], s.Rcw, sizeof(s.Rcw)), memcpy(&fixed_tcw[3 * k], s.tcw, sizeof(s.tcw));
  }
  std::vector<double> points, obs;
  std::vector<int32_t> begin{0}, edge_kf;
  std::vector<float> w;
  std::vector<uint8_t> stereo, close;
  std::vector<std::pair<KeyFrame*, MapPoint*>> edge_of;
  std::vector<MapPoint*> vpPoints(lLocalMapPoints.begin(), lLocalMapPoints.end());
  for (MapPoint* pMP : vpPoints) {
    float X[3];
    Access::world_pos(pMP, X);
    for (int k = 0; k < 3; k++) points.push_back((double)X[k]);
    const auto observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrame* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) continue;
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex == -1) continue;
      const auto it = index.find(pKFi);
      if (it == index.end()) continue;  // marked fixed but bad when it was met (:3157-3161): it has no vertex, g2o drops the edge
      const auto& kpUn = pKFi->mvKeysUn[(size_t)leftIndex];
      const float ur = pKFi->mvuRight[(size_t)leftIndex];
      obs.push_back((double)kpUn.pt.x), obs.push_back((double)kpUn.pt.y), obs.push_back((double)ur);
      w.push_back(pKFi->mvInvLevelSigma2[(size_t)kpUn.octave]);  // / uncertainty2 == 1 for the pinhole
      stereo.push_back(ur < 0 ? 0 : 1);
      close.push_back(pMP->mTrackDepth < gfs_li::kTrackDepthClose ? 1 : 0);
      edge_kf.push_back(it->second);
      edge_of.emplace_back(pKFi, pMP);
    }
    begin.push_back((int32_t)edge_kf.size());
  }
  const size_t n_e = edge_kf.size(), n_p = vpPoints.size();
  P.n_points = (int)n_p, P.n_edges = (int)n_e;
  P.window = window.data(), P.window_imu = window_imu.data(), P.inertial = inertial.data();
  P.fixed_Rcw = fixed_Rcw.data(), P.fixed_tcw = fixed_tcw.data(), P.points = points.data(), P.point_edge_begin = begin.data();
  P.edge_kf = edge_kf.data(), P.obs = obs.data(), P.inv_sigma2 = w.data(), P.stereo = stereo.data(), P.close = close.data();
  std::vector<double> points_out(3 * n_p + 1), chi2(n_e + 1);
  std::vector<uint8_t> depth_positive(n_e + 1), erase(n_e + 1);
  gfs_lba_inertial_solution S{};
  S.window = window_out.data(), S.points = points_out.data(), S.edge_chi2 = chi2.data(), S.edge_depth_positive = depth_positive.data();
  S.edge_erase = erase.data();
  solve(P, S);
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  const float err = S.err, err_end = S.err_end;
  if (((float)gfs_li::kFailGateFactor * err < err_end || std::isnan(err) || std::isnan(err_end)) && !bLarge) return false;
  for (size_t e = 0; e < n_e; e++)
    if (erase[e] && !edge_of[e].second->isBad()) {
      edge_of[e].first->EraseMapPointMatch(edge_of[e].second);
      edge_of[e].second->EraseObservation(edge_of[e].first);
    }
  for (KeyFrame* pKFi : lFixedKeyFrames) pKFi->mnBAFixedForKF = 0;
  for (int i = 0; i < N; i++) {
    Access::set_pose_velocity_bias(vpOptimizableKFs[i], window_out[(size_t)i]);
    vpOptimizableKFs[i]->mnBALocalForKF = 0;
  }
  for (size_t l = 0; l < n_p; l++) {
    Access::set_world_pos(vpPoints[l], &points_out[3 * l]);
    vpPoints[l]->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
  return true;
}

// numeric core: one window on the device
class LocalInertialBADevice {
 public:
  explicit LocalInertialBADevice(int max_points = 8192, int max_edges = 131072, int max_opt = gfs_li::kMaxWindowLarge,
                                 int max_fixed = gfs_li::kMaxFixKF, int device = 0) {
    check(gfs_lba_inertial_create(device, max_opt, max_fixed, max_points, max_edges, &h_), "gfs_lba_inertial_create");
  }
  ~LocalInertialBADevice() { gfs_lba_inertial_destroy(h_); }
  LocalInertialBADevice(const LocalInertialBADevice&) = delete;
  LocalInertialBADevice& operator=(const LocalInertialBADevice&) = delete;
  void solve(const gfs_lba_inertial_problem& p, gfs_lba_inertial_solution& s) { check(gfs_lba_inertial_solve(h_, &p, &s), "gfs_lba_inertial_solve"); }

 private:
  gfs_lba_inertial* h_ = nullptr;
};

}  // namespace gfs_host

// The drop-ins written against the reference's own types (cv::Mat, cv::KeyPoint, Eigen, Sophus, ORB_SLAM3::ORBextractor as a base
// class, small_gicp::RegistrationResult) are in gfs_reference_dropins.hpp beside this file.

