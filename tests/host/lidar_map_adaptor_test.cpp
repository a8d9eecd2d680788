// Test harness for gfs_host::GatherLidarKeyFrames / LidarLocalMapper (geoflowslam_amd/host/gfs_adaptors.hpp): LidarMapping::viewer's
// loop body (reference src/LidarMapping.cc:162-182) over plain-struct key-frames (bad ones, ones without a cloud, ones with an empty
// cloud).  The gather is recorded; the map comes from the CPU restatement (tests/host/lidar_map_restatement.cpp through dlopen) or from
// the GPU library (LidarLocalMapper::Update, then gfs_lidar_map_fetch).  Built by tests/test_lidar_map_adaptor.py.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <list>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

namespace {
struct MockKeyFrame {
  bool bad = false, has_cloud = true;
  float q[4], t[3];
  const float* cloud = nullptr;
  int n = 0;
};
struct Access {
  static bool is_bad(const MockKeyFrame* k) { return k->bad; }
  static const float* cloud(const MockKeyFrame* k, int* n) {
    *n = k->n;
    return k->has_cloud ? k->cloud : nullptr;
  }
  static void get_pose(const MockKeyFrame* k, float* q, float* t) {
    std::memcpy(q, k->q, 16);
    std::memcpy(t, k->t, 12);
  }
};
}  // namespace

// seen_*: what the gather handed on (seen_sizes = key-frames, points); out_xyz / info: the map.  Returns the builder's status.
extern "C" int lidar_map_adaptor_test(const char* restatement_lib, int n_kf, const float* q, const float* t, const uint8_t* bad,
                                      const uint8_t* has_cloud, const int32_t* cloud_begin, const float* cloud, float resolution,
                                      int32_t* seen_sizes, float* seen_q, float* seen_t, int32_t* seen_cloud_begin, float* seen_cloud,
                                      float* out_xyz, int cap, int32_t* info /* [6] */) {
  try {
    static const float none = 0.0f;
    std::vector<MockKeyFrame> kfs((size_t)n_kf);
    std::list<MockKeyFrame*> lNewKeyFrames;
    for (int k = 0; k < n_kf; k++) {
      kfs[k].bad = bad[k] != 0;
      kfs[k].has_cloud = has_cloud[k] != 0;
      std::memcpy(kfs[k].q, q + 4 * k, 16);
      std::memcpy(kfs[k].t, t + 3 * k, 12);
      kfs[k].n = cloud_begin[k + 1] - cloud_begin[k];
      kfs[k].cloud = kfs[k].n ? cloud + 3 * (size_t)cloud_begin[k] : &none;
      lNewKeyFrames.push_back(&kfs[k]);
    }
    auto record = [&](const gfs_host::LidarMapFlat& f) {
      seen_sizes[0] = f.n_keyframes();
      seen_sizes[1] = f.cloud_begin.back();
      std::memcpy(seen_q, f.q.data(), f.q.size() * 4);
      std::memcpy(seen_t, f.t.data(), f.t.size() * 4);
      std::memcpy(seen_cloud_begin, f.cloud_begin.data(), f.cloud_begin.size() * 4);
      std::memcpy(seen_cloud, f.cloud.data(), f.cloud.size() * 4);
    };
    if (restatement_lib) {
      void* so = dlopen(restatement_lib, RTLD_NOW | RTLD_LOCAL);
      if (!so) return -101;
      typedef int (*fn_t)(int, const float*, const float*, const int32_t*, const float*, float, float*, int, int32_t*);
      fn_t fn = (fn_t)dlsym(so, "lmr_build");
      if (!fn) return -102;
      gfs_host::LidarMapFlat f;
      gfs_host::GatherLidarKeyFrames<Access>(lNewKeyFrames.begin(), lNewKeyFrames.end(), f);
      record(f);
      return fn(f.n_keyframes(), f.q.data(), f.t.data(), f.cloud_begin.data(), f.cloud.data(), resolution, out_xyz, cap, info);
    }
    gfs_host::LidarLocalMapper mapper(std::max(cloud_begin[n_kf], 1), std::max(n_kf, 1));
    gfs_lidar_map* map = nullptr;
    gfs_host::check(gfs_lidar_map_create(0, std::max(cap, 5), &map), "gfs_lidar_map_create");
    int rc = 0;
    try {
      const gfs_lidar_map_info I = mapper.Update<Access>(lNewKeyFrames.begin(), lNewKeyFrames.end(), resolution, map);
      std::memcpy(info, &I, sizeof I);
      int32_t n = 0;
      rc = gfs_lidar_map_fetch(map, out_xyz, cap, &n);
    } catch (const std::exception&) {
      rc = -103;
    }
    record(mapper.gathered());
    gfs_lidar_map_destroy(map);
    return rc;
  } catch (const std::exception& ex) {
    fprintf(stderr, "lidar_map_adaptor_test: %s\n", ex.what());
    return -1;
  }
}
