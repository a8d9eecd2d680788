// Test harness of the frame-cloud adaptor (geoflowslam_amd/host/gfs_adaptors.hpp: FrameCloudConfigFrom, FrameCloudExtractor) over a
// plain stand-in for the reference's LidarParam.  fca_config: the configuration the adaptor derives (CPU).  fca_extract: one Extract
// call (GPU); returns the GFS_ERR_* code of a refusal.
#include <cstring>
#include <vector>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"

namespace {
struct LidarParam {  // the getters Frame::Frame reads (reference include/Lidar.h)
  double horizontal_angle, max_distance, local_map_resolution;
  double getHorizontalAngle() const { return horizontal_angle; }
  double getMaxDistance() const { return max_distance; }
  double getLocalMapResolution() const { return local_map_resolution; }
};
}  // namespace

extern "C" {

void fca_config(double horizontal_angle, double max_distance, double local_map_resolution, float downsize, double out5[5]) {
  const gfs_frame_cloud_config c = gfs_host::FrameCloudConfigFrom(LidarParam{horizontal_angle, max_distance, local_map_resolution}, downsize);
  out5[0] = c.horizontal_angle;
  out5[1] = c.max_distance;
  out5[2] = c.local_map_resolution;
  out5[3] = c.downsize_resolution;
  out5[4] = c.angle_guard_deg;
}

int fca_extract(double horizontal_angle, double max_distance, double local_map_resolution, float downsize, const float* xyzw, int n,
                float* cloud, float* down, int32_t* info13) {
  try {
    gfs_host::FrameCloudExtractor ex(LidarParam{horizontal_angle, max_distance, local_map_resolution}, downsize, n > 0 ? n : 1);
    std::vector<float> c, d;
    const gfs_frame_cloud_info info = ex.Extract(xyzw, n, c, d);
    std::memcpy(info13, &info, sizeof info);
    if (!c.empty()) std::memcpy(cloud, c.data(), c.size() * sizeof(float));
    if (!d.empty()) std::memcpy(down, d.data(), d.size() * sizeof(float));
    return 0;
  } catch (const std::exception&) {
    return -100;
  }
}

}  // extern "C"
