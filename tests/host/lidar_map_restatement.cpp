// Sequential CPU restatement of the lidar local-map build (LidarMapping::viewer's loop body, reference src/LidarMapping.cc:162-182)
// under the rule of DESIGN.md section 11: transformPointCloud (:107-127) with toMatrix4d(SE3f(q, t).inverse()), concatenation in
// list order, pcl::VoxelGrid<PointXYZRGBA>::applyFilter with default settings (stable order inside a voxel, float centroid by a true
// division), the passthrough branch and the refusals.  One thread, no vector instructions of its own choosing: built with
// g++ -O2 -ffp-contract=off by tests/lidar_map_support.py.  The GPU library is compared with this bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int kOk = 0, kInvalid = -1, kCapacity = -4, kUnsupported = -5;  // gfs_status values
constexpr long long kIntMax = 2147483647LL;

// Converter::toMatrix4d(Sophus::SE3f(q, t).inverse()) as a row-major 3 x 4 of doubles.  SE3f::inverse: so3().inverse() is the
// conjugate; the SO3 constructor normalises (coeffs /= norm, norm = sqrt of the squares added left to right); the translation is
// inverse_rotation * (t * -1); SO3 * point is p + w uv + q.vec x uv with uv = 2 (q.vec x p); matrix() is Eigen's toRotationMatrix.
void inverse_pose_matrix(const float* q, const float* t, double* M) {
  float c[4] = {-q[0], -q[1], -q[2], q[3]};
  float n2 = c[0] * c[0];
  n2 = n2 + c[1] * c[1];
  n2 = n2 + c[2] * c[2];
  n2 = n2 + c[3] * c[3];
  const float len = std::sqrt(n2);
  for (float& v : c) v = v / len;
  const float x = c[0], y = c[1], z = c[2], w = c[3];
  const float p[3] = {t[0] * -1.0f, t[1] * -1.0f, t[2] * -1.0f};
  float uv[3] = {y * p[2] - z * p[1], z * p[0] - x * p[2], x * p[1] - y * p[0]};
  for (float& v : uv) v = v + v;
  const float cr[3] = {y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]};
  const float tr[3] = {(p[0] + w * uv[0]) + cr[0], (p[1] + w * uv[1]) + cr[1], (p[2] + w * uv[2]) + cr[2]};
  const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const float R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}};
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) M[4 * r + k] = (double)R[r][k];
    M[4 * r + 3] = (double)tr[r];
  }
}

void transform_cloud(const double* M, const float* in, int n, float* out) {
  for (int i = 0; i < n; i++) {
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    for (int r = 0; r < 3; r++) {
      double v = M[4 * r] * (double)x;
      v = v + M[4 * r + 1] * (double)y;
      v = v + M[4 * r + 2] * (double)z;
      v = v + M[4 * r + 3];
      out[3 * i + r] = (float)v;
    }
  }
}

struct Info {
  int32_t n_in, n_out, passthrough, div[3];
};

// pcl::VoxelGrid::applyFilter on n >= 1 points -> status; out gets at most cap points (more: kCapacity, nothing written)
int voxel_filter(const float* xyz, int n, float leaf, float* out, int cap, Info* info) {
  *info = Info{n, 0, 0, {0, 0, 0}};
  if (n < 1 || !(leaf > 0.0f) || !std::isfinite(leaf)) return kInvalid;
  for (int i = 0; i < 3 * n; i++)
    if (!std::isfinite(xyz[i]) || !(std::fabs(xyz[i]) < 1e6f)) return kInvalid;
  const float inv = 1.0f / leaf;
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) mn[a] = mx[a] = xyz[a];
  for (int i = 1; i < n; i++)
    for (int a = 0; a < 3; a++) {
      mn[a] = std::min(mn[a], xyz[3 * i + a]);
      mx[a] = std::max(mx[a], xyz[3 * i + a]);
    }
  bool pass = false;
  long long cells = 1;
  for (int a = 0; a < 3 && !pass; a++) {
    const float fd = (mx[a] - mn[a]) * inv;
    if (!(fd < 2147483648.0f)) {  // (beyond int64 too in the limit; NaN when inv is infinite and the extent 0)
      pass = true;
      break;
    }
    cells = cells * ((long long)fd + 1);  // each factor <= 2^31 and the running product <= INT32_MAX: no overflow
    if (cells > kIntMax) pass = true;
  }
  if (pass) {  // "Leaf size is too small for the input dataset": output = input
    info->passthrough = 1;
    info->n_out = n;
    if (n > cap) return kCapacity;
    std::memcpy(out, xyz, (size_t)n * 12);
    return kOk;
  }
  int min_b[3];
  long long div[3];
  for (int a = 0; a < 3; a++) {
    const float fl = std::floor(mn[a] * inv), fh = std::floor(mx[a] * inv);
    if (!(std::fabs(fl) < 2147483648.0f) || !(std::fabs(fh) < 2147483648.0f)) return kUnsupported;
    min_b[a] = (int)fl;
    div[a] = (long long)(int)fh - (long long)min_b[a] + 1;
  }
  if (div[0] * div[1] > kIntMax || div[0] * div[1] * div[2] > kIntMax) return kUnsupported;
  for (int a = 0; a < 3; a++) info->div[a] = (int32_t)div[a];
  struct Pair {
    unsigned idx;
    int i;
  };
  std::vector<Pair> pairs((size_t)n);
  const unsigned d0 = (unsigned)div[0], d01 = (unsigned)div[0] * (unsigned)div[1];
  for (int i = 0; i < n; i++) {
    unsigned ijk[3];
    for (int a = 0; a < 3; a++) ijk[a] = (unsigned)(int)(std::floor(xyz[3 * i + a] * inv) - (float)min_b[a]);
    pairs[i] = Pair{ijk[0] + ijk[1] * d0 + ijk[2] * d01, i};
  }
  std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.idx < b.idx; });
  int n_out = 0;
  for (int j = 0; j < n; j++)
    if (j == 0 || pairs[j].idx != pairs[j - 1].idx) n_out++;
  info->n_out = n_out;
  if (n_out > cap) return kCapacity;
  int o = 0;
  for (int j = 0; j < n;) {
    float s[3] = {0.0f, 0.0f, 0.0f};
    int e = j;
    for (; e < n && pairs[e].idx == pairs[j].idx; e++)
      for (int a = 0; a < 3; a++) s[a] = s[a] + xyz[3 * pairs[e].i + a];
    const float cnt = (float)(e - j);
    for (int a = 0; a < 3; a++) out[3 * o + a] = s[a] / cnt;
    o++;
    j = e;
  }
  return kOk;
}

}  // namespace

extern "C" {

void lmr_pose_matrix(const float* q, const float* t, double* M /* [12] */) { inverse_pose_matrix(q, t, M); }

// transformPointCloud over the key-frame list, concatenated: world [cloud_begin[n_kf]][3]
void lmr_transform(int n_kf, const float* q, const float* t, const int32_t* cloud_begin, const float* cloud, float* world) {
  for (int k = 0; k < n_kf; k++) {
    double M[12];
    inverse_pose_matrix(q + 4 * k, t + 3 * k, M);
    transform_cloud(M, cloud + 3 * (size_t)cloud_begin[k], cloud_begin[k + 1] - cloud_begin[k], world + 3 * (size_t)cloud_begin[k]);
  }
}

int lmr_voxel_filter(const float* xyz, int n, float leaf, float* out, int cap, int32_t* info /* [6] */) {
  Info I;
  const int rc = voxel_filter(xyz, n, leaf, out, cap, &I);
  std::memcpy(info, &I, sizeof I);
  return rc;
}

// The whole build: the map's points in map-index order; the refusals of gfs_lidar_map_build (a map of fewer than 5 points included)
int lmr_build(int n_kf, const float* q, const float* t, const int32_t* cloud_begin, const float* cloud, float leaf, float* out, int cap,
              int32_t* info /* [6] */) {
  const int n = n_kf > 0 ? cloud_begin[n_kf] : 0;
  Info I{n, 0, 0, {0, 0, 0}};
  std::memcpy(info, &I, sizeof I);
  if (!(leaf > 0.0f) || !std::isfinite(leaf) || n < 5) return kInvalid;
  std::vector<float> world((size_t)n * 3);
  lmr_transform(n_kf, q, t, cloud_begin, cloud, world.data());
  const int rc = voxel_filter(world.data(), n, leaf, out, cap, &I);
  std::memcpy(info, &I, sizeof I);
  if (rc) return rc;
  return I.n_out < 5 ? kInvalid : kOk;
}

}  // extern "C"
