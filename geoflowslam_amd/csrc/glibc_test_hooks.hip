// Test hooks: the restated glibc functions (glibc_math.hpp) evaluated on the device, for tests/test_gpu_glibc_logf.py and
// tests/test_gpu_glibc_math.py (and exp: tests/test_gpu_sim3_opt.py).
#include "gfs_common.hpp"
#include "glibc_math.hpp"

namespace {

__global__ void k_test_logf(const float* __restrict__ x, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = gfs_glibc::logf(x[i]);
}

__global__ void k_test_glibc_math(const double* __restrict__ x, int n, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = gfs_glibc::sin(x[i]);
  out[n + i] = gfs_glibc::cos(x[i]);
  out[2 * (size_t)n + i] = gfs_glibc::pow3(x[i]);
}

__global__ void k_test_glibc_exp(const double* __restrict__ x, int n, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = gfs_glibc::exp(x[i]);
}

}  // namespace

extern "C" {

int gfs_test_glibc_exp(int device, const double* x, int n, double* out) {
  GFS_REQUIRE(x && out && n >= 0, GFS_ERR_INVALID_ARG, "gfs_test_glibc_exp: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  if (n == 0) return GFS_OK;
  GFS_HIP(hipSetDevice(device));
  gfs::DevBuf<double> d_x, d_o;
  int rc = d_x.alloc(n);
  if (!rc) rc = d_o.alloc(n);
  if (rc) return rc;
  GFS_HIP(hipMemcpy(d_x.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
  GFS_LAUNCH("k_test_glibc_exp", k_test_glibc_exp, dim3(gfs::div_up(n, 256)), dim3(256), 0, (hipStream_t)0, d_x.p, n, d_o.p);
  GFS_HIP(hipMemcpy(out, d_o.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return GFS_OK;
}

int gfs_test_glibc_logf(int device, const float* x, int n, float* out) {
  GFS_REQUIRE(x && out && n >= 0, GFS_ERR_INVALID_ARG, "gfs_test_glibc_logf: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  if (n == 0) return GFS_OK;
  gfs::DevBuf<float> dx, dy;
  int rc = dx.alloc(n);
  if (!rc) rc = dy.alloc(n);
  if (rc) return rc;
  GFS_HIP(hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_test_logf, dim3((n + 255) / 256), dim3(256), 0, 0, (const float*)dx.p, n, dy.p);
  GFS_HIP(hipGetLastError());
  GFS_HIP(hipMemcpy(out, dy.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return GFS_OK;
}

int gfs_test_glibc_math(int device, const double* x, int n, double* sin_out, double* cos_out, double* pow3_out) {
  GFS_REQUIRE(x && sin_out && cos_out && pow3_out && n >= 0, GFS_ERR_INVALID_ARG, "gfs_test_glibc_math: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  if (n == 0) return GFS_OK;
  GFS_HIP(hipSetDevice(device));
  gfs::DevBuf<double> d_x, d_o;
  int rc = d_x.alloc(n);
  if (!rc) rc = d_o.alloc((size_t)3 * n);
  if (rc) return rc;
  GFS_HIP(hipMemcpy(d_x.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
  GFS_LAUNCH("k_test_glibc_math", k_test_glibc_math, dim3(gfs::div_up(n, 256)), dim3(256), 0, (hipStream_t)0, d_x.p, n, d_o.p);
  GFS_HIP(hipMemcpy(sin_out, d_o.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(cos_out, d_o.p + n, (size_t)n * 8, hipMemcpyDeviceToHost));
  GFS_HIP(hipMemcpy(pow3_out, d_o.p + 2 * (size_t)n, (size_t)n * 8, hipMemcpyDeviceToHost));
  return GFS_OK;
}

}  // extern "C"
