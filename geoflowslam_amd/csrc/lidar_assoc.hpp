// The shared half of the point-to-plane lidar edges (EdgeSE3LidarPoint2Plane, reference include/G2oTypes.h:574-600, built by
// Optimizer::GenerateLidarEdge, src/Optimizer.cc:8339-8421): the uploaded local map and its hash grid, the float Sophus pose of the
// association, the per-point body of the association (5-NN, the float ColPivHouseholderQR plane, the gates, the weight), and the edge's
// error.  Used by pose_lidar.hip (PoseLidarVisualOptimization, k_pl_assoc; the window association of LocalVisualLidarBA,
// k_lba_lidar_assoc) and lba.hip (the lidar edges of LocalVisualLidarBA's error and linearisation kernels).
//
// GenerateLidarEdge's literals stay in pose_lidar.hip: lidar_point_edge takes them from its template parameter G
// (G::kSqDisGate, G::kPlaneGate, G::kWeightSlope, G::kMinWeight).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "g2o_se3_dev.hpp"
#include "gfs_common.hpp"

struct gfs_lidar_map {
  int device, max_points, n = 0, nb = 0;
  gfs::DevBuf<float4> d_pts;  // sorted by bucket; w = original index (bits)
  gfs::DevBuf<int> d_start;   // [nb + 1]
};

namespace gfs_lidar {

// The map grid: cells of 1.25 m.  A map point whose float squared distance to a query is < 1.0 differs from it by at most 1 m
// (exactly) on every axis; cells are taken of q +- 1.01 (in double), so at most 3 cells per axis, and every such point is visited.
constexpr double kInvCell = 0.8;

// ------------------------------------------------------------------ Sophus::SE3f arithmetic (float)

__device__ inline void so3f_normalize(float* q) {  // Quaternionf::norm left to right, coeffs /= norm
  float s = q[0] * q[0];
  s = s + q[1] * q[1];
  s = s + q[2] * q[2];
  s = s + q[3] * q[3];
  const float len = sqrtf(s);
  for (int i = 0; i < 4; i++) q[i] /= len;
}
__device__ inline void init_pose_f(const float* q, const float* t, double* M) {  // Converter::toMatrix4d(SE3f(q, t).inverse())
  float qi[4] = {-q[0], -q[1], -q[2], q[3]};
  so3f_normalize(qi);
  const float p[3] = {t[0] * -1.0f, t[1] * -1.0f, t[2] * -1.0f};
  float uv[3] = {qi[1] * p[2] - qi[2] * p[1], qi[2] * p[0] - qi[0] * p[2], qi[0] * p[1] - qi[1] * p[0]};
  for (int i = 0; i < 3; i++) uv[i] += uv[i];
  const float cr[3] = {qi[1] * uv[2] - qi[2] * uv[1], qi[2] * uv[0] - qi[0] * uv[2], qi[0] * uv[1] - qi[1] * uv[0]};
  const float x = qi[0], y = qi[1], z = qi[2], w = qi[3];
  const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const float R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * r + c] = (double)R[3 * r + c];
    M[4 * r + 3] = (double)((p[r] + w * uv[r]) + cr[r]);
  }
}

__device__ __host__ inline long long cell_of(double v) { return (long long)floor(v * kInvCell); }
__device__ __host__ inline unsigned cell_hash(long long x, long long y, long long z, int nb) {
  return (((unsigned)x * 73856093u) ^ ((unsigned)y * 19349663u) ^ ((unsigned)z * 83492791u)) & (unsigned)(nb - 1);
}

// (d, i) < (d', i'): the float squared distance, ties by the lower map index
__device__ __forceinline__ bool knn_less(float d, int i, float d2, int i2) { return d < d2 || (d == d2 && i < i2); }

// Eigen ColPivHouseholderQR<Matrix<float, 5, 3>>(A).solve(-1) (see the restatement for the line-by-line references).  Every index is
// a compile-time constant; the run-time pivot column is matched against its possible values.
__device__ __forceinline__ float sq_tail(const float (&A)[5][3], int col, int from) {
  float s = 0.0f;
#pragma unroll
  for (int r = 0; r < 5; r++)
    if (r >= from) {
      const float v = A[r][col] * A[r][col];
      s = r == from ? v : s + v;
    }
  return s;
}
__device__ inline void qr_plane(float (&A)[5][3], float* x) {
  const float eps = 1.1920928955078125e-07f, fmin_ = 1.17549435e-38f;
  float hc[3], nU[3], nD[3];
  int tr[3];
#pragma unroll
  for (int k = 0; k < 3; k++) nU[k] = nD[k] = sqrtf(sq_tail(A, k, 0));
  float maxn = nU[0];
  if (nU[1] > maxn) maxn = nU[1];
  if (nU[2] > maxn) maxn = nU[2];
  const float th_help = ((maxn * eps) * (maxn * eps)) / 5.0f;
  const float downdate_th = sqrtf(eps);
  int nz = 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int bi = k;
    float bv = nU[k];
#pragma unroll
    for (int j = k + 1; j < 3; j++)
      if (nU[j] > bv) {
        bv = nU[j];
        bi = j;
      }
    if (nz == 3 && bv * bv < th_help * (float)(5 - k)) nz = k;
    tr[k] = bi;
#pragma unroll
    for (int j = k + 1; j < 3; j++)
      if (bi == j) {
#pragma unroll
        for (int r = 0; r < 5; r++) {
          const float tmp = A[r][k];
          A[r][k] = A[r][j];
          A[r][j] = tmp;
        }
        float tmp = nU[k];
        nU[k] = nU[j];
        nU[j] = tmp;
        tmp = nD[k];
        nD[k] = nD[j];
        nD[j] = tmp;
      }
    const float tailSq = sq_tail(A, k, k + 1), c0 = A[k][k];
    float tau, beta;
    if (tailSq <= fmin_) {
      tau = 0.0f;
      beta = c0;
#pragma unroll
      for (int r = k + 1; r < 5; r++) A[r][k] = 0.0f;
    } else {
      beta = sqrtf(c0 * c0 + tailSq);
      if (c0 >= 0.0f) beta = -beta;
      const float den = c0 - beta;
#pragma unroll
      for (int r = k + 1; r < 5; r++) A[r][k] = A[r][k] / den;
      tau = (beta - c0) / beta;
    }
    A[k][k] = beta;
    hc[k] = tau;
    if (tau != 0.0f) {
#pragma unroll
      for (int j = k + 1; j < 3; j++) {
        float tmp = 0.0f;
#pragma unroll
        for (int r = k + 1; r < 5; r++) {
          const float v = A[r][k] * A[r][j];
          tmp = r == k + 1 ? v : tmp + v;
        }
        tmp += A[k][j];
        A[k][j] -= tau * tmp;
#pragma unroll
        for (int r = k + 1; r < 5; r++) A[r][j] -= (tau * A[r][k]) * tmp;
      }
    }
#pragma unroll
    for (int j = k + 1; j < 3; j++) {
      if (nU[j] != 0.0f) {
        float temp = fabsf(A[k][j]) / nU[j];
        temp = (1.0f + temp) * (1.0f - temp);
        temp = temp < 0.0f ? 0.0f : temp;
        const float ratio = nU[j] / nD[j];
        const float temp2 = temp * (ratio * ratio);
        if (temp2 <= downdate_th) {
          nD[j] = sqrtf(sq_tail(A, j, k + 1));
          nU[j] = nD[j];
        } else {
          nU[j] *= sqrtf(temp);
        }
      }
    }
  }
  if (nz == 0) {
    x[0] = x[1] = x[2] = 0.0f;
    return;
  }
  float c[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (k >= nz || hc[k] == 0.0f) continue;
    const float tau = hc[k];
    float tmp = 0.0f;
#pragma unroll
    for (int r = k + 1; r < 5; r++) {
      const float v = A[r][k] * c[r];
      tmp = r == k + 1 ? v : tmp + v;
    }
    tmp += c[k];
    c[k] -= tau * tmp;
#pragma unroll
    for (int r = k + 1; r < 5; r++) c[r] -= (tau * A[r][k]) * tmp;
  }
#pragma unroll
  for (int i = 2; i >= 0; i--) {
    if (i < nz && c[i] != 0.0f) {
      c[i] /= A[i][i];
#pragma unroll
      for (int r = 0; r < i; r++) c[r] -= c[i] * A[r][i];
    }
  }
  // x[perm[i]] = c[i], perm = identity with the transpositions tr[0], tr[1], tr[2] applied on the right
  int perm[3] = {0, 1, 2};
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int j = k + 1; j < 3; j++)
      if (tr[k] == j) {
        const int t = perm[k];
        perm[k] = perm[j];
        perm[j] = t;
      }
  float o[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float v = i < nz ? c[i] : 0.0f;
#pragma unroll
    for (int j = 0; j < 3; j++)
      if (perm[i] == j) o[j] = v;
  }
  x[0] = o[0];
  x[1] = o[1];
  x[2] = o[2];
}

// GenerateLidarEdge for one cloud point po (camera frame) of a frame whose initPose (Converter::toMatrix4d(Tcw.inverse()), row-major
// 3 x 4) is M: pointAssociateToMap, the exact 5-NN in the map's grid, the plane, the gates.  true and (plane, s) when the point gets
// an edge.  d / ind / slot: the caller's 5-NN registers (squared distance; map index, the tie rule; position in the grid's sorted copy).
template <class G>
__device__ __forceinline__ bool lidar_point_edge(const double* M, const float* po, const float4* __restrict__ map_pts,
                                                 const int* __restrict__ map_start, int map_nb, float (&d)[5], int (&ind)[5],
                                                 int (&slot)[5], float4* plane, float* s_out) {
  const float ox = po[0], oy = po[1], oz = po[2];
  float q[3];
#pragma unroll
  for (int r = 0; r < 3; r++)  // pointAssociateToMap: double expression, stored as float
    q[r] = (float)(M[4 * r] * (double)ox + M[4 * r + 1] * (double)oy + M[4 * r + 2] * (double)oz + M[4 * r + 3]);
  if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) return false;
  // map points lie within 1e6 m (gfs_lidar_map_set): a query beyond 2e6 m on any axis is more than 1 m from every one of them and
  // fails the gate in the brute force too; skipping it here also keeps cell_of's conversion to long long in range
  if (fabsf(q[0]) > 2e6f || fabsf(q[1]) > 2e6f || fabsf(q[2]) > 2e6f) return false;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    d[k] = __builtin_inff();
    ind[k] = 0x7fffffff;
    slot[k] = 0;
  }
  long long lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = cell_of((double)q[a] - 1.01);
    hi[a] = cell_of((double)q[a] + 1.01);
  }
  for (long long cz = lo[2]; cz <= hi[2]; cz++)
    for (long long cy = lo[1]; cy <= hi[1]; cy++)
      for (long long cx = lo[0]; cx <= hi[0]; cx++) {
        const unsigned b = cell_hash(cx, cy, cz, map_nb);
        const int e = map_start[b + 1];
        for (int m = map_start[b]; m < e; m++) {
          const float4 P = map_pts[m];
          // the bucket may hold other cells' points (hash collisions): each point is taken in its own cell only
          if (cell_of((double)P.x) != cx || cell_of((double)P.y) != cy || cell_of((double)P.z) != cz) continue;
          const float dx = q[0] - P.x, dy = q[1] - P.y, dz = q[2] - P.z;
          float dd = 0.0f;  // FLANN L2: ((0 + dx^2) + dy^2) + dz^2
          dd += dx * dx;
          dd += dy * dy;
          dd += dz * dz;
          const int mi = __float_as_int(P.w);
          if (!knn_less(dd, mi, d[4], ind[4])) continue;
#pragma unroll
          for (int k = 4; k >= 0; k--) {  // insertion from the back: slot k - 1 is read before it is overwritten
            const int kp = k > 0 ? k - 1 : 0;
            const bool lt_k = knn_less(dd, mi, d[k], ind[k]);
            const bool lt_prev = k > 0 && knn_less(dd, mi, d[kp], ind[kp]);
            if (lt_k) {
              d[k] = lt_prev ? d[kp] : dd;
              ind[k] = lt_prev ? ind[kp] : mi;
              slot[k] = lt_prev ? slot[kp] : m;
            }
          }
        }
      }
  if (ind[4] == 0x7fffffff || !(d[4] < G::kSqDisGate)) return false;
  float N[5][3], A[5][3];  // matA0: the neighbours as rows, in distance order
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const float4 P = map_pts[slot[k]];
    N[k][0] = A[k][0] = P.x;
    N[k][1] = A[k][1] = P.y;
    N[k][2] = A[k][2] = P.z;
  }
  float X[3];
  qr_plane(A, X);
  float pa = X[0], pb = X[1], pc = X[2], pd = 1;
  const float ps = sqrtf(pa * pa + pb * pb + pc * pc);
  pa /= ps;
  pb /= ps;
  pc /= ps;
  pd /= ps;
  bool valid = true;
#pragma unroll
  for (int k = 0; k < 5; k++)
    if ((double)fabsf(pa * N[k][0] + pb * N[k][1] + pc * N[k][2] + pd) > G::kPlaneGate) valid = false;
  if (!valid) return false;
  const float pd2 = pa * q[0] + pb * q[1] + pc * q[2] + pd;
  const float s = (float)(1 - G::kWeightSlope * (double)fabsf(pd2) / (double)sqrtf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])));
  if (!((double)s > G::kMinWeight)) return false;
  *plane = make_float4(pa, pb, pc, pd);
  *s_out = s;
  return true;
}

// ------------------------------------------------------------------ the edge (EdgeSE3LidarPoint2Plane::computeError)

__device__ __forceinline__ void se3_inverse(const double* q, const double* t, double* W) {  // SE3Quat::inverse -> W = (q', t')
  W[0] = -q[0];
  W[1] = -q[1];
  W[2] = -q[2];
  W[3] = q[3];
  const double nt[3] = {t[0] * -1., t[1] * -1., t[2] * -1.};
  gfs_se3::quat_rotate(W, nt, W + 4);
}
__device__ __forceinline__ double lidar_err(const double* W, const double* p, const float4 pl, float s) {
  double pw[3];
  gfs_se3::quat_rotate(W, p, pw);
  pw[0] += W[4];
  pw[1] += W[5];
  pw[2] += W[6];
  const double dot = pw[0] * (double)pl.x + pw[1] * (double)pl.y + pw[2] * (double)pl.z;
  return (double)s * (dot + (double)pl.w);
}

// ------------------------------------------------------------------ the window association of LocalVisualLidarBA (pose_lidar.hip)
struct WindowKF {  // one key-frame of a window that gets lidar edges
  int pose;        // its index in the gfs_lba_problem
  int begin, n;    // its cloud in the window's concatenated cloud
  float q[4], t[3];  // Tcw as the float Sophus pose the association uses ((float) of the problem's double pose)
};
// GenerateLidarEdge's cloud-size gate (a key-frame with fewer points gets no edge)
int min_cloud();
// EdgeSE3LidarPoint2Plane's information (1e2) and Huber delta ((float) sqrt(1.0)): the one definition is pose_lidar.hip's
double edge_information();
double edge_huber_delta();
// One launch over the window's concatenated cloud: flag[i] = 1 and (plane[i], s[i]) when point i gets an edge.  Asynchronous on s.
int launch_window_assoc(const gfs_lidar_map* map, const WindowKF* d_kf, int n_kf, int max_n, const float* d_cloud, uint8_t* d_flag,
                        float4* d_plane, float* d_s, hipStream_t s);

}  // namespace gfs_lidar
