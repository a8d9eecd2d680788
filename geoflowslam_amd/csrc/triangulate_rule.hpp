// The rule of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:803-1127) for single-camera pinhole key frames, stated
// once for the device and the host: the candidate gates of ORBmatcher::SearchForTriangulation
// (src/ORBmatcher.cc:1244-1319), the rotation histogram (:1331-1365) and the per-match triangulation with its gates
// (src/LocalMapping.cc:904-1100).  float, every operation rounded once, sums left to right, double where the source promotes; the
// translation units that include this are built with -ffp-contract=off.  Two written rules stand where the reference's arithmetic
// depends on a library: the null vector of the 4 x 4 system (null_vector below, for Eigen::JacobiSVD) and the stereo parallax
// cosine (cos_stereo below, for cosf(2 * atan2f(mb / 2, depth))).
#pragma once
#include <cmath>
#include <cstdint>

#if !defined(GFS_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFS_HD __host__ __device__ inline
#else
#define GFS_HD inline
#endif
#endif

namespace gfs_tri {

constexpr int kThLow = 50;                    // ORBmatcher::TH_LOW
constexpr int kHisto = 30;                    // ORBmatcher::HISTO_LENGTH
constexpr float kEpipoleFactor = 100.0f;      // 100 * mvScaleFactors[kp2.octave] (src/ORBmatcher.cc:1274)
constexpr double kEpipolarChi2 = 3.84;        // dsqr < 3.84 * unc (src/CameraModels/Pinhole.cpp:128)
constexpr double kCosParallax = 0.9998;       // src/LocalMapping.cc:1008
constexpr double kCosParallaxInertial = 0.9996;  // :1007
constexpr double kChi2Mono = 5.991;           // :1045, :1068
constexpr double kChi2Stereo = 7.8;           // :1055, :1077
constexpr float kRatioFactor = 1.5f;          // ratioFactor = 1.5f * mfScaleFactor (:840; the caller multiplies)
constexpr int kNeighbours = 10, kNeighboursMono = 30;  // nn (:805-807)
constexpr int kNoCandidate = 255;             // a pair that can never match, in the candidate matrix
constexpr int kJacobiSweeps = 30;
constexpr double kJacobiEps = 2.220446049250313e-16;  // 2^-52

// where the loop body of :904-1100 ends for an idx1 (GFS_TRI_* of include/gfs_abi.h)
enum Exit {
  kNoMatch = 0, kLowParallax = 1, kSvdWZero = 2, kUnprojectFailed = 3, kBehind1 = 4, kBehind2 = 5, kReproj1 = 6, kReproj2 = 7,
  kZeroDist = 8, kFar = 9, kScale = 10, kCreated = 11
};

struct Cam {  // what the rule reads of a key frame besides its key-points
  float Tcw[12], Ow[3], Rwc[9], twc[3];
  float fx, fy, cx, cy, invfx, invfy, mbf, mb;
  int n_levels;
  float scale[16], sigma2[16];
};

struct Kp {  // one key-point: mvKeysUn position / octave / angle, mvKeys position, mvuRight, mvDepth
  float x, y, angle, kx, ky, ur, depth;
  int oct;
};

struct Line {  // the epipolar line of kp1 in the second image, l = x1' F12 = [a b c] (Pinhole.cpp:115-117)
  float a, b, c;
};

GFS_HD Line epipolar_line(const float* F12, float x1, float y1) {  // F12 row-major
  Line l;
  l.a = (x1 * F12[0] + y1 * F12[3]) + F12[6];
  l.b = (x1 * F12[1] + y1 * F12[4]) + F12[7];
  l.c = (x1 * F12[2] + y1 * F12[5]) + F12[8];
  return l;
}

// the epipole gate (src/ORBmatcher.cc:1270-1277) and, unless bCoarse, Pinhole::epipolarConstrain (Pinhole.cpp:119-128) of one pair
// whose descriptor distance is already <= TH_LOW.  stereo1 / stereo2: mvuRight >= 0; scale2 / sigma2_2 at kp2's octave.
GFS_HD bool candidate_ok(const Line& l, const float* ep, bool stereo1, bool stereo2, float x2, float y2, float scale2, float sigma2_2, bool coarse) {
  if (!stereo1 && !stereo2) {
    const float ex = ep[0] - x2, ey = ep[1] - y2;
    if (ex * ex + ey * ey < kEpipoleFactor * scale2) return false;
  }
  if (coarse) return true;
  const float num = (l.a * x2 + l.b * y2) + l.c;
  const float den = l.a * l.a + l.b * l.b;
  if (den == 0) return false;
  const float dsqr = num * num / den;
  return (double)dsqr < kEpipolarChi2 * (double)sigma2_2;
}

// the rotation bin of a match (src/ORBmatcher.cc:1332-1335)
GFS_HD int rot_bin(float angle1, float angle2) {
  float rot = angle1 - angle2;
  if (rot < 0.0) rot += 360.0f;
  int bin = (int)roundf(rot * (1.0f / kHisto));
  if (bin == kHisto) bin = 0;
  return bin;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:2542-2583) over the bin counts
GFS_HD void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  ind1 = ind2 = ind3 = -1;
  for (int i = 0; i < kHisto; i++) {
    const int s = hist[i];
    if (s > max1) {
      max3 = max2;
      max2 = max1;
      max1 = s;
      ind3 = ind2;
      ind2 = ind1;
      ind1 = i;
    } else if (s > max2) {
      max3 = max2;
      max2 = s;
      ind3 = ind2;
      ind2 = i;
    } else if (s > max3) {
      max3 = s;
      ind3 = i;
    }
  }
  if (max2 < 0.1f * (float)max1) {
    ind2 = -1;
    ind3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    ind3 = -1;
  }
}

// Written rule 1 (for cos(2 * atan2(mb / 2, depth)), :993-996): the float nearest to (d^2 - h^2) / (d^2 + h^2) in double, h = mb / 2
GFS_HD float cos_stereo(float mb, float depth) {
  const float h = mb / 2;
  const double d2 = (double)depth * (double)depth, h2 = (double)h * (double)h;
  return (float)((d2 - h2) / (d2 + h2));
}

// one rotation of columns P, Q of the one-sided Jacobi; true iff the columns were rotated
template <int P, int Q>
GFS_HD bool jacobi_pair(double (&A)[4][4], double (&V)[4][4]) {
  const double alpha = ((A[0][P] * A[0][P] + A[1][P] * A[1][P]) + A[2][P] * A[2][P]) + A[3][P] * A[3][P];
  const double beta = ((A[0][Q] * A[0][Q] + A[1][Q] * A[1][Q]) + A[2][Q] * A[2][Q]) + A[3][Q] * A[3][Q];
  const double gamma = ((A[0][P] * A[0][Q] + A[1][P] * A[1][Q]) + A[2][P] * A[2][Q]) + A[3][P] * A[3][Q];
  if (!(fabs(gamma) > kJacobiEps * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double r = fabs(zeta) + sqrt(1.0 + zeta * zeta);
  const double t = zeta < 0.0 ? -1.0 / r : 1.0 / r;
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  for (int k = 0; k < 4; k++) {
    const double ap = A[k][P], aq = A[k][Q];
    A[k][P] = c * ap - s * aq;
    A[k][Q] = s * ap + c * aq;
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
  return true;
}

// Written rule 2 (for Eigen::JacobiSVD<Matrix4f>(A, ComputeFullV).matrixV().col(3)): one-sided (Hestenes) Jacobi on the columns of
// the float matrix converted to double, cyclic order, at most 30 sweeps; the column of V of the smallest column norm of the rotated A
// (lowest index on ties), each component rounded to float.
GFS_HD void null_vector(const float (&Af)[4][4], float* x3Dh) {
  double A[4][4], V[4][4];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      A[r][c] = (double)Af[r][c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    bool rotated = jacobi_pair<0, 1>(A, V);
    rotated |= jacobi_pair<0, 2>(A, V);
    rotated |= jacobi_pair<0, 3>(A, V);
    rotated |= jacobi_pair<1, 2>(A, V);
    rotated |= jacobi_pair<1, 3>(A, V);
    rotated |= jacobi_pair<2, 3>(A, V);
    if (!rotated) break;
  }
  double n[4];
  for (int c = 0; c < 4; c++) n[c] = ((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]) + A[3][c] * A[3][c];
  double best = n[0];
  double v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
  for (int c = 1; c < 4; c++)
    if (n[c] < best) {
      best = n[c];
      for (int k = 0; k < 4; k++) v[k] = V[k][c];
    }
  for (int k = 0; k < 4; k++) x3Dh[k] = (float)v[k];
}

// GeometricTools::Triangulate (src/GeometricTools.cc:48-72) with written rule 2
GFS_HD bool triangulate(const float* xn1, const float* xn2, const float* T1, const float* T2, float* x3D) {
  float A[4][4];
  for (int c = 0; c < 4; c++) {
    A[0][c] = xn1[0] * T1[8 + c] - T1[c];
    A[1][c] = xn1[1] * T1[8 + c] - T1[4 + c];
    A[2][c] = xn2[0] * T2[8 + c] - T2[c];
    A[3][c] = xn2[1] * T2[8 + c] - T2[4 + c];
  }
  float h[4];
  null_vector(A, h);
  if (h[3] == 0) return false;
  for (int k = 0; k < 3; k++) x3D[k] = h[k] / h[3];
  return true;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:852-866): mvKeys, not mvKeysUn
GFS_HD bool unproject_stereo(const Cam& C, const Kp& k, float* x3D) {
  const float z = k.depth;
  if (!(z > 0)) return false;
  const float x = (k.kx - C.cx) * z * C.invfx, y = (k.ky - C.cy) * z * C.invfy;
  for (int r = 0; r < 3; r++) x3D[r] = ((C.Rwc[3 * r] * x + C.Rwc[3 * r + 1] * y) + C.Rwc[3 * r + 2] * z) + C.twc[r];
  return true;
}

GFS_HD float row_dot(const float* T, int r, const float* p) { return ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3]; }

// the reprojection gate of one view (:1035-1079); mbf is the CURRENT key frame's in both views (:1049, :1071)
GFS_HD bool reprojection_ok(const Cam& C, const Kp& k, const float* x3D, float z, float mbf) {
  const float sigma2 = C.sigma2[k.oct];
  const float x = row_dot(C.Tcw, 0, x3D), y = row_dot(C.Tcw, 1, x3D);
  const float invz = (float)(1.0 / (double)z);
  if (!(k.ur >= 0)) {
    const float u = C.fx * x / z + C.cx, v = C.fy * y / z + C.cy;
    const float ex = u - k.x, ey = v - k.y;
    return !((double)(ex * ex + ey * ey) > kChi2Mono * (double)sigma2);
  }
  const float u = C.fx * x * invz + C.cx;
  const float u_r = u - mbf * invz;
  const float v = C.fy * y * invz + C.cy;
  const float ex = u - k.x, ey = v - k.y, er = u_r - k.ur;
  return !((double)((ex * ex + ey * ey) + er * er) > kChi2Stereo * (double)sigma2);
}

// One match (idx1 of the current key frame C1, idx2 of the neighbour C2): the body of the loop :904-1100 up to "Triangulation is
// succesfull".  x3D is the point where the exit is >= kBehind1, zeros before; point_stereo is bPointStereo.
GFS_HD int triangulate_match(const Cam& C1, const Cam& C2, const Kp& k1, const Kp& k2, bool inertial, bool far_points, float th_far,
                             float ratio_factor, float* x3D, int* point_stereo) {
  x3D[0] = x3D[1] = x3D[2] = 0.0f;
  *point_stereo = 0;
  const bool st1 = k1.ur >= 0, st2 = k2.ur >= 0;
  const float xn1[3] = {(k1.x - C1.cx) / C1.fx, (k1.y - C1.cy) / C1.fy, 1.0f};
  const float xn2[3] = {(k2.x - C2.cx) / C2.fx, (k2.y - C2.cy) / C2.fy, 1.0f};
  float ray1[3], ray2[3];  // Rwc = Rcw^T of the 3 x 4 pose
  for (int r = 0; r < 3; r++) {
    ray1[r] = (C1.Tcw[r] * xn1[0] + C1.Tcw[4 + r] * xn1[1]) + C1.Tcw[8 + r] * xn1[2];
    ray2[r] = (C2.Tcw[r] * xn2[0] + C2.Tcw[4 + r] * xn2[1]) + C2.Tcw[8 + r] * xn2[2];
  }
  const float dot = (ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2];
  const float n1 = sqrtf((ray1[0] * ray1[0] + ray1[1] * ray1[1]) + ray1[2] * ray1[2]);
  const float n2 = sqrtf((ray2[0] * ray2[0] + ray2[1] * ray2[1]) + ray2[2] * ray2[2]);
  const float cos_rays = dot / (n1 * n2);
  const float cos_plus = cos_rays + 1;
  float cs1 = cos_plus, cs2 = cos_plus;
  if (st1)
    cs1 = cos_stereo(C1.mb, k1.depth);
  else if (st2)
    cs2 = cos_stereo(C2.mb, k2.depth);
  const float cs = cs2 < cs1 ? cs2 : cs1;  // std::min(cs1, cs2)
  bool stereo = false;
  if (cos_rays < cs && cos_rays > 0 && (st1 || st2 || (double)cos_rays < (inertial ? kCosParallaxInertial : kCosParallax))) {
    if (!triangulate(xn1, xn2, C1.Tcw, C2.Tcw, x3D)) {
      x3D[0] = x3D[1] = x3D[2] = 0.0f;
      return kSvdWZero;
    }
  } else if (st1 && cs1 < cs2) {
    stereo = true;
    if (!unproject_stereo(C1, k1, x3D)) return *point_stereo = 1, kUnprojectFailed;
  } else if (st2 && cs2 < cs1) {
    stereo = true;
    if (!unproject_stereo(C2, k2, x3D)) return *point_stereo = 1, kUnprojectFailed;
  } else {
    return kLowParallax;
  }
  *point_stereo = stereo ? 1 : 0;
  const float z1 = row_dot(C1.Tcw, 2, x3D);
  if (z1 <= 0) return kBehind1;
  const float z2 = row_dot(C2.Tcw, 2, x3D);
  if (z2 <= 0) return kBehind2;
  if (!reprojection_ok(C1, k1, x3D, z1, C1.mbf)) return kReproj1;
  if (!reprojection_ok(C2, k2, x3D, z2, C1.mbf)) return kReproj2;
  const float a[3] = {x3D[0] - C1.Ow[0], x3D[1] - C1.Ow[1], x3D[2] - C1.Ow[2]};
  const float b[3] = {x3D[0] - C2.Ow[0], x3D[1] - C2.Ow[1], x3D[2] - C2.Ow[2]};
  const float dist1 = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  const float dist2 = sqrtf((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  if (dist1 == 0 || dist2 == 0) return kZeroDist;
  if (far_points && (dist1 >= th_far || dist2 >= th_far)) return kFar;
  const float ratio_dist = dist2 / dist1;
  const float ratio_octave = C1.scale[k1.oct] / C2.scale[k2.oct];
  if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor) return kScale;
  return kCreated;
}

}  // namespace gfs_tri
