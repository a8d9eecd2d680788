// Eigen 3.4 SelfAdjointEigenSolver<Matrix3d>::computeDirect (closed form) for the covariances of gicp.hip's k_knn_cov,
// k_knn_cov_far and k_knn_cov_far_wg, stated once for the device and the host: double, every operation
// rounded once, in Eigen's order; the translation units that include this are built with -ffp-contract=off.
//
// No private array is indexed at run time.  The shifted matrix is symmetric, so it is carried as its six distinct entries
// (Sym3); the column with the largest absolute diagonal entry and its two followers are picked by three-way selects on i0, the
// larger of the two cross products is picked before its three divisions, and the eigenvalue pair and the two outer columns of V
// are exchanged by one flag (Eigen's swap(k, l)).  An array indexed by i0 or by k / l stays in registers on gfx950 but costs a
// compare-and-select chain over all of its elements for every read (16 v_cndmask_b32 a double out of nine).
// tests/test_eig3_direct_forms.py holds this form bit-equal to the indexed one on the host.
#pragma once
#include <cmath>

#include "glibc_math.hpp"

namespace gfs_eig3 {

struct Vec3 {
  double x, y, z;
};
// symmetric 3x3: column 0 = (d0, a, b), column 1 = (a, d1, c), column 2 = (b, c, d2)
struct Sym3 {
  double d0, a, b, d1, c, d2;
};

GFS_HD Vec3 cross3(const Vec3& a, const Vec3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
GFS_HD double sqn3(const Vec3& a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
GFS_HD double pick3(int i, double v0, double v1, double v2) { return i == 0 ? v0 : (i == 1 ? v1 : v2); }
GFS_HD Vec3 pick(bool first, const Vec3& a, const Vec3& b) { return {first ? a.x : b.x, first ? a.y : b.y, first ? a.z : b.z}; }

// Eigen's extract_kernel: rep = the column i0 of the largest absolute diagonal entry (strict >, so the first of equal ones);
// res = the larger of rep x column (i0 + 1) % 3 and rep x column (i0 + 2) % 3, normalised (strict >: the second of equal ones)
GFS_HD void extract_kernel(const Sym3& m, Vec3* res, Vec3* rep) {
  int i0 = 0;
  double best = fabs(m.d0);
  if (fabs(m.d1) > best) {
    best = fabs(m.d1);
    i0 = 1;
  }
  if (fabs(m.d2) > best) i0 = 2;
  // columns i0, i0 + 1, i0 + 2 (mod 3), row by row
  const Vec3 r = {pick3(i0, m.d0, m.a, m.b), pick3(i0, m.a, m.d1, m.c), pick3(i0, m.b, m.c, m.d2)};
  const Vec3 u = {pick3(i0, m.a, m.b, m.d0), pick3(i0, m.d1, m.c, m.a), pick3(i0, m.c, m.d2, m.b)};
  const Vec3 v = {pick3(i0, m.b, m.d0, m.a), pick3(i0, m.c, m.a, m.d1), pick3(i0, m.d2, m.b, m.c)};
  *rep = r;
  const Vec3 c0 = cross3(r, u), c1 = cross3(r, v);
  const double n0 = sqn3(c0), n1 = sqn3(c1);
  const bool first = n0 > n1;
  const Vec3 c = pick(first, c0, c1);
  const double d = sqrt(first ? n0 : n1);
  *res = {c.x / d, c.y / d, c.z / d};
}

// cov6: the lower triangle (xx, xy, xz, yy, yz, zz).  V column-major 3x3 (columns = eigenvectors, ascending eigenvalues).
GFS_HD void eig3_direct(const double* cov6, double* V) {
  const double shift = (cov6[0] + cov6[3] + cov6[5]) / 3.0;
  Sym3 s = {cov6[0] - shift, cov6[1], cov6[2], cov6[3] - shift, cov6[4], cov6[5] - shift};
  // the largest absolute entry of the nine; the three mirrored ones are the maximum of what is already in
  double scale = 0;
  scale = fmax(scale, fabs(s.d0));
  scale = fmax(scale, fabs(s.a));
  scale = fmax(scale, fabs(s.b));
  scale = fmax(scale, fabs(s.d1));
  scale = fmax(scale, fabs(s.c));
  scale = fmax(scale, fabs(s.d2));
  if (scale > 0) {
    s.d0 /= scale;
    s.a /= scale;
    s.b /= scale;
    s.d1 /= scale;
    s.c /= scale;
    s.d2 /= scale;
  }
  double ev0, ev1, ev2;
  {
    const double s_inv3 = 1.0 / 3.0, s_sqrt3 = sqrt(3.0);
    const double c0 = s.d0 * s.d1 * s.d2 + 2.0 * s.a * s.b * s.c - s.d0 * s.c * s.c - s.d1 * s.b * s.b - s.d2 * s.a * s.a;
    const double c1 = s.d0 * s.d1 - s.a * s.a + s.d0 * s.d2 - s.b * s.b + s.d1 * s.d2 - s.c * s.c;
    const double c2 = s.d0 + s.d1 + s.d2;
    const double c2_over_3 = c2 * s_inv3;
    double a_over_3 = (c2 * c2_over_3 - c1) * s_inv3;
    a_over_3 = fmax(a_over_3, 0.0);
    const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
    double q = a_over_3 * a_over_3 * a_over_3 - half_b * half_b;
    q = fmax(q, 0.0);
    const double rho = sqrt(a_over_3);
    const double theta = atan2(sqrt(q), half_b) * s_inv3;
    const double cos_theta = gfs_glibc::cos(theta), sin_theta = gfs_glibc::sin(theta);
    ev0 = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    ev1 = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    ev2 = c2_over_3 + 2.0 * rho * cos_theta;
  }
  const double eps = 2.220446049250313e-16;
  if ((ev2 - ev0) <= eps) {
    V[0] = 1.0, V[1] = 0.0, V[2] = 0.0;
    V[3] = 0.0, V[4] = 1.0, V[5] = 0.0;
    V[6] = 0.0, V[7] = 0.0, V[8] = 1.0;
    return;
  }
  double d0 = ev2 - ev1;
  const double d1 = ev1 - ev0;
  const bool sw = d0 > d1;  // Eigen: swap(k, l); d0 = d1  (k = 0, l = 2 before)
  if (sw) d0 = d1;
  const double evk = sw ? ev2 : ev0, evl = sw ? ev0 : ev2;
  Sym3 tmp = s;
  tmp.d0 -= evk;
  tmp.d1 -= evk;
  tmp.d2 -= evk;
  Vec3 colk, coll;
  extract_kernel(tmp, &colk, &coll);
  if (d0 <= 2 * eps * d1) {
    const double dot = colk.x * coll.x + colk.y * coll.y + colk.z * coll.z;
    coll.x -= dot * coll.x;
    coll.y -= dot * coll.y;
    coll.z -= dot * coll.z;
    const double nn = sqrt(sqn3(coll));
    coll.x /= nn;
    coll.y /= nn;
    coll.z /= nn;
  } else {
    tmp = s;
    tmp.d0 -= evl;
    tmp.d1 -= evl;
    tmp.d2 -= evl;
    Vec3 dummy;
    extract_kernel(tmp, &coll, &dummy);
  }
  const Vec3 v0 = pick(sw, coll, colk), v2 = pick(sw, colk, coll);  // columns k and l
  const Vec3 c1v = cross3(v2, v0);
  const double nn = sqrt(sqn3(c1v));
  V[0] = v0.x, V[1] = v0.y, V[2] = v0.z;
  V[3] = c1v.x / nn, V[4] = c1v.y / nn, V[5] = c1v.z / nn;
  V[6] = v2.x, V[7] = v2.y, V[8] = v2.z;
}

}  // namespace gfs_eig3
