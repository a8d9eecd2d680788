// Sequential CPU restatement of Sim3Solver::iterate (reference src/Sim3Solver.cc:207-275) on the flat problem of include/gfs_abi.h:
// one hypothesis after another, the reference's own bookkeeping (mnBestInliers, the >= update, the > minInliers return), with the
// arithmetic of geoflowslam_amd/csrc/sim3_ransac_rule.hpp.  It does NOT use the rule's pick(): the loop below is written the way the
// reference writes it, so that the device's pick over all scores is checked against the loop it stands for.  Traces: the count of
// every hypothesis that ran, and both errors of every pair under the returned hypothesis.
// Built by tests/sim3_ransac_support.py with g++ -ffp-contract=off.
#include <cstring>
#include <vector>

#include "../../include/gfs_abi.h"
#include "../../geoflowslam_amd/csrc/sim3_ransac_rule.hpp"

namespace s3rr {

struct Scored {
  gfs_s3r::Hyp h;
  int count;
};

// ComputeSim3 + CheckInliers of iteration `it`; mask / err1 / err2 may be NULL
inline Scored hypothesis(const gfs_sim3_ransac_problem& p, int it, const float* p1im1, const float* p2im2, uint8_t* mask, float* err1,
                         float* err2) {
  const int N = p.n_pairs;
  // vAvailableIndices = mvAllIndices and the three draws, with the list the reference keeps
  std::vector<int> avail(N);
  for (int i = 0; i < N; i++) avail[i] = i;
  float P1[3][3], P2[3][3];
  for (int k = 0; k < 3; k++) {
    const int randi = p.draws[3 * it + k];
    const int idx = avail[randi];
    for (int r = 0; r < 3; r++) {
      P1[k][r] = p.x3d_c1[3 * idx + r];
      P2[k][r] = p.x3d_c2[3 * idx + r];
    }
    avail[randi] = avail.back();
    avail.pop_back();
  }
  Scored s;
  gfs_s3r::compute_sim3(P1, P2, p.fix_scale != 0, s.h);
  const float cam1[4] = {p.fx1, p.fy1, p.cx1, p.cy1}, cam2[4] = {p.fx2, p.fy2, p.cx2, p.cy2};
  s.count = 0;
  for (int i = 0; i < N; i++) {
    float e1, e2;
    const bool in = gfs_s3r::pair_errors(s.h, cam1, cam2, p.x3d_c1 + 3 * i, p.x3d_c2 + 3 * i, p1im1 + 2 * i, p2im2 + 2 * i, p.max_err1[i],
                                         p.max_err2[i], &e1, &e2);
    if (mask) mask[i] = in;
    if (err1) err1[i] = e1;
    if (err2) err2[i] = e2;
    s.count += in;
  }
  return s;
}

inline void write_best(const gfs_s3r::Hyp& h, gfs_sim3_ransac_solution& s) {
  std::memset(s.T12, 0, sizeof(s.T12));
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) s.T12[4 * r + c] = h.T12[4 * r + c];
  s.T12[15] = 1.0f;
  std::memcpy(s.R12, h.R, sizeof(s.R12));
  std::memcpy(s.t12, h.t, sizeof(s.t12));
  s.s12 = h.s;
}

}  // namespace s3rr

extern "C" {

// early_stop != 0: the reference's loop.  early_stop == 0: the same loop with its return taken out, so that every hypothesis is
// scored (s.counts, when given, then holds all n_iterations counts; with the early stop the entries behind the last iteration that
// ran are left as they were).  err1 / err2 [N] (may be NULL): the errors of every pair under the returned hypothesis.
int s3rr_solve(const gfs_sim3_ransac_problem* pp, int early_stop, gfs_sim3_ransac_solution* sp, float* err1, float* err2) {
  const gfs_sim3_ransac_problem& p = *pp;
  gfs_sim3_ransac_solution& s = *sp;
  const int N = p.n_pairs;
  for (int i = 0; i < N; i++) s.inlier[i] = 0;
  s.n_inliers = 0;
  if (N < p.min_inliers || N < 3) {  // :215-218 (and N < 3, where the reference would index out of range)
    std::memset(s.T12, 0, sizeof(s.T12));
    std::memset(s.R12, 0, sizeof(s.R12));
    s.T12[0] = s.T12[5] = s.T12[10] = s.T12[15] = 1.0f;
    s.R12[0] = s.R12[4] = s.R12[8] = 1.0f;
    s.t12[0] = s.t12[1] = s.t12[2] = 0.0f;
    s.s12 = 1.0f;
    s.iterations = 0;
    s.status = GFS_SIM3_RANSAC_TOO_FEW;
    return 0;
  }
  // FromCameraToImage (:113-114)
  std::vector<float> p1im1(2 * N), p2im2(2 * N);
  const float cam1[4] = {p.fx1, p.fy1, p.cx1, p.cy1}, cam2[4] = {p.fx2, p.fy2, p.cx2, p.cy2};
  for (int i = 0; i < N; i++) {
    gfs_s3r::project(cam1, p.x3d_c1 + 3 * i, &p1im1[2 * i]);
    gfs_s3r::project(cam2, p.x3d_c2 + 3 * i, &p2im2[2 * i]);
  }
  int mnIterations = 0, mnBestInliers = 0, best_it = -1;
  std::vector<uint8_t> mvbInliersi(N);
  bool bConverge = false;
  while (mnIterations < p.n_iterations) {
    const int it = mnIterations++;
    const s3rr::Scored sc = s3rr::hypothesis(p, it, p1im1.data(), p2im2.data(), mvbInliersi.data(), nullptr, nullptr);
    if (s.counts) s.counts[it] = sc.count;
    if (bConverge) continue;  // (only without the early stop: the result stays the converged one)
    if (sc.count >= mnBestInliers) {
      mnBestInliers = sc.count;
      best_it = it;
      s3rr::write_best(sc.h, s);
      std::memcpy(s.inlier, mvbInliersi.data(), N);
      s.n_inliers = sc.count;
      if (sc.count > p.min_inliers) {
        bConverge = true;
        s.iterations = mnIterations;
        if (early_stop) break;
      }
    }
  }
  if (!bConverge) s.iterations = mnIterations;
  s.status = bConverge ? GFS_SIM3_RANSAC_CONVERGED : GFS_SIM3_RANSAC_NO_MORE;
  if (err1 || err2) s3rr::hypothesis(p, best_it, p1im1.data(), p2im2.data(), nullptr, err1, err2);
  return 0;
}

int s3rr_solve_batch(const gfs_sim3_ransac_problem* p, int B, gfs_sim3_ransac_solution* s) {
  for (int f = 0; f < B; f++) s3rr_solve(p + f, 1, s + f, nullptr, nullptr);
  return 0;
}

// ComputeSim3 alone on two triples (P1 / P2 [3][3]: point k at 3 k) -> R [9], t [3], s [1], T12 [12], T21 [12]
void s3rr_compute_sim3(const float* P1, const float* P2, int fix_scale, float* R, float* t, float* s, float* T12, float* T21) {
  float A[3][3], B[3][3];
  std::memcpy(A, P1, sizeof(A));
  std::memcpy(B, P2, sizeof(B));
  gfs_s3r::Hyp h;
  gfs_s3r::compute_sim3(A, B, fix_scale != 0, h);
  std::memcpy(R, h.R, sizeof(h.R));
  std::memcpy(t, h.t, sizeof(h.t));
  *s = h.s;
  std::memcpy(T12, h.T12, sizeof(h.T12));
  std::memcpy(T21, h.T21, sizeof(h.T21));
}

void s3rr_resolve_draws(int N, const int32_t* r, int32_t* idx) {
  int out[3];
  gfs_s3r::resolve_draws(N, r[0], r[1], r[2], out);
  for (int k = 0; k < 3; k++) idx[k] = out[k];
}

void s3rr_pick(const int32_t* counts, int H, int min_inliers, int32_t* out3) {
  const gfs_s3r::Pick pk = gfs_s3r::pick(counts, H, min_inliers);
  out3[0] = pk.index, out3[1] = pk.iterations, out3[2] = pk.status;
}

int s3rr_iterations(int N, double probability, int min_inliers, int max_iterations) {
  return gfs_s3r::ransac_iterations(N, probability, min_inliers, max_iterations);
}

// what the rule compiles in: 9.210, the defaults of SetRansacParameters, the Jacobi's sweeps and threshold
void s3rr_constants(double* out) {
  out[0] = gfs_s3r::kChi2;
  out[1] = gfs_s3r::kDefaultProbability;
  out[2] = gfs_s3r::kDefaultMinInliers;
  out[3] = gfs_s3r::kDefaultMaxIterations;
  out[4] = gfs_s3r::kJacobiSweeps;
  out[5] = gfs_s3r::kJacobiEps;
}

}  // extern "C"
