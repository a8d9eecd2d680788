// Sim3Solver (reference src/Sim3Solver.cc) on MI355X: the RANSAC step of LoopClosing::DetectCommonRegionsFromBoW
// (src/LoopClosing.cc:742-759), between SearchByBoW (bow_search.hip) and the first Sim3 projection search (sim3_search.hip).
//
// The reference runs its hypotheses one after another and stops at the first that converges.  Given the draws, the hypotheses
// are independent, so every one of them is scored at once and the sequential outcome is a pick over the scores
// (sim3_ransac_rule.hpp states the rule and the derivation of the pick).
//   k_sim3_ransac_score  grid (ceil(H / 4), B), 256 threads.  The workgroup stages its problem's points, their own projections and
//                        thresholds in LDS (problems of up to kLdsPairs pairs; beyond that the walk reads the global arrays and
//                        recomputes the own projections).  One lane per hypothesis resolves the draws and runs ComputeSim3 -- the
//                        double Jacobi of the group's hypotheses side by side in one wave -- and parks the hypothesis in LDS.  Then a wave
//                        per hypothesis (4 waves, one hypothesis each) walks the pairs in chunks of 64: both projections and both tests
//                        per lane, counted by ballot + popcount.  Counts and hypotheses go to global memory.
//   k_sim3_ransac_pick   one workgroup per problem: a min-reduction for the first converging index, a (count, index) max-reduction
//                        for the last of the maxima, the picked hypothesis rescored for its mask, the solution record.
// No atomics; a problem's result does not depend on what else is in the call.  4 hypotheses a workgroup, 75 workgroups for 300: the
// ComputeSim3 phase costs the same for 1 or 64 active lanes, so fewer hypotheses a workgroup only shorten the walk behind it, at the
// price of staging the points in more workgroups, which is a few KB each.  Measured: 36 / 38 / 40 / 45 / 53 us a call for 4 / 8 / 16 /
// 32 / 64 a workgroup.
#include <memory>
#include <mutex>

#include "gfs_common.hpp"
#include "sim3_ransac_rule.hpp"
#include "staging.hpp"

using gfs_s3r::Hyp;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
#ifndef GFS_SIM3_RANSAC_HYPS_PER_GROUP
#define GFS_SIM3_RANSAC_HYPS_PER_GROUP 4  // one a wave (builds with 4 .. 64 are how the choice was measured: DESIGN.md section 23)
#endif
constexpr int kHypsPerGroup = GFS_SIM3_RANSAC_HYPS_PER_GROUP, kHypsPerWave = kHypsPerGroup / kWaves;
constexpr int kLdsPairs = 1024;  // 12 floats a pair: 48 KB of LDS
static_assert(kHypsPerGroup <= 64 && kHypsPerGroup % kWaves == 0, "one wave solves the group's hypotheses");

struct RansacHead {
  float cam1[4], cam2[4];
  int n, H, fix_scale, min_inliers;  // H == 0: nothing is iterated (GFS_SIM3_RANSAC_TOO_FEW)
};
struct RansacOut {
  float T12[16], R12[9], t12[3], s12;
  int n_inliers, iterations, status;
};

// The pairs of one problem as the walk reads them: from LDS (own projections staged) or from global memory (recomputed)
struct PairSource {
  const float *X1, *X2, *max1, *max2, *p1, *p2;  // p1 / p2 NULL: recompute
};

__device__ __forceinline__ bool pair_inlier(const PairSource& S, const Hyp& h, const float* cam1, const float* cam2, int i) {
  const float X1[3] = {S.X1[3 * i], S.X1[3 * i + 1], S.X1[3 * i + 2]};
  const float X2[3] = {S.X2[3 * i], S.X2[3 * i + 1], S.X2[3 * i + 2]};
  float p1[2], p2[2];
  if (S.p1) {
    p1[0] = S.p1[2 * i], p1[1] = S.p1[2 * i + 1];
    p2[0] = S.p2[2 * i], p2[1] = S.p2[2 * i + 1];
  } else {  // FromCameraToImage (:113-114)
    gfs_s3r::project(cam1, X1, p1);
    gfs_s3r::project(cam2, X2, p2);
  }
  float e1, e2;
  return gfs_s3r::pair_errors(h, cam1, cam2, X1, X2, p1, p2, S.max1[i], S.max2[i], &e1, &e2);
}

// S: pairs per problem, HS: hypotheses per problem (the strides of this call)
__global__ __launch_bounds__(kThreads) void k_sim3_ransac_score(const RansacHead* __restrict__ heads, const float* __restrict__ X1_all,
                                                                const float* __restrict__ X2_all, const float* __restrict__ max1_all,
                                                                const float* __restrict__ max2_all, const int* __restrict__ draws_all, int S,
                                                                int HS, Hyp* __restrict__ hyps_all, int* __restrict__ counts_all) {
  __shared__ float s_X1[3 * kLdsPairs], s_X2[3 * kLdsPairs], s_p1[2 * kLdsPairs], s_p2[2 * kLdsPairs], s_max1[kLdsPairs], s_max2[kLdsPairs];
  __shared__ Hyp s_hyp[kHypsPerGroup];
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RansacHead& F = heads[f];
  const int n = F.n, H = F.H;
  const int h0 = blockIdx.x * kHypsPerGroup;
  if (h0 >= H) return;  // (uniform)
  const float* X1 = X1_all + (size_t)f * S * 3;
  const float* X2 = X2_all + (size_t)f * S * 3;
  const float* max1 = max1_all + (size_t)f * S;
  const float* max2 = max2_all + (size_t)f * S;
  float cam1[4], cam2[4];
  for (int k = 0; k < 4; k++) cam1[k] = F.cam1[k], cam2[k] = F.cam2[k];
  const bool staged = n <= kLdsPairs;
  if (staged) {
    for (int i = tid; i < n; i += kThreads) {
      const float a[3] = {X1[3 * i], X1[3 * i + 1], X1[3 * i + 2]}, b[3] = {X2[3 * i], X2[3 * i + 1], X2[3 * i + 2]};
      float pa[2], pb[2];
      gfs_s3r::project(cam1, a, pa);
      gfs_s3r::project(cam2, b, pb);
      for (int k = 0; k < 3; k++) s_X1[3 * i + k] = a[k], s_X2[3 * i + k] = b[k];
      for (int k = 0; k < 2; k++) s_p1[2 * i + k] = pa[k], s_p2[2 * i + k] = pb[k];
      s_max1[i] = max1[i];
      s_max2[i] = max2[i];
    }
  }
  // one lane per hypothesis: the draws (checked by the host: every index is inside [0, n)) and ComputeSim3, from global memory
  if (tid < kHypsPerGroup && h0 + tid < H) {
    const int* d = draws_all + ((size_t)f * HS + h0 + tid) * 3;
    int idx[3];
    gfs_s3r::resolve_draws(n, d[0], d[1], d[2], idx);
    float P1[3][3], P2[3][3];
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) {
        P1[c][r] = X1[3 * idx[c] + r];
        P2[c][r] = X2[3 * idx[c] + r];
      }
    Hyp h;
    gfs_s3r::compute_sim3(P1, P2, F.fix_scale != 0, h);
    s_hyp[tid] = h;
    hyps_all[(size_t)f * HS + h0 + tid] = h;
  }
  __syncthreads();
  const PairSource src = staged ? PairSource{s_X1, s_X2, s_max1, s_max2, s_p1, s_p2} : PairSource{X1, X2, max1, max2, nullptr, nullptr};
  for (int k = 0; k < kHypsPerWave; k++) {
    const int slot = wave * kHypsPerWave + k;
    if (h0 + slot >= H) break;  // (uniform in the wave)
    const Hyp h = s_hyp[slot];
    int count = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool in = i < n && pair_inlier(src, h, cam1, cam2, i);
      count += __popcll(__ballot(in));
    }
    if (lane == 0) counts_all[(size_t)f * HS + h0 + slot] = count;
  }
}

__global__ __launch_bounds__(kThreads) void k_sim3_ransac_pick(const RansacHead* __restrict__ heads, const float* __restrict__ X1_all,
                                                               const float* __restrict__ X2_all, const float* __restrict__ max1_all,
                                                               const float* __restrict__ max2_all, int S, int HS,
                                                               const Hyp* __restrict__ hyps_all, const int* __restrict__ counts_all,
                                                               uint8_t* __restrict__ mask_all, RansacOut* __restrict__ outs) {
  __shared__ int s_first[kWaves];
  __shared__ long long s_best[kWaves];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RansacHead& F = heads[f];
  const int n = F.n, H = F.H;
  uint8_t* mask = mask_all + (size_t)f * S;
  if (H == 0) {  // (uniform) bNoMore at once: Identity, no inlier
    for (int i = tid; i < n; i += kThreads) mask[i] = 0;
    if (tid == 0) {
      RansacOut O;
      for (int k = 0; k < 16; k++) O.T12[k] = (k % 5 == 0) ? 1.0f : 0.0f;
      for (int k = 0; k < 9; k++) O.R12[k] = (k % 4 == 0) ? 1.0f : 0.0f;
      O.t12[0] = O.t12[1] = O.t12[2] = 0.0f;
      O.s12 = 1.0f;
      O.n_inliers = O.iterations = 0;
      O.status = gfs_s3r::kTooFew;
      outs[f] = O;
    }
    return;
  }
  const int* counts = counts_all + (size_t)f * HS;
  // gfs_s3r::pick as two reductions: the first index with c > min_inliers; the largest (c, index), which is the last of the maxima
  int first = 0x7fffffff;
  long long best = -1;
  for (int h = tid; h < H; h += kThreads) {
    const int c = counts[h];
    if (c > F.min_inliers) first = min(first, h);
    best = max(best, ((long long)c << 32) | (long long)h);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    first = min(first, __shfl_xor(first, o, 64));
    best = max(best, __shfl_xor(best, o, 64));
  }
  if (lane == 0) s_first[wave] = first, s_best[wave] = best;
  __syncthreads();
  for (int w = 0; w < kWaves; w++) first = min(first, s_first[w]), best = max(best, s_best[w]);
  const bool converged = first != 0x7fffffff;
  const int picked = converged ? first : (int)(best & 0xffffffffLL);
  const Hyp h = hyps_all[(size_t)f * HS + picked];
  float cam1[4], cam2[4];
  for (int k = 0; k < 4; k++) cam1[k] = F.cam1[k], cam2[k] = F.cam2[k];
  const PairSource src{X1_all + (size_t)f * S * 3, X2_all + (size_t)f * S * 3, max1_all + (size_t)f * S, max2_all + (size_t)f * S, nullptr, nullptr};
  for (int i = tid; i < n; i += kThreads) mask[i] = pair_inlier(src, h, cam1, cam2, i) ? 1 : 0;
  if (tid == 0) {
    RansacOut O;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) O.T12[4 * r + c] = h.T12[4 * r + c];
    O.T12[12] = O.T12[13] = O.T12[14] = 0.0f;
    O.T12[15] = 1.0f;
    for (int k = 0; k < 9; k++) O.R12[k] = h.R[k];
    for (int k = 0; k < 3; k++) O.t12[k] = h.t[k];
    O.s12 = h.s;
    O.n_inliers = counts[picked];
    O.iterations = converged ? picked + 1 : H;
    O.status = converged ? gfs_s3r::kConverged : gfs_s3r::kNoMore;
    outs[f] = O;
  }
}

}  // namespace

struct gfs_sim3_ransac {
  int device, max_batch, max_pairs, max_iterations;
  hipStream_t stream;
  std::mutex mu;
  // one pinned block mirroring one device block for the inputs, one for the outputs: a call is one copy in, two kernels, one copy out
  struct Layout {  // S: pairs per problem, HS: hypotheses per problem
    gfs::Block<256> in, res;
    gfs::Field<RansacHead> heads;
    gfs::Field<float, 3> X1, X2;
    gfs::Field<float> max1, max2;
    gfs::Field<int, 3> draws;
    gfs::Field<RansacOut> out;
    gfs::Field<int> counts;
    gfs::Field<uint8_t> mask;
    Layout(size_t B, size_t S, size_t HS)
        : heads(in, B), X1(in, B * S), X2(in, B * S), max1(in, B * S), max2(in, B * S), draws(in, B * HS), out(res, B), counts(res, B * HS),
          mask(res, B * S) {}
  };
  gfs::Mirror in, res;
  gfs::DevBuf<Hyp> d_hyps;
};

extern "C" {

int gfs_sim3_ransac_iterations(int n_pairs, double probability, int min_inliers, int max_iterations) {
  return gfs_s3r::ransac_iterations(n_pairs, probability, min_inliers, max_iterations);
}

int gfs_sim3_ransac_create(int device, int max_batch, int max_pairs, int max_iterations, gfs_sim3_ransac** out) {
  GFS_REQUIRE(out && max_batch > 0 && max_pairs > 0 && max_iterations > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_ransac_create: invalid argument");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_sim3_ransac> h(new gfs_sim3_ransac);
  h->device = device;
  h->max_batch = max_batch;
  h->max_pairs = max_pairs;
  h->max_iterations = max_iterations;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t Smax = gfs::align_up((size_t)max_pairs, 64), Hmax = gfs::align_up((size_t)max_iterations, kHypsPerGroup);
  const gfs_sim3_ransac::Layout L{(size_t)max_batch, Smax, Hmax};
  int rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->res.alloc(L.res.bytes());
  if (!rc) rc = h->d_hyps.alloc(Hmax * max_batch);
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_sim3_ransac_destroy(gfs_sim3_ransac* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_sim3_ransac_solve(gfs_sim3_ransac* h, const gfs_sim3_ransac_problem* problems, int B, gfs_sim3_ransac_solution* solutions) {
  GFS_REQUIRE(h && problems && solutions && B > 0, GFS_ERR_INVALID_ARG, "gfs_sim3_ransac_solve: invalid argument");
  GFS_REQUIRE(B <= h->max_batch, GFS_ERR_CAPACITY, "gfs_sim3_ransac_solve: batch %d exceeds capacity %d", B, h->max_batch);
  // every refusal before anything is staged
  int S = 64, HS = kHypsPerGroup;  // strides of the per-problem arrays in this call
  for (int f = 0; f < B; f++) {
    const gfs_sim3_ransac_problem& p = problems[f];
    GFS_REQUIRE(p.n_pairs >= 0, GFS_ERR_INVALID_ARG, "gfs_sim3_ransac_solve: problem %d has n_pairs = %d", f, p.n_pairs);
    GFS_REQUIRE(p.n_pairs <= h->max_pairs, GFS_ERR_CAPACITY, "gfs_sim3_ransac_solve: problem %d has %d pairs (capacity %d)", f, p.n_pairs,
                h->max_pairs);
    GFS_REQUIRE(p.n_pairs == 0 || (p.x3d_c1 && p.x3d_c2 && p.max_err1 && p.max_err2 && solutions[f].inlier), GFS_ERR_INVALID_ARG,
                "gfs_sim3_ransac_solve: problem %d has NULL pair arrays", f);
    S = std::max(S, (int)gfs::align_up((size_t)p.n_pairs, 64));
    if (p.n_pairs < p.min_inliers || p.n_pairs < 3) continue;  // nothing is iterated: the draws are not read
    GFS_REQUIRE(p.n_iterations >= 1, GFS_ERR_INVALID_ARG, "gfs_sim3_ransac_solve: problem %d has n_iterations = %d", f, p.n_iterations);
    GFS_REQUIRE(p.n_iterations <= h->max_iterations, GFS_ERR_CAPACITY, "gfs_sim3_ransac_solve: problem %d has %d iterations (capacity %d)", f,
                p.n_iterations, h->max_iterations);
    GFS_REQUIRE(p.draws, GFS_ERR_INVALID_ARG, "gfs_sim3_ransac_solve: problem %d has NULL draws", f);
    for (int i = 0; i < p.n_iterations; i++)
      GFS_REQUIRE(gfs_s3r::draws_in_range(p.n_pairs, p.draws[3 * i], p.draws[3 * i + 1], p.draws[3 * i + 2]), GFS_ERR_INVALID_ARG,
                  "gfs_sim3_ransac_solve: problem %d, iteration %d: draw (%d, %d, %d) outside [0, N-1], [0, N-2], [0, N-3] with N = %d", f, i,
                  p.draws[3 * i], p.draws[3 * i + 1], p.draws[3 * i + 2], p.n_pairs);
    HS = std::max(HS, (int)gfs::align_up((size_t)p.n_iterations, kHypsPerGroup));
  }
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs_sim3_ransac::Layout L{(size_t)B, (size_t)S, (size_t)HS};
  uint8_t* hi = h->in.h.p;
  int Hcall = 0;
  for (int f = 0; f < B; f++) {
    const gfs_sim3_ransac_problem& p = problems[f];
    RansacHead& F = L.heads.at(hi)[f];
    const float cam1[4] = {p.fx1, p.fy1, p.cx1, p.cy1}, cam2[4] = {p.fx2, p.fy2, p.cx2, p.cy2};
    for (int k = 0; k < 4; k++) F.cam1[k] = cam1[k], F.cam2[k] = cam2[k];
    F.n = p.n_pairs;
    F.H = (p.n_pairs < p.min_inliers || p.n_pairs < 3) ? 0 : p.n_iterations;
    F.fix_scale = p.fix_scale != 0;
    F.min_inliers = p.min_inliers;
    const size_t n = (size_t)p.n_pairs;
    L.X1.put(hi, (size_t)f * S, p.x3d_c1, n);
    L.X2.put(hi, (size_t)f * S, p.x3d_c2, n);
    L.max1.put(hi, (size_t)f * S, p.max_err1, n);
    L.max2.put(hi, (size_t)f * S, p.max_err2, n);
    L.draws.put(hi, (size_t)f * HS, p.draws, (size_t)F.H);
    Hcall = std::max(Hcall, F.H);
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.in.bytes())) return rc;
  const uint8_t* di = h->in.d.p;
  uint8_t* dr = h->res.d.p;
  if (Hcall > 0)
    GFS_LAUNCH("k_sim3_ransac_score", k_sim3_ransac_score, dim3(gfs::div_up(Hcall, kHypsPerGroup), B), dim3(kThreads), 0, s, L.heads.at(di),
               L.X1.at(di), L.X2.at(di), L.max1.at(di), L.max2.at(di), L.draws.at(di), S, HS, h->d_hyps.p, L.counts.at(dr));
  GFS_LAUNCH("k_sim3_ransac_pick", k_sim3_ransac_pick, dim3(B), dim3(kThreads), 0, s, L.heads.at(di), L.X1.at(di), L.X2.at(di), L.max1.at(di),
             L.max2.at(di), S, HS, h->d_hyps.p, L.counts.at(dr), L.mask.at(dr), L.out.at(dr));
  if (int rc = h->res.download(s, 0, L.res.bytes())) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* hr = h->res.h.p;
  for (int f = 0; f < B; f++) {
    const RansacOut& O = L.out.at(hr)[f];
    gfs_sim3_ransac_solution& r = solutions[f];
    const int H = L.heads.at(hi)[f].H;
    memcpy(r.T12, O.T12, sizeof(r.T12));
    memcpy(r.R12, O.R12, sizeof(r.R12));
    memcpy(r.t12, O.t12, sizeof(r.t12));
    r.s12 = O.s12;
    r.n_inliers = O.n_inliers;
    r.iterations = O.iterations;
    r.status = O.status;
    L.mask.get(r.inlier, hr, (size_t)f * S, (size_t)problems[f].n_pairs);
    if (r.counts) L.counts.get(r.counts, hr, (size_t)f * HS, (size_t)H);
  }
  return GFS_OK;
}

}  // extern "C"
