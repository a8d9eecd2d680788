// MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:376-448, :468-532) for any
// number of map points in one call: gfs_map_points_create / _destroy / _update (include/gfs_abi.h section 7b).
// The rule is map_point_rule.hpp, shared with the host.
//
// One launch of k_map_points, a wave per point, four points a workgroup; the points are independent, so there is nothing between
// workgroups and nothing between the waves of one.
//   normal   the wave walks the point's observations 64 at a time: a lane computes the term (Pos - Ow) / |Pos - Ow| of its
//            observation; the sum is then taken in list order over the flagged lanes, one v_readlane per component and term (every
//            lane runs the same serial sum, lane 0 stores it): a tree would change the bits.
//   median   staging has compacted the point's IN_DESC observations.  At most 64 of them: lane j keeps descriptor j in 8 registers,
//            row i is broadcast with v_readlane, each lane computes d(i, j), and the row's k-th smallest value is the least v with
//            popcount(ballot(d <= v)) > k, found by bisection over 0..256: no sort.  More than 64: the row's distances go into a
//            257-bin histogram of the wave in LDS, 64 columns at a time, and the k-th smallest value is read off its prefix sums.
//            Both count the same integers, so they agree.  Rows ascend and a row replaces the best only with a smaller median.
// No global atomics, no library primitives.
#include <memory>

#include "block_layouts.hpp"
#include "gfs_common.hpp"
#include "map_point_rule.hpp"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kHistSlots = 320;  // the 257 bins of the distances 0..256, rounded up to 5 a lane

static_assert(gfs_mp::kObsInNormal == GFS_MAP_POINT_OBS_IN_NORMAL && gfs_mp::kObsInDesc == GFS_MAP_POINT_OBS_IN_DESC &&
                  gfs_mp::kNormalSet == GFS_MAP_POINT_NORMAL_SET && gfs_mp::kDescSet == GFS_MAP_POINT_DESC_SET, "the rule's bits are the ABI's");

struct MpArgs {  // device pointers into the handle's two blocks
  int n_points, with_desc;
  const int* obs_start;   // [n_points + 1]
  const int* dsc_start;   // [n_points + 1] into dsc_words / dsc_obs (with_desc only)
  const float* obs_Ow;    // [n_obs][3]
  const uint8_t* obs_flags;
  const uint32_t* dsc_words;  // [n_dsc][8] the IN_DESC observations' descriptors, compacted in list order
  const int* dsc_obs;     // [n_dsc] their indices in the point's own list
  const float* pos;       // [n_points][3]
  const float* ref_Ow;    // [n_points][3]
  const float* level_scale;
  const float* max_scale;
  int* best_obs;
  int* best_median;
  float* normal;  // [n_points][3]
  float* min_dist;
  float* max_dist;
  uint8_t* status;
};

#define MP_WAVE_SYNC()                                     \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

__device__ __forceinline__ float readlane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

__global__ __launch_bounds__(kThreads) void k_map_points(const MpArgs A) {
  __shared__ int s_hist[kWaves][kHistSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * kWaves + wave;
  if (p >= A.n_points) return;  // (wave-uniform; no workgroup barrier follows)
  const int o0 = A.obs_start[p], n_obs = A.obs_start[p + 1] - o0;
  if (n_obs <= 0) {  // observations.empty(): the point is not touched
    if (lane == 0) {
      A.best_obs[p] = -1;
      A.best_median[p] = -1;
      A.normal[3 * (size_t)p] = A.normal[3 * (size_t)p + 1] = A.normal[3 * (size_t)p + 2] = 0.0f;
      A.min_dist[p] = A.max_dist[p] = 0.0f;
      A.status[p] = 0;
    }
    return;
  }
  // ---- UpdateNormalAndDepth
  const float pos[3] = {A.pos[3 * (size_t)p], A.pos[3 * (size_t)p + 1], A.pos[3 * (size_t)p + 2]};
  float sum[3] = {0.0f, 0.0f, 0.0f};
  int cnt = 0;
  for (int c = 0; c < n_obs; c += 64) {
    const int i = c + lane;
    const bool in = i < n_obs && (A.obs_flags[o0 + i] & gfs_mp::kObsInNormal);
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (in) {
      const float* q = A.obs_Ow + 3 * (size_t)(o0 + i);
      const float Ow[3] = {q[0], q[1], q[2]};
      gfs_mp::normal_term(pos, Ow, t);
    }
    unsigned long long m = __ballot(in);
    cnt += __popcll(m);
    while (m) {  // list order: the lowest flagged lane first
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      sum[0] = sum[0] + readlane_f(t[0], b);
      sum[1] = sum[1] + readlane_f(t[1], b);
      sum[2] = sum[2] + readlane_f(t[2], b);
    }
  }
  if (lane == 0) {
    const float ref[3] = {A.ref_Ow[3 * (size_t)p], A.ref_Ow[3 * (size_t)p + 1], A.ref_Ow[3 * (size_t)p + 2]};
    float nrm[3], dmin, dmax;
    gfs_mp::finish_normal(sum, cnt, pos, ref, A.level_scale[p], A.max_scale[p], nrm, &dmin, &dmax);
    A.normal[3 * (size_t)p] = nrm[0];
    A.normal[3 * (size_t)p + 1] = nrm[1];
    A.normal[3 * (size_t)p + 2] = nrm[2];
    A.min_dist[p] = dmin;
    A.max_dist[p] = dmax;
  }
  // ---- ComputeDistinctiveDescriptors
  const int d0 = A.with_desc ? A.dsc_start[p] : 0, nd = A.with_desc ? A.dsc_start[p + 1] - d0 : 0;
  int best = 0x7fffffff, best_row = -1;
  if (nd > 0) {
    const int k = gfs_mp::median_index(nd);
    if (nd <= 64) {
      uint32_t w[8];
      {
        const uint4* q = reinterpret_cast<const uint4*>(A.dsc_words + 8 * (size_t)(d0 + (lane < nd ? lane : 0)));
        const uint4 a = q[0], b = q[1];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
      }
      for (int i = 0; i < nd; i++) {
        int d = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) d += __popc(w[q] ^ (uint32_t)__builtin_amdgcn_readlane((int)w[q], i));
        if (lane >= nd) d = 1 << 20;  // not a column
        int lo = 0, hi = 256;         // the least v with #(d <= v) > k
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (__popcll(__ballot(d <= mid)) > k) hi = mid; else lo = mid + 1;
        }
        if (gfs_mp::better_median(lo, best)) {
          best = lo;
          best_row = i;
        }
      }
    } else {
      int* hist = s_hist[wave];
      for (int i = 0; i < nd; i++) {
#pragma unroll
        for (int q = 0; q < kHistSlots / 64; q++) hist[lane + 64 * q] = 0;
        MP_WAVE_SYNC();
        const uint4* r = reinterpret_cast<const uint4*>(A.dsc_words + 8 * (size_t)(d0 + i));  // (wave-uniform address)
        const uint4 ra = r[0], rb = r[1];
        for (int c = 0; c < nd; c += 64) {
          const int j = c + lane;
          if (j < nd) {
            const uint4* q = reinterpret_cast<const uint4*>(A.dsc_words + 8 * (size_t)(d0 + j));
            const uint4 a = q[0], b = q[1];
            const int d = (__popc(a.x ^ ra.x) + __popc(a.y ^ ra.y) + __popc(a.z ^ ra.z) + __popc(a.w ^ ra.w)) +
                          (__popc(b.x ^ rb.x) + __popc(b.y ^ rb.y) + __popc(b.z ^ rb.z) + __popc(b.w ^ rb.w));
            atomicAdd(&hist[d], 1);  // LDS
          }
        }
        MP_WAVE_SYNC();
        // lane l owns bins 5 l .. 5 l + 4: the bin where the running count first exceeds k
        int mine[kHistSlots / 64], tot = 0;
#pragma unroll
        for (int q = 0; q < kHistSlots / 64; q++) {
          mine[q] = hist[(kHistSlots / 64) * lane + q];
          tot += mine[q];
        }
        int incl = tot;  // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(incl, o);
          if (lane >= o) incl += up;
        }
        const unsigned long long over = __ballot(incl > k);  // never empty: the last lane's prefix is nd > k
        const int owner = __ffsll((long long)over) - 1;
        int v = 0;
        if (lane == owner) {
          int run = incl - tot;
          v = (kHistSlots / 64) * lane;
#pragma unroll
          for (int q = 0; q < kHistSlots / 64; q++) {
            run += mine[q];
            if (run > k) break;
            v++;
          }
        }
        v = __builtin_amdgcn_readlane(v, owner);
        if (gfs_mp::better_median(v, best)) {
          best = v;
          best_row = i;
        }
        MP_WAVE_SYNC();  // the next row clears the bins
      }
    }
  }
  if (lane == 0) {
    A.best_obs[p] = best_row >= 0 ? A.dsc_obs[d0 + best_row] : -1;
    A.best_median[p] = best_row >= 0 ? best : -1;
    A.status[p] = (uint8_t)(gfs_mp::kNormalSet | (best_row >= 0 ? gfs_mp::kDescSet : 0));
  }
}

}  // namespace

// One pinned block and one device block for the inputs, one of each for the outputs, sized by the reserve; a call lays its arrays
// out for its own sizes, so that what travels is what the call holds.
struct gfs_map_points {
  int device, max_points, max_obs;
  hipStream_t stream;
  std::mutex mu;
  gfs::Mirror in, out;
};

extern "C" {

int gfs_map_points_create(int device, int max_points, int max_observations, gfs_map_points** out) {
  GFS_REQUIRE(out && max_points > 0 && max_observations > 0, GFS_ERR_INVALID_ARG, "gfs_map_points_create: invalid argument");
  GFS_REQUIRE((size_t)max_observations <= (size_t)1 << 26 && (size_t)max_points <= (size_t)1 << 26, GFS_ERR_UNSUPPORTED,
              "gfs_map_points_create: at most 2^26 points and observations");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  std::unique_ptr<gfs_map_points> h(new gfs_map_points);
  h->device = device;
  h->max_points = max_points;
  h->max_obs = max_observations;
  const gfs::MpLayout L{(size_t)max_points, (size_t)max_observations};
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  int rc = 0;
  if (!rc) rc = h->in.alloc(L.in.bytes());
  if (!rc) rc = h->out.alloc(L.out.bytes());
  if (rc) {
    (void)hipStreamDestroy(h->stream);
    return rc;
  }
  *out = h.release();
  return GFS_OK;
}

void gfs_map_points_destroy(gfs_map_points* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_map_points_update(gfs_map_points* h, const gfs_map_points_problem* pr, gfs_map_points_result* res) {
  GFS_REQUIRE(h && pr && res, GFS_ERR_INVALID_ARG, "gfs_map_points_update: invalid argument");
  GFS_REQUIRE(pr->mode == GFS_MAP_POINTS_FULL || pr->mode == GFS_MAP_POINTS_NORMALS_ONLY, GFS_ERR_INVALID_ARG,
              "gfs_map_points_update: unknown mode %d", pr->mode);
  GFS_REQUIRE(pr->n_points >= 0, GFS_ERR_INVALID_ARG, "gfs_map_points_update: negative n_points");
  GFS_REQUIRE(pr->n_points <= h->max_points, GFS_ERR_CAPACITY, "gfs_map_points_update: %d points exceed the reserve of %d", pr->n_points,
              h->max_points);
  const int P = pr->n_points;
  const bool with_desc = pr->mode == GFS_MAP_POINTS_FULL;
  GFS_REQUIRE(pr->obs_start, GFS_ERR_INVALID_ARG, "gfs_map_points_update: obs_start is NULL");
  GFS_REQUIRE(pr->obs_start[0] == 0, GFS_ERR_INVALID_ARG, "gfs_map_points_update: obs_start[0] is %d, not 0", pr->obs_start[0]);
  for (int p = 0; p < P; p++) {
    GFS_REQUIRE(pr->obs_start[p + 1] >= pr->obs_start[p], GFS_ERR_INVALID_ARG, "gfs_map_points_update: obs_start decreases at point %d", p);
    GFS_REQUIRE(pr->obs_start[p + 1] <= h->max_obs, GFS_ERR_CAPACITY, "gfs_map_points_update: more than the %d observations reserved",
                h->max_obs);
  }
  if (P == 0) return GFS_OK;
  const int O = pr->obs_start[P];
  GFS_REQUIRE(pr->pos && pr->ref_Ow && pr->level_scale && pr->max_scale, GFS_ERR_INVALID_ARG, "gfs_map_points_update: a NULL point array");
  GFS_REQUIRE(O == 0 || (pr->obs_Ow && pr->obs_flags && (pr->obs_desc || !with_desc)), GFS_ERR_INVALID_ARG,
              "gfs_map_points_update: a NULL observation array");
  GFS_REQUIRE(res->best_obs && res->best_median && res->normal && res->min_dist && res->max_dist && res->status, GFS_ERR_INVALID_ARG,
              "gfs_map_points_update: a NULL result array");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const gfs::MpLayout L{(size_t)P, (size_t)O};
  // ---- staging: one block; the IN_DESC descriptors are compacted per point, in list order
  uint8_t* in = h->in.h.p;
  L.obs_start.put(in, 0, pr->obs_start, (size_t)P + 1);
  L.pos.put(in, 0, pr->pos, (size_t)P);
  L.ref.put(in, 0, pr->ref_Ow, (size_t)P);
  L.lscale.put(in, 0, pr->level_scale, (size_t)P);
  L.mscale.put(in, 0, pr->max_scale, (size_t)P);
  L.Ow.put(in, 0, pr->obs_Ow, (size_t)O);
  L.flags.put(in, 0, pr->obs_flags, (size_t)O);
  int n_dsc = 0;
  if (with_desc) {
    int *dsc_start = L.dsc_start.at(in), *dsc_obs = L.dsc_obs.at(in);
    for (int p = 0; p < P; p++) {
      dsc_start[p] = n_dsc;
      const int o0 = pr->obs_start[p], o1 = pr->obs_start[p + 1];
      for (int o = o0; o < o1; o++)
        if (pr->obs_flags[o] & GFS_MAP_POINT_OBS_IN_DESC) {
          dsc_obs[n_dsc] = o - o0;
          L.words.put(in, (size_t)n_dsc, pr->obs_desc + 32 * (size_t)o, 1);
          n_dsc++;
        }
    }
    dsc_start[P] = n_dsc;
  }
  hipStream_t s = h->stream;
  if (int rc = h->in.upload(s, 0, L.words.off + L.words.bytes((size_t)n_dsc))) return rc;  // (n_dsc = 0 without descriptors)
  MpArgs A{};
  A.n_points = P;
  A.with_desc = with_desc ? 1 : 0;
  const uint8_t* di = h->in.d.p;
  uint8_t* dout = h->out.d.p;
  A.obs_start = L.obs_start.at(di);
  A.dsc_start = L.dsc_start.at(di);
  A.obs_Ow = L.Ow.at(di);
  A.obs_flags = L.flags.at(di);
  A.dsc_words = L.words.at(di);
  A.dsc_obs = L.dsc_obs.at(di);
  A.pos = L.pos.at(di);
  A.ref_Ow = L.ref.at(di);
  A.level_scale = L.lscale.at(di);
  A.max_scale = L.mscale.at(di);
  A.best_obs = L.best.at(dout);
  A.best_median = L.median.at(dout);
  A.normal = L.normal.at(dout);
  A.min_dist = L.dmin.at(dout);
  A.max_dist = L.dmax.at(dout);
  A.status = L.status.at(dout);
  GFS_LAUNCH("k_map_points", k_map_points, dim3(gfs::div_up(P, kWaves)), dim3(kThreads), 0, s, A);
  if (int rc = h->out.download(s, 0, L.status.off + L.status.bytes((size_t)P))) return rc;
  GFS_HIP(hipStreamSynchronize(s));
  const uint8_t* o = h->out.h.p;
  L.best.get(res->best_obs, o, 0, (size_t)P);
  L.median.get(res->best_median, o, 0, (size_t)P);
  L.normal.get(res->normal, o, 0, (size_t)P);
  L.dmin.get(res->min_dist, o, 0, (size_t)P);
  L.dmax.get(res->max_dist, o, 0, (size_t)P);
  L.status.get(res->status, o, 0, (size_t)P);
  return GFS_OK;
}

}  // extern "C"
