// Brute-force 256-bit Hamming matcher for gfx950.
//
// Replaces cv::BFMatcher(cv::NORM_HAMMING).match(d1, d2, matches) at the reference's
// src/ORBmatcher.cc:755-756 / 805-806 / 888-889 and ORBmatcher::DescriptorDistance
// (src/ORBmatcher.cc:2536-2550).  Integer work, bit-exact by construction.
//
// Kernel shape (CDNA4, gfx950): the distance is a matrix product on the i8 matrix cores.  Write a train bit as the
// byte 0 / 1 and a query bit b as the signed byte 2b - 1.  Over the 256 bit positions
//   dot(train01, query+-1) = #(t = 1, q = 1) - #(t = 1, q = 0)   and   hamming = #(t = 1, q = 0) + #(t = 0, q = 1),
// so hamming(q, t) = popcount(q) - dot, exactly, in int32, for every input: per query the smallest distance is the
// largest dot, and popcount(q) enters once, at the end.  (The 0 / 1 side costs three VALU operations a word to unpack
// where +-1 costs six; the train side is the one unpacked again for every tile and workgroup.)
//
// One workgroup = 4 waves takes kQPerBlock = 256 queries of one frame against all of its train rows; a wave owns
// kQB = 2 blocks of 32 queries and keeps their +-1 fragments in registers for the whole kernel (8 K-steps x 16 bytes
// a lane = 32 VGPRs a block).  Train rows stream through LDS in tiles of 128 rows, unpacked to 256 bytes a row when
// the tile is staged (once a tile and workgroup, never a pair); the next tile's global load is in flight meanwhile.
// v_mfma_i32_32x32x32_i8 takes the train rows as the rows of A and the queries as the columns of B: a lane's 16
// accumulator registers are then 16 train rows of ONE query (column lane & 31), and the running best is in-lane.
//
// K order: lane (r = lane & 31, h = lane >> 5) hands K-step s the 16 bytes unpacked from bits [32 s + 16 h, + 16) of
// its row, on the train side and on the query side alike.  Which k the hardware gives each of those bytes does not
// matter: both operands use the same lane map, and a dot product does not care about the order of its terms.
//
// LDS image: row stride 272 B = 256 + 16.  A ds_read_b128 is served in four groups of 16 lanes; within a group every
// lane reads the same 16-byte column of a different row, and 68 dwords a row put those 16 rows on 16 different
// 4-bank groups (a 256-byte stride would put all of them on one).  The staging stores, 8 consecutive rows an
// 8-lane group, are conflict-free for the same reason.
//
// Running best: key = (dot + 256) << 20 | (0xFFFFF - idx), larger is better, so an unsigned max picks the smallest
// distance and, among equals, the LOWEST train index whatever the order of the visits (OpenCV's batchDistance; idx <
// 2^20 - 1, so a real key is never 0 and 0 stands for "no row").  An accumulator entry costs one v_lshl_add_u32 and
// its share of a v_max3_u32; a block of 32 rows adds its base once.  Rows at or beyond nt exist only in the last
// block of the last tile: they are staged as zeros and that block alone masks them.  The two lanes that share a
// query meet in one cross-lane step at the end; no query is shared between waves, so there is no cross-wave merge.
#include "gfs_common.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_bf_hamming uses v_mfma_i32_32x32x32_i8, the double-K i8 MFMA of gfx950"
#endif

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kQB = 2;                    // blocks of 32 queries a wave
constexpr int kQPerBlock = 4 * 32 * kQB;  // queries a workgroup
constexpr int kTile = 128;                // train rows a tile
constexpr int kRowStride = 256 + 16;      // bytes a row of the LDS image (see above)

// 4 bits -> 4 bytes 0 / 1: bit i of x lands on bit 8 i (the products i + 7 k are distinct, so nothing carries)
__device__ __forceinline__ unsigned int spread4(unsigned int x) { return __umul24(x, 0x204081u) & 0x01010101u; }

// 16 bits -> 16 bytes 0 / 1
__device__ __forceinline__ v4i unpack01(unsigned int h) {
  v4i r;
  r.x = (int)spread4(h & 15u);
  r.y = (int)spread4((h >> 4) & 15u);
  r.z = (int)spread4((h >> 8) & 15u);
  r.w = (int)spread4((h >> 12) & 15u);
  return r;
}

// 16 bits -> 16 bytes -1 / +1: 0xFF - 0xFE m per byte, no carries between bytes
__device__ __forceinline__ v4i unpack_pm1(unsigned int h) {
  v4i m = unpack01(h), r;
  r.x = (int)(0xFFFFFFFFu - (unsigned int)m.x * 0xFEu);
  r.y = (int)(0xFFFFFFFFu - (unsigned int)m.y * 0xFEu);
  r.z = (int)(0xFFFFFFFFu - (unsigned int)m.z * 0xFEu);
  r.w = (int)(0xFFFFFFFFu - (unsigned int)m.w * 0xFEu);
  return r;
}

// The per-register part of a key: register r of a lane is train row (r & 3) + 8 (r >> 2) + 4 h of its 32 x 32 block
// (the C / D map of the 32 x 32 MFMAs).  The 4 h goes into the lane's block base, so these 16 are uniform and sit in
// SGPRs; the empty asm keeps each one a register, so that an entry is ONE v_lshl_add_u32 (acc << 20) + c and not a
// shift, a subtract and an add of a literal.  A real entry is >= 5, so 0 can stand for a masked one.
struct KeyConsts {
  unsigned int c[16];
  __device__ __forceinline__ KeyConsts() {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      c[r] = (256u << 20) + 32u - (unsigned int)((r & 3) + 8 * (r >> 2));
      asm volatile("" : "+s"(c[r]));
    }
  }
};

// The best key of one accumulator block, without the block's base.  kMasked: rows at or beyond lim, counted in the
// block, give 0 (h4 = 4 h).
template <bool kMasked>
__device__ __forceinline__ unsigned int block_best(const v16i& acc, const KeyConsts& kc, int h4, int lim) {
  unsigned int m = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    unsigned int k = ((unsigned int)acc[r] << 20) + kc.c[r];
    if (kMasked) k = ((r & 3) + 8 * (r >> 2) + h4 < lim) ? k : 0u;
    m = max(m, k);
  }
  return m;
}

// (waves_per_eu 3: at most 168 registers, so that the accumulators are VGPRs the VALU reads without v_accvgpr_read)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_bf_hamming(const uint8_t* __restrict__ query, const int* __restrict__ nq_arr,
                                                    const uint8_t* __restrict__ train, const int* __restrict__ nt_arr,
                                                    int stride_rows, int* __restrict__ out_idx,
                                                    int* __restrict__ out_dist) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[kTile * kRowStride];
  const int b = blockIdx.y;
  const int nq = nq_arr[b], nt = nt_arr[b];
  const int q0 = blockIdx.x * kQPerBlock;
  if (q0 >= nq) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const uint4* qb = reinterpret_cast<const uint4*>(query + (size_t)b * stride_rows * 32);
  const uint4* tb = reinterpret_cast<const uint4*>(train + (size_t)b * stride_rows * 32);
  const int wq0 = q0 + wave * (32 * kQB);  // a wave with no query below nq only helps to stage

  // the queries' fragments and popcounts; a query at or beyond nq is read as zeros and never written
  v4i bq[kQB][8];
  int pq[kQB];
#pragma unroll
  for (int j = 0; j < kQB; ++j) {
    const int q = wq0 + 32 * j + col;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (q < nq) {
      lo = qb[2 * (size_t)q];
      hi = qb[2 * (size_t)q + 1];
    }
    const unsigned int w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    pq[j] = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      pq[j] += __popc(w[s]);
      bq[j][s] = unpack_pm1(h ? w[s] >> 16 : w[s] & 0xFFFFu);
    }
  }
  unsigned int best[kQB];
#pragma unroll
  for (int j = 0; j < kQB; ++j) best[j] = 0u;

  // staging: thread (row = tid & 127, half = tid >> 7) unpacks 16 bytes of its row into 8 chunks of 16 bytes
  const int srow = tid & 127, shalf = tid >> 7;
  unsigned char* sdst = tile + srow * kRowStride + shalf * 128;
  const unsigned char* aread = tile + col * kRowStride + h * 16;
  const KeyConsts kc;
  uint4 nxt = make_uint4(0, 0, 0, 0);
  if (srow < nt) nxt = tb[2 * (size_t)srow + shalf];
  for (int t0 = 0; t0 < nt; t0 += kTile) {
    __syncthreads();  // every wave has read the tile before
    const unsigned int sw[4] = {nxt.x, nxt.y, nxt.z, nxt.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<v4i*>(sdst + 32 * i) = unpack01(sw[i] & 0xFFFFu);
      *reinterpret_cast<v4i*>(sdst + 32 * i + 16) = unpack01(sw[i] >> 16);
    }
    nxt = make_uint4(0, 0, 0, 0);
    if (t0 + kTile + srow < nt) nxt = tb[2 * (size_t)(t0 + kTile + srow) + shalf];
    __syncthreads();
    if (wq0 >= nq) continue;
    const int rows = min(kTile, nt - t0);
    for (int r0 = 0; r0 < rows; r0 += 32) {
      v16i acc[kQB];
#pragma unroll
      for (int j = 0; j < kQB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const v4i a = *reinterpret_cast<const v4i*>(aread + r0 * kRowStride + s * 32);
#pragma unroll
        for (int j = 0; j < kQB; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[j][s], acc[j], 0, 0, 0);
      }
      // low 20 bits of a key: (32 - row in block + 4 h) + (0xFFFFF - 32 - block base - 4 h) = 0xFFFFF - idx
      const unsigned int bc = 0xFFFFFu - 32u - (unsigned int)(t0 + r0) - 4u * (unsigned int)h;
      if (rows - r0 >= 32) {
#pragma unroll
        for (int j = 0; j < kQB; ++j) best[j] = max(best[j], block_best<false>(acc[j], kc, 4 * h, 32) + bc);
      } else {
#pragma unroll
        for (int j = 0; j < kQB; ++j) {
          const unsigned int m = block_best<true>(acc[j], kc, 4 * h, rows - r0);
          best[j] = max(best[j], m ? m + bc : 0u);
        }
      }
    }
  }
  if (wq0 >= nq) return;
  int* oi = out_idx + (size_t)b * stride_rows;
  int* od = out_dist + (size_t)b * stride_rows;
#pragma unroll
  for (int j = 0; j < kQB; ++j) {
    const unsigned int k = max(best[j], (unsigned int)__shfl_xor((int)best[j], 32));
    const int q = wq0 + 32 * j + col;
    if (h == 0 && q < nq) {
      if (k == 0u) {
        oi[q] = -1;
        od[q] = 0x7fffffff;
      } else {
        oi[q] = (int)(0xFFFFFu - (k & 0xFFFFFu));
        od[q] = pq[j] - ((int)(k >> 20) - 256);  // hamming = popcount(q) - dot
      }
    }
  }
}

}  // namespace

struct gfs_matcher {
  int device, max_q, max_t, max_b;
  hipStream_t stream;
  gfs::DevBuf<uint8_t> d_q, d_t;
  gfs::DevBuf<int> d_nq, d_nt, d_idx, d_dist;
  std::mutex mu;
};

extern "C" {

// ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2536-2550): same value, computed with popcount.
int gfs_hamming256(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 4; i++) {
    uint64_t x, y;
    memcpy(&x, a + 8 * i, 8);
    memcpy(&y, b + 8 * i, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

int gfs_matcher_create(int device, int max_query, int max_train, int max_batch, gfs_matcher** out) {
  GFS_REQUIRE(out && max_query > 0 && max_train > 0 && max_batch > 0, GFS_ERR_INVALID_ARG,
              "gfs_matcher_create: invalid argument");
  GFS_REQUIRE(max_train < (1 << 20), GFS_ERR_UNSUPPORTED, "gfs_matcher_create: max_train must be < 2^20");
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  gfs_matcher* h = new gfs_matcher;
  h->device = device;
  h->max_q = max_query;
  h->max_t = max_train;
  h->max_b = max_batch;
  int rc;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t rows = (size_t)std::max(max_query, max_train);
  if ((rc = h->d_q.alloc(rows * 32)) || (rc = h->d_t.alloc(rows * 32)) || (rc = h->d_nq.alloc(1)) ||
      (rc = h->d_nt.alloc(1)) || (rc = h->d_idx.alloc(rows)) || (rc = h->d_dist.alloc(rows))) {
    delete h;
    return rc;
  }
  *out = h;
  return GFS_OK;
}

void gfs_matcher_destroy(gfs_matcher* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_bf_match_hamming_batch_device(gfs_matcher* h, const void* dev_query, const void* dev_nq, const void* dev_train,
                                      const void* dev_nt, int B, int stride_rows, void* dev_train_idx, void* dev_dist,
                                      void* stream) {
  GFS_REQUIRE(h && dev_query && dev_nq && dev_train && dev_nt && dev_train_idx && dev_dist && B > 0 && stride_rows > 0,
              GFS_ERR_INVALID_ARG, "gfs_bf_match_hamming_batch_device: invalid argument");
  GFS_REQUIRE(stride_rows < (1 << 20), GFS_ERR_UNSUPPORTED, "stride_rows must be < 2^20");
  GFS_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  dim3 grid(gfs::div_up(stride_rows, kQPerBlock), B);
  GFS_LAUNCH("k_bf_hamming", k_bf_hamming, grid, dim3(256), 0, s, (const uint8_t*)dev_query, (const int*)dev_nq,
             (const uint8_t*)dev_train, (const int*)dev_nt, stride_rows, (int*)dev_train_idx, (int*)dev_dist);
  return GFS_OK;
}

int gfs_bf_match_hamming(gfs_matcher* h, const uint8_t* query, int nq, const uint8_t* train, int nt,
                         int32_t* train_idx, int32_t* dist) {
  GFS_REQUIRE(h && nq >= 0 && nt >= 0, GFS_ERR_INVALID_ARG, "gfs_bf_match_hamming: invalid argument");
  if (nq == 0 || nt == 0) return 0;  // OpenCV: empty train set -> no matches
  GFS_REQUIRE(query && train && train_idx && dist, GFS_ERR_INVALID_ARG, "gfs_bf_match_hamming: NULL buffer");
  GFS_REQUIRE(nq <= h->max_q && nt <= h->max_t, GFS_ERR_CAPACITY, "gfs_bf_match_hamming: %d x %d exceeds handle capacity %d x %d",
              nq, nt, h->max_q, h->max_t);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int stride_rows = std::max(h->max_q, h->max_t);
  GFS_HIP(hipMemcpyAsync(h->d_q.p, query, (size_t)nq * 32, hipMemcpyHostToDevice, s));
  GFS_HIP(hipMemcpyAsync(h->d_t.p, train, (size_t)nt * 32, hipMemcpyHostToDevice, s));
  GFS_HIP(hipMemcpyAsync(h->d_nq.p, &nq, sizeof(int), hipMemcpyHostToDevice, s));
  GFS_HIP(hipMemcpyAsync(h->d_nt.p, &nt, sizeof(int), hipMemcpyHostToDevice, s));
  int rc = gfs_bf_match_hamming_batch_device(h, h->d_q.p, h->d_nq.p, h->d_t.p, h->d_nt.p, 1, stride_rows, h->d_idx.p,
                                             h->d_dist.p, s);
  if (rc) return rc;
  GFS_HIP(hipMemcpyAsync(train_idx, h->d_idx.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipMemcpyAsync(dist, h->d_dist.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
  GFS_HIP(hipStreamSynchronize(s));
  return nq;
}

}  // extern "C"
