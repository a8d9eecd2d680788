// cv::CLAHE (8-bit, single channel) on MI355X: the equalisation the reference applies to Frame::image before
// cv::buildOpticalFlowPyramid when UseClahe is 1 (src/Frame.cc:366-369, 499-500; read again by Tracking::EstimatePoseByOF,
// src/Tracking.cc:1961).  The rule is DESIGN.md section 16, a written restatement of OpenCV's imgproc/src/clahe.cpp; the sequential
// statement is tests/host/clahe_restatement.cpp and this file computes the same bytes.
//
// Two launches per call.  k_clahe_lut: one workgroup of 256 threads per (tile, frame) takes the tile's histogram in the image
// extended by BORDER_REFLECT_101, clips it, redistributes the excess and writes the tile's 256-byte look-up table.  Counts are
// integers: no order of the atomic adds or of the reductions can change a bit.  k_clahe_interp: a thread handles 4 consecutive
// pixels of a row, blends the four neighbouring tiles' table entries of each in the float order the rule fixes, and stores one
// dword.  A pixel's output depends on its own input byte and on the tables only, so the image may be equalised in place.
#include <memory>
#include <mutex>

#include "clahe_handle.hpp"

namespace {

using gfs::DevBuf;
using gfs::PinBuf;

constexpr int kClaheMaxTiles = 16;
constexpr int kClaheMaxSide = 8192;

struct ClaheGeom {
  int width, height, tiles_x, tiles_y, tile_w, tile_h, clip, variant;
  float lut_scale, inv_tw, inv_th;
};

__device__ __forceinline__ int clahe_reflect101(int p, int len) {  // the loop of klt.hip's reflect101: p may lie beyond 2 * len
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lut [B][tiles_y][tiles_x][256].  LDS: one 256-bin histogram per wave (a wave's lanes hit one bin at a time wherever the image is
// flat, and four private copies keep the waves from queueing behind each other as well), merged by the thread that owns the bin.
__global__ void __launch_bounds__(256) k_clahe_lut(ClaheGeom G, const uint8_t* __restrict__ src, int stride, long long src_frame,
                                                    uint8_t* __restrict__ lut) {
  __shared__ unsigned s_hist[4][256];
  __shared__ int s_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < 4; w++) s_hist[w][tid] = 0;
  __syncthreads();
  const int tile = blockIdx.x, ty = tile / G.tiles_x, tx = tile - ty * G.tiles_x;
  const int x0 = tx * G.tile_w, y0 = ty * G.tile_h;
  const uint8_t* img = src + (long long)blockIdx.y * src_frame;
  unsigned* hw = s_hist[wave];
  const int ng = (G.tile_w + 3) >> 2, ntasks = ng * G.tile_h;  // runs of 4 pixels of a tile row
  for (int t = tid; t < ntasks; t += 256) {
    const int r = t / ng, g = t - r * ng, x = x0 + 4 * g;
    const int cnt = min(4, G.tile_w - 4 * g);
    const uint8_t* row = img + (long long)clahe_reflect101(y0 + r, G.height) * stride;
    if (cnt == 4 && x + 3 < G.width) {  // the run lies inside the image: one (unaligned) dword
      unsigned v;
      __builtin_memcpy(&v, row + x, 4);
      atomicAdd(&hw[v & 0xff], 1u);
      atomicAdd(&hw[(v >> 8) & 0xff], 1u);
      atomicAdd(&hw[(v >> 16) & 0xff], 1u);
      atomicAdd(&hw[v >> 24], 1u);
    } else {  // the extension band (or a tile narrower than the run)
      for (int k = 0; k < cnt; k++) atomicAdd(&hw[row[clahe_reflect101(x + k, G.width)]], 1u);
    }
  }
  __syncthreads();
  int h = (int)(s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid]);  // thread i owns bin i
  if (G.clip > 0) {
    const int excess = wave_sum_i32(max(h - G.clip, 0));
    if (lane == 0) s_part[wave] = excess;
    __syncthreads();
    const int clipped = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    __syncthreads();  // s_part is used again by the scan
    const int batch = clipped >> 8, residual = clipped - (batch << 8);
    h = min(h, G.clip) + batch;
    if (residual != 0) {
      if (G.variant == GFS_CLAHE_RESIDUAL_STEPPED) {
        const int step = max(256 / residual, 1), q = tid / step;
        if (tid - q * step == 0 && q < residual) h++;
      } else if (tid < residual) {
        h++;
      }
    }
  }
  int sum = h;  // inclusive prefix sum over the 256 bins
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(sum, o, 64);
    if (lane >= o) sum += up;
  }
  if (lane == 63) s_part[wave] = sum;
  __syncthreads();
  for (int w = 0; w < wave; w++) sum += s_part[w];
  const int v = __float2int_rn(__fmul_rn((float)sum, G.lut_scale));  // cvRound: to nearest, ties to even
  lut[((long long)blockIdx.y * gridDim.x + tile) * 256 + tid] = (uint8_t)min(max(v, 0), 255);
}

// Thread = 4 consecutive pixels of a row; block = 64 x 4 threads = 256 columns of 4 rows.
// src and dst are not __restrict__: they may be the same image.
// fetch(tile_row, tile_col, v) -> the table entry as float
template <class Fetch>
__device__ __forceinline__ void clahe_blend_run(const ClaheGeom& G, int x, int y, const uint8_t* in, uint8_t* out, Fetch fetch) {
  const float tyf = __fsub_rn(__fmul_rn((float)y, G.inv_th), 0.5f);
  const int ty1u = (int)floorf(tyf);
  const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
  const int ty1 = min(max(ty1u, 0), G.tiles_y - 1), ty2 = min(ty1u + 1, G.tiles_y - 1);  // (the upper clamp of ty1 never binds: y < height)
  const int n = min(4, G.width - x);
  unsigned v = 0;
  if (n == 4) {
    __builtin_memcpy(&v, in, 4);
  } else {
    for (int k = 0; k < n; k++) v |= (unsigned)in[k] << (8 * k);
  }
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k < n) {
      const float txf = __fsub_rn(__fmul_rn((float)(x + k), G.inv_tw), 0.5f);
      const int tx1u = (int)floorf(txf);
      const float xa = __fsub_rn(txf, (float)tx1u), xa1 = __fsub_rn(1.0f, xa);
      const int tx1 = min(max(tx1u, 0), G.tiles_x - 1), tx2 = min(tx1u + 1, G.tiles_x - 1), b = (int)((v >> (8 * k)) & 0xff);
      const float top = __fadd_rn(__fmul_rn(fetch(ty1, tx1, b), xa1), __fmul_rn(fetch(ty1, tx2, b), xa));
      const float bot = __fadd_rn(__fmul_rn(fetch(ty2, tx1, b), xa1), __fmul_rn(fetch(ty2, tx2, b), xa));
      const int r = __float2int_rn(__fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya)));
      o |= (unsigned)min(max(r, 0), 255) << (8 * k);
    }
  }
  if (n == 4) {
    __builtin_memcpy(out, &o, 4);
  } else {
    for (int k = 0; k < n; k++) out[k] = (uint8_t)(o >> (8 * k));
  }
}

// The tables are read through the cache: a frame's tables are 16 KB at 8 x 8 tiles and the lanes of a wave read neighbouring
// entries of a few of them.  Staging a block's tables in LDS first was measured and not kept.
__global__ void __launch_bounds__(256) k_clahe_interp(ClaheGeom G, const uint8_t* src, int in_stride, long long in_frame,
                                                       const uint8_t* __restrict__ lut, uint8_t* dst, int out_stride, long long out_frame) {
  const int x = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= G.width || y >= G.height) return;
  const uint8_t* in = src + (long long)blockIdx.z * in_frame + (long long)y * in_stride + x;
  uint8_t* out = dst + (long long)blockIdx.z * out_frame + (long long)y * out_stride + x;
  const uint8_t* L = lut + (long long)blockIdx.z * G.tiles_x * G.tiles_y * 256;
  clahe_blend_run(G, x, y, in, out, [&](int tr, int tc, int b) { return (float)L[(tr * G.tiles_x + tc) * 256 + b]; });
}

void clahe_geom(const gfs_clahe_config& cfg, int width, int height, ClaheGeom& G) {
  G.width = width;
  G.height = height;
  G.tiles_x = cfg.tiles_x;
  G.tiles_y = cfg.tiles_y;
  const bool whole = width % cfg.tiles_x == 0 && height % cfg.tiles_y == 0;
  const int ew = whole ? width : width + (cfg.tiles_x - width % cfg.tiles_x);  // a side that divides grows by a whole tiles_x
  const int eh = whole ? height : height + (cfg.tiles_y - height % cfg.tiles_y);
  G.tile_w = ew / cfg.tiles_x;
  G.tile_h = eh / cfg.tiles_y;
  const int area = G.tile_w * G.tile_h;
  G.lut_scale = 255.0f / (float)area;
  G.clip = 0;
  if (cfg.clip_limit > 0.0) {
    const double c = cfg.clip_limit * area / 256;  // (a limit beyond int clips nothing: no bin exceeds the area)
    G.clip = c >= 2147483647.0 ? 2147483647 : ((int)c > 1 ? (int)c : 1);
  }
  G.variant = cfg.residual_variant;
  G.inv_tw = 1.0f / (float)G.tile_w;
  G.inv_th = 1.0f / (float)G.tile_h;
}

}  // namespace

struct gfs_clahe {
  int device = 0, max_width = 0, max_height = 0, max_batch = 0;
  gfs_clahe_config cfg{};
  hipStream_t stream = nullptr;
  std::mutex mu;
  DevBuf<uint8_t> d_img;  // staging for host images; the equalised image of the pyramid build that was given no destination
  DevBuf<uint8_t> d_lut;  // [max_batch][tiles_y][tiles_x][256]
  PinBuf<uint8_t> h_img;
  int last_frames = 0;    // frames whose tables d_lut holds
};

gfs_clahe_core gfs_clahe_core_of(gfs_clahe* h) { return {h->device, h->max_width, h->max_height, h->max_batch, &h->mu, h->d_img.p}; }

int gfs_clahe_enqueue(gfs_clahe* h, const uint8_t* dev_in, int width, int height, int in_stride, int B, uint8_t* dev_out,
                      int out_stride, hipStream_t s) {
  ClaheGeom G;
  clahe_geom(h->cfg, width, height, G);
  GFS_LAUNCH("k_clahe_lut", k_clahe_lut, dim3(G.tiles_x * G.tiles_y, B), dim3(256), 0, s, G, dev_in, in_stride,
             (long long)in_stride * height, h->d_lut.p);
  GFS_LAUNCH("k_clahe_interp", k_clahe_interp, dim3(gfs::div_up(gfs::div_up(width, 4), 64), gfs::div_up(height, 4), B), dim3(64, 4), 0, s,
             G, dev_in, in_stride, (long long)in_stride * height, (const uint8_t*)h->d_lut.p, dev_out, out_stride,
             (long long)out_stride * height);
  h->last_frames = B;
  return GFS_OK;
}

extern "C" {

void gfs_clahe_default_config(gfs_clahe_config* cfg) {
  if (!cfg) return;
  cfg->clip_limit = 3.0;  // cv::createCLAHE(3.0, cv::Size(8, 8)), src/Frame.cc:367
  cfg->tiles_x = 8;
  cfg->tiles_y = 8;
  cfg->residual_variant = GFS_CLAHE_RESIDUAL_STEPPED;
}

int gfs_clahe_create(int device, int max_width, int max_height, int max_batch, const gfs_clahe_config* cfg, gfs_clahe** out) {
  GFS_REQUIRE(out, GFS_ERR_INVALID_ARG, "gfs_clahe_create: out is NULL");
  *out = nullptr;
  GFS_REQUIRE(cfg && max_width > 0 && max_height > 0 && max_batch > 0, GFS_ERR_INVALID_ARG, "gfs_clahe_create: invalid argument");
  GFS_REQUIRE(cfg->tiles_x >= 1 && cfg->tiles_x <= kClaheMaxTiles && cfg->tiles_y >= 1 && cfg->tiles_y <= kClaheMaxTiles,
              GFS_ERR_INVALID_ARG, "gfs_clahe_create: %d x %d tiles (1 .. %d per side)", cfg->tiles_x, cfg->tiles_y, kClaheMaxTiles);
  GFS_REQUIRE(cfg->residual_variant == GFS_CLAHE_RESIDUAL_STEPPED || cfg->residual_variant == GFS_CLAHE_RESIDUAL_CONTIGUOUS,
              GFS_ERR_INVALID_ARG, "gfs_clahe_create: unknown residual variant %d", cfg->residual_variant);
  GFS_REQUIRE(cfg->clip_limit == cfg->clip_limit, GFS_ERR_INVALID_ARG, "gfs_clahe_create: clip limit is NaN");
  GFS_REQUIRE(max_batch <= 65535, GFS_ERR_CAPACITY, "gfs_clahe_create: batch %d beyond 65535", max_batch);
  GFS_REQUIRE(max_width <= kClaheMaxSide && max_height <= kClaheMaxSide, GFS_ERR_CAPACITY, "gfs_clahe_create: image larger than %d x %d",
              kClaheMaxSide, kClaheMaxSide);
  if (!gfs::device_ok(device)) return GFS_ERR_NO_DEVICE;
  GFS_HIP(hipSetDevice(device));
  auto h = std::make_unique<gfs_clahe>();
  h->device = device;
  h->max_width = max_width;
  h->max_height = max_height;
  h->max_batch = max_batch;
  h->cfg = *cfg;
  const size_t NI = (size_t)max_batch * max_width * max_height;
  int rc = h->d_img.alloc(NI);
  if (!rc) rc = h->h_img.alloc(NI);
  if (!rc) rc = h->d_lut.alloc((size_t)max_batch * cfg->tiles_x * cfg->tiles_y * 256);
  if (rc) return rc;
  GFS_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  *out = h.release();
  return GFS_OK;
}

void gfs_clahe_destroy(gfs_clahe* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamDestroy(h->stream);
  delete h;
}

int gfs_clahe_apply(gfs_clahe* h, const uint8_t* const* images, int width, int height, int stride, int B, uint8_t* const* out,
                    int out_stride) {
  GFS_REQUIRE(h && images && out && B > 0 && width > 0 && height > 0, GFS_ERR_INVALID_ARG, "gfs_clahe_apply: invalid argument");
  GFS_REQUIRE(stride >= width && out_stride >= width, GFS_ERR_INVALID_ARG, "gfs_clahe_apply: stride %d / %d < width %d", stride,
              out_stride, width);
  GFS_REQUIRE(B <= h->max_batch && width <= h->max_width && height <= h->max_height, GFS_ERR_CAPACITY,
              "gfs_clahe_apply: %d frames of %d x %d exceed the reserve (%d of %d x %d)", B, width, height, h->max_batch, h->max_width,
              h->max_height);
  for (int f = 0; f < B; f++) GFS_REQUIRE(images[f] && out[f], GFS_ERR_INVALID_ARG, "gfs_clahe_apply: image %d is NULL", f);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  const size_t frame = (size_t)width * height;
  for (int f = 0; f < B; f++)
    for (int y = 0; y < height; y++) memcpy(h->h_img.p + f * frame + (size_t)y * width, images[f] + (size_t)y * stride, width);
  GFS_HIP(hipMemcpyAsync(h->d_img.p, h->h_img.p, B * frame, hipMemcpyHostToDevice, h->stream));
  const int rc = gfs_clahe_enqueue(h, h->d_img.p, width, height, width, B, h->d_img.p, width, h->stream);
  if (rc) return rc;
  GFS_HIP(hipMemcpyAsync(h->h_img.p, h->d_img.p, B * frame, hipMemcpyDeviceToHost, h->stream));
  GFS_HIP(hipStreamSynchronize(h->stream));
  for (int f = 0; f < B; f++)
    for (int y = 0; y < height; y++) memcpy(out[f] + (size_t)y * out_stride, h->h_img.p + f * frame + (size_t)y * width, width);
  return GFS_OK;
}

int gfs_clahe_apply_device(gfs_clahe* h, const void* dev_in, int width, int height, int in_stride, int B, void* dev_out, int out_stride,
                           void* stream) {
  GFS_REQUIRE(h && dev_in && dev_out && B > 0 && width > 0 && height > 0, GFS_ERR_INVALID_ARG, "gfs_clahe_apply_device: invalid argument");
  GFS_REQUIRE(in_stride >= width && out_stride >= width, GFS_ERR_INVALID_ARG, "gfs_clahe_apply_device: stride %d / %d < width %d",
              in_stride, out_stride, width);
  GFS_REQUIRE(dev_out != dev_in || out_stride == in_stride, GFS_ERR_INVALID_ARG,
              "gfs_clahe_apply_device: in place needs equal strides (%d, %d)", in_stride, out_stride);
  GFS_REQUIRE(B <= h->max_batch && width <= h->max_width && height <= h->max_height, GFS_ERR_CAPACITY,
              "gfs_clahe_apply_device: %d frames of %d x %d exceed the reserve (%d of %d x %d)", B, width, height, h->max_batch,
              h->max_width, h->max_height);
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int rc = gfs_clahe_enqueue(h, (const uint8_t*)dev_in, width, height, in_stride, B, (uint8_t*)dev_out, out_stride, s);
  if (rc) return rc;
  if (!stream) GFS_HIP(hipStreamSynchronize(s));
  return GFS_OK;
}

int gfs_clahe_download_luts(gfs_clahe* h, int f, uint8_t* lut) {
  GFS_REQUIRE(h && lut, GFS_ERR_INVALID_ARG, "gfs_clahe_download_luts: invalid argument");
  std::lock_guard<std::mutex> lk(h->mu);
  GFS_REQUIRE(f >= 0 && f < h->last_frames, GFS_ERR_INVALID_ARG, "gfs_clahe_download_luts: frame %d of %d", f, h->last_frames);
  GFS_HIP(hipSetDevice(h->device));
  GFS_HIP(hipDeviceSynchronize());  // the last call may have run on the caller's or a tracker's stream
  const size_t n = (size_t)h->cfg.tiles_x * h->cfg.tiles_y * 256;
  GFS_HIP(hipMemcpy(lut, h->d_lut.p + f * n, n, hipMemcpyDeviceToHost));
  return GFS_OK;
}

}  // extern "C"
