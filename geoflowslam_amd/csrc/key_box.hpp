// The key box of the voxel and cell sorts (gicp.hip: k_radix_sort, k_cell_sort_lds, k_cell_build; voxel_qsort.hpp: the three
// k_voxel_qsort_top* kernels).  A sort key packs three coordinate fields, x | y << sy | z << sz (sy / sz = 21 / 42 for voxel keys,
// 25 / 45 for cell sort keys), but one cloud spans only a few hundred cells an axis.  Re-basing every field to the cloud's minimum
// and packing the fields tightly is order preserving and leaves keys of bits[0] + bits[1] + bits[2] bits: fewer radix passes, and
// below 32 bits a sort on 4-byte keys.  Equality and the invalid key (all ones: it sorts last) are preserved.
// The first part is plain C++ (tests/host/key_box_check.cpp includes it without HIP); the device part collects the box of a cloud
// with one workgroup.
#pragma once

#if defined(__HIPCC__)
#include "gfs_common.hpp"
#define GFS_KB_HD __host__ __device__ __forceinline__
#else
#define GFS_KB_HD inline
#endif

namespace gfs_kb {

typedef unsigned long long u64;
constexpr u64 kInvalid64 = ~0ull;
constexpr unsigned kInvalid32 = 0xffffffffu;

// kinfo[8 c + slot]: what a sort leaves about cloud c for the kernels behind it
constexpr int kInfoStride = 8;
constexpr int kInfoMin = 0;        // .. 2: the minima of the three fields
constexpr int kInfoBitsX = 3, kInfoBitsY = 4;  // widths of the x and y fields (the z field is what lies above them)
constexpr int kInfoBitsTotal = 5;  // bits of a packed key (the voxel sort's kernels only: <= 31 selects the leaf kernels' 4-byte keys)
constexpr int kInfoLeft = 6;       // voxel sort: 0 = sorted by the kernel that wrote it, else the cloud is left for the next kernel

// The smallest b >= 1 with range < 2^b (0 <= range < 2^30)
GFS_KB_HD int nbits(int range) {
  int b = 1;
  while ((1 << b) <= range) b++;
  return b;
}

struct KeyBox {
  int mn[3];    // minimum of every field over the cloud's valid keys
  int bits[3];  // width of every re-based field
  GFS_KB_HD int total() const { return bits[0] + bits[1] + bits[2]; }
};

// The box of a cloud without a valid key
GFS_KB_HD KeyBox empty_box() { return KeyBox{{0, 0, 0}, {1, 1, 1}}; }
// The box of the field extents mn[a] .. mx[a]
GFS_KB_HD KeyBox box_of(const int* mn, const int* mx) {
  KeyBox b;
  for (int a = 0; a < 3; a++) {
    b.mn[a] = mn[a];
    b.bits[a] = nbits(mx[a] - mn[a]);
  }
  return b;
}

// The three fields of a valid key
GFS_KB_HD void split(u64 k, int sy, int sz, int* f) {
  f[0] = (int)(k & ((1ull << sy) - 1));
  f[1] = (int)((k >> sy) & ((1ull << (sz - sy)) - 1));
  f[2] = (int)(k >> sz);
}

GFS_KB_HD u64 pack64(const KeyBox& b, u64 k, int sy, int sz) {
  if (k == kInvalid64) return kInvalid64;
  const u64 x = (k & ((1ull << sy) - 1)) - b.mn[0], y = ((k >> sy) & ((1ull << (sz - sy)) - 1)) - b.mn[1], z = (k >> sz) - b.mn[2];
  return x | (y << b.bits[0]) | (z << (b.bits[0] + b.bits[1]));
}

// Widest box whose keys a kernel sorts as 4-byte keys; clouds beyond it are left to the next kernel.  Up to 31 bits no valid key
// packs to kInvalid32; at 32 the largest one can: the cell sort takes such boxes (it has no invalid keys), the voxel sort does not.
constexpr int kMaxBits32WithInvalid = 31, kMaxBits32 = 32;

GFS_KB_HD unsigned pack32(const KeyBox& b, u64 k, int sy, int sz) {
  if (k == kInvalid64) return kInvalid32;
  return (unsigned)((k & ((1ull << sy) - 1)) - b.mn[0]) | ((unsigned)(((k >> sy) & ((1ull << (sz - sy)) - 1)) - b.mn[1]) << b.bits[0]) |
         ((unsigned)((k >> sz) - b.mn[2]) << (b.bits[0] + b.bits[1]));
}

// The fields of the key that a VALID packed key came from (bits[2] is not needed: the z field is everything above x and y)
GFS_KB_HD void unpack_fields(const KeyBox& b, u64 packed, int* f) {
  f[0] = (int)(packed & ((1ull << b.bits[0]) - 1)) + b.mn[0];
  f[1] = (int)((packed >> b.bits[0]) & ((1ull << b.bits[1]) - 1)) + b.mn[1];
  f[2] = (int)(packed >> (b.bits[0] + b.bits[1])) + b.mn[2];
}
GFS_KB_HD u64 unpack(const KeyBox& b, u64 packed, int sy, int sz) {
  if (packed == kInvalid64) return kInvalid64;
  int f[3];
  unpack_fields(b, packed, f);
  return (u64)f[0] | ((u64)f[1] << sy) | ((u64)f[2] << sz);
}

// kinfo slots 0 - 4: all that k_radix_sort and k_cell_sort_lds leave, and all that unpack needs
GFS_KB_HD void store(int* ki, const KeyBox& b) {
  for (int a = 0; a < 3; a++) ki[kInfoMin + a] = b.mn[a];
  ki[kInfoBitsX] = b.bits[0];
  ki[kInfoBitsY] = b.bits[1];
}
GFS_KB_HD void store_with_total(int* ki, const KeyBox& b) {  // slots 0 - 5: the voxel sort
  store(ki, b);
  ki[kInfoBitsTotal] = b.total();
}
GFS_KB_HD KeyBox load(const int* ki) {  // (the width of z is not kept: 0)
  return KeyBox{{ki[kInfoMin], ki[kInfoMin + 1], ki[kInfoMin + 2]}, {ki[kInfoBitsX], ki[kInfoBitsY], 0}};
}

#if defined(__HIPCC__)
// One thread's share of a cloud's box: every kernel loads its keys its own way and feeds them one at a time; finish() is then
// called by ALL threads of the workgroup (a barrier) and returns the cloud's box to every one of them.
struct BoxAcc {
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-1, -1, -1};
  __device__ __forceinline__ void add(u64 k, int sy, int sz) {
    if (k == kInvalid64) return;
    int f[3];
    split(k, sy, sz, f);
    for (int a = 0; a < 3; a++) {
      mn[a] = min(mn[a], f[a]);
      mx[a] = max(mx[a], f[a]);
    }
  }
  // s_mn, s_mx: three ints of the workgroup's LDS each.  begin() -- all threads, one barrier -- goes in front of the kernel's key
  // loads: a wave that has its keys then reduces while the others still wait for theirs.
  static __device__ __forceinline__ void begin(int* s_mn, int* s_mx) {
    if (threadIdx.x < 3) {
      s_mn[threadIdx.x] = 0x7fffffff;
      s_mx[threadIdx.x] = -1;
    }
    __syncthreads();
  }
  __device__ __forceinline__ KeyBox finish(int* s_mn, int* s_mx) {
    for (int a = 0; a < 3; a++) {  // one LDS atomic a wave, not one a thread
      mn[a] = gfs::wave_min_i32(mn[a]);
      mx[a] = gfs::wave_max_i32(mx[a]);
      if ((threadIdx.x & 63) == 0 && mx[a] >= 0) {
        atomicMin(&s_mn[a], mn[a]);
        atomicMax(&s_mx[a], mx[a]);
      }
    }
    __syncthreads();
    return s_mx[0] >= 0 ? box_of(s_mn, s_mx) : empty_box();
  }
};
#endif

}  // namespace gfs_kb
