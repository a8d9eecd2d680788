// The staging pattern of the matcher, pose and map handles, stated once: everything a call reads is laid out in ONE pinned block that
// mirrors ONE device block, so that a call is one copy in, its kernels, one copy out and one synchronisation.
//   Block<Align>  the cursor of such a block; Field<T, K> f{block, n} takes the next n items of K elements of T from it.  A field knows
//                 its byte offset and its element type, so the element size of an array is written once.
//   Mirror        the pinned block and its device twin (HIP only).
// The layouts built from these are block_layouts.hpp's.  The first part is plain C++: a host program can include it without HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#if defined(__HIPCC__)
#include "gfs_common.hpp"
#endif

namespace gfs {

template <size_t Align>
struct Block {
  static_assert(Align >= alignof(max_align_t) && (Align & (Align - 1)) == 0, "every field starts aligned for any element type");
  size_t end = 0;
  Block() {}  // (not an aggregate: a layout's sizes cannot spill into its cursor)
  size_t bytes() const { return end; }  // of the whole block, once every field is taken
};

// An array of `items` x K elements of T, taken from a block's cursor: at(base, i) is item i's first element, bytes(n) what n items take.
template <class T, int K = 1>
struct Field {
  size_t off;
  template <size_t Align>
  Field(Block<Align>& b, size_t items) : off(b.end) {
    b.end += (bytes(items) + Align - 1) / Align * Align;
  }
  T* at(uint8_t* base, size_t item = 0) const { return reinterpret_cast<T*>(base + off) + item * K; }
  const T* at(const uint8_t* base, size_t item = 0) const { return reinterpret_cast<const T*>(base + off) + item * K; }
  static constexpr size_t bytes(size_t items) { return items * K * sizeof(T); }
  // n items from src to item `item` on of the block at base, or from there to dst; n = 0 copies nothing (the pointer may be NULL)
  void put(uint8_t* base, size_t item, const void* src, size_t n) const { if (n) memcpy(at(base, item), src, bytes(n)); }
  void get(void* dst, const uint8_t* base, size_t item, size_t n) const { if (n) memcpy(dst, at(base, item), bytes(n)); }
};

#if defined(__HIPCC__)
struct Mirror {
  PinBuf<uint8_t> h;
  DevBuf<uint8_t> d;
  int alloc(size_t bytes) {
    const int rc = d.alloc(bytes);
    return rc ? rc : h.alloc(bytes);
  }
  // bytes [from, to) of the block, host to device / device to host
  int upload(hipStream_t s, size_t from, size_t to) {
    GFS_HIP(hipMemcpyAsync(d.p + from, h.p + from, to - from, hipMemcpyHostToDevice, s));
    return GFS_OK;
  }
  int download(hipStream_t s, size_t from, size_t to) {
    GFS_HIP(hipMemcpyAsync(h.p + from, d.p + from, to - from, hipMemcpyDeviceToHost, s));
    return GFS_OK;
  }
};
#endif

}  // namespace gfs
