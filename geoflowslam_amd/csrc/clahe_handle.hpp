// What klt.hip needs of a gfs_clahe handle (the struct itself is clahe.hip's): its device, lock, reserve and scratch image, and
// the two launches on a stream of the caller's choice.
#pragma once
#include "gfs_common.hpp"

struct gfs_clahe_core {
  int device, max_width, max_height, max_batch;
  std::mutex* mu;
  uint8_t* scratch;  // [max_batch][max_height][max_width] bytes
};

gfs_clahe_core gfs_clahe_core_of(gfs_clahe* h);  // clahe.hip
// k_clahe_lut + k_clahe_interp for B frames of [height][in_stride] bytes on stream s; dev_out may be dev_in when the strides are equal.
// The caller holds the handle's lock and has checked the sizes against the reserve.
int gfs_clahe_enqueue(gfs_clahe* h, const uint8_t* dev_in, int width, int height, int in_stride, int B, uint8_t* dev_out,
                      int out_stride, hipStream_t s);
