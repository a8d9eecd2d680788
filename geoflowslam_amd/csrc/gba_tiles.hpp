// Tiled storage of the reduced pose system of the global bundle adjustment (gfs_gba_solve): the lower triangle of the 6F x 6F
// Schur complement as square tiles of kP rows, tile (ti, tj), ti >= tj, at position ti (ti + 1) / 2 + tj, every tile kP x kP
// doubles row-major.  The last tile row is padded to a full tile (the assembly puts an identity on the padded diagonal).  Diagonal
// tiles are stored whole; only their lower triangle is meaningful.  Host and device share this arithmetic; everything is size_t:
// at n = 24 000 a byte offset passes 2^31 long before the last tile.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define GFS_GBA_HD __host__ __device__ __forceinline__
#else
#define GFS_GBA_HD inline
#endif

namespace gba_sys {

constexpr int kP = 96;  // panel rows: a multiple of 6 (a pose block never straddles two tiles) and of 16 (the matrix-core tile)
static_assert(kP % 6 == 0 && kP % 16 == 0, "a panel holds whole pose blocks and whole 16 x 16 matrix-core tiles");

GFS_GBA_HD size_t panels(size_t n) { return (n + kP - 1) / kP; }
GFS_GBA_HD size_t tile_index(size_t ti, size_t tj) { return ti * (ti + 1) / 2 + tj; }             // ti >= tj
GFS_GBA_HD size_t tile_offset(size_t ti, size_t tj) { return tile_index(ti, tj) * kP * kP; }      // in doubles
GFS_GBA_HD size_t elem_offset(size_t r, size_t c) {                                               // r >= c, in doubles
  return tile_offset(r / kP, c / kP) + (r % kP) * kP + (c % kP);
}
GFS_GBA_HD size_t storage_doubles(size_t n) { return tile_index(panels(n), 0) * kP * kP; }
GFS_GBA_HD size_t storage_bytes(size_t n) { return storage_doubles(n) * sizeof(double); }
GFS_GBA_HD size_t padded_rows(size_t n) { return panels(n) * kP; }

}  // namespace gba_sys
