// The CLAHE restatement as a program of its own, for a build under -fsanitize=address,undefined (CPU only; never loaded into
// python): the sizes whose extension band is where an index can go wrong -- 5 x 3 (the extension is longer than the image),
// 163 x 117 (extended both ways), 160 x 117 (the width divides and grows by a whole 8 columns) -- both residual variants, packed and
// padded rows, out of place and in place, every buffer allocated at its exact size.  Prints the byte sums of the outputs, which
// tests/test_clahe_restatement.py compares with the same calls through the shared library.
#include <cstdio>
#include <cstdlib>

#include "clahe_restatement.cpp"

static uint8_t pixel(int x, int y) { return (uint8_t)(100 + (x * 7 + y * 13 + (x * y) % 5) % 40); }

int main() {
  const int sizes[3][2] = {{5, 3}, {163, 117}, {160, 117}};
  for (const auto& s : sizes)
    for (int variant = 0; variant < 2; variant++)
      for (int pad = 0; pad <= 13; pad += 13) {
        const int W = s[0], H = s[1], stride = W + pad;
        // the last row ends at its last pixel: a read of the padding behind it is out of bounds
        std::vector<uint8_t> src((size_t)(H - 1) * stride + W), dst((size_t)(H - 1) * stride + W), luts(64 * 256);
        for (int y = 0; y < H; y++)
          for (int x = 0; x < W; x++) src[(size_t)y * stride + x] = pixel(x, y);
        std::vector<int32_t> info(64 * 2);
        std::vector<uint8_t> lut_tie(64 * 256), pix_tie((size_t)W * H);
        if (cr_clahe(src.data(), W, H, stride, 3.0, 8, 8, variant, dst.data(), stride, luts.data(), info.data(), lut_tie.data(), pix_tie.data()))
          return 1;
        unsigned long long sum = 0, lsum = 0;
        for (int y = 0; y < H; y++)
          for (int x = 0; x < W; x++) sum += dst[(size_t)y * stride + x];
        for (uint8_t v : luts) lsum += v;
        std::vector<uint8_t> lut2(64 * 256);
        if (cr_clahe(src.data(), W, H, stride, 3.0, 8, 8, variant, src.data(), stride, lut2.data(), nullptr, nullptr, nullptr)) return 1;  // in place
        for (int y = 0; y < H; y++)
          for (int x = 0; x < W; x++)
            if (src[(size_t)y * stride + x] != dst[(size_t)y * stride + x]) return 2;
        printf("%d %d %d %d %llu %llu\n", W, H, variant, pad, sum, lsum);
      }
  printf("clahe_restatement_main: ok\n");
  return 0;
}
