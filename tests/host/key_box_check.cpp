// Host check of the plain part of geoflowslam_amd/csrc/key_box.hpp, for both field layouts (voxel keys: y at bit 21, z at 42, fields
// of 21 bits; cell sort keys: y at 25, z at 45, fields of 25 / 20 / 19 bits) and seeded random boxes whose per-field ranges include
// 0, 2^b - 1 and 2^b:  every width is the smallest b >= 1 with range < 2^b;  unpack(pack(k)) == k;  pack keeps the order of any two
// valid keys;  the invalid key stays the maximum;  a box of 31 bits keeps every valid 4-byte key below the invalid one, a box of 32
// bits does not (the voxel sort leaves it to the next kernel, the cell sort -- no invalid keys -- takes it), 33 bits fit no 4-byte
// key;  the kinfo slots hold what load() reads back.
// Plain C++: g++ -std=c++17 -I <repo root>; exit code 0 and "ok" when all hold.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "geoflowslam_amd/csrc/key_box.hpp"

using namespace gfs_kb;

static int g_bad = 0;
static long g_checked = 0;
#define CHECK(cond, ...)   \
  do {                     \
    g_checked++;           \
    if (!(cond)) {         \
      if (g_bad++ < 20) {  \
        printf("BAD ");    \
        printf(__VA_ARGS__); \
        printf("\n");      \
      }                    \
    }                      \
  } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dull;
}

struct Layout {
  const char* name;
  int sy, sz, width[3];
};
// (the z field of a cell key tried with 18 of its 19 bits: with all 64 bits set a key would BE the invalid key)
static const Layout kLayouts[2] = {{"voxel", 21, 42, {21, 21, 21}}, {"cell", 25, 45, {25, 20, 18}}};

static u64 join(const Layout& L, const int* f) { return (u64)f[0] | ((u64)f[1] << L.sy) | ((u64)f[2] << L.sz); }

static int width_by_definition(int range) {
  for (int b = 1;; b++)
    if ((long long)range < (1ll << b)) return b;
}

// keys inside [mn, mn + range] per field, the corners among them; checks everything a cloud with this box promises
static void check_box(const Layout& L, const int* mn, const int* range, int n_keys) {
  std::vector<u64> keys;
  int lo[3], hi[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = mn[a];
    hi[a] = mn[a] + range[a];
  }
  keys.push_back(join(L, lo));
  keys.push_back(join(L, hi));
  for (int i = 0; i < n_keys; i++) {
    int f[3];
    for (int a = 0; a < 3; a++) {
      const int pick = (int)(rnd() % 4);  // the ends of a field's range more often than chance would
      f[a] = pick == 0 ? lo[a] : pick == 1 ? hi[a] : lo[a] + (int)(rnd() % ((u64)range[a] + 1));
    }
    keys.push_back(join(L, f));
  }
  // the extents as a kernel collects them
  int emn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, emx[3] = {-1, -1, -1};
  for (u64 k : keys) {
    int f[3];
    split(k, L.sy, L.sz, f);
    CHECK(join(L, f) == k, "%s: split loses bits of %llx", L.name, k);
    for (int a = 0; a < 3; a++) {
      emn[a] = f[a] < emn[a] ? f[a] : emn[a];
      emx[a] = f[a] > emx[a] ? f[a] : emx[a];
    }
  }
  const KeyBox box = box_of(emn, emx);
  for (int a = 0; a < 3; a++) {
    CHECK(box.mn[a] == mn[a], "%s: minimum of field %d: %d, expected %d", L.name, a, box.mn[a], mn[a]);
    CHECK(box.bits[a] == width_by_definition(range[a]) && box.bits[a] >= 1 && (long long)range[a] < (1ll << box.bits[a]) &&
              (box.bits[a] == 1 || (long long)range[a] >= (1ll << (box.bits[a] - 1))),
          "%s: width of field %d with range %d: %d", L.name, a, range[a], box.bits[a]);
  }
  const int total = box.total();
  CHECK(total == box.bits[0] + box.bits[1] + box.bits[2], "%s: total", L.name);
  const bool fits32 = total <= kMaxBits32, fits32_invalid = total <= kMaxBits32WithInvalid;
  std::vector<u64> p64;
  std::vector<unsigned> p32;
  for (u64 k : keys) {
    const u64 p = pack64(box, k, L.sy, L.sz);
    p64.push_back(p);
    CHECK(total >= 64 || (p >> total) == 0, "%s: %llx packs to %llx, wider than %d bits", L.name, k, p, total);
    CHECK(unpack(box, p, L.sy, L.sz) == k, "%s: unpack(pack64(%llx)) = %llx", L.name, k, unpack(box, p, L.sy, L.sz));
    CHECK(p < kInvalid64, "%s: the invalid key is not above pack64(%llx)", L.name, k);
    if (fits32) {
      const unsigned q = pack32(box, k, L.sy, L.sz);
      p32.push_back(q);
      CHECK((u64)q == p, "%s: pack32(%llx) = %x, pack64 = %llx", L.name, k, q, p);
      CHECK(unpack(box, (u64)q, L.sy, L.sz) == k, "%s: unpack(pack32(%llx))", L.name, k);
      if (fits32_invalid) CHECK(q < kInvalid32, "%s: %d bits: pack32(%llx) = %x reaches the invalid key", L.name, total, k, q);
    }
  }
  for (size_t i = 0; i < keys.size(); i++)
    for (size_t j = 0; j < keys.size(); j++) {
      CHECK((keys[i] < keys[j]) == (p64[i] < p64[j]) && (keys[i] == keys[j]) == (p64[i] == p64[j]), "%s: pack64 reorders %llx, %llx", L.name,
            keys[i], keys[j]);
      if (fits32)
        CHECK((keys[i] < keys[j]) == (p32[i] < p32[j]) && (keys[i] == keys[j]) == (p32[i] == p32[j]), "%s: pack32 reorders %llx, %llx",
              L.name, keys[i], keys[j]);
    }
  CHECK(pack64(box, kInvalid64, L.sy, L.sz) == kInvalid64 && unpack(box, kInvalid64, L.sy, L.sz) == kInvalid64, "%s: invalid key, 64 bits",
        L.name);
  if (fits32) CHECK(pack32(box, kInvalid64, L.sy, L.sz) == kInvalid32, "%s: invalid key, 32 bits", L.name);
  // kinfo
  int ki[kInfoStride];
  for (int s = 0; s < kInfoStride; s++) ki[s] = -77;
  store(ki, box);
  CHECK(ki[kInfoBitsTotal] == -77 && ki[kInfoLeft] == -77 && ki[7] == -77, "%s: store() writes slots beyond 4", L.name);
  store_with_total(ki, box);
  CHECK(ki[kInfoBitsTotal] == total && ki[kInfoLeft] == -77 && ki[7] == -77, "%s: store_with_total(): slots 5 - 7", L.name);
  const KeyBox back = load(ki);
  CHECK(ki[0] == mn[0] && ki[1] == mn[1] && ki[2] == mn[2] && ki[3] == box.bits[0] && ki[4] == box.bits[1], "%s: kinfo slots 0 - 4", L.name);
  for (u64 p : p64) CHECK(unpack(back, p, L.sy, L.sz) == unpack(box, p, L.sy, L.sz), "%s: unpack with the box read back from kinfo", L.name);
}

// a box whose widths are exactly b[0..3): ranges 2^b - 1, the largest key packs to all ones of b0 + b1 + b2 bits
static void check_limit(const Layout& L, int b0, int b1, int b2) {
  const int b[3] = {b0, b1, b2};
  int mn[3], mx[3];
  for (int a = 0; a < 3; a++) {
    mn[a] = 5 + a;
    mx[a] = mn[a] + (1 << b[a]) - 1;
  }
  const KeyBox box = box_of(mn, mx);
  const int total = b0 + b1 + b2;
  CHECK(box.total() == total, "%s: limit box of %d bits has %d", L.name, total, box.total());
  const u64 top = pack64(box, join(L, mx), L.sy, L.sz);
  CHECK(top == (1ull << total) - 1, "%s: the largest key of a %d-bit box packs to %llx", L.name, total, top);
  if (total == 31)
    CHECK(box.total() <= kMaxBits32WithInvalid && box.total() <= kMaxBits32 && pack32(box, join(L, mx), L.sy, L.sz) == 0x7fffffffu,
          "%s: 31 bits: a 4-byte key with room for the invalid one", L.name);
  if (total == 32)
    CHECK(box.total() > kMaxBits32WithInvalid && box.total() <= kMaxBits32 && pack32(box, join(L, mx), L.sy, L.sz) == kInvalid32 &&
              pack32(box, join(L, mn), L.sy, L.sz) == 0u,
          "%s: 32 bits: a 4-byte key, the largest one equal to the invalid one", L.name);
  if (total == 33) CHECK(box.total() > kMaxBits32, "%s: 33 bits: no 4-byte key", L.name);
}

int main() {
  static_assert(kInfoMin == 0 && kInfoBitsX == 3 && kInfoBitsY == 4 && kInfoBitsTotal == 5 && kInfoLeft == 6 && kInfoStride == 8,
                "the kinfo layout the kernels and the test hooks rely on");
  static_assert(kMaxBits32WithInvalid == 31 && kMaxBits32 == 32, "the limits of the 4-byte sorts");
  // the width rule on its own: every range up to 2^12, and the three ranges around every power of two a field can reach
  for (int r = 0; r <= 4096; r++) CHECK(nbits(r) == width_by_definition(r), "nbits(%d) = %d", r, nbits(r));
  CHECK(nbits(0) == 1 && nbits(1) == 1 && nbits(2) == 2, "nbits of 0, 1, 2");
  for (int b = 1; b <= 25; b++) {
    CHECK(nbits((1 << b) - 1) == b, "nbits(2^%d - 1) = %d", b, nbits((1 << b) - 1));
    CHECK(nbits(1 << b) == b + 1, "nbits(2^%d) = %d", b, nbits(1 << b));
    CHECK(nbits((1 << b) + 1) == b + 1, "nbits(2^%d + 1) = %d", b, nbits((1 << b) + 1));
  }
  const KeyBox e = empty_box();
  CHECK(e.mn[0] == 0 && e.mn[1] == 0 && e.mn[2] == 0 && e.bits[0] == 1 && e.bits[1] == 1 && e.bits[2] == 1, "empty box");
  for (const Layout& L : kLayouts) {
    for (int trial = 0; trial < 300; trial++) {
      int mn[3], range[3];
      for (int a = 0; a < 3; a++) {
        const int cap = 1 << L.width[a];  // field values are < cap
        const int b = 1 + (int)(rnd() % (L.width[a] - 1));  // 2^b < cap
        const int kind = (int)(rnd() % 5);
        range[a] = kind == 0 ? 0 : kind == 1 ? (1 << b) - 1 : kind == 2 ? (1 << b) : (int)(rnd() % (u64)(1 << b));
        mn[a] = (int)(rnd() % (u64)(cap - range[a]));
        if (trial % 7 == 0) mn[a] = cap - 1 - range[a];  // the box against the top of the field
        if (trial % 11 == 0) mn[a] = 0;
      }
      check_box(L, mn, range, 24);
    }
    {  // one point; the whole field space
      const int mn0[3] = {3, 1, 4}, r0[3] = {0, 0, 0};
      check_box(L, mn0, r0, 4);
      const int z[3] = {0, 0, 0}, full[3] = {(1 << L.width[0]) - 1, (1 << L.width[1]) - 1, (1 << L.width[2]) - 1};
      check_box(L, z, full, 24);
    }
    check_limit(L, 11, 10, 10);  // 31
    check_limit(L, 12, 10, 10);  // 32
    check_limit(L, 12, 11, 10);  // 33
    check_limit(L, 19, 11, 1);   // 31, lopsided
    check_limit(L, 1, 16, 15);   // 32, lopsided
  }
  if (g_bad) {
    printf("FAILED: %d of %ld checks\n", g_bad, g_checked);
    return 1;
  }
  printf("ok: %ld checks\n", g_checked);
  return 0;
}
