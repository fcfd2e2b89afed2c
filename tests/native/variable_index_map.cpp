// tests/native/variable_index_map.cpp -- host check of the variable-rate offset
// index and the sub-box decoder's addressing (cuzfp_amd/csrc/variable_index.hpp,
// region.hpp, make_region in launch.hpp), the functions the kernel itself
// calls.
//   - For every block count 1 .. 200 and several seeded fillings of `lengths`
//     (random, all 65535, all 1, all 0): the index built by the format's rule
//     and variable_block_offset give every block the 64-bit running sum; the
//     loads, seen through recording views, touch no length at or past the
//     block itself (so none at or past nblocks) and no index entry at or past T.
//   - For every array shape up to 9 x 9 x 9 (1D, 2D and 3D) and every box
//     inside it: region_block visits each block of the box exactly once and
//     nothing else, and the loads of each one's offset stay inside
//     lengths[0 .. nblocks) and index[0 .. T).
//   - With hostile contents -- all ones, offsets past the stream, offsets near
//     2^64, random bits -- in both arrays: for each type and dimension, the
//     budget never exceeds the type's longest block (the LDS column), and every
//     stream dword the copy-in rule loads (variable_stream_dword, dwords 0 ..
//     Dl of the block) is below stream_dwords, its index formed without
//     wrapping (checked in 128-bit arithmetic).
// Prints the number of failures ("0" = pass).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cuzfp_amd/csrc/launch.hpp"
#include "../../cuzfp_amd/csrc/variable_index.hpp"
#include "../../cuzfp_amd/csrc/zfp_block.hpp"

using namespace cuzfp;
typedef unsigned __int128 u128;

static long failures = 0;
static void fail(const char* what, uint64_t a, uint64_t b, uint64_t c) {
  if (failures++ < 10) fprintf(stderr, "FAIL %s (%llu, %llu, %llu)\n", what, (unsigned long long)a,
                               (unsigned long long)b, (unsigned long long)c);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// An array seen through operator[], recording the largest element read.
template <typename T>
struct View {
  const T* p;
  mutable int64_t hi = -1;
  T operator[](uint64_t i) const {
    if ((int64_t)i > hi) hi = (int64_t)i;
    return p[i];
  }
};

// the format's rule (include/cuzfp_hip.h): index[t] = sum of lengths[0 .. 64 t), index[T] = the total
static std::vector<uint64_t> build_index(const std::vector<uint16_t>& len) {
  const uint32_t n = (uint32_t)len.size(), T = variable_index_tiles(n);
  std::vector<uint64_t> idx(T + 1);
  uint64_t sum = 0;
  for (uint32_t b = 0; b < n; b++) {
    if (b % 64 == 0) idx[b / 64] = sum;
    sum += len[b];
  }
  idx[T] = sum;
  return idx;
}

// the loads of block b's offset: its value against `want`, and their range
static void check_offset(const std::vector<uint64_t>& idx, const std::vector<uint16_t>& len, uint32_t b,
                         uint64_t want, bool compare) {
  const uint32_t n = (uint32_t)len.size(), T = variable_index_tiles(n);
  View<uint64_t> vi{idx.data()};
  View<uint16_t> vl{len.data()};
  const uint64_t got = variable_block_offset(vi, vl, b);
  if (compare && got != want) fail("offset", n, b, got);
  if (vl.hi >= (int64_t)b || vl.hi >= (int64_t)n) fail("length load at or past the block", n, b, (uint64_t)vl.hi);
  if (vi.hi < 0 || vi.hi >= (int64_t)T) fail("index load at or past T", n, b, (uint64_t)vi.hi);
  // the pointers themselves, as the kernel passes them
  if (variable_block_offset(idx.data(), len.data(), b) != got) fail("pointer form differs", n, b, 0);
}

static void check_counts() {
  for (uint32_t n = 1; n <= 200; n++) {
    if (variable_index_tiles(n) != (n + 63) / 64) fail("tiles", n, 0, 0);
    for (int fill = 0; fill < 6; fill++) {
      std::vector<uint16_t> len(n);
      for (uint32_t b = 0; b < n; b++)
        len[b] = fill == 0 ? 65535 : fill == 1 ? 1 : fill == 2 ? 0 : fill == 3 ? (uint16_t)(rnd() % 4172)
                                                                              : (uint16_t)rnd();
      const std::vector<uint64_t> idx = build_index(len);
      uint64_t sum = 0;
      for (uint32_t b = 0; b < n; b++) {
        check_offset(idx, len, b, sum, true);
        sum += len[b];
      }
      if (idx[variable_index_tiles(n)] != sum) fail("total", n, fill, 0);
    }
  }
  // a tile of 65535s far into a long stream: the in-tile sum stays exact beside a large entry
  {
    std::vector<uint16_t> len(64 * 3, 65535);
    std::vector<uint64_t> idx = build_index(len);
    for (uint64_t& v : idx) v += (1ull << 40) + 12345;
    for (uint32_t b = 0; b < len.size(); b++) check_offset(idx, len, b, (1ull << 40) + 12345 + 65535ull * b, true);
  }
}

static Geometry geometry(unsigned dims, uint32_t nx, uint32_t ny, uint32_t nz) {
  Geometry g;
  memset(&g, 0, sizeof g);
  g.nx = nx;
  g.ny = dims > 1 ? ny : 1;
  g.nz = dims > 2 ? nz : 1;
  g.bx = (g.nx + 3) / 4;
  g.by = (g.ny + 3) / 4;
  g.nblocks = (uint32_t)((uint64_t)g.bx * g.by * ((g.nz + 3) / 4));
  g.maxbits = 64;
  return g;
}

template <int DIMS>
static void check_shape(uint32_t nx, uint32_t ny, uint32_t nz) {
  const Geometry g = geometry(DIMS, nx, ny, nz);
  std::vector<uint16_t> len(g.nblocks);
  for (uint16_t& l : len) l = (uint16_t)rnd();
  const std::vector<uint64_t> idx = build_index(len);
  std::vector<uint64_t> want(g.nblocks);
  uint64_t sum = 0;
  for (uint32_t b = 0; b < g.nblocks; b++) {
    want[b] = sum;
    sum += len[b];
  }
  std::vector<uint8_t> cnt(g.nblocks);
  for (uint32_t oz = 0; oz < g.nz; oz++)
    for (uint32_t ez = 1; oz + ez <= g.nz; ez++)
      for (uint32_t oy = 0; oy < g.ny; oy++)
        for (uint32_t ey = 1; oy + ey <= g.ny; ey++)
          for (uint32_t ox = 0; ox < g.nx; ox++)
            for (uint32_t ex = 1; ox + ex <= g.nx; ex++) {
              const Region r = make_region(g, ox, oy, oz, ex, ey, ez, 0, 0, 0);
              cnt.assign(g.nblocks, 0);
              for (uint32_t i = 0; i < r.nrb; i++) {
                const uint32_t b = region_block<DIMS>(r, i).b;
                if (b >= g.nblocks) {
                  fail("region block past the array", i, b, g.nblocks);
                  continue;
                }
                cnt[b]++;
                check_offset(idx, len, b, want[b], true);
              }
              // exactly the blocks the box touches, once each
              for (uint32_t b = 0; b < g.nblocks; b++) {
                const uint32_t ix = b % g.bx, iy = (b / g.bx) % g.by, iz = b / (g.bx * g.by);
                const bool in = 4 * ix + 3 >= ox && 4 * ix < ox + ex && 4 * iy + 3 >= oy && 4 * iy < oy + ey &&
                                4 * iz + 3 >= oz && 4 * iz < oz + ez;
                if (cnt[b] != (in ? 1 : 0)) fail("coverage", b, ox + 16 * oy + 256 * oz, ex + 16 * ey + 256 * ez);
              }
            }
}

// The copy-in of one block (region_variable_kernels.hpp, variable_kernels.hpp)
// from an offset and a raw length that nothing vouches for.
template <typename Scalar, int DIMS>
static void check_copy_in(uint64_t off, uint32_t raw, uint64_t stream_dwords) {
  constexpr uint32_t kMaxLen = max_block_bits<Scalar, DIMS>(traits<Scalar>::prec);
  constexpr uint32_t D = (kMaxLen + 31) / 32;
  const uint32_t len = variable_budget(raw, kMaxLen, traits<Scalar>::ebits);
  if (len > kMaxLen || (len && len < traits<Scalar>::ebits + 2u) || len > raw) fail("budget", raw, len, kMaxLen);
  const uint32_t Dl = (len + 31) >> 5;
  if (Dl > D) fail("column overflow", raw, Dl, D);
  for (uint32_t j = 0; j <= Dl; j++) {
    if (!Dl) break;  // a zero block loads nothing
    uint64_t d = 0;
    const bool in = variable_stream_dword(off, j, stream_dwords, d);
    const u128 exact = (u128)(off >> 5) + j;
    if ((u128)d != exact) fail("dword index wrapped", off, j, d);
    if (in != (exact < (u128)stream_dwords)) fail("bound test", off, j, stream_dwords);
    if (in && d >= stream_dwords) fail("load past the stream", off, j, d);
  }
}

template <typename Scalar, int DIMS>
static void check_hostile_type() {
  static const uint64_t kStreams[] = {0, 1, 2, 3, 131, 132, 133, 1000, 1ull << 27, (1ull << 32) + 6};
  static const uint32_t kRaw[] = {0, 1, 2, 9, 10, 12, 13, 14, 31, 32, 33, 1000, 4170, 4171, 4172, 32767, 65535};
  const uint32_t n = 200;
  for (uint64_t sd : kStreams)
    for (int fill = 0; fill < 5; fill++) {
      std::vector<uint16_t> len(n);
      std::vector<uint64_t> idx(variable_index_tiles(n) + 1);
      for (uint16_t& l : len) l = fill == 0 ? 65535 : fill == 4 ? kRaw[rnd() % 17] : (uint16_t)rnd();
      for (uint64_t& v : idx)
        v = fill == 0   ? ~0ull                           // all ones
            : fill == 1 ? 32 * sd + rnd() % 100000        // past the stream
            : fill == 2 ? ~0ull - rnd() % (64 * 65535)    // near 2^64: the in-tile sum wraps
            : fill == 3 ? rnd()
                        : 32 * sd - rnd() % (32 * sd + 1);  // around the stream's end
      for (uint32_t b = 0; b < n; b++) {
        check_offset(idx, len, b, 0, false);
        check_copy_in<Scalar, DIMS>(variable_block_offset(idx.data(), len.data(), b), len[b], sd);
      }
    }
  // every offset around the end of a small stream, every raw length
  for (uint64_t sd : {1ull, 2ull, 131ull, 140ull})
    for (uint64_t off = 32 * sd > 5000 ? 32 * sd - 5000 : 0; off < 32 * sd + 70; off++)
      for (uint32_t raw : kRaw) check_copy_in<Scalar, DIMS>(off, raw, sd);
  for (uint64_t k = 0; k < 5000; k++)
    for (uint32_t raw : kRaw) check_copy_in<Scalar, DIMS>(~0ull - k, raw, 1ull << 20);
}

int main() {
  check_counts();
  for (uint32_t nx = 1; nx <= 9; nx++) {
    check_shape<1>(nx, 1, 1);
    for (uint32_t ny = 1; ny <= 9; ny++) {
      check_shape<2>(nx, ny, 1);
      for (uint32_t nz = 1; nz <= 9; nz++) check_shape<3>(nx, ny, nz);
    }
  }
  // more than one tile under a box: runs that straddle tiles
  check_shape<1>(300, 1, 1);
  check_shape<2>(37, 30, 1);
  check_hostile_type<float, 1>();
  check_hostile_type<float, 2>();
  check_hostile_type<float, 3>();
  check_hostile_type<double, 1>();
  check_hostile_type<double, 2>();
  check_hostile_type<double, 3>();
  printf("%ld\n", failures);
  return failures ? 1 : 0;
}
