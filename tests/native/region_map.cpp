// tests/native/region_map.cpp -- host check of the sub-box decoder's index and
// clip arithmetic (cuzfp_amd/csrc/region.hpp, make_region in launch.hpp), the
// functions the kernel itself calls.  For every array shape up to 9 x 9 x 9
// (1D, 2D and 3D) and every box inside it:
//   - region block r -> (rx, ry, rz) and global block, against / and %;
//   - the stores of all region blocks cover every box element exactly once
//     and nothing else, each at the offset plain signed arithmetic gives
//     (contiguous, and padded negative strides);
//   - for maxbits in {9, 33, 64, 100, 128}: each block's dword index and shift
//     equal b * maxbits in 128-bit arithmetic, every dword that holds a bit of
//     the block is inside the stream, and no load of the copy-in's three forms
//     (register reader, funnel shift, 16-byte) addresses a dword at or past
//     the stream's end.
// Plus shapes whose nblocks * maxbits exceeds 2^40 (and one with more than
// 2^31 blocks).  Prints the number of failures ("0" = pass).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../cuzfp_amd/csrc/launch.hpp"

using namespace cuzfp;
typedef unsigned __int128 u128;

static long failures = 0;
static void fail(const char* what, uint32_t a, uint32_t b, uint32_t c) {
  if (failures++ < 10) fprintf(stderr, "FAIL %s (%u, %u, %u)\n", what, a, b, c);
}

static Geometry geometry(unsigned dims, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t maxbits) {
  Geometry g;
  memset(&g, 0, sizeof g);
  g.nx = nx;
  g.ny = dims > 1 ? ny : 1;
  g.nz = dims > 2 ? nz : 1;
  g.bx = (g.nx + 3) / 4;
  g.by = (g.ny + 3) / 4;
  g.nblocks = (uint32_t)((uint64_t)g.bx * g.by * ((g.nz + 3) / 4));
  g.maxbits = maxbits;
  return g;
}

// The loads of region block b's copy-in (region_kernels.hpp), checked against
// the stream's end.
template <int DIMS>
static void check_bits(const Geometry& g, const Region& r, uint32_t b) {
  uint64_t d0;
  uint32_t s0;
  region_block_bits(b, g.maxbits, d0, s0);
  const u128 bit = (u128)b * g.maxbits;
  if ((u128)d0 != (bit >> 5) || s0 != (uint32_t)(bit & 31)) fail("block bits", b, g.maxbits, 0);
  const u128 end = (((u128)g.nblocks * g.maxbits + 63) / 64) * 2;
  if ((u128)r.stream_dwords != end) fail("stream_dwords", b, g.maxbits, 0);
  // every dword that holds a bit of the block exists (so a dword replaced by
  // zero never held one)
  const uint64_t last = (uint64_t)((bit + g.maxbits - 1) >> 5);
  for (uint64_t d = d0; d <= last; d++)
    if (!region_in_stream(r, d)) fail("block dword past the stream", b, g.maxbits, (uint32_t)(d - d0));
  const uint32_t D = (g.maxbits + 31) >> 5;
  if (DIMS <= 2 && g.maxbits <= 64) {  // the register reader
    const uint64_t a[3] = {d0, region_clamp(r, d0 + 1), region_clamp(r, d0 + 2)};
    for (int i = 0; i < 3; i++)
      if ((u128)a[i] >= end) fail("register load past the stream", b, g.maxbits, i);
    if (last > d0 + 2) fail("register reader: block past three dwords", b, g.maxbits, 0);
  } else if (g.maxbits % 128 == 0) {   // 16-byte loads: dwords d0 .. d0 + D - 1
    if (s0 || (d0 & 3)) fail("16-byte block not aligned", b, g.maxbits, s0);
    if ((u128)d0 + D > end) fail("16-byte load past the stream", b, g.maxbits, 0);
  } else {                             // funnel shift: d0, and d0 + j + 1 where it exists
    if ((u128)d0 >= end) fail("first load past the stream", b, g.maxbits, 0);
    for (uint32_t j = 0; j < D; j++) {
      const uint64_t d = d0 + j + 1;
      if (region_in_stream(r, d) && (u128)d >= end) fail("carry load past the stream", b, g.maxbits, j);
    }
    if (last > d0 + D) fail("funnel shift: block past D + 1 dwords", b, g.maxbits, 0);
  }
}

template <int DIMS>
static void check_box(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t ox, uint32_t oy, uint32_t oz,
                      uint32_t ex, uint32_t ey, uint32_t ez, bool strided, std::vector<uint8_t>& cnt) {
  static const uint32_t kBits[] = {9, 33, 64, 100, 128};
  Geometry g = geometry(DIMS, nx, ny, nz, kBits[0]);
  // padded, negative strides: element (0, 0, 0) is the last of the buffer's used part
  const int64_t px = 2, py = (int64_t)(2 * ex + 1), pz = py * ey + 3;
  const int64_t sx = strided ? -px : 0, sy = strided ? -py : 0, sz = strided ? -pz : 0;
  Region r = make_region(g, ox, oy, oz, ex, ey, ez, sx, sy, sz);
  const int64_t base = strided ? px * (ex - 1) + py * (ey - 1) + pz * (ez - 1) : 0;
  const size_t span = strided ? (size_t)base + 1 : (size_t)ex * ey * ez;
  cnt.assign(span, 0);
  Geometry gm[5];
  Region rm[5];
  for (int k = 0; k < 5; k++) {
    gm[k] = geometry(DIMS, nx, ny, nz, kBits[k]);
    rm[k] = make_region(gm[k], ox, oy, oz, ex, ey, ez, sx, sy, sz);
  }
  const uint32_t bx0 = ox / 4, by0 = oy / 4, bz0 = oz / 4;
  const uint32_t rbx = (ox + ex + 3) / 4 - bx0, rby = (oy + ey + 3) / 4 - by0, rbz = (oz + ez + 3) / 4 - bz0;
  if (r.rbx != rbx || r.rby != rby || r.rbz != rbz || r.nrb != rbx * rby * rbz) fail("region blocks", ox, oy, oz);
  for (uint32_t i = 0; i < r.nrb; i++) {
    const RegionBlock p = region_block<DIMS>(r, i);
    const uint32_t rx = i % rbx, ry = (i / rbx) % rby, rz = i / (rbx * rby);
    const uint32_t b = ((bz0 + rz) * g.by + by0 + ry) * g.bx + bx0 + rx;
    if (p.rx != rx || p.ry != ry || p.rz != rz || p.b != b || b >= g.nblocks) fail("region_block", i, b, 0);
    for (uint32_t z = 0; z < (DIMS > 2 ? 4u : 1u); z++)
      for (uint32_t y = 0; y < (DIMS > 1 ? 4u : 1u); y++)
        for (uint32_t x = 0; x < 4; x++) {
          const long gx = 4L * (bx0 + rx) + x, gy = 4L * (by0 + ry) + y, gz = 4L * (bz0 + rz) + z;
          const bool in = gx >= (long)ox && gx < (long)ox + ex && gy >= (long)oy && gy < (long)oy + ey &&
                          gz >= (long)oz && gz < (long)oz + ez;
          int64_t off;
          if (region_out_offset(r, p, x, y, z, off) != in) { fail("clip", i, x + 4 * y + 16 * z, 0); continue; }
          if (!in) continue;
          const int64_t want = (gx - ox) * r.sx + (gy - oy) * r.sy + (gz - oz) * r.sz;
          if (off != want || base + off < 0 || (size_t)(base + off) >= span) { fail("offset", i, x, y); continue; }
          cnt[(size_t)(base + off)]++;
        }
    for (int k = 0; k < 5; k++) check_bits<DIMS>(gm[k], rm[k], p.b);
  }
  // every box element exactly once, nothing else
  size_t ones = 0;
  for (uint32_t z = 0; z < ez; z++)
    for (uint32_t y = 0; y < ey; y++)
      for (uint32_t x = 0; x < ex; x++) ones += cnt[(size_t)(base + x * r.sx + y * r.sy + z * r.sz)] == 1;
  size_t total = 0;
  for (uint8_t c : cnt) total += c;
  if (ones != (size_t)ex * ey * ez || total != ones) fail("coverage", ox, oy, oz);
}

template <int DIMS>
static void check_shape(uint32_t nx, uint32_t ny, uint32_t nz, std::vector<uint8_t>& cnt) {
  const bool strided = (nx + ny + nz) & 1;
  for (uint32_t oz = 0; oz < nz; oz++)
    for (uint32_t ez = 1; oz + ez <= nz; ez++)
      for (uint32_t oy = 0; oy < ny; oy++)
        for (uint32_t ey = 1; oy + ey <= ny; ey++)
          for (uint32_t ox = 0; ox < nx; ox++)
            for (uint32_t ex = 1; ox + ex <= nx; ex++) check_box<DIMS>(nx, ny, nz, ox, oy, oz, ex, ey, ez, strided, cnt);
}

// A box of a large array: block indices and bit offsets only (no coverage).
template <int DIMS>
static void check_large(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t maxbits, uint32_t ox, uint32_t oy,
                        uint32_t oz, uint32_t ex, uint32_t ey, uint32_t ez) {
  const Geometry g = geometry(DIMS, nx, ny, nz, maxbits);
  const Region r = make_region(g, ox, oy, oz, ex, ey, ez, 0, 0, 0);
  if ((u128)g.nblocks * maxbits <= ((u128)1 << 40)) fail("large shape is not large", nx, ny, nz);
  for (uint32_t i = 0; i < r.nrb; i++) {
    const RegionBlock p = region_block<DIMS>(r, i);
    const uint32_t rx = i % r.rbx, ry = (i / r.rbx) % r.rby, rz = i / (r.rbx * r.rby);
    const u128 b = ((u128)(r.bz0 + rz) * g.by + r.by0 + ry) * g.bx + r.bx0 + rx;
    if (p.rx != rx || p.ry != ry || p.rz != rz || (u128)p.b != b || b >= g.nblocks) fail("large region_block", i, p.b, 0);
    check_bits<DIMS>(g, r, p.b);
  }
}

int main() {
  std::vector<uint8_t> cnt;
  for (uint32_t nx = 1; nx <= 9; nx++) {
    check_shape<1>(nx, 1, 1, cnt);
    for (uint32_t ny = 1; ny <= 9; ny++) {
      check_shape<2>(nx, ny, 1, cnt);
      for (uint32_t nz = 1; nz <= 9; nz++) check_shape<3>(nx, ny, nz, cnt);
    }
  }
  // nblocks * maxbits = 2^42 (1D), 2^42 (3D, 2^30 blocks), and a 3D array of
  // 3.375e9 blocks (> 2^31) at 16384 bits: the far corner with the stream's
  // last block, and a box inside
  check_large<1>(1u << 30, 1, 1, 16384, (1u << 30) - 1000, 0, 0, 1000, 1, 1);
  check_large<1>(1u << 30, 1, 1, 16383, 12345, 0, 0, 1001, 1, 1);
  check_large<3>(4096, 4096, 4096, 4096, 4090, 4085, 4079, 6, 11, 17);
  check_large<3>(4096, 4096, 4096, 1100, 1001, 2002, 3003, 9, 9, 9);
  check_large<3>(6000, 6000, 6000, 16384, 5990, 5989, 5988, 10, 11, 12);
  check_large<3>(6000, 6000, 6000, 1033, 2999, 3001, 5000, 13, 6, 7);
  check_large<2>(1u << 17, 1u << 17, 1, 4099, (1u << 17) - 9, (1u << 17) - 5, 0, 9, 5, 1);
  printf("%ld\n", failures);
  return failures ? 1 : 0;
}
