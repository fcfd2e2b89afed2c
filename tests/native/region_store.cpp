// tests/native/region_store.cpp -- host check of the sub-box encoder's store
// spans (region_span in cuzfp_amd/csrc/region.hpp), the function the kernel's
// copy-out calls.  For every maxbits in 1..200 and 511, 512, 513, 1024, 16384,
// block counts whose nblocks * maxbits is and is not a multiple of 64, and
// blocks that include index 0, the array's last block and blocks past bit
// 2^32 of the stream:
//   - the head mask, the whole dwords and the tail mask cover exactly the
//     block's bits [b * maxbits, (b + 1) * maxbits), in 128-bit arithmetic;
//   - they share no bit with the spans of the blocks before and after;
//   - they name no dword at or past stream_dwords (make_region's).
// Prints the number of failures ("0" = pass).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../cuzfp_amd/csrc/launch.hpp"

using namespace cuzfp;
typedef unsigned __int128 u128;

static long failures = 0;
static void fail(const char* what, uint32_t b, uint32_t maxbits, uint32_t nblocks) {
  if (failures++ < 10) fprintf(stderr, "FAIL %s (block %u, maxbits %u, nblocks %u)\n", what, b, maxbits, nblocks);
}

// bits of the stream a span names: [lo, hi) per piece, in 128-bit arithmetic
struct Piece {
  u128 lo, hi;
};

static std::vector<Piece> pieces(const RegionSpan& s) {
  std::vector<Piece> v;
  auto masked = [&](uint64_t dword, uint32_t mask) {
    // the masks are runs of ones: [ctz, 32 - clz)
    const u128 base = (u128)dword * 32;
    v.push_back(Piece{base + (unsigned)__builtin_ctz(mask), base + 32u - (unsigned)__builtin_clz(mask)});
  };
  if (s.head_mask) masked(s.head, s.head_mask);
  if (s.nwhole) v.push_back(Piece{(u128)s.whole * 32, ((u128)s.whole + s.nwhole) * 32});
  if (s.tail_mask) masked(s.tail, s.tail_mask);
  return v;
}

static bool run_of_ones(uint32_t m) {
  if (!m) return true;
  const uint32_t x = m >> __builtin_ctz(m);
  return (x & (x + 1)) == 0;
}

static void check_block(uint32_t b, uint32_t maxbits, uint32_t nblocks, uint64_t stream_dwords) {
  const RegionSpan s = region_span(b, maxbits);
  const u128 lo = (u128)b * maxbits, hi = lo + maxbits;
  if (!run_of_ones(s.head_mask) || !run_of_ones(s.tail_mask)) fail("mask shape", b, maxbits, nblocks);
  // exactly the block's bits, in order and without gaps
  const std::vector<Piece> v = pieces(s);
  u128 at = lo;
  for (const Piece& p : v) {
    if (p.lo != at || p.hi <= p.lo) fail("cover", b, maxbits, nblocks);
    at = p.hi;
  }
  if (v.empty() || at != hi) fail("cover end", b, maxbits, nblocks);
  // the pieces' order in the stream: head, whole, tail
  if (s.head_mask && s.nwhole && s.whole != s.head + 1) fail("whole after head", b, maxbits, nblocks);
  if (s.tail_mask && s.nwhole && s.tail != s.whole + s.nwhole) fail("tail after whole", b, maxbits, nblocks);
  // a whole dword is the block's alone: both neighbours' spans stay out of it
  // (and out of the masked bits), i.e. the spans are disjoint
  for (int side = -1; side <= 1; side += 2) {
    if ((side < 0 && b == 0) || (side > 0 && b + 1 >= nblocks)) continue;
    for (const Piece& q : pieces(region_span(b + side, maxbits)))
      for (const Piece& p : v)
        if (q.lo < p.hi && p.lo < q.hi) fail("overlap", b, maxbits, nblocks);
  }
  // nothing at or past the stream's end
  if (s.head_mask && s.head >= stream_dwords) fail("head past end", b, maxbits, nblocks);
  if (s.nwhole && s.whole + s.nwhole > stream_dwords) fail("whole past end", b, maxbits, nblocks);
  if (s.tail_mask && s.tail >= stream_dwords) fail("tail past end", b, maxbits, nblocks);
  // the first dword and shift are region_block_bits'
  uint64_t d0;
  uint32_t s0;
  region_block_bits(b, maxbits, d0, s0);
  if (s.head != d0 || (u128)d0 * 32 + s0 != lo) fail("first dword", b, maxbits, nblocks);
  if ((s0 != 0) != (s.head_mask != 0)) fail("head iff unaligned", b, maxbits, nblocks);
}

static void check_stream(uint32_t nblocks, uint32_t maxbits) {
  // a 1D array of nblocks blocks: stream_dwords as the launcher computes it
  Geometry g;
  memset(&g, 0, sizeof g);
  g.nx = 4;  // (make_region reads the block counts only)
  g.ny = g.nz = 1;
  g.bx = nblocks;
  g.by = 1;
  g.nblocks = nblocks;
  g.maxbits = maxbits;
  const Region r = make_region(g, 0, 0, 0, 1, 1, 1, 0, 0, 0);
  if ((u128)r.stream_dwords * 32 < (u128)nblocks * maxbits || r.stream_dwords % 2)
    fail("stream_dwords", 0, maxbits, nblocks);
  // blocks: the first ones, the last ones, and those around bit 2^32 and 2^33
  std::vector<uint32_t> bs;
  for (uint32_t b = 0; b < 70 && b < nblocks; b++) bs.push_back(b);
  for (uint32_t b = nblocks > 70 ? nblocks - 70 : 0; b < nblocks; b++) bs.push_back(b);
  for (int k = 32; k <= 33; k++) {
    const uint64_t mid = (1ull << k) / maxbits;
    for (uint64_t b = mid > 3 ? mid - 3 : 0; b < mid + 4 && b < nblocks; b++) bs.push_back((uint32_t)b);
  }
  for (uint32_t b : bs) check_block(b, maxbits, nblocks, r.stream_dwords);
}

int main() {
  std::vector<uint32_t> mbs;
  for (uint32_t mb = 1; mb <= 200; mb++) mbs.push_back(mb);
  for (uint32_t mb : {511u, 512u, 513u, 1024u, 16384u}) mbs.push_back(mb);
  long with64 = 0, without64 = 0, past32 = 0;
  for (uint32_t mb : mbs) {
    // small streams, and streams that pass bit 2^32 (2^33 / maxbits blocks and a few more)
    // (at most 2^32 - 65 blocks, make_problem's bound)
    const uint64_t most = (1ull << 32) - 65 - 64;
    const uint32_t big = (uint32_t)((1ull << 33) / mb < most ? (1ull << 33) / mb : most);
    for (uint32_t nblocks : {1u, 2u, 3u, 63u, 64u, 65u, 301u, big + 1u, big + 6u, big + 64u}) {
      ((uint64_t)nblocks * mb % 64 ? without64 : with64)++;
      if ((uint64_t)nblocks * mb > (1ull << 32)) past32++;
      check_stream(nblocks, mb);
    }
  }
  // the coverage the header promises
  if (!with64 || !without64 || !past32) fail("coverage", 0, 0, 0);
  printf("%ld\n", failures);
  return failures != 0;
}
