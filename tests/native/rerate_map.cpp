// tests/native/rerate_map.cpp -- host check of cuzfp_hip_truncate's position
// arithmetic (cuzfp_amd/csrc/rerate.hpp), the functions the kernels of
// truncate.hip call.  A random source bit string of nblocks blocks M bits
// apart is cut down to m bits a block twice: every output word through
// rerate_word (general path) or rerate_unit_src (word path, 8- and 16-byte
// units), and bit by bit from the definition
//   output bit b*m + i = source bit b*M + i (i < m), zero past nblocks*m.
// Every 1 <= m <= M <= 130 with 1..70 blocks, and a few large pairs.  Source
// dwords at or past the source's end are missing: the loader returns zero for
// them (the source's bits are random, so a prefix bit asked of one shows), and
// none is asked for beyond the two carry dwords after the last one.
// Then spot checks of the index functions at word indices around 2^26 and
// 2^40 against 128-bit arithmetic.  Prints the number of failures ("0" = pass).
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "../../cuzfp_amd/csrc/launch.hpp"
#include "../../cuzfp_amd/csrc/rerate.hpp"

using namespace cuzfp;
typedef unsigned __int128 u128;

static long failures = 0;
static void fail(const char* what, uint64_t w, uint32_t M, uint32_t m, uint32_t nblocks) {
  if (failures++ < 10)
    fprintf(stderr, "FAIL %s (word %llu, M %u, m %u, nblocks %u)\n", what, (unsigned long long)w, M, m, nblocks);
}

static std::mt19937_64 rng(20260);

static void check_pair(uint32_t nblocks, uint32_t M, uint32_t m) {
  const uint64_t src_words = ((uint64_t)nblocks * M + 63) / 64, out_words = ((uint64_t)nblocks * m + 63) / 64;
  // every bit of the source random, the padding of its last word included
  std::vector<uint64_t> src(src_words);
  for (uint64_t& v : src) v = rng();
  const uint64_t src_dwords = 2 * src_words;
  auto src_bit = [&](uint64_t i) { return (src[i >> 6] >> (i & 63)) & 1; };
  // bit at a time
  std::vector<uint64_t> want(out_words, 0);
  for (uint32_t b = 0; b < nblocks; b++)
    for (uint32_t i = 0; i < m; i++) {
      const uint64_t o = (uint64_t)b * m + i;
      want[o >> 6] |= src_bit((uint64_t)b * M + i) << (o & 63);
    }
  // general path
  uint64_t farthest = 0;
  auto load = [&](uint64_t d) -> uint32_t {
    if (d >= src_dwords) {
      if (d > farthest) farthest = d;
      return 0u;
    }
    return (uint32_t)(src[d >> 1] >> (32 * (d & 1)));
  };
  for (uint64_t w = 0; w < out_words; w++) {
    if (rerate_word(w, nblocks, M, m, load) != want[w]) fail("rerate_word", w, M, m, nblocks);
    uint64_t b;
    uint32_t off;
    rerate_word_first(w, m, b, off);
    if ((u128)b * m + off != (u128)w * 64 || off >= m) fail("rerate_word_first", w, M, m, nblocks);
  }
  // only the two carry dwords of a segment can lie past the end
  if (farthest > src_dwords + 1) fail("load far past the end", farthest, M, m, nblocks);
  // word path: 8-byte units, 16-byte units, 32- and 64-bit indices
  if (!((M | m) & 63)) {
    for (uint64_t w = 0; w < out_words; w++) {
      const uint64_t s64 = rerate_unit_src<uint64_t>(w, m / 64, M / 64);
      const uint32_t s32 = rerate_unit_src<uint32_t>((uint32_t)w, m / 64, M / 64);
      if (s64 >= src_words || s32 != s64 || src[s64] != want[w]) fail("rerate_unit_src 8", w, M, m, nblocks);
    }
  }
  if (!((M | m) & 127)) {
    for (uint64_t q = 0; q < out_words / 2; q++) {
      const uint64_t s = rerate_unit_src<uint64_t>(q, m / 128, M / 128);
      if (2 * s + 1 >= src_words || src[2 * s] != want[2 * q] || src[2 * s + 1] != want[2 * q + 1])
        fail("rerate_unit_src 16", q, M, m, nblocks);
    }
  }
}

// the index functions far into a stream, against 128-bit arithmetic
static void check_far(uint64_t w, uint32_t M, uint32_t m) {
  uint64_t b;
  uint32_t off;
  rerate_word_first(w, m, b, off);
  if ((u128)b * m + off != (u128)w * 64 || off >= m) fail("far rerate_word_first", w, M, m, 0);
  uint64_t d;
  uint32_t s;
  rerate_segment_src(b, off, M, d, s);
  if ((u128)d * 32 + s != (u128)b * M + off || s >= 32) fail("far rerate_segment_src", w, M, m, 0);
  if (!((M | m) & 63)) {
    const uint32_t mu = m / 64, Mu = M / 64;
    const uint64_t src = rerate_unit_src<uint64_t>(w, mu, Mu);
    if ((u128)src != (u128)(w / mu) * Mu + w % mu) fail("far rerate_unit_src", w, M, m, 0);
    if ((w / mu + 1) * (uint64_t)Mu < (1ull << 31) &&
        rerate_unit_src<uint32_t>((uint32_t)w, mu, Mu) != src)
      fail("far rerate_unit_src 32", w, M, m, 0);
  }
}

int main() {
  for (uint32_t M = 1; M <= 130; M++)
    for (uint32_t m = 1; m <= M; m++)
      for (uint32_t nblocks = 1; nblocks <= 70; nblocks++) check_pair(nblocks, M, m);
  const uint32_t big[][2] = {{16384, 16383}, {4171, 4170}, {16384, 8192}, {1280, 512}, {2048, 1920}, {512, 256}};
  for (const auto& p : big)
    for (uint32_t nblocks : {1u, 2u, 3u, 63u, 64u, 67u}) check_pair(nblocks, p[0], p[1]);
  // the funnel shift and the mask
  if (rerate_funnel(0x89abcdefu, 0x01234567u, 0) != 0x01234567u || rerate_funnel(0x89abcdefu, 0x01234567u, 4) != 0xf0123456u ||
      rerate_funnel(0x89abcdefu, 0x01234567u, 31) != 0x13579bdeu)
    fail("rerate_funnel", 0, 0, 0, 0);
  if (rerate_lowmask(1) != 1 || rerate_lowmask(63) != ~0ull >> 1 || rerate_lowmask(64) != ~0ull)
    fail("rerate_lowmask", 0, 0, 0, 0);
  const uint32_t far[][2] = {{16384, 16383}, {16384, 8192}, {16384, 9},   {4171, 4170}, {512, 256},
                             {1280, 128},    {100, 33},     {65, 64},     {33, 1},      {130, 129}};
  for (const auto& p : far)
    for (uint64_t centre : {1ull << 26, 1ull << 40})
      for (uint64_t w = centre - 70; w < centre + 70; w++) {
        // an output of at most 2^46 bits: w < 2^40
        if (w < (1ull << 40)) check_far(w, p[0], p[1]);
      }
  printf("%ld\n", failures);
  return failures != 0;
}
