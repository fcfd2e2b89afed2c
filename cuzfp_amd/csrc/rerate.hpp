// cuzfp_amd/csrc/rerate.hpp -- position arithmetic of cuzfp_hip_truncate, for
// host and device: the kernels (truncate.hip) and tests/native/rerate_map.cpp
// form every output word through the same functions.
//
// zfp's coder is embedded: a block coded with a budget of m bits is the first
// m bits of the same block coded with any larger budget M.  A stream at M bits
// a block therefore becomes the stream at m <= M by keeping bits
// [b*M, b*M + m) of every block b and packing them m apart:
//   output bit b*m + i (i < m)  =  source bit b*M + i,
// zero from nblocks*m up to the end of the last 64-bit word.  All positions
// are 64-bit: nblocks * M reaches 2^46.
#pragma once
#include <stdint.h>

#include "region.hpp"

namespace cuzfp {

// Word path (M and m both multiples of 64 bits, or both of 128 with `unit`s of
// 16 bytes): mu and Mu units a block, output unit i is source unit
// (i / mu) * Mu + i % mu.  Idx: uint32_t when the source's unit count is below
// 2^31 (the launcher's choice), else uint64_t.
template <typename Idx>
CUZFP_HD Idx rerate_unit_src(Idx i, uint32_t mu, uint32_t Mu) {
  const Idx b = i / (Idx)mu;
  return b * (Idx)Mu + (i - b * (Idx)mu);
}

// General path.  Output word w covers output bits [64w, 64w + 64): its first
// bit is bit `off` of block `b`.
CUZFP_HD void rerate_word_first(uint64_t w, uint32_t m, uint64_t& b, uint32_t& off) {
  const uint64_t bit = w << 6;  // w < 2^40
  if (!(bit >> 32)) {
    const uint32_t q = (uint32_t)bit / m;
    b = q;
    off = (uint32_t)bit - q * m;
  } else {
    b = bit / m;
    off = (uint32_t)(bit - b * m);
  }
}

// Bit `off` of block b of the source: bit `shift` of source dword `dword`.
CUZFP_HD void rerate_segment_src(uint64_t b, uint32_t off, uint32_t M, uint64_t& dword, uint32_t& shift) {
  const uint64_t bit = b * M + off;
  dword = bit >> 5;
  shift = (uint32_t)bit & 31u;
}

// bits [s, s + 32) of hi:lo, s < 32 (v_alignbit_b32 on the device)
CUZFP_HD uint32_t rerate_funnel(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u));
#endif
}

CUZFP_HD uint64_t rerate_lowmask(uint32_t n) {  // n in 1..64
  return ~0ull >> (64u - n);
}

// Output word w of the stream at m bits a block, from the source at M >= m
// bits a block with `nblocks` blocks.  The word is met by at most
// ceil(64 / m) + 1 blocks; each contributes a segment of up to 64 bits, fetched
// as three dwords from (dword, shift) on.  load(d) gives source dword d, or
// zero when d lies at or past the source's end (only the two carry dwords of a
// segment can: the first one holds a bit of the block's prefix).  Blocks at or
// past nblocks contribute nothing, so the last word's padding comes out zero.
template <typename Load>
CUZFP_HD uint64_t rerate_word(uint64_t w, uint32_t nblocks, uint32_t M, uint32_t m, Load load) {
  uint64_t b;
  uint32_t off;
  rerate_word_first(w, m, b, off);
  uint64_t out = 0;
  uint32_t filled = 0;
  while (filled < 64 && b < nblocks) {
    const uint32_t len = m - off < 64 - filled ? m - off : 64 - filled;
    uint64_t d;
    uint32_t s;
    rerate_segment_src(b, off, M, d, s);
    const uint32_t a0 = load(d), a1 = load(d + 1), a2 = load(d + 2);
    const uint64_t v = ((uint64_t)rerate_funnel(a1, a0, s) | ((uint64_t)rerate_funnel(a2, a1, s) << 32)) &
                       rerate_lowmask(len);
    out |= v << filled;
    filled += len;
    off += len;
    if (off == m) {
      off = 0;
      b++;
    }
  }
  return out;
}

}  // namespace cuzfp
