// cuzfp_amd/csrc/rerate_variable.hpp -- the per-block arithmetic of
// cuzfp_hip_truncate_variable, for host and device: the kernels
// (truncate_variable.hip) and tests/native/variable_truncate_emulate.cpp find
// every block's new length through the same function.
//
// A mode is (maxprec, minexp).  A block coded in a variable-rate mode is the
// first L bits of the same block coded without a budget (zfp_block.hpp,
// block_length), L ending after plane intprec - p, p = precision_variable(emax,
// maxprec, minexp).  At a mode (maxprec', minexp') with maxprec' <= maxprec and
// minexp' >= minexp, p' <= p for every exponent, so the block at the coarser
// mode is the first L' <= L bits of the block at the finer one -- with one
// exception: p' == 0 codes the block in the one-bit form, the single bit 0,
// while the finer block starts with the non-zero flag 1.
//
// L' = 1 + ebits + the bits of the first p' coded planes.  It is found by
// walking the plane code and moving only the cursor: per plane, the n verbatim
// bits, then group tests -- a 1 followed by the run up to and including the
// next 1 (the one at position N - 1 is implied), until a 0 test or n == N; n
// carries over to the next plane.  plane_bits (zfp_block.hpp) states the same
// grammar from the encoder's side.  Nothing is deposited, transposed or
// converted.
#pragma once
#include <stdint.h>

#include "zfp_block.hpp"

namespace cuzfp {

// The longest block of the type and the shortest coded one: a source length is
// clamped to the first, and one below the second (other than the zero block's
// 1) is no block's length and reads as a zero block -- the decoder's rule
// (variable_kernels.hpp, zfp_decode_variable_body).
template <typename Scalar, int DIMS>
ZFP_HD constexpr unsigned variable_longest_block() {
  return max_block_bits<Scalar, DIMS>(traits<Scalar>::prec);
}

// Bits [0, pos') of a block whose plane code starts at bit `head`: pos' is the
// end of the first `planes` >= 1 coded planes, or `limit` if the code runs to
// or past it first.  rd.window(pos) gives the block's bits [pos, pos + 64)
// (what lies past the block is never used: the walk ends at `limit`); `w0` is
// rd.window(0), which the caller has read.
//
// One loop, one group test a trip, whichever plane the test belongs to: on the
// device the lanes of a wave then wait for each other once, at the end, not at
// the end of every plane.  A trip that ends its plane (a 0 test, or n == N)
// also skips the next plane's n verbatim bits; once n == N every further plane
// is N verbatim bits, and the walk ends in closed form.  Every trip moves the
// cursor by at least one bit towards `limit`, so arbitrary bits end the walk
// within `limit` trips.
template <int DIMS, typename Reader>
ZFP_HD unsigned coded_prefix_bits(Reader& rd, uint64_t w0, unsigned head, unsigned limit, unsigned planes) {
  constexpr unsigned N = 1u << (2 * DIMS);
  unsigned pos = head, n = 0, k = 0;
  uint64_t buf = w0;  // the block's bits [wpos, wpos + 64)
  unsigned wpos = 0;
  while (pos < limit) {
    unsigned off = pos - wpos;
    if (off >= 64u) {
      buf = rd.window(pos);
      wpos = pos;
      off = 0;
    }
    const uint64_t v = buf >> off;  // bits [pos, wpos + 64), zero above them
    const bool more = (v & 1u) != 0;  // the group test
    unsigned adv = 1;
    if (more) {
      // the run: zeros up to the next one, over at most lim = N - 1 - n
      // positions (the one at position N - 1 is not coded)
      const unsigned lim = N - 1u - n;  // n < N here
      const unsigned avail = 63u - off;  // bits of the run the window holds
      unsigned z = ctz64_or_64(v >> 1);
      if (z >= avail && avail < lim) {
        buf = rd.window(pos);
        wpos = pos;
        z = ctz64_or_64(buf >> 1);
      }
      if (z < lim) {
        adv += z + 1u;
        n += z + 1u;  // <= N - 1
      } else {
        adv += lim;
        n = N;
      }
    }
    pos += adv;
    if (!more || n == N) {  // the plane's end
      k++;
      if (k == planes) break;
      if (n == N) {
        pos += (planes - k) * N;
        break;
      }
      pos += n;  // the next plane's bits of the coefficients already significant
    }
  }
  return pos < limit ? pos : limit;
}

// The length of a block at the mode (new_maxprec, new_minexp), from the block
// as a finer mode coded it in src_len bits: 1 for the one-bit form (the new
// block is then the single bit 0, not the source's first bit), else a prefix
// length, at most the clamped src_len.  A src_len of 0 gives 0.
template <typename Scalar, int DIMS, typename Reader>
ZFP_HD unsigned truncated_block_length(Reader& rd, unsigned src_len, unsigned new_maxprec, int new_minexp) {
  typedef traits<Scalar> T;
  static_assert(!T::is_int, "the variable-rate modes are defined for floats");
  constexpr unsigned kLongest = variable_longest_block<Scalar, DIMS>();
  src_len = src_len < kLongest ? src_len : kLongest;
  if (src_len < T::ebits + 2u) return src_len ? 1u : 0u;  // the zero block, or no block's length
  const uint64_t w = rd.window(0);
  if (!(w & 1u)) return 1u;  // the zero block's flag
  const int emax = (int)((uint32_t)(w >> 1) & ((1u << T::ebits) - 1u)) - T::ebias;
  const unsigned p = precision_variable<DIMS>(emax, new_maxprec, new_minexp);
  if (!p) return 1u;  // below the new mode's precision: the one-bit form
  return coded_prefix_bits<DIMS>(rd, w, 1u + T::ebits, src_len, p);
}

// (maxprec, minexp) -> (new_maxprec, new_minexp) only coarsens
ZFP_HD bool variable_mode_coarsens(unsigned maxprec, int minexp, unsigned new_maxprec, int new_minexp) {
  return new_maxprec <= maxprec && new_minexp >= minexp;
}

}  // namespace cuzfp
