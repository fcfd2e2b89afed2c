// cuzfp_amd/csrc/variable_coarse.hpp -- the per-block arithmetic of
// cuzfp_hip_decode_region_variable_coarse, for host and device: the kernel
// (region_variable_coarse_kernels.hpp) and
// tests/native/variable_coarse_emulate.cpp go through the same functions.
//
// A block of a variable-rate stream is decoded at a target mode (maxprec,
// minexp) by the unchanged decode_block with a budget of
//
//   L' = truncated_block_length(block, its source length, maxprec, minexp)
//
// bits (rerate_variable.hpp), L' <= 1 being the zero block: a block decoded
// with a budget of exactly the bits a mode writes of it is what zfp_decompress
// returns in that mode.  The walk ends at the block's source length, so a
// target finer than the mode that wrote the stream decodes what the stream
// holds: the result is the array at (the smaller maxprec, the larger minexp).
//
// The LDS column of a lane is sized from the target: a block a mode with
// `maxprec` planes writes has at most max_block_bits(maxprec) bits.  Arbitrary
// bits, or an index of another stream, can make the walk return more (its group
// tests are not limited by that formula), so the budget is clamped to the
// column; such a block decodes to unspecified values.
#pragma once
#include <stdint.h>

#include "rerate_variable.hpp"
#include "variable_index.hpp"

namespace cuzfp {

// Dwords of a lane's column at the target precision maxprec (1 .. the type's)
template <typename Scalar, int DIMS>
CUZFP_HD uint32_t variable_coarse_column_dwords(uint32_t maxprec) {
  const uint32_t longest = variable_longest_block<Scalar, DIMS>();
  const uint32_t bits = max_block_bits<Scalar, DIMS>(maxprec);
  return ((bits < longest ? bits : longest) + 31u) / 32u;
}

// The budget a block is decoded with: `raw` its index entry, `walked` the
// walk's L' for it, column_bits the bits of the lane's column (32 x
// variable_coarse_column_dwords), max_len the type's longest block.  0 -- the
// zero block, nothing further is read -- where the source is a zero block or no
// block's length (variable_budget) or the target codes no plane of it (L' <=
// 1); else L' clamped to the source's clamped length and the column: a value in
// [ebits + 2, min(clamped raw, column_bits)].
CUZFP_HD uint32_t variable_coarse_budget(uint32_t raw, uint32_t walked, uint32_t column_bits, uint32_t max_len,
                                         uint32_t ebits) {
  const uint32_t src = variable_budget(raw, max_len, ebits);
  if (!src || walked < ebits + 2u) return 0u;
  const uint32_t len = walked < src ? walked : src;
  return len < column_bits ? len : column_bits;
}

}  // namespace cuzfp
