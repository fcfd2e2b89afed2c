// cuzfp_amd/csrc/variable_index.hpp -- the persistent offset index of a
// variable-rate stream (cuzfp_hip_variable_index) and the copy-in bounds of the
// variable-rate decoders, for host and device: the index builder and the
// sub-box decoder (region_variable_kernels.hpp) and
// tests/native/variable_index_map.cpp go through the same functions.
//
// A variable-rate stream is its blocks back to back, block b taking
// lengths[b] bits (variable_kernels.hpp).  The index holds the bit offset of
// every kIndexTile-th block and the stream's bit count:
//
//   index[t] = sum of lengths[0 .. 64 t)   t = 0 .. T - 1, T = ceil(nblocks / 64)
//   index[T] = sum of all lengths
//
// (the raw uint16 values summed, as the scan does), 8 (T + 1) bytes.  A
// block's offset is its tile's entry plus the lengths of the blocks before it
// in the tile: at most 63 lengths, a sum below 2^22.
#pragma once
#include <stdint.h>

#include "region.hpp"

namespace cuzfp {

constexpr uint32_t kIndexTile = 64;  // blocks an index entry: a wave of the whole-array coder

// T: entries 0 .. T - 1 are tile offsets, entry T the total (nblocks < 2^32 - 64)
CUZFP_HD uint32_t variable_index_tiles(uint32_t nblocks) { return (nblocks + kIndexTile - 1) / kIndexTile; }

// The bit offset of block b (< nblocks).  `index` and `lengths` are anything
// with operator[] (the device pointers; the host check's recording views).
// Reads index[b / 64], never entry T or beyond, and lengths[64 (b / 64) .. b),
// all before b: no length at or past nblocks.  The loads are 2 bytes each, so
// `lengths` needs no alignment beyond a uint16's.
template <typename Index, typename Lengths>
CUZFP_HD uint64_t variable_block_offset(const Index& index, const Lengths& lengths, uint32_t b) {
  const uint32_t b0 = b & ~(kIndexTile - 1);
  uint32_t s = 0;  // <= 63 * 65535
  for (uint32_t i = b0; i < b; i++) s += (uint32_t)(uint16_t)lengths[i];
  return (uint64_t)index[b / kIndexTile] + s;
}

// The budget a block is decoded with from its index entry `raw`: clamped to
// the type's longest block max_len (the LDS column is sized for it); 0 -- the
// zero block, nothing is read -- for 0, 1 and the lengths no coded block has
// (2 .. ebits + 1).
CUZFP_HD uint32_t variable_budget(uint32_t raw, uint32_t max_len, uint32_t ebits) {
  const uint32_t len = raw < max_len ? raw : max_len;
  return len < ebits + 2u ? 0u : len;
}

// The copy-in of a block of `len` (variable_budget) bits at bit `off` fills
// Dl = ceil(len / 32) dwords of its column from stream dwords (off >> 5) + j,
// j = 0 .. Dl (dword j and, as the funnel shift's carry, j + 1).  Whether
// dword j of those exists, and its index: a missing one reads as zero and is
// not loaded.  off >> 5 < 2^59 and j <= 131, so the sum cannot wrap.
CUZFP_HD bool variable_stream_dword(uint64_t off, uint32_t j, uint64_t stream_dwords, uint64_t& d) {
  d = (off >> 5) + j;
  return d < stream_dwords;
}

}  // namespace cuzfp
