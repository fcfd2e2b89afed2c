// cuzfp_amd/csrc/source_window.hpp -- the 64-bit window on a variable-rate
// stream that truncated_block_length (rerate_variable.hpp) walks through on the
// device: the lengths pass of truncate_variable.hip and the coarse sub-box
// decoder (region_variable_coarse_kernels.hpp) read a block's bits with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cuzfp {

// 64 bits of the source from a block's first bit on; dwords at or past the
// stream's end read as zero
struct SourceWindow {
  const uint32_t* __restrict__ base;
  uint64_t dwords;
  uint64_t off;
  __device__ __forceinline__ uint64_t window(uint32_t pos) const {
    const uint64_t bit = off + pos;
    const uint64_t d = bit >> 5;
    const uint32_t s = (uint32_t)bit & 31u;
    const uint32_t a0 = d < dwords ? base[d] : 0u;
    const uint32_t a1 = d + 1 < dwords ? base[d + 1] : 0u;
    const uint32_t a2 = d + 2 < dwords ? base[d + 2] : 0u;
    return (uint64_t)__builtin_amdgcn_alignbit(a1, a0, s) | ((uint64_t)__builtin_amdgcn_alignbit(a2, a1, s) << 32);
  }
};

}  // namespace cuzfp
