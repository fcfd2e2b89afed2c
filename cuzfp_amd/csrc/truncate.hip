// cuzfp_amd/csrc/truncate.hip -- cuzfp_hip_truncate: a stream at M bits a block
// cut down to the stream at m <= M bits a block (rerate.hpp has the property
// and the position arithmetic).  Type-independent: bits are moved, nothing is
// decoded.
//
// Both kernels are output-centric -- a lane owns a piece of the output and
// gathers its source -- so the stores are full-width and coalesced, and the
// loads are runs of m bits, M bits apart.
#include <algorithm>

#include "kernels.hpp"
#include "rerate.hpp"

namespace cuzfp {

// Word path: M and m multiples of 64 (Vec = uint64_t) or of 128 with both
// bases 16-byte aligned (Vec = uint4).  n: output units; mu, Mu: units a block.
// The grid cap and grid-stride loop of copy16_nt (capi.hip); Idx = uint32_t
// only where i + stride cannot wrap (launch_truncate).
template <typename Idx, typename Vec>
__global__ __launch_bounds__(256) void truncate_units(const Vec* __restrict__ src, Vec* __restrict__ dst, Idx n,
                                                      uint32_t mu, uint32_t Mu) {
  const Idx stride = (Idx)gridDim.x * blockDim.x;
  for (Idx i = (Idx)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Idx s = rerate_unit_src<Idx>(i, mu, Mu);
    if constexpr (sizeof(Vec) == 16)
      st16<true>(dst + i, ld16<true>(src + s));
    else
      __builtin_nontemporal_store(__builtin_nontemporal_load(src + s), dst + i);
  }
}

// General path: one lane per output 64-bit word (rerate_word).  A segment's
// carry dwords past the source's end are loaded through a clamped address and
// selected to zero.
__global__ __launch_bounds__(256) void truncate_bits(const uint32_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                     uint64_t nwords, uint64_t src_dwords, uint32_t nblocks,
                                                     uint32_t M, uint32_t m) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  auto load = [&](uint64_t d) -> uint32_t {
    const bool in = d < src_dwords;
    const uint32_t v = src[in ? d : src_dwords - 1];
    return in ? v : 0u;
  };
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride)
    dst[w] = rerate_word(w, nblocks, M, m, load);
}

template <typename Vec>
static void launch_units(const void* src, void* dst, uint64_t n_out, uint64_t n_src, uint32_t mu, uint32_t Mu,
                         hipStream_t st) {
  // one grid over the output up to 16 Mi workgroups; the loop covers the rest
  const unsigned grid = (unsigned)std::min<uint64_t>((n_out + 255) / 256, 1u << 24);
  // 32-bit indices: i < n_out <= n_src < 2^31 and stride <= n_out + 255, so
  // neither the source index nor i + stride wraps
  if (n_src < (1ull << 31))
    hipLaunchKernelGGL((truncate_units<uint32_t, Vec>), dim3(grid), dim3(256), 0, st, (const Vec*)src, (Vec*)dst,
                       (uint32_t)n_out, mu, Mu);
  else
    hipLaunchKernelGGL((truncate_units<uint64_t, Vec>), dim3(grid), dim3(256), 0, st, (const Vec*)src, (Vec*)dst,
                       n_out, mu, Mu);
}

int launch_truncate(const uint64_t* src, uint64_t* dst, uint32_t nblocks, uint32_t M, uint32_t m, hipStream_t st) {
  const uint64_t out_words = ((uint64_t)nblocks * m + 63) / 64, src_words = ((uint64_t)nblocks * M + 63) / 64;
  if (!((M | m) & 63)) {
    const bool v16 = !((M | m) & 127) && !(((uintptr_t)src | (uintptr_t)dst) & 15);
    if (v16)
      launch_units<uint4>(src, dst, out_words / 2, src_words / 2, m / 128, M / 128, st);
    else
      launch_units<uint64_t>(src, dst, out_words, src_words, m / 64, M / 64, st);
  } else {
    const unsigned grid = (unsigned)std::min<uint64_t>((out_words + 255) / 256, 1u << 24);
    hipLaunchKernelGGL(truncate_bits, dim3(grid), dim3(256), 0, st, (const uint32_t*)src, dst, out_words,
                       2 * src_words, nblocks, M, m);
  }
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

}  // namespace cuzfp
