// cuzfp_amd/csrc/truncate_variable.hip -- cuzfp_hip_truncate_variable: a
// variable-rate stream at the mode (maxprec, minexp) cut down to the stream at
// a coarser mode (rerate_variable.hpp has the property and the per-block
// walk).  Bits are moved, nothing is decoded.
//
//   scan                           source lengths             -> source offsets
//   zfp_truncate_variable_lengths  one lane a block: the exponent field and
//                                  the walk over the plane code, through a
//                                  64-bit window on the source -> new lengths
//   scan                           new lengths                -> new offsets, total
//   variable_zero_shared           the words two waves' segments can share
//   zfp_truncate_variable_copy     one wave for 64 blocks: every lane ORs its
//                                  block's prefix into the wave's segment
//                                  [offsets[b0], offsets[b0 + 64)) in LDS,
//                                  which the wave copies out as the
//                                  variable-rate encoder does
//
// The source index is not trusted (the decoder's rule, variable_kernels.hpp):
// a length is clamped to the type's longest block, a length no coded block can
// have reads as a zero block, and every source dword is loaded behind
// `d < src_dwords`.  A new length never exceeds the clamped source length, and
// the new offsets are the scan of the new lengths, so the segment's bounds
// hold whatever the source index holds.
#include "kernels.hpp"
#include "rerate_variable.hpp"
#include "source_window.hpp"  // SourceWindow: 64 bits of the source from a block's first bit on

namespace cuzfp {

// Lengths pass: one lane, one block.  The walk diverges by lane (its trip count
// is the block's own); the loads around it are per lane and bounded.
template <typename Scalar, int DIMS>
__global__ __launch_bounds__(256) void zfp_truncate_variable_lengths(const uint32_t* __restrict__ src,
                                                                     uint64_t src_dwords,
                                                                     const uint16_t* __restrict__ src_lengths,
                                                                     const uint64_t* __restrict__ src_offsets,
                                                                     uint32_t nblocks, uint32_t new_maxprec,
                                                                     int new_minexp, uint16_t* __restrict__ lengths) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  if (b >= nblocks) return;
  SourceWindow rd{src, src_dwords, src_offsets[b]};
  lengths[b] = (uint16_t)truncated_block_length<Scalar, DIMS>(rd, src_lengths[b], new_maxprec, new_minexp);
}

// Copy pass.  One wave a workgroup; the wave's 64 new blocks are contiguous in
// the output: bits [off0, off0 + S - sh0), sh0 = off0 mod 64.  seg[k] is output
// word (off0 >> 6) + k.  A block of one bit is the bit 0 and a block of no bits
// is nothing: neither touches the zeroed segment.  A longer block is its
// source's first len bits, fetched 64 at a time and OR-ed in at the lane's
// place.  Only the segment's first word, and its last when the segment ends
// inside it, can hold another wave's bits; those are OR-ed into the stream,
// which variable_zero_shared zeroed there, and every other word is stored
// whole.  No word at or past cap_words is touched.
//
// LDS: (longest block of the type + 2) words: 32.6 KiB for 3D double, 16.6 KiB
// for 3D float.
template <typename Scalar, int DIMS>
__global__ __launch_bounds__(kLanes) void zfp_truncate_variable_copy(const uint32_t* __restrict__ src,
                                                                     uint64_t src_dwords,
                                                                     const uint64_t* __restrict__ src_offsets,
                                                                     const uint16_t* __restrict__ lengths,
                                                                     const uint64_t* __restrict__ offsets,
                                                                     uint32_t nblocks, uint64_t* __restrict__ dst,
                                                                     uint64_t cap_words) {
  constexpr uint32_t kLongest = variable_longest_block<Scalar, DIMS>();
  constexpr uint32_t kSegWords = kLongest + 2;  // 64 blocks of kLongest bits from bit sh0 < 64 on: <= kLongest + 1 words
  __shared__ uint64_t seg[kSegWords];
  const uint32_t lane = threadIdx.x;
  const uint32_t b = blockIdx.x * kLanes + lane;
  uint32_t len = 0;
  uint64_t off = 0, soff = 0;
  if (b < nblocks) {
    len = lengths[b];
    off = offsets[b];
    soff = src_offsets[b];
  }
  len = len < kLongest ? len : kLongest;  // (what the lengths pass wrote never exceeds it)
  const uint64_t off0 = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)off) |
                        ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(off >> 32)) << 32);
  const uint32_t sh0 = (uint32_t)off0 & 63u;
  // the lane's place in the segment; the offsets are the scan of the lengths,
  // so rel <= sh0 + the lengths of the lanes before it; clamped all the same
  const uint64_t rel64 = off - off0 + sh0;
  const uint32_t rel = len ? (uint32_t)(rel64 < 64ull * kLongest ? rel64 : 64ull * kLongest) : 0u;
  if (rel + len > 64u * kSegWords) len = 0;  // (cannot happen with scanned offsets)
  uint32_t S = rel + len;
  for (int o = 32; o; o >>= 1) S = max(S, (uint32_t)__shfl_xor((int)S, o));
  const uint32_t nseg = (S + 63) >> 6;  // <= kSegWords
  for (uint32_t k = lane; k < nseg; k += kLanes) seg[k] = 0;
  __syncthreads();
  if (len > 1u) {
    SourceWindow rd{src, src_dwords, soff};
    const uint32_t nw = (len + 63) >> 6;
    for (uint32_t j = 0; j < nw; j++) {
      uint64_t v = rd.window(64 * j);
      const uint32_t left = len - 64 * j;
      if (left < 64) v &= lowmask(left);
      const uint32_t bit = rel + 64 * j, k = bit >> 6, sh = bit & 63u;
      const uint64_t lo = v << sh;
      const uint64_t hi = sh ? v >> (64 - sh) : 0ull;
      if (lo) atomicOr((unsigned long long*)&seg[k], (unsigned long long)lo);
      if (hi) atomicOr((unsigned long long*)&seg[k + 1], (unsigned long long)hi);  // k + 1 < nseg: the block has bits there
    }
  }
  __syncthreads();
  const uint64_t w0 = off0 >> 6;
  const bool open_end = (S & 63u) != 0;  // the segment ends inside its last word
  for (uint32_t k = lane; k < nseg; k += kLanes) {
    const uint64_t v = seg[k];
    const uint64_t w = w0 + k;
    if (w >= cap_words) break;
    if (k == 0 || (k + 1 == nseg && open_end)) {
      if (v) atomicOr((unsigned long long*)&dst[w], (unsigned long long)v);
    } else {
      dst[w] = v;
    }
  }
}

template <typename Scalar, int DIMS>
static int launch_truncate_variable_t(const uint64_t* src, size_t src_bytes, const uint16_t* src_lengths,
                                      uint32_t nblocks, uint32_t new_maxprec, int new_minexp, uint64_t* dst,
                                      uint64_t cap_words, uint16_t* lengths, uint64_t* total, uint64_t* src_offsets,
                                      uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  int rc = launch_variable_scan(src_lengths, nblocks, src_offsets, partials, nullptr, st);
  if (rc) return rc;
  const uint64_t dwords = (uint64_t)(src_bytes / 4);
  hipLaunchKernelGGL((zfp_truncate_variable_lengths<Scalar, DIMS>), dim3((nblocks + 255) / 256), dim3(256), 0, st,
                     (const uint32_t*)src, dwords, src_lengths, (const uint64_t*)src_offsets, nblocks, new_maxprec,
                     new_minexp, lengths);
  rc = launch_variable_scan(lengths, nblocks, offsets, partials, total, st);
  if (rc) return rc;
  if (!cap_words) return CUZFP_SUCCESS;  // the size query: lengths and total only
  rc = launch_variable_zero(dst, cap_words, offsets, nblocks, total, st);
  if (rc) return rc;
  hipLaunchKernelGGL((zfp_truncate_variable_copy<Scalar, DIMS>), dim3((nblocks + kLanes - 1) / kLanes), dim3(kLanes), 0,
                     st, (const uint32_t*)src, dwords, (const uint64_t*)src_offsets, (const uint16_t*)lengths,
                     (const uint64_t*)offsets, nblocks, dst, cap_words);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

template <typename Scalar>
static int launch_truncate_variable_type(unsigned dims, const uint64_t* src, size_t src_bytes,
                                         const uint16_t* src_lengths, uint32_t nblocks, uint32_t new_maxprec,
                                         int new_minexp, uint64_t* dst, uint64_t cap_words, uint16_t* lengths,
                                         uint64_t* total, uint64_t* src_offsets, uint64_t* offsets,
                                         uint64_t* partials, hipStream_t st) {
  switch (dims) {
    case 1: return launch_truncate_variable_t<Scalar, 1>(src, src_bytes, src_lengths, nblocks, new_maxprec, new_minexp, dst, cap_words, lengths, total, src_offsets, offsets, partials, st);
    case 2: return launch_truncate_variable_t<Scalar, 2>(src, src_bytes, src_lengths, nblocks, new_maxprec, new_minexp, dst, cap_words, lengths, total, src_offsets, offsets, partials, st);
    default: return launch_truncate_variable_t<Scalar, 3>(src, src_bytes, src_lengths, nblocks, new_maxprec, new_minexp, dst, cap_words, lengths, total, src_offsets, offsets, partials, st);
  }
}

int launch_truncate_variable(bool is_double, unsigned dims, const uint64_t* src, size_t src_bytes,
                             const uint16_t* src_lengths, uint32_t nblocks, uint32_t new_maxprec, int new_minexp,
                             uint64_t* dst, uint64_t cap_words, uint16_t* lengths, uint64_t* total,
                             uint64_t* src_offsets, uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  if (is_double)
    return launch_truncate_variable_type<double>(dims, src, src_bytes, src_lengths, nblocks, new_maxprec, new_minexp,
                                                 dst, cap_words, lengths, total, src_offsets, offsets, partials, st);
  return launch_truncate_variable_type<float>(dims, src, src_bytes, src_lengths, nblocks, new_maxprec, new_minexp, dst,
                                              cap_words, lengths, total, src_offsets, offsets, partials, st);
}

}  // namespace cuzfp
