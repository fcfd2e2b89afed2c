// cuzfp_amd/csrc/region_variable_crop_kernels.hpp -- crop and paste of a
// block-aligned box of a variable-rate stream in the compressed domain
// (cuzfp_hip_extract_region_variable, cuzfp_hip_insert_region_variable).  zfp
// codes every block on its own, and an aligned box keeps, for every block it
// holds, the block's values and which of its elements lie inside the array: the
// box's blocks, back to back in the box's raster order, are the stream of the
// sub-array.  Bits are moved, nothing is decoded.
//
//   crop:   zfp_crop_variable_lengths   source lengths of the box's blocks  -> box lengths
//           scan (variable_kernels.hpp) box lengths                         -> box offsets, total
//           variable_zero_shared        the words two waves' segments can share
//           zfp_crop_variable_copy      one wave for 64 box blocks: a lane's source
//                                       offset from the source index
//                                       (variable_block_offset), its bits OR-ed
//                                       into the wave's segment in LDS; the box's
//                                       index
//   paste:  copy (hipMemcpyAsync)       source lengths                      -> new lengths
//           zfp_paste_variable_lengths  box lengths over the touched blocks -> new lengths
//           scan, variable_zero_shared  as above, over the archive's blocks
//           zfp_paste_variable_copy     one wave for 64 archive blocks: an
//                                       untouched lane copies from the source at
//                                       the wave's index entry plus the in-wave
//                                       prefix sum (zfp_update_variable_copy's
//                                       lanes), a touched lane from the box stream
//                                       through the box's index; the new index
//
// Both copy kernels end in copy_wave_segment, the segment scheme of
// zfp_truncate_variable_copy (truncate_variable.hip): the wave's 64 blocks are
// contiguous in the output, only the segment's first word and an open last one
// can hold another wave's bits and are OR-ed into the stream, every other word
// is stored whole, and no word at or past cap_words is touched.
//
// No index and no lengths array is trusted, the source's or the box's: a copied
// length is clamped to the type's longest block, every source dword is loaded
// behind a bound test (SourceWindow), a lane whose place falls outside its
// wave's segment copies nothing, and the new offsets are the scan of the new
// lengths.  index[b / 64] and lengths[64 (b / 64) .. b) are the only entries a
// block's offset reads (variable_block_offset), b below the array's, or the
// box's, block count.
//
// Instantiated per scalar type in region_variable_crop_{f32,f64}.hip.
#pragma once
#include "kernels.hpp"
#include "rerate_variable.hpp"
#include "source_window.hpp"
#include "variable_index.hpp"

namespace cuzfp {

// crop: lengths[r] = the raw source length of box block r
template <int DIMS>
__global__ __launch_bounds__(256) void zfp_crop_variable_lengths(const uint16_t* __restrict__ src_lengths, Region rg,
                                                                 uint16_t* __restrict__ lengths) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= rg.nrb) return;
  lengths[r] = src_lengths[region_block<DIMS>(rg, r).b];
}

// paste: the box's raw lengths over the touched entries of the new lengths
template <int DIMS>
__global__ __launch_bounds__(256) void zfp_paste_variable_lengths(const uint16_t* __restrict__ box_lengths, Region rg,
                                                                  uint16_t* __restrict__ lengths) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= rg.nrb) return;
  lengths[region_block<DIMS>(rg, r).b] = box_lengths[r];
}

// The tail of a copy kernel of one wave a workgroup.  The lane's block: its raw
// new length `len` (0 for a lane past the last block), its new offset `off`,
// and its bits at bit `soff` of `src`.  The wave's blocks are the output bits
// [off0, off0 + S - sh0), off0 lane 0's offset and sh0 = off0 mod 64; seg[k] is
// output word (off0 >> 6) + k, kLongest + 2 words (64 blocks of kLongest bits
// from bit sh0 < 64 on take at most kLongest + 1).  A block of one bit is the
// bit 0 and a block of no bits is nothing: neither touches the zeroed segment.
// Lane 0 stores the wave's entry of the new index, and wave 0 the total.
template <uint32_t kLongest>
__device__ __forceinline__ void copy_wave_segment(uint64_t* seg, uint32_t lane, const uint32_t* __restrict__ src,
                                                  uint64_t src_dwords, uint64_t soff, uint32_t len, uint64_t off,
                                                  uint64_t* __restrict__ dst, uint64_t cap_words,
                                                  uint64_t* __restrict__ dst_index,
                                                  const uint64_t* __restrict__ total) {
  constexpr uint32_t kSegWords = kLongest + 2;
  len = len < kLongest ? len : kLongest;  // a copied length is the source's, whatever it holds
  const uint64_t off0 = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)off) |
                        ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(off >> 32)) << 32);
  if (dst_index && lane == 0) {
    dst_index[blockIdx.x] = off0;
    if (blockIdx.x == 0) dst_index[gridDim.x] = *total;
  }
  const uint32_t sh0 = (uint32_t)off0 & 63u;
  // the lane's place in the segment: with legal lengths rel <= sh0 + the
  // lengths of the lanes before it; raw lengths past kLongest can push a lane
  // out of the segment, and such a lane copies nothing
  const uint64_t rel64 = off - off0 + sh0;
  const uint32_t rel = len ? (uint32_t)(rel64 < 64ull * kLongest ? rel64 : 64ull * kLongest) : 0u;
  if (rel + len > 64u * kSegWords) len = 0;
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

// Crop's copy pass.  One wave a workgroup, wave w for box blocks 64 w .. 64 w +
// 63, which are contiguous in the output and scattered in the source: a lane
// finds its block through the source index, as zfp_decode_region_variable does.
// lengths, offsets: the box's (nrb entries); dst_index may be null.
template <typename Scalar, int DIMS>
__global__ __launch_bounds__(kLanes) void zfp_crop_variable_copy(
    const uint32_t* __restrict__ src, uint64_t src_dwords, const uint16_t* __restrict__ src_lengths,
    const uint64_t* __restrict__ src_index, const uint16_t* __restrict__ lengths,
    const uint64_t* __restrict__ offsets, Region rg, uint64_t* __restrict__ dst, uint64_t cap_words,
    uint64_t* __restrict__ dst_index, const uint64_t* __restrict__ total) {
  constexpr uint32_t kLongest = variable_longest_block<Scalar, DIMS>();
  __shared__ uint64_t seg[kLongest + 2];
  const uint32_t lane = threadIdx.x;
  const uint32_t r = blockIdx.x * kLanes + lane;
  uint32_t len = 0;
  uint64_t off = 0, soff = 0;
  if (r < rg.nrb) {
    len = lengths[r];
    off = offsets[r];
    if (len > 1u) soff = variable_block_offset(src_index, src_lengths, region_block<DIMS>(rg, r).b);
  }
  copy_wave_segment<kLongest>(seg, lane, src, src_dwords, soff, len, off, dst, cap_words, dst_index, total);
}

// Paste's copy pass.  One wave a workgroup, wave w for archive blocks 64 w ..
// 64 w + 63, contiguous in the output and in the source.  An untouched lane's
// source offset is src_index[w] plus the wave's exclusive prefix sum of the raw
// source lengths (< 2^22); a touched lane's block is box block r, found through
// the box's index.  lengths, offsets: the result's (nblocks entries).
template <typename Scalar, int DIMS>
__global__ __launch_bounds__(kLanes) void zfp_paste_variable_copy(
    const uint32_t* __restrict__ src, uint64_t src_dwords, const uint16_t* __restrict__ src_lengths,
    const uint64_t* __restrict__ src_index, const uint32_t* __restrict__ box, uint64_t box_dwords,
    const uint16_t* __restrict__ box_lengths, const uint64_t* __restrict__ box_index,
    const uint16_t* __restrict__ lengths, const uint64_t* __restrict__ offsets, Geometry g, Region rg,
    uint64_t* __restrict__ dst, uint64_t cap_words, uint64_t* __restrict__ dst_index,
    const uint64_t* __restrict__ total) {
  constexpr uint32_t kLongest = variable_longest_block<Scalar, DIMS>();
  __shared__ uint64_t seg[kLongest + 2];
  const uint32_t lane = threadIdx.x;
  const uint32_t b = blockIdx.x * kLanes + lane;
  uint32_t len = 0, slen = 0, r = 0;
  uint64_t off = 0;
  bool touched = false;
  if (b < g.nblocks) {
    len = lengths[b];
    off = offsets[b];
    slen = src_lengths[b];
    const BlockPos bp = block_pos<DIMS>(g, b);
    const uint32_t rx = bp.ix - rg.bx0, ry = bp.iy - rg.by0, rz = bp.iz - rg.bz0;
    touched = rx < rg.rbx && ry < rg.rby && rz < rg.rbz;
    r = (rz * rg.rby + ry) * rg.rbx + rx;  // < nrb when touched
  }
  uint32_t inc = slen;  // inclusive prefix sum over the wave, <= 64 * 65535
  for (uint32_t d = 1; d < kLanes; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
    if (lane >= d) inc += t;
  }
  uint64_t soff = src_index[blockIdx.x] + (inc - slen);
  if (touched) soff = len > 1u ? variable_block_offset(box_index, box_lengths, r) : 0ull;
  copy_wave_segment<kLongest>(seg, lane, touched ? box : src, touched ? box_dwords : src_dwords, soff, len, off, dst,
                              cap_words, dst_index, total);
}

static inline int crop_launch_status() {
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

// rg: the box in the source array.  lengths, dst_index and the workspace
// (offsets: nrb words, partials: variable_tiles(nrb)) are the box's.
template <typename Scalar, int DIMS>
int launch_extract_region_variable_t(const Region& rg, const uint64_t* src, size_t src_bytes,
                                     const uint16_t* src_lengths, const uint64_t* src_index, uint64_t* dst,
                                     uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                                     uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  hipLaunchKernelGGL((zfp_crop_variable_lengths<DIMS>), dim3((rg.nrb + 255) / 256), dim3(256), 0, st, src_lengths, rg,
                     lengths);
  int rc = crop_launch_status();
  if (rc) return rc;
  rc = launch_variable_scan(lengths, rg.nrb, offsets, partials, total, st);
  if (rc) return rc;
  if (!cap_words && !dst_index) return CUZFP_SUCCESS;  // the size query: lengths and total only
  rc = launch_variable_zero(dst, cap_words, offsets, rg.nrb, total, st);
  if (rc) return rc;
  hipLaunchKernelGGL((zfp_crop_variable_copy<Scalar, DIMS>), dim3((rg.nrb + kLanes - 1) / kLanes), dim3(kLanes), 0, st,
                     (const uint32_t*)src, (uint64_t)(src_bytes / 4), src_lengths, src_index,
                     (const uint16_t*)lengths, (const uint64_t*)offsets, rg, dst, cap_words, dst_index,
                     (const uint64_t*)total);
  return crop_launch_status();
}

// g, rg: the archive and the box in it.  lengths, dst_index and the workspace
// (offsets: nblocks words, partials: variable_tiles(nblocks)) are the result's.
template <typename Scalar, int DIMS>
int launch_insert_region_variable_t(const Geometry& g, const Region& rg, const uint64_t* box, size_t box_bytes,
                                    const uint16_t* box_lengths, const uint64_t* box_index, const uint64_t* src,
                                    size_t src_bytes, const uint16_t* src_lengths, const uint64_t* src_index,
                                    uint64_t* dst, uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index,
                                    uint64_t* total, uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(lengths, src_lengths, 2 * (size_t)g.nblocks, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) {
    t_last_hip = e;
    return CUZFP_ERROR_HIP;
  }
  hipLaunchKernelGGL((zfp_paste_variable_lengths<DIMS>), dim3((rg.nrb + 255) / 256), dim3(256), 0, st, box_lengths, rg,
                     lengths);
  int rc = crop_launch_status();
  if (rc) return rc;
  rc = launch_variable_scan(lengths, g.nblocks, offsets, partials, total, st);
  if (rc) return rc;
  if (!cap_words && !dst_index) return CUZFP_SUCCESS;  // the size query: lengths and total only
  rc = launch_variable_zero(dst, cap_words, offsets, g.nblocks, total, st);
  if (rc) return rc;
  hipLaunchKernelGGL((zfp_paste_variable_copy<Scalar, DIMS>), dim3((g.nblocks + kLanes - 1) / kLanes), dim3(kLanes), 0,
                     st, (const uint32_t*)src, (uint64_t)(src_bytes / 4), src_lengths, src_index,
                     (const uint32_t*)box, (uint64_t)(box_bytes / 4), box_lengths, box_index,
                     (const uint16_t*)lengths, (const uint64_t*)offsets, g, rg, dst, cap_words, dst_index,
                     (const uint64_t*)total);
  return crop_launch_status();
}

template <typename Scalar>
int launch_extract_region_variable_type(unsigned dims, const Region& rg, const uint64_t* src, size_t src_bytes,
                                        const uint16_t* src_lengths, const uint64_t* src_index, uint64_t* dst,
                                        uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                                        uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  switch (dims) {
    case 1: return launch_extract_region_variable_t<Scalar, 1>(rg, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
    case 2: return launch_extract_region_variable_t<Scalar, 2>(rg, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
    default: return launch_extract_region_variable_t<Scalar, 3>(rg, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
  }
}

template <typename Scalar>
int launch_insert_region_variable_type(const Problem& p, const Region& rg, const uint64_t* box, size_t box_bytes,
                                       const uint16_t* box_lengths, const uint64_t* box_index, const uint64_t* src,
                                       size_t src_bytes, const uint16_t* src_lengths, const uint64_t* src_index,
                                       uint64_t* dst, uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index,
                                       uint64_t* total, uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_insert_region_variable_t<Scalar, 1>(p.g, rg, box, box_bytes, box_lengths, box_index, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
    case 2: return launch_insert_region_variable_t<Scalar, 2>(p.g, rg, box, box_bytes, box_lengths, box_index, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
    default: return launch_insert_region_variable_t<Scalar, 3>(p.g, rg, box, box_bytes, box_lengths, box_index, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
  }
}

}  // namespace cuzfp
