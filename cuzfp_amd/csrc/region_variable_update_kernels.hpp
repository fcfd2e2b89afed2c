// cuzfp_amd/csrc/region_variable_update_kernels.hpp -- out-of-place update of
// a sub-box of a variable-rate stream (cuzfp_hip_encode_region_variable): the
// blocks the box touches are coded anew at the call's mode, every other block
// is copied bit for bit, and all of them are packed back to back again.
//
//   copy (hipMemcpyAsync)         source lengths               -> new lengths
//   zfp_update_region_variable    ENCODE = false: one lane a touched block;
//                                 its values, block_length     -> new lengths[b]
//   scan (variable_kernels.hpp)   new lengths                  -> new offsets, total
//   variable_zero_shared          the words two waves' segments can share
//   zfp_update_variable_copy      one wave for 64 blocks: untouched lanes OR
//                                 their source bits into the wave's segment in
//                                 LDS (truncate_variable.hip's copy), touched
//                                 lanes leave a hole of zeros; the new index
//   zfp_update_region_variable    ENCODE = true: one lane a touched block; its
//                                 values again, encode_block behind an
//                                 LdsOrWriter limited to new lengths[b], the
//                                 column shifted into the block's hole
//
// A touched block's values are encode_region's (region_update_kernels.hpp),
// chosen per launch on the host: covered (MERGE = false) gathers from the box
// and pads; merge (MERGE = true) copies the block's old bits in from the
// source through the index (zfp_decode_region_variable's copy-in), decodes
// them with the budget of its old length, overlays the box's elements and pads
// elements outside the array by the whole-array encoder's rule.  Both passes
// over the touched blocks build the values; nothing is kept between them.
//
// Stores of the encode pass.  Stream words wholly inside the block take plain
// stores: the copy pass, an earlier launch, left them zero and no other lane
// of this launch owns a bit of them.  The block's first and last word may hold
// bits of a neighbour, touched or not, and take a device-scope atomic OR.
// Every stream word is stored behind `word < cap_words`.
//
// Neither the source index nor the source lengths are trusted, as in the
// decoders: a merged block's budget is clamped to the type's longest block, a
// length no coded block has reads as a zero block, every source dword is
// loaded behind a bound test, a copied block's length and place in its wave's
// segment are clamped to the segment, and the new offsets are the scan of the
// new lengths.
//
// Instantiated per scalar type in region_variable_update_{f32,f64}.hip.
#pragma once
#include "region_update_kernels.hpp"
#include "rerate_variable.hpp"
#include "source_window.hpp"
#include "variable_index.hpp"

namespace cuzfp {

// The encoder's words a column without the slack rows, as zfp_encode_variable
// sizes them (variable_column_words, variable_kernels.hpp): the longest block
// of the mode; 1D columns take the type's longest whatever maxprec is, because
// the 1D pair coder does not settle a full lane.
template <typename Scalar, int DIMS>
inline uint32_t variable_update_column_words(uint32_t maxprec) {
  const uint32_t bits = max_block_bits<Scalar, DIMS>(DIMS == 1 ? (uint32_t)traits<Scalar>::prec : maxprec);
  return (bits + 63) / 64;
}

// static LDS of zfp_update_region_variable: the decoder's tables for the merge
// variant, the encoder's (over them) for the encode pass
template <int DIMS, bool MERGE, bool ENCODE>
constexpr size_t variable_update_tab_bytes() {
  constexpr size_t enc = ENCODE ? kSpreadTabBytes + (DIMS == 1 ? sizeof(Pair1dLut) : 0) : 16;
  constexpr size_t dec = MERGE ? chunk_lut_bytes<DIMS>() + (DIMS == 1 ? sizeof(Plane1dDecLut) : 0) : 16;
  return enc > dec ? enc : dec;
}

// The lane's coded block, `len` bits in its column, -> bits [off, off + len)
// of the stream (see the header for the stores).
__device__ __forceinline__ void store_block_variable(uint64_t* __restrict__ dst, uint64_t cap_words,
                                                     const uint64_t* mine, uint64_t off, uint32_t len) {
  if (len <= 1u) return;  // the one-bit zero block: its hole is the bit
  const uint64_t w0 = off >> 6;
  const uint32_t sh = (uint32_t)off & 63u;
  const uint32_t nw = (len + 63) >> 6;       // words of the column
  const uint32_t nd = (sh + len + 63) >> 6;  // words of the stream: nw or nw + 1
  uint64_t prev = 0;
  for (uint32_t k = 0; k < nd; k++) {
    uint64_t cur = 0;
    if (k < nw) {
      cur = mine[k * 64];
      const uint32_t left = len - 64 * k;
      if (left < 64) cur &= lowmask(left);
    }
    const uint64_t v = sh ? (cur << sh) | (prev >> (64 - sh)) : cur;
    prev = cur;
    const uint64_t w = w0 + k;
    if (w >= cap_words) break;
    if (k == 0 || k + 1 == nd) {
      if (v) atomicOr((unsigned long long*)&dst[w], (unsigned long long)v);
    } else {
      dst[w] = v;
    }
  }
}

// Waves a SIMD the launch bounds ask for: encode_region's for the encode pass;
// the lengths pass in 3D takes 2 (block_length holds the 64 coefficients and
// their planes: at 4 waves a SIMD the float covered variant spilled 7 VGPRs).
template <typename Scalar, int DIMS, bool MERGE, bool ENCODE> struct variable_update_occupancy {
  static constexpr int value = (!ENCODE && DIMS == 3) ? 2 : update_occupancy<Scalar, DIMS, MERGE>::value;
};

// g: the array (nx, ny, nz), the encoder's column (maxbits = 64 W) and the
// launch (wave_end, lds_words, row_stage: the covered variant's row loads).
template <typename Scalar, int DIMS, bool MERGE, bool ENCODE>
__global__ __launch_bounds__(kLanes * kUpdWaves, (variable_update_occupancy<Scalar, DIMS, MERGE, ENCODE>::value)) void
zfp_update_region_variable(const Scalar* __restrict__ box, Geometry g, Region rg, uint32_t maxprec, int minexp,
                           const uint64_t* __restrict__ src, uint64_t src_dwords,
                           const uint16_t* __restrict__ src_lengths, const uint64_t* __restrict__ src_index,
                           uint16_t* __restrict__ lengths, const uint64_t* __restrict__ offsets,
                           uint64_t* __restrict__ dst, uint64_t cap_words) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_all[];
  __shared__ __attribute__((aligned(16))) uint32_t tabs[variable_update_tab_bytes<DIMS, MERGE, ENCODE>() / 4];
  constexpr int N = 1 << (2 * DIMS);
  const uint32_t wig = wave_in_group();
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + wig;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = wave * kLanes + lane;
  const bool live_wave = wave < g.wave_end;
  const bool live = live_wave && r < rg.nrb;
  uint64_t* lds = lds_all + (size_t)wig * g.lds_words;
  uint64_t* mine = lds + lane;
  Scalar f[N];
  if constexpr (MERGE) {
    // the decoder's tables and the block's old bits (zfp_decode_region_variable_body)
    constexpr uint32_t kMaxLen = max_block_bits<Scalar, DIMS>(traits<Scalar>::prec);
    uint32_t* ctab = tabs;
    uint16_t* dtab = (uint16_t*)(tabs + chunk_lut_bytes<DIMS>() / 4);
    constexpr uint32_t kLutEnd = chunk_lut_bytes<DIMS>() / 16;
    for (uint32_t i = threadIdx.x; i < kLutEnd; i += blockDim.x) ((uint4*)ctab)[i] = ((const uint4*)g_chunk_lut.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Plane1dDecLut) / 16; i += blockDim.x)
        ((uint4*)dtab)[i] = ((const uint4*)g_plane1d_lut.e)[i];
    uint32_t* L = (uint32_t*)lds + lane;
    uint32_t olen = 0;  // a lane past the last region block decodes a zero block and loads nothing
    uint64_t ooff = 0;
    if (live) {
      const uint32_t b = region_block<DIMS>(rg, r).b;
      olen = variable_budget(src_lengths[b], kMaxLen, traits<Scalar>::ebits);
      if (olen) ooff = variable_block_offset(src_index, src_lengths, b);  // (a zero block reads nothing)
    }
    const uint32_t Dl = (olen + 31) >> 5;  // dwords of the lane's block, <= D
    if (live_wave) {
      const uint32_t* base = (const uint32_t*)src;
      const uint32_t s0 = (uint32_t)ooff & 31u;
      uint64_t d;
      uint32_t prev = (Dl && variable_stream_dword(ooff, 0, src_dwords, d)) ? base[d] : 0u;
      // rows: the longest block of the wave (<= D) and the reader's slack
      uint32_t rows = Dl;
      for (int o = 32; o; o >>= 1) rows = max(rows, (uint32_t)__shfl_xor((int)rows, o));
      rows += 5;
      for (uint32_t j = 0; j < rows; j++) {
        uint32_t v = 0;
        if (j < Dl) {
          const uint32_t nxt = variable_stream_dword(ooff, j + 1, src_dwords, d) ? base[d] : 0u;
          v = __builtin_amdgcn_alignbit(nxt, prev, s0);
          prev = nxt;
          // the block reads as zeros past its last bit (the plane steps rely on it)
          if (j + 1 == Dl && (olen & 31u)) v &= (1u << (olen & 31u)) - 1u;
        }
        L[j * 64] = v;
      }
    }
    __syncthreads();
    if (live_wave) {
      wave_lds_sync();
      LdsReader<false> rd;
      rd.lds32 = L;
      rd.lut32 = ctab;
      rd.d1d = dtab;
      rd.init(0);
      // (a zero column's first bit is 0: decode_block takes it as the zero block whatever the budget is)
      if (!decode_block<Scalar, DIMS>(f, olen ? olen : traits<Scalar>::ebits + 2u, rd)) {
#pragma unroll
        for (int i = 0; i < N; i++) f[i] = (Scalar)0;
      }
      // the values are final here (see zfp_decode_region_body)
#pragma unroll
      for (int i = 0; i < N; i++) asm volatile("" : "+v"(f[i]));
      if (r < rg.nrb) {
        uint32_t r2 = r;
        asm volatile("" : "+v"(r2));
        const RegionBlock rb = region_block<DIMS>(rg, r2);
        overlay_region<Scalar, DIMS>(box, rg, rb, f);
        pad_block<Scalar, DIMS>(g, rg, rb, f);
      }
      wave_lds_sync();  // the decoder's reads of the image
    }
    if constexpr (ENCODE) __syncthreads();  // every wave has read the decoder's tables for the last time
  } else {
    if (live) {
      gather_region<Scalar, DIMS>(box, g, rg, region_block<DIMS>(rg, r), g.row_stage != 0, f);
    } else {
#pragma unroll
      for (int i = 0; i < N; i++) f[i] = (Scalar)0;
    }
  }
  if constexpr (!ENCODE) {
    if (live) {
      uint32_t r2 = r;
      asm volatile("" : "+v"(r2));
      lengths[region_block<DIMS>(rg, r2).b] = (uint16_t)block_length<Scalar, DIMS>(f, maxprec, minexp);
    }
  } else {
    // the encoder's tables (over the decoder's) and the zeroed column
    uint32_t* stab = tabs;
    uint32_t* ptab = tabs + kSpreadTabBytes / 4;
    for (uint32_t i = threadIdx.x; i < kSpreadTabBytes / 16; i += blockDim.x)
      ((uint4*)stab)[i] = ((const uint4*)g_spread_tab.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Pair1dLut) / 16; i += blockDim.x)
        ((uint4*)ptab)[i] = ((const uint4*)g_pair1d_lut.e)[i];
    const uint32_t W = g.maxbits >> 6;
    if (live_wave)
      for (uint32_t j = 0; j < W + kSlackWords; j++) mine[j * 64] = 0;
    // the writer's limit: the length the first pass found (a lane past the last
    // region block codes a zero block with limit 0 and stores nothing)
    uint32_t len = 0;
    if (live) len = min((uint32_t)lengths[region_block<DIMS>(rg, r).b], g.maxbits);
    if (len <= 1u) {  // the zero block, as zfp_encode_variable codes it
#pragma unroll
      for (int i = 0; i < N; i++) f[i] = (Scalar)0;
    }
    __syncthreads();
    if (!live_wave) return;
    wave_lds_sync();
    {
      LdsOrWriter<false> wr{mine, (lds_spread*)stab, 0, len, (P1dPtr)ptab, uniform_const64(0x7fffu)};
      encode_block<Scalar, DIMS>(f, g.maxbits, wr);
    }
    wave_lds_sync();
    if (r < rg.nrb) {
      // the block's place again, from r alone (nothing else stays live across the coder)
      uint32_t r2 = r;
      asm volatile("" : "+v"(r2));
      const uint32_t b = region_block<DIMS>(rg, r2).b;
      store_block_variable(dst, cap_words, mine, offsets[b], min((uint32_t)lengths[b], g.maxbits));
    }
  }
}

// Copy pass.  One wave a workgroup, wave w for blocks 64 w .. 64 w + 63, which
// are contiguous in both streams.  The source offset of a lane's block is
// src_index[w] plus the wave's exclusive prefix sum of the raw source lengths
// (< 2^22).  Untouched lanes OR their block's bits into the segment at the new
// offsets, exactly as zfp_truncate_variable_copy does; a touched lane adds
// nothing, so its block's place stays zero for the encode pass.  Lane 0 stores
// the wave's entry of the new index, and wave 0 the total.
//
// LDS: (longest block of the type + 2) words, as the truncate copy.
template <typename Scalar, int DIMS>
__global__ __launch_bounds__(kLanes) void zfp_update_variable_copy(
    const uint32_t* __restrict__ src, uint64_t src_dwords, const uint16_t* __restrict__ src_lengths,
    const uint64_t* __restrict__ src_index, const uint16_t* __restrict__ lengths,
    const uint64_t* __restrict__ offsets, Geometry g, Region rg, uint64_t* __restrict__ dst, uint64_t cap_words,
    uint64_t* __restrict__ dst_index, const uint64_t* __restrict__ total) {
  constexpr uint32_t kLongest = variable_longest_block<Scalar, DIMS>();
  constexpr uint32_t kSegWords = kLongest + 2;  // 64 blocks of kLongest bits from bit sh0 < 64 on: <= kLongest + 1 words
  __shared__ uint64_t seg[kSegWords];
  const uint32_t lane = threadIdx.x;
  const uint32_t b = blockIdx.x * kLanes + lane;
  uint32_t len = 0, slen = 0;
  uint64_t off = 0;
  bool touched = false;
  if (b < g.nblocks) {
    len = lengths[b];
    off = offsets[b];
    slen = src_lengths[b];
    const BlockPos bp = block_pos<DIMS>(g, b);
    touched = bp.ix - rg.bx0 < rg.rbx && bp.iy - rg.by0 < rg.rby && bp.iz - rg.bz0 < rg.rbz;
  }
  uint32_t inc = slen;  // inclusive prefix sum over the wave, <= 64 * 65535
  for (uint32_t d = 1; d < kLanes; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
    if (lane >= d) inc += t;
  }
  const uint64_t soff = src_index[blockIdx.x] + (inc - slen);
  len = len < kLongest ? len : kLongest;  // an untouched length is the source's, whatever it holds
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
  if (len > 1u && !touched) {
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

template <typename Scalar, int DIMS, bool ENCODE>
static int launch_update_region_variable_pass(const Scalar* box, const Geometry& g0, const Region& rg, bool covered,
                                              uint32_t maxprec, int minexp, const uint64_t* src, uint64_t src_dwords,
                                              const uint16_t* src_lengths, const uint64_t* src_index,
                                              uint16_t* lengths, const uint64_t* offsets, uint64_t* dst,
                                              uint64_t cap_words, hipStream_t st) {
  Geometry g = g0;
  constexpr uint32_t D = (max_block_bits<Scalar, DIMS>(traits<Scalar>::prec) + 31) / 32;
  const uint32_t enc = ENCODE ? ((g.maxbits >> 6) + kSlackWords) * 64 : 0u;  // the encoder's column
  const uint32_t dec = covered ? 0u : (D + 5) * 32;                          // the decoder's
  g.lds_words = enc > dec ? enc : dec;
  const size_t kStatic =
      covered ? variable_update_tab_bytes<DIMS, false, ENCODE>() : variable_update_tab_bytes<DIMS, true, ENCODE>();
  if ((size_t)g.lds_words * 8 + kStatic > lds_cap_bytes()) return CUZFP_ERROR_INVALID_ARGUMENT;
  const uint32_t wpg = waves_per_group(g.lds_words, kStatic, kUpdWaves);
  const dim3 grid((g.wave_end + wpg - 1) / wpg), block(kLanes * wpg);
  const size_t lds = (size_t)wpg * g.lds_words * 8;
  if (covered)
    hipLaunchKernelGGL((zfp_update_region_variable<Scalar, DIMS, false, ENCODE>), grid, block, lds, st, box, g, rg,
                       maxprec, minexp, src, src_dwords, src_lengths, src_index, lengths, offsets, dst, cap_words);
  else
    hipLaunchKernelGGL((zfp_update_region_variable<Scalar, DIMS, true, ENCODE>), grid, block, lds, st, box, g, rg,
                       maxprec, minexp, src, src_dwords, src_lengths, src_index, lengths, offsets, dst, cap_words);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

// covered, rows: as launch_encode_region_t.  offsets (nblocks words) and
// partials (variable_tiles) are the workspace; dst_index may be null.
template <typename Scalar, int DIMS>
int launch_encode_region_variable_t(const void* box, const Geometry& g0, const Region& rg, bool covered, bool rows,
                                    uint32_t maxprec, int minexp, const uint64_t* src, size_t src_bytes,
                                    const uint16_t* src_lengths, const uint64_t* src_index, uint64_t* dst,
                                    uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                                    uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  Geometry g = g0;
  g.maxbits = 64 * variable_update_column_words<Scalar, DIMS>(maxprec);
  g.wave0 = 0;
  g.wave_end = (rg.nrb + kLanes - 1) / kLanes;
  g.row_stage = covered && rows;
  const Scalar* d = (const Scalar*)box;
  const uint64_t dwords = (uint64_t)(src_bytes / 4);
  hipError_t e = hipMemcpyAsync(lengths, src_lengths, 2 * (size_t)g.nblocks, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) {
    t_last_hip = e;
    return CUZFP_ERROR_HIP;
  }
  int rc = launch_update_region_variable_pass<Scalar, DIMS, false>(d, g, rg, covered, maxprec, minexp, src, dwords,
                                                                   src_lengths, src_index, lengths, offsets, dst,
                                                                   cap_words, st);
  if (rc) return rc;
  rc = launch_variable_scan(lengths, g.nblocks, offsets, partials, total, st);
  if (rc) return rc;
  rc = launch_variable_zero(dst, cap_words, offsets, g.nblocks, total, st);
  if (rc) return rc;
  hipLaunchKernelGGL((zfp_update_variable_copy<Scalar, DIMS>), dim3((g.nblocks + kLanes - 1) / kLanes), dim3(kLanes), 0,
                     st, (const uint32_t*)src, dwords, src_lengths, src_index, (const uint16_t*)lengths,
                     (const uint64_t*)offsets, g, rg, dst, cap_words, dst_index, (const uint64_t*)total);
  e = hipGetLastError();
  t_last_hip = e;
  if (e != hipSuccess) return CUZFP_ERROR_HIP;
  return launch_update_region_variable_pass<Scalar, DIMS, true>(d, g, rg, covered, maxprec, minexp, src, dwords,
                                                                src_lengths, src_index, lengths, offsets, dst,
                                                                cap_words, st);
}

template <typename Scalar>
int launch_encode_region_variable_type(const Problem& p, const Region& r, const void* box, bool covered, bool rows,
                                       uint32_t maxprec, int minexp, const uint64_t* src, size_t src_bytes,
                                       const uint16_t* src_lengths, const uint64_t* src_index, uint64_t* dst,
                                       uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                                       uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_encode_region_variable_t<Scalar, 1>(box, p.g, r, covered, rows, maxprec, minexp, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
    case 2: return launch_encode_region_variable_t<Scalar, 2>(box, p.g, r, covered, rows, maxprec, minexp, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
    default: return launch_encode_region_variable_t<Scalar, 3>(box, p.g, r, covered, rows, maxprec, minexp, src, src_bytes, src_lengths, src_index, dst, cap_words, lengths, dst_index, total, offsets, partials, st);
  }
}

}  // namespace cuzfp
