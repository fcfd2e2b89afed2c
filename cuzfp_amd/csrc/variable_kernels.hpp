// cuzfp_amd/csrc/variable_kernels.hpp -- the variable-rate modes (fixed
// precision, fixed accuracy: cuzfp_hip_encode_variable / _decode_variable).
//
// A variable-rate stream is the blocks of the array in raster order, back to
// back, block b taking lengths[b] bits (zfp_block.hpp, block_length); the
// index `lengths` is what lets one lane own one block on either side.
//
//   encode:  zfp_variable_lengths   L_b of every block            -> lengths
//            scan (three launches)  exclusive sum, 64-bit         -> offsets, total
//            variable_zero_shared   the words two waves' segments can share
//            zfp_encode_variable    encode_block behind an LdsOrWriter whose
//                                   limit is the lane's own L_b (reloaded),
//                                   the wave's columns packed into its
//                                   segment [offsets[b0], offsets[b0 + 64))
//                                   in LDS and copied out
//   decode:  scan                                                  -> offsets
//            zfp_decode_variable    the region decoder's lane-owned copy-in
//                                   from offsets[b], decode_block with budget
//                                   L_b, the whole-array decoder's store
//
// The scan is reduce-then-scan over separate launches: no workgroup waits on
// another.  The coder functions are the fixed-rate kernels', unchanged.
//
// Instantiated per scalar type in variable_{f32,f64}.hip.
#pragma once
#include <algorithm>

#include "kernels.hpp"

namespace cuzfp {

// ---------------------------------------------------------------------------
// Offsets: exclusive scan of the uint16 lengths to 64-bit bit offsets.  A tile
// is kScanTile lengths, one workgroup of kScanThreads threads with kScanItems
// consecutive lengths a thread.
constexpr uint32_t kScanThreads = 256, kScanItems = 4, kScanTile = kScanThreads * kScanItems;

static_assert(kScanTile == kVariableScanTile, "variable_tiles (launch.hpp) sizes the workspace");

// inclusive scan of one value a thread over the workgroup (Hillis-Steele in
// LDS); returns the thread's inclusive sum, `all` the workgroup's total
__device__ __forceinline__ uint64_t group_scan(uint64_t v, uint64_t* sh, uint64_t& all) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
    const uint64_t a = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const uint64_t r = sh[t];
  all = sh[kScanThreads - 1];
  __syncthreads();
  return r;
}

#if defined(CUZFP_VARIABLE_SHARED_UNIT)  // the type-independent kernels: one unit defines them
// tile sums
__global__ __launch_bounds__(kScanThreads) void variable_tile_sums(const uint16_t* __restrict__ lengths, uint32_t n,
                                                                   uint64_t* __restrict__ partials) {
  __shared__ uint64_t sh[kScanThreads];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint64_t v = 0;
  for (uint32_t k = 0; k < kScanItems; k++)
    if (i0 + k < n) v += lengths[i0 + k];
  uint64_t all;
  group_scan(v, sh, all);
  if (threadIdx.x == 0) partials[blockIdx.x] = all;
}

// the tile sums to their exclusive prefix, in place, by one workgroup (a chunk
// of kScanThreads sums a trip, the running total carried); the grand total to
// *total when it is not null
__global__ __launch_bounds__(kScanThreads) void variable_scan_partials(uint64_t* __restrict__ partials, uint32_t ntiles,
                                                                       uint64_t* __restrict__ total) {
  __shared__ uint64_t sh[kScanThreads];
  uint64_t carry = 0;
  for (uint32_t c = 0; c < ntiles; c += kScanThreads) {
    const uint32_t i = c + threadIdx.x;
    const uint64_t v = i < ntiles ? partials[i] : 0ull;
    uint64_t all;
    const uint64_t inc = group_scan(v, sh, all);
    if (i < ntiles) partials[i] = carry + inc - v;
    carry += all;
  }
  if (total && threadIdx.x == 0) *total = carry;
}

// offsets[b] = the tile's prefix + the exclusive sum inside the tile
__global__ __launch_bounds__(kScanThreads) void variable_tile_offsets(const uint16_t* __restrict__ lengths, uint32_t n,
                                                                      const uint64_t* __restrict__ partials,
                                                                      uint64_t* __restrict__ offsets) {
  __shared__ uint64_t sh[kScanThreads];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint32_t l[kScanItems];
  uint64_t v = 0;
  for (uint32_t k = 0; k < kScanItems; k++) {
    l[k] = i0 + k < n ? lengths[i0 + k] : 0u;
    v += l[k];
  }
  uint64_t all;
  uint64_t o = partials[blockIdx.x] + group_scan(v, sh, all) - v;
  for (uint32_t k = 0; k < kScanItems; k++) {
    if (i0 + k < n) offsets[i0 + k] = o;
    o += l[k];
  }
}

// The stream words that wave segments can share, zeroed: the word holding the
// first bit of every wave's segment (thread i < nwaves: block 64 i) and the
// word the stream ends in (thread nwaves).  These are the words the encoder
// ORs into (zfp_encode_variable's copy-out); every other word it stores whole.
__global__ __launch_bounds__(256) void variable_zero_shared(uint64_t* __restrict__ stream, uint64_t cap_words,
                                                            const uint64_t* __restrict__ offsets, uint32_t nwaves,
                                                            const uint64_t* __restrict__ total) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > nwaves) return;
  const uint64_t bit = i < nwaves ? offsets[(uint64_t)i * kLanes] : *total;
  if (i == nwaves && !(bit & 63)) return;  // the stream ends with a whole word
  const uint64_t w = bit >> 6;
  if (w < cap_words) stream[w] = 0;
}

int launch_variable_scan(const uint16_t* lengths, uint32_t nblocks, uint64_t* offsets, uint64_t* partials,
                         uint64_t* total, hipStream_t st) {
  const uint32_t nt = variable_tiles(nblocks);
  hipLaunchKernelGGL(variable_tile_sums, dim3(nt), dim3(kScanThreads), 0, st, lengths, nblocks, partials);
  hipLaunchKernelGGL(variable_scan_partials, dim3(1), dim3(kScanThreads), 0, st, partials, nt, total);
  hipLaunchKernelGGL(variable_tile_offsets, dim3(nt), dim3(kScanThreads), 0, st, lengths, nblocks,
                     (const uint64_t*)partials, offsets);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

int launch_variable_zero(uint64_t* stream, uint64_t cap_words, const uint64_t* offsets, uint32_t nblocks,
                         const uint64_t* total, hipStream_t st) {
  if (!cap_words) return CUZFP_SUCCESS;
  const uint32_t nwaves = (nblocks + kLanes - 1) / kLanes;
  hipLaunchKernelGGL(variable_zero_shared, dim3(nwaves / 256 + 1), dim3(256), 0, st, stream, cap_words, offsets,
                     nwaves, total);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}
#endif  // CUZFP_VARIABLE_SHARED_UNIT

// ---------------------------------------------------------------------------
// Length pass: one lane, one block.

template <typename Scalar, int DIMS, bool FAST>
__global__ __launch_bounds__(256) void zfp_variable_lengths(const Scalar* __restrict__ data, Geometry g,
                                                            uint32_t maxprec, int minexp,
                                                            uint16_t* __restrict__ lengths) {
  constexpr int N = 1 << (2 * DIMS);
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  if (b >= g.nblocks) return;
  Scalar f[N];
  gather<Scalar, DIMS, FAST>(data, g, block_pos<DIMS>(g, b), f);
  lengths[b] = (uint16_t)block_length<Scalar, DIMS>(f, maxprec, minexp);
}

// ---------------------------------------------------------------------------
// Encode pass.  One wave a workgroup.  The wave's image is the fixed-rate
// encoder's lane-interleaved one (word j of lane l's block at lds[64 j + l]):
// W = g.maxbits / 64 words a column, covering the longest block the mode can
// produce, plus kSlackWords rows.  A lane's writer stops at its own length:
// what the coder produces past it lands in the column's rows after it
// (LdsOrWriter::settle) and is masked off below.  A block whose length is 1 --
// all zero, or below the mode's precision -- is coded as the zero block by
// zeroing its values.
//
// The wave's 64 blocks are contiguous in the stream: bits [off0, off0 + S).
// Its lanes pack their columns into a second LDS array `seg`, word k of which
// is stream word (off0 >> 6) + k (ds_or_b64 at each lane's bit position, the
// LDS writer's own idiom), and the wave copies seg out in lane order.  Only
// the segment's first word, and its last when the segment ends inside it, can
// hold another wave's bits -- a whole wave of 1-bit blocks lies inside one
// such word -- and those are OR-ed into the stream, which
// variable_zero_shared zeroed there; every other word is stored whole.  No
// word at or past cap_words is touched.
//
// LDS a wave: ((W + 6) * 64 + 64 W + 2) * 8 bytes beside 2 KiB of tables (6
// KiB in 1D): 70.7 KiB for 3D double (W = 66), 36.5 KiB for 3D float.
template <typename Scalar, int DIMS, bool FAST>
__global__ __launch_bounds__(kLanes) void zfp_encode_variable(const Scalar* __restrict__ data, Geometry g,
                                                              const uint16_t* __restrict__ lengths,
                                                              const uint64_t* __restrict__ offsets,
                                                              uint64_t* __restrict__ stream, uint64_t cap_words) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_all[];
  __shared__ __attribute__((aligned(16))) uint32_t stab[512];  // LDS address 0 (static): the spread tables
  __shared__ __attribute__((aligned(16))) uint32_t ptab[DIMS == 1 ? 1024 : 4];  // 1D: the pair table
  constexpr int N = 1 << (2 * DIMS);
  const uint32_t lane = threadIdx.x;
  const uint32_t b = blockIdx.x * kLanes + lane;
  for (uint32_t i = lane; i < kSpreadTabBytes / 16; i += kLanes) ((uint4*)stab)[i] = ((const uint4*)g_spread_tab.e)[i];
  if constexpr (DIMS == 1)
    for (uint32_t i = lane; i < sizeof(Pair1dLut) / 16; i += kLanes) ((uint4*)ptab)[i] = ((const uint4*)g_pair1d_lut.e)[i];
  const uint32_t W = g.maxbits >> 6;
  uint64_t* mine = lds_all + lane;
  uint64_t* seg = lds_all + (size_t)(W + kSlackWords) * kLanes;
  Scalar f[N];
  uint32_t len = 0;
  uint64_t off = 0;
  if (b < g.nblocks) {
    gather<Scalar, DIMS, FAST>(data, g, block_pos<DIMS>(g, b), f);
    len = lengths[b];
    off = offsets[b];
  }
  // (a lane past the last block codes a zero block with limit 0 and packs nothing)
  if (len <= 1u) {
#pragma unroll
    for (int i = 0; i < N; i++) f[i] = (Scalar)0;
  }
  // the segment: from lane 0's offset (always a live block) over S bits, the
  // end of the last live block; a lane's place in it is rel
  const uint64_t off0 = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)off) |
                        ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(off >> 32)) << 32);
  const uint32_t sh0 = (uint32_t)off0 & 63u;
  const uint32_t rel = len ? (uint32_t)(off - off0) + sh0 : 0u;  // < 64 + 64 * 64 W
  uint32_t S = rel + len, wmax = len;
  for (int o = 32; o; o >>= 1) {
    S = max(S, (uint32_t)__shfl_xor((int)S, o));
    wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, o));
  }
  const uint32_t nseg = (S + 63) >> 6;  // <= 64 W + 1 words
  // own column: the rows the longest block of the wave reaches plus the slack
  // (1D: the whole column, see variable_column_words)
  const uint32_t rows = (DIMS == 1 ? W : min(W, (wmax + 63) >> 6)) + kSlackWords;
  for (uint32_t j = 0; j < rows; j++) mine[j * 64] = 0;
  for (uint32_t k = lane; k < nseg; k += kLanes) seg[k] = 0;
  __syncthreads();  // the tables, the zeroed image and segment (one wave: its own writes)
  {
    LdsOrWriter<false> wr{mine, (lds_spread*)stab, 0, len, (lds_spread*)ptab, uniform_const64(0x7fffu)};
    encode_block<Scalar, DIMS>(f, g.maxbits, wr);
  }
  wave_lds_sync();
  const uint32_t nw = (len + 63) >> 6;  // <= W
  for (uint32_t j = 0; j < nw; j++) {
    uint64_t v = mine[j * 64];
    const uint32_t left = len - 64 * j;
    if (left < 64) v &= lowmask(left);
    const uint32_t bit = rel + 64 * j, k = bit >> 6, sh = bit & 63u;
    const uint64_t lo = v << sh;
    const uint64_t hi = sh ? v >> (64 - sh) : 0ull;
    if (lo) atomicOr((unsigned long long*)&seg[k], (unsigned long long)lo);
    if (hi) atomicOr((unsigned long long*)&seg[k + 1], (unsigned long long)hi);  // k + 1 < nseg: the block has bits there
  }
  wave_lds_sync();
  __syncthreads();
  const uint64_t w0 = off0 >> 6;
  const bool open_end = (S & 63u) != 0;  // the segment ends inside its last word
  for (uint32_t k = lane; k < nseg; k += kLanes) {
    const uint64_t v = seg[k];
    const uint64_t w = w0 + k;
    if (w >= cap_words) break;
    if (k == 0 || (k + 1 == nseg && open_end)) {
      if (v) atomicOr((unsigned long long*)&stream[w], (unsigned long long)v);
    } else {
      stream[w] = v;
    }
  }
}

// the image's words a column (without the slack rows): the longest block of
// the mode; 1D columns take the type's longest whatever maxprec is (the 1D
// pair coder does not settle a full lane, so a column holds all a 1D block
// can ever produce)
template <typename Scalar, int DIMS>
inline uint32_t variable_column_words(uint32_t maxprec) {
  const uint32_t bits = max_block_bits<Scalar, DIMS>(DIMS == 1 ? (uint32_t)traits<Scalar>::prec : maxprec);
  return (bits + 63) / 64;
}

template <typename Scalar, int DIMS>
int launch_encode_variable_t(const void* data, const Geometry& g0, bool fast, uint32_t maxprec, int minexp,
                             uint64_t* stream, uint64_t cap_words, uint16_t* lengths, uint64_t* total,
                             uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  Geometry g = g0;
  const Scalar* d = (const Scalar*)data;
  const uint32_t W = variable_column_words<Scalar, DIMS>(maxprec);
  g.maxbits = 64 * W;
  const size_t lds = ((size_t)(W + kSlackWords) * kLanes + (size_t)kLanes * W + 2) * 8;  // image + segment
  if (lds + sizeof(SpreadTab) + sizeof(Pair1dLut) > lds_cap_bytes()) return CUZFP_ERROR_INVALID_ARGUMENT;
  const dim3 lgrid((g.nblocks + 255) / 256), lblock(256);
  if (fast)
    hipLaunchKernelGGL((zfp_variable_lengths<Scalar, DIMS, true>), lgrid, lblock, 0, st, d, g, maxprec, minexp, lengths);
  else
    hipLaunchKernelGGL((zfp_variable_lengths<Scalar, DIMS, false>), lgrid, lblock, 0, st, d, g, maxprec, minexp, lengths);
  int rc = launch_variable_scan(lengths, g.nblocks, offsets, partials, total, st);
  if (rc) return rc;
  rc = launch_variable_zero(stream, cap_words, offsets, g.nblocks, total, st);
  if (rc) return rc;
  const dim3 grid((g.nblocks + kLanes - 1) / kLanes), block(kLanes);
  if (fast)
    hipLaunchKernelGGL((zfp_encode_variable<Scalar, DIMS, true>), grid, block, lds, st, d, g, (const uint16_t*)lengths,
                       (const uint64_t*)offsets, stream, cap_words);
  else
    hipLaunchKernelGGL((zfp_encode_variable<Scalar, DIMS, false>), grid, block, lds, st, d, g, (const uint16_t*)lengths,
                       (const uint64_t*)offsets, stream, cap_words);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

// ---------------------------------------------------------------------------
// Decode pass: the region decoder's lane-owned copy-in (region_kernels.hpp)
// with a per-lane bit offset and a per-lane budget.  Every lane's column is
// D = ceil(longest block of the type / 32) dwords plus the reader's 5 slack
// rows; a lane fills the dwords its own length covers and zeroes the rest up
// to the wave's longest block and the slack.
//
// The index is not trusted.  A length is clamped to the type's longest block,
// a length that no coded block can have (2 .. ebits + 1) reads as a zero
// block, and every stream dword is loaded behind `d < stream_dwords` (a dword
// outside the stream reads as zero), so no load leaves [stream, stream +
// stream_bytes) whatever the index holds; the image's bounds follow from the
// clamp.
template <typename Scalar, int DIMS, bool FAST>
__device__ __forceinline__ void zfp_decode_variable_body(const uint64_t* __restrict__ stream, uint64_t stream_dwords,
                                                         const uint16_t* __restrict__ lengths,
                                                         const uint64_t* __restrict__ offsets, const Geometry& g,
                                                         Scalar* __restrict__ out, uint32_t* ctab, uint16_t* dtab) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_all[];
  constexpr int N = 1 << (2 * DIMS);
  constexpr uint32_t kMaxLen = max_block_bits<Scalar, DIMS>(traits<Scalar>::prec);
  constexpr uint32_t D = (kMaxLen + 31) / 32;
  const uint32_t wig = wave_in_group();
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + wig;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t b = wave * kLanes + lane;
  const bool live = b < g.nblocks;
  uint64_t* lds = lds_all + (size_t)wig * g.lds_words;
  uint32_t* L = (uint32_t*)lds + lane;
  {
    constexpr uint32_t kLutEnd = DIMS == 1 ? kLutPairs * 4 / 16 : sizeof(ChunkLut) / 16;
    for (uint32_t i = threadIdx.x; i < kLutEnd; i += blockDim.x) ((uint4*)ctab)[i] = ((const uint4*)g_chunk_lut.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Plane1dDecLut) / 16; i += blockDim.x)
        ((uint4*)dtab)[i] = ((const uint4*)g_plane1d_lut.e)[i];
  }
  uint32_t len = 1;  // a lane past the last block decodes a zero block (its stores are skipped)
  uint64_t off = 0;
  if (live) {
    len = lengths[b];
    off = offsets[b];
  }
  len = len < kMaxLen ? len : kMaxLen;
  if (len < traits<Scalar>::ebits + 2u) len = 0;  // the zero block, or no block's length: nothing is read
  const uint32_t Dl = (len + 31) >> 5;  // dwords of the lane's block, <= D
  if (wave * kLanes < g.nblocks) {
    const uint32_t* base = (const uint32_t*)stream;
    const uint64_t d0 = off >> 5;
    const uint32_t s0 = (uint32_t)off & 31u;
    uint32_t prev = (Dl && d0 < stream_dwords) ? base[d0] : 0u;
    // rows: the longest block of the wave (<= D) and the reader's slack
    uint32_t rows = Dl;
    for (int o = 32; o; o >>= 1) rows = max(rows, (uint32_t)__shfl_xor((int)rows, o));
    rows += 5;
    for (uint32_t j = 0; j < rows; j++) {
      uint32_t v = 0;
      if (j < Dl) {
        const uint64_t d = d0 + j + 1;
        const uint32_t nxt = d < stream_dwords ? base[d] : 0u;
        v = __builtin_amdgcn_alignbit(nxt, prev, s0);
        prev = nxt;
        // the block reads as zeros past its last bit (the plane steps rely on it)
        if (j + 1 == Dl && (len & 31u)) v &= (1u << (len & 31u)) - 1u;
      }
      L[j * 64] = v;
    }
  }
  __syncthreads();
  if (wave * kLanes >= g.nblocks) return;
  wave_lds_sync();
  Scalar f[N];
  LdsReader<false> rd;
  rd.lds32 = L;
  rd.lut32 = ctab;
  rd.d1d = dtab;
  rd.init(0);
  // (a zero column's first bit is 0: decode_block takes it as the zero block whatever len is)
  const bool coded = decode_block<Scalar, DIMS>(f, len ? len : traits<Scalar>::ebits + 2u, rd);
  if (!coded) {
#pragma unroll
    for (int i = 0; i < N; i++) f[i] = (Scalar)0;
  }
  if (live) scatter<Scalar, DIMS, FAST>(out, g, block_pos<DIMS>(g, b), f);
}

template <typename Scalar, int DIMS, bool FAST>
__global__ __launch_bounds__(kLanes * kDecWaves) void zfp_decode_variable(const uint64_t* __restrict__ stream,
                                                                         uint64_t stream_dwords,
                                                                         const uint16_t* __restrict__ lengths,
                                                                         const uint64_t* __restrict__ offsets,
                                                                         Geometry g, Scalar* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t ctab[chunk_lut_bytes<DIMS>() / 4];  // LDS address 0 (static)
  __shared__ __attribute__((aligned(16))) uint16_t dtab[DIMS == 1 ? sizeof(Plane1dDecLut) / 2 : 8];
  zfp_decode_variable_body<Scalar, DIMS, FAST>(stream, stream_dwords, lengths, offsets, g, out, ctab, dtab);
}

template <typename Scalar, int DIMS>
int launch_decode_variable_t(const uint64_t* stream, size_t stream_bytes, const uint16_t* lengths,
                             const Geometry& g0, bool fast, void* out, uint64_t* offsets, uint64_t* partials,
                             hipStream_t st) {
  Geometry g = g0;
  constexpr uint32_t D = (max_block_bits<Scalar, DIMS>(traits<Scalar>::prec) + 31) / 32;
  g.lds_words = (D + 5) * 32;  // (dwords a column + 5 slack rows) x 64 lanes
  g.row_stage = 0;
  const size_t kStatic = chunk_lut_bytes<DIMS>() + (DIMS == 1 ? sizeof(Plane1dDecLut) : 16);
  if ((size_t)g.lds_words * 8 + kStatic > lds_cap_bytes()) return CUZFP_ERROR_INVALID_ARGUMENT;
  int rc = launch_variable_scan(lengths, g.nblocks, offsets, partials, nullptr, st);
  if (rc) return rc;
  const uint32_t nwaves = (g.nblocks + kLanes - 1) / kLanes;
  const uint32_t wpg = waves_per_group(g.lds_words, kStatic, kDecWaves);
  const dim3 grid((nwaves + wpg - 1) / wpg), block(kLanes * wpg);
  const size_t lds = (size_t)wpg * g.lds_words * 8;
  const uint64_t dwords = (uint64_t)(stream_bytes / 4);
  Scalar* d = (Scalar*)out;
  if (fast)
    hipLaunchKernelGGL((zfp_decode_variable<Scalar, DIMS, true>), grid, block, lds, st, stream, dwords, lengths,
                       (const uint64_t*)offsets, g, d);
  else
    hipLaunchKernelGGL((zfp_decode_variable<Scalar, DIMS, false>), grid, block, lds, st, stream, dwords, lengths,
                       (const uint64_t*)offsets, g, d);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

template <typename Scalar>
int launch_encode_variable_type(const Problem& p, const void* data, bool fast, uint32_t maxprec, int minexp,
                                uint64_t* stream, uint64_t cap_words, uint16_t* lengths, uint64_t* total,
                                uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_encode_variable_t<Scalar, 1>(data, p.g, fast, maxprec, minexp, stream, cap_words, lengths, total, offsets, partials, st);
    case 2: return launch_encode_variable_t<Scalar, 2>(data, p.g, fast, maxprec, minexp, stream, cap_words, lengths, total, offsets, partials, st);
    default: return launch_encode_variable_t<Scalar, 3>(data, p.g, fast, maxprec, minexp, stream, cap_words, lengths, total, offsets, partials, st);
  }
}

template <typename Scalar>
int launch_decode_variable_type(const Problem& p, const uint64_t* stream, size_t stream_bytes,
                                const uint16_t* lengths, bool fast, void* out, uint64_t* offsets,
                                uint64_t* partials, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_decode_variable_t<Scalar, 1>(stream, stream_bytes, lengths, p.g, fast, out, offsets, partials, st);
    case 2: return launch_decode_variable_t<Scalar, 2>(stream, stream_bytes, lengths, p.g, fast, out, offsets, partials, st);
    default: return launch_decode_variable_t<Scalar, 3>(stream, stream_bytes, lengths, p.g, fast, out, offsets, partials, st);
  }
}

}  // namespace cuzfp
