// cuzfp_amd/csrc/region_variable_coarse_kernels.hpp -- the decode of a sub-box
// of a variable-rate stream at a coarser mode than the one that wrote it
// (cuzfp_hip_decode_region_variable_coarse), straight from the fine stream.
//
//   decode:  zfp_decode_region_variable_coarse   one launch, no workspace
//
// The kernel is zfp_decode_region_variable (region_variable_kernels.hpp: its
// lane mapping, its offset rule, its copy-in bounds, its stores) with one step
// between the lane's offset and its copy-in: the lane walks its own block with
// truncated_block_length (rerate_variable.hpp) through a 64-bit window on the
// stream (source_window.hpp) to the block's length L' at the target mode, and
// decodes with a budget of L' bits -- the zero block, reading nothing further,
// where L' <= 1 (variable_coarse.hpp has the rule and the budget).  The
// copy-in then brings in ceil(L' / 32) dwords, not the source block's, and the
// wave's rows are the longest of the new counts.  decode_block and the stores
// are unchanged.
//
// The image is sized on the host from the target: a column of D =
// ceil(max_block_bits(target maxprec) / 32) dwords and the reader's 5 slack
// rows.  No block a mode with that maxprec codes is longer; the walk over
// arbitrary bits can be, so the budget is clamped to 32 D bits.
//
// Bounds, whatever the stream, the lengths and the index hold: the loads of
// lengths and index are the existing decoder's; the walk loads stream dwords
// behind `d < dwords` only (SourceWindow), moves its cursor by at least one bit
// a trip and ends at the source length clamped to the type's longest block;
// the copy-in loads behind variable_stream_dword and fills Dl <= D rows of the
// rows <= D + 5 the wave writes; the store is scatter_region's, clipped to the
// box.
//
// Instantiated per scalar type in region_variable_coarse_{f32,f64}.hip.
#pragma once
#include "region_kernels.hpp"
#include "source_window.hpp"
#include "variable_coarse.hpp"

namespace cuzfp {

// g: the launch (lds_words = (D + 5) x 32) and, for FAST, the box as an array
// of its own (zfp_decode_region_variable_body).
template <typename Scalar, int DIMS, bool FAST>
__device__ __forceinline__ void zfp_decode_region_variable_coarse_body(
    const uint64_t* __restrict__ stream, uint64_t stream_dwords, const uint16_t* __restrict__ lengths,
    const uint64_t* __restrict__ index, uint32_t maxprec, int minexp, const Geometry& g, const Region& rg,
    Scalar* __restrict__ out, uint32_t* ctab, uint16_t* dtab) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_all[];
  constexpr int N = 1 << (2 * DIMS);
  constexpr uint32_t kMaxLen = max_block_bits<Scalar, DIMS>(traits<Scalar>::prec);
  const uint32_t wig = wave_in_group();
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + wig;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = wave * kLanes + lane;
  const bool wave_live = wave * kLanes < rg.nrb;
  uint64_t* lds = lds_all + (size_t)wig * g.lds_words;
  uint32_t* L = (uint32_t*)lds + lane;
  const uint32_t column_bits = g.lds_words - 5u * 32u;  // 32 D: (lds_words / 32 - 5) dwords of 32 bits
  {
    constexpr uint32_t kLutEnd = DIMS == 1 ? kLutPairs * 4 / 16 : sizeof(ChunkLut) / 16;
    for (uint32_t i = threadIdx.x; i < kLutEnd; i += blockDim.x) ((uint4*)ctab)[i] = ((const uint4*)g_chunk_lut.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Plane1dDecLut) / 16; i += blockDim.x)
        ((uint4*)dtab)[i] = ((const uint4*)g_plane1d_lut.e)[i];
  }
  // the lane's block: its bit offset, the walk to its length at the target
  // mode, its budget (a lane past the last region block, a zero block and a
  // block the target codes no plane of decode a zero block and load nothing
  // further; the first's stores are skipped)
  uint32_t len = 0;
  uint64_t off = 0;
  if (r < rg.nrb) {
    const uint32_t b = region_block<DIMS>(rg, r).b;
    const uint32_t raw = lengths[b];
    if (variable_budget(raw, kMaxLen, traits<Scalar>::ebits)) {
      off = variable_block_offset(index, lengths, b);
      SourceWindow rd{(const uint32_t*)stream, stream_dwords, off};
      const uint32_t walked = truncated_block_length<Scalar, DIMS>(rd, raw, maxprec, minexp);
      len = variable_coarse_budget(raw, walked, column_bits, kMaxLen, traits<Scalar>::ebits);
    }
  }
  const uint32_t Dl = (len + 31) >> 5;  // dwords of the lane's block at the target, <= D
  if (wave_live) {
    const uint32_t* base = (const uint32_t*)stream;
    const uint32_t s0 = (uint32_t)off & 31u;
    uint64_t d;
    uint32_t prev = (Dl && variable_stream_dword(off, 0, stream_dwords, d)) ? base[d] : 0u;
    // rows: the longest block of the wave at the target (<= D) and the reader's slack
    uint32_t rows = Dl;
    for (int o = 32; o; o >>= 1) rows = max(rows, (uint32_t)__shfl_xor((int)rows, o));
    rows += 5;
    for (uint32_t j = 0; j < rows; j++) {
      uint32_t v = 0;
      if (j < Dl) {
        const uint32_t nxt = variable_stream_dword(off, j + 1, stream_dwords, d) ? base[d] : 0u;
        v = __builtin_amdgcn_alignbit(nxt, prev, s0);
        prev = nxt;
        // the block reads as zeros past its last bit at the target (the plane
        // steps rely on it; the source's next planes lie there)
        if (j + 1 == Dl && (len & 31u)) v &= (1u << (len & 31u)) - 1u;
      }
      L[j * 64] = v;
    }
  }
  __syncthreads();
  if (!wave_live) return;
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
  if constexpr (!FAST) {
    // the values are final here (zfp_decode_region_body: keeps the inverse
    // transform's last step out of the store branches)
#pragma unroll
    for (int i = 0; i < N; i++) asm volatile("" : "+v"(f[i]));
  }
  if (r < rg.nrb) {
    // the block's position again, from r alone: only r stays live across the decoder
    uint32_t r2 = r;
    asm volatile("" : "+v"(r2));
    const RegionBlock sb = region_block<DIMS>(rg, r2);
    if constexpr (FAST)
      scatter<Scalar, DIMS, true>(out, g, BlockPos{sb.rx, sb.ry, sb.rz}, f);
    else
      scatter_region<Scalar, DIMS>(out, rg, sb, f);
  }
}

template <typename Scalar, int DIMS, bool FAST>
__global__ __launch_bounds__(kLanes * kDecWaves) void zfp_decode_region_variable_coarse(
    const uint64_t* __restrict__ stream, uint64_t stream_dwords, const uint16_t* __restrict__ lengths,
    const uint64_t* __restrict__ index, uint32_t maxprec, int minexp, Geometry g, Region rg,
    Scalar* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t ctab[chunk_lut_bytes<DIMS>() / 4];  // LDS address 0 (static)
  __shared__ __attribute__((aligned(16))) uint16_t dtab[DIMS == 1 ? sizeof(Plane1dDecLut) / 2 : 8];
  zfp_decode_region_variable_coarse_body<Scalar, DIMS, FAST>(stream, stream_dwords, lengths, index, maxprec, minexp, g,
                                                             rg, out, ctab, dtab);
}

// launch_decode_region_variable_t with the image sized from the target
// precision (1 .. the type's: checked by the caller)
template <typename Scalar, int DIMS>
int launch_decode_region_variable_coarse_t(const uint64_t* stream, size_t stream_bytes, const uint16_t* lengths,
                                           const uint64_t* index, uint32_t maxprec, int minexp, const Geometry& g0,
                                           const Region& rg, bool fast, void* out, hipStream_t st) {
  Geometry g = g0;
  const uint32_t D = variable_coarse_column_dwords<Scalar, DIMS>(maxprec);
  // the box as an array of its own (the fast row stores)
  g.nx = rg.ex;
  g.ny = rg.ey;
  g.nz = rg.ez;
  g.lds_words = (D + 5) * 32;  // (dwords a column + 5 slack rows) x 64 lanes
  g.row_stage = 0;
  const size_t kStatic = chunk_lut_bytes<DIMS>() + (DIMS == 1 ? sizeof(Plane1dDecLut) : 16);
  if ((size_t)g.lds_words * 8 + kStatic > lds_cap_bytes()) return CUZFP_ERROR_INVALID_ARGUMENT;
  const uint32_t nwaves = (rg.nrb + kLanes - 1) / kLanes;
  const uint32_t wpg = waves_per_group(g.lds_words, kStatic, kDecWaves);
  const dim3 grid((nwaves + wpg - 1) / wpg), block(kLanes * wpg);
  const size_t lds = (size_t)wpg * g.lds_words * 8;
  const uint64_t dwords = (uint64_t)(stream_bytes / 4);
  Scalar* d = (Scalar*)out;
  if (fast)
    hipLaunchKernelGGL((zfp_decode_region_variable_coarse<Scalar, DIMS, true>), grid, block, lds, st, stream, dwords,
                       lengths, index, maxprec, minexp, g, rg, d);
  else
    hipLaunchKernelGGL((zfp_decode_region_variable_coarse<Scalar, DIMS, false>), grid, block, lds, st, stream, dwords,
                       lengths, index, maxprec, minexp, g, rg, d);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

template <typename Scalar>
int launch_decode_region_variable_coarse_type(const Problem& p, const Region& r, const uint64_t* stream,
                                              size_t stream_bytes, const uint16_t* lengths, const uint64_t* index,
                                              uint32_t maxprec, int minexp, bool fast, void* out, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_decode_region_variable_coarse_t<Scalar, 1>(stream, stream_bytes, lengths, index, maxprec, minexp, p.g, r, fast, out, st);
    case 2: return launch_decode_region_variable_coarse_t<Scalar, 2>(stream, stream_bytes, lengths, index, maxprec, minexp, p.g, r, fast, out, st);
    default: return launch_decode_region_variable_coarse_t<Scalar, 3>(stream, stream_bytes, lengths, index, maxprec, minexp, p.g, r, fast, out, st);
  }
}

}  // namespace cuzfp
