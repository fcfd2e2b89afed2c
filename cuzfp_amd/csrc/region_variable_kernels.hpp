// cuzfp_amd/csrc/region_variable_kernels.hpp -- the offset index of a
// variable-rate stream (cuzfp_hip_variable_index) and the decode of a sub-box
// through it (cuzfp_hip_decode_region_variable).
//
//   index:   scan (variable_kernels.hpp)  exclusive sum of the lengths -> the
//                                         workspace's offsets, the total -> index[T]
//            variable_pick_index          offsets[64 t]                -> index[t]
//   decode:  zfp_decode_region_variable   one launch, no workspace
//
// The decoder is the sub-box decoder's lane mapping and clipped store
// (region.hpp, region_kernels.hpp: one lane a region block, waves over the
// box's blocks in raster order) around the variable-rate decoder's copy-in
// (variable_kernels.hpp: a per-lane bit offset and budget, a column of D + 5
// rows, a bound test on every stream dword).  A wave's lanes fall into runs of
// rbx consecutive blocks that may straddle index tiles, so nothing is assumed
// of the wave: every lane rebuilds its own offset from its tile's index entry
// and the lengths before it in the tile (variable_index.hpp).
//
// Neither the index nor the lengths are trusted.  The box was checked against
// the array on the host, so every region block b is below nblocks: the loads
// are lengths[64 (b / 64) .. b] and index[b / 64], inside lengths[0 .. nblocks)
// and index[0 .. T).  Whatever they hold, the budget is clamped to the type's
// longest block (the column's size) and every stream dword is loaded behind
// variable_stream_dword, so nothing outside [stream, stream + stream_bytes) is
// read; the store is scatter_region's, clipped to the box.
//
// Instantiated per scalar type in region_variable_{f32,f64}.hip.
#pragma once
#include "region_kernels.hpp"
#include "variable_index.hpp"

namespace cuzfp {

#if defined(CUZFP_VARIABLE_INDEX_UNIT)  // the type-independent part: one unit defines it
// index[t] = offsets[64 t], t < ntiles (64 t < nblocks: the tile is not empty)
__global__ __launch_bounds__(256) void variable_pick_index(const uint64_t* __restrict__ offsets, uint32_t ntiles,
                                                           uint64_t* __restrict__ index) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < ntiles) index[t] = offsets[(uint64_t)t * kIndexTile];
}

int launch_variable_index(const uint16_t* lengths, uint32_t nblocks, uint64_t* index, uint64_t* offsets,
                          uint64_t* partials, hipStream_t st) {
  const uint32_t T = variable_index_tiles(nblocks);
  const int rc = launch_variable_scan(lengths, nblocks, offsets, partials, index + T, st);
  if (rc) return rc;
  hipLaunchKernelGGL(variable_pick_index, dim3((T + 255) / 256), dim3(256), 0, st, (const uint64_t*)offsets, T, index);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}
#endif  // CUZFP_VARIABLE_INDEX_UNIT

// g: the launch (lds_words) and, for FAST, the box as an array of its own
// (nx, ny, nz = ex, ey, ez: the row stores of scatter).
template <typename Scalar, int DIMS, bool FAST>
__device__ __forceinline__ void zfp_decode_region_variable_body(const uint64_t* __restrict__ stream,
                                                                uint64_t stream_dwords,
                                                                const uint16_t* __restrict__ lengths,
                                                                const uint64_t* __restrict__ index,
                                                                const Geometry& g, const Region& rg,
                                                                Scalar* __restrict__ out, uint32_t* ctab,
                                                                uint16_t* dtab) {
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
  {
    constexpr uint32_t kLutEnd = DIMS == 1 ? kLutPairs * 4 / 16 : sizeof(ChunkLut) / 16;
    for (uint32_t i = threadIdx.x; i < kLutEnd; i += blockDim.x) ((uint4*)ctab)[i] = ((const uint4*)g_chunk_lut.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Plane1dDecLut) / 16; i += blockDim.x)
        ((uint4*)dtab)[i] = ((const uint4*)g_plane1d_lut.e)[i];
  }
  // the lane's block: its budget and bit offset (a lane past the last region
  // block decodes a zero block and loads nothing; its stores are skipped)
  uint32_t len = 0;
  uint64_t off = 0;
  if (r < rg.nrb) {
    const uint32_t b = region_block<DIMS>(rg, r).b;
    len = variable_budget(lengths[b], kMaxLen, traits<Scalar>::ebits);
    if (len) off = variable_block_offset(index, lengths, b);  // (a zero block reads nothing)
  }
  const uint32_t Dl = (len + 31) >> 5;  // dwords of the lane's block, <= D
  if (wave_live) {
    const uint32_t* base = (const uint32_t*)stream;
    const uint32_t s0 = (uint32_t)off & 31u;
    uint64_t d;
    uint32_t prev = (Dl && variable_stream_dword(off, 0, stream_dwords, d)) ? base[d] : 0u;
    // rows: the longest block of the wave (<= D) and the reader's slack
    uint32_t rows = Dl;
    for (int o = 32; o; o >>= 1) rows = max(rows, (uint32_t)__shfl_xor((int)rows, o));
    rows += 5;
    for (uint32_t j = 0; j < rows; j++) {
      uint32_t v = 0;
      if (j < Dl) {
        const uint32_t nxt = variable_stream_dword(off, j + 1, stream_dwords, d) ? base[d] : 0u;
        v = __builtin_amdgcn_alignbit(nxt, prev, s0);
        prev = nxt;
        // the block reads as zeros past its last bit (the plane steps rely on it)
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
__global__ __launch_bounds__(kLanes * kDecWaves) void zfp_decode_region_variable(
    const uint64_t* __restrict__ stream, uint64_t stream_dwords, const uint16_t* __restrict__ lengths,
    const uint64_t* __restrict__ index, Geometry g, Region rg, Scalar* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t ctab[chunk_lut_bytes<DIMS>() / 4];  // LDS address 0 (static)
  __shared__ __attribute__((aligned(16))) uint16_t dtab[DIMS == 1 ? sizeof(Plane1dDecLut) / 2 : 8];
  zfp_decode_region_variable_body<Scalar, DIMS, FAST>(stream, stream_dwords, lengths, index, g, rg, out, ctab, dtab);
}

// The variable-rate decoder's image and workgroups (launch_decode_variable_t)
// over the region's waves.
template <typename Scalar, int DIMS>
int launch_decode_region_variable_t(const uint64_t* stream, size_t stream_bytes, const uint16_t* lengths,
                                    const uint64_t* index, const Geometry& g0, const Region& rg, bool fast,
                                    void* out, hipStream_t st) {
  Geometry g = g0;
  constexpr uint32_t D = (max_block_bits<Scalar, DIMS>(traits<Scalar>::prec) + 31) / 32;
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
    hipLaunchKernelGGL((zfp_decode_region_variable<Scalar, DIMS, true>), grid, block, lds, st, stream, dwords, lengths,
                       index, g, rg, d);
  else
    hipLaunchKernelGGL((zfp_decode_region_variable<Scalar, DIMS, false>), grid, block, lds, st, stream, dwords, lengths,
                       index, g, rg, d);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

template <typename Scalar>
int launch_decode_region_variable_type(const Problem& p, const Region& r, const uint64_t* stream, size_t stream_bytes,
                                       const uint16_t* lengths, const uint64_t* index, bool fast, void* out,
                                       hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_decode_region_variable_t<Scalar, 1>(stream, stream_bytes, lengths, index, p.g, r, fast, out, st);
    case 2: return launch_decode_region_variable_t<Scalar, 2>(stream, stream_bytes, lengths, index, p.g, r, fast, out, st);
    default: return launch_decode_region_variable_t<Scalar, 3>(stream, stream_bytes, lengths, index, p.g, r, fast, out, st);
  }
}

}  // namespace cuzfp
