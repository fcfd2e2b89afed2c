// cuzfp_amd/csrc/region_kernels.hpp -- decode of a sub-box of a fixed-rate
// stream (cuzfp_hip_decode_region): the whole-array decoder's block decoder
// (kernels.hpp, zfp_block.hpp) behind a lane-owned copy-in and a two-sided
// clipped store.
//
// One lane decodes one region block (region.hpp), waves run over the region's
// blocks in raster order.  A wave's blocks are runs of at most rbx blocks that
// are contiguous in the stream, each run starting at an arbitrary bit, so the
// wave has no segment of its own: every lane loads its block from its own bit
// offset b * maxbits (64-bit) into its column of the lane-interleaved image.
// Within a run consecutive lanes read consecutive blocks (maxbits / 8 bytes
// apart, as the whole-array decoder's lane-owned fallback); runs are bx (and
// bx * by) blocks apart.
//
// maxbits has two roles, kept apart: the stride between blocks in the stream
// is Region::maxbits; the budget each block is decoded with -- the bits read,
// the image's size and masks, decode_block's argument, the register path --
// is Geometry::maxbits.  cuzfp_hip_decode_region passes the same value for
// both; cuzfp_hip_decode_region_prefix a budget below the stride, which
// decodes each block's prefix (zfp's coder is embedded: rerate.hpp) and reads
// nothing of a block past it.
//
// Instantiated per scalar type in region_{f32,f64,i32,i64}.hip.
#pragma once
#include "kernels.hpp"

namespace cuzfp {

// Store of one decoded block of the region: only the elements inside the box
// (region_clip on each axis, as region_out_offset).  Rows and planes outside
// the box are skipped as a whole, and each row's address is formed where the
// row is stored, so that no offset stays in a register beside the 4^d values.
template <typename Scalar, int DIMS>
__device__ __forceinline__ void scatter_region(Scalar* __restrict__ out, const Region& rg,
                                               const RegionBlock& rb, const Scalar* f) {
  constexpr int NY = DIMS > 1 ? 4 : 1, NZ = DIMS > 2 ? 4 : 1;
  const uint32_t gx = 4 * (rg.bx0 + rb.rx), gy = 4 * (rg.by0 + rb.ry), gz = 4 * (rg.bz0 + rb.rz);
#pragma unroll
  for (int z = 0; z < NZ; z++) {
    uint32_t iz;
    if (!region_clip(gz + z, rg.oz, rg.ez, iz)) continue;
#pragma unroll
    for (int y = 0; y < NY; y++) {
      uint32_t iy;
      if (!region_clip(gy + y, rg.oy, rg.ey, iy)) continue;
      Scalar* row = out + (int64_t)iz * rg.sz + (int64_t)iy * rg.sy;
#pragma unroll
      for (int x = 0; x < 4; x++) {
        uint32_t ix;
        if (region_clip(gx + x, rg.ox, rg.ex, ix)) row[(int64_t)ix * rg.sx] = f[16 * z + 4 * y + x];
      }
    }
  }
}

// g: the launch (maxbits, wave_end, vec_io, lds_words) and, for FAST, the box
// as an array of its own (nx, ny, nz = ex, ey, ez: the row stores of scatter).
// REG: 0 = the LDS image; 64 = a 1D/2D block of at most 64 bits, read into a
// register (RegReader).
template <typename Scalar, int DIMS, bool FAST, int REG = 0>
__device__ __forceinline__ void zfp_decode_region_body(const uint64_t* __restrict__ stream, const Geometry& g,
                                                       const Region& rg, Scalar* __restrict__ out,
                                                       uint32_t* ctab, uint16_t* dtab) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_all[];
  constexpr int N = 1 << (2 * DIMS);
  const uint32_t wig = wave_in_group();
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + wig;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = wave * kLanes + lane;
  const bool live = wave < g.wave_end && r < rg.nrb;
  uint64_t* lds = lds_all + (size_t)wig * g.lds_words;
  // the lane's block: dword d0, bit s0 of the stream (a lane past the last
  // region block takes block 0's place and loads nothing)
  const RegionBlock rb = region_block<DIMS>(rg, live ? r : 0u);
  uint64_t d0;
  uint32_t s0;
  region_block_bits(rb.b, rg.maxbits, d0, s0);
  const uint32_t* base = (const uint32_t*)stream;
  uint32_t* lut = ctab;
  auto copy_tabs = [&]() {
    // (1D reads chunk-1 entries only: the state-2 table, the first kLutPairs entries)
    constexpr uint32_t kLutEnd = DIMS == 1 ? kLutPairs * 4 / 16 : sizeof(ChunkLut) / 16;
    for (uint32_t i = threadIdx.x; i < kLutEnd; i += blockDim.x)
      ((uint4*)lut)[i] = ((const uint4*)g_chunk_lut.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Plane1dDecLut) / 16; i += blockDim.x)
        ((uint4*)dtab)[i] = ((const uint4*)g_plane1d_lut.e)[i];
  };
  uint32_t* L = (uint32_t*)lds + lane;
  uint64_t blk = 0;
  if constexpr (REG) {
    // bits [s0, s0 + maxbits) from dword d0 on: three dwords at most; the two
    // after d0 may lie past the stream's end and then read as zero (clamped
    // addresses and selects, as reg_block)
    if (live) {
      const uint32_t a0 = base[d0];
      uint32_t a1 = base[region_clamp(rg, d0 + 1)];
      uint32_t a2 = base[region_clamp(rg, d0 + 2)];
      a1 = region_in_stream(rg, d0 + 1) ? a1 : 0u;
      a2 = region_in_stream(rg, d0 + 2) ? a2 : 0u;
      blk = ((uint64_t)__builtin_amdgcn_alignbit(a1, a0, s0) |
             ((uint64_t)__builtin_amdgcn_alignbit(a2, a1, s0) << 32)) & lowmask(g.maxbits);
    }
    copy_tabs();
  } else {
    const uint32_t D = (g.maxbits + 31) >> 5;  // dwords per block
    // stride and budget multiples of 128 and a 16-byte aligned stream: every
    // block starts 16-byte aligned (s0 = 0, d0 a multiple of 4) and is read in
    // whole 16-byte pieces
    const bool vec = ((g.maxbits | rg.maxbits) & 127) == 0 && g.vec_io;
    constexpr uint32_t kHeld = 8;  // 16-byte pieces held in registers (maxbits <= 1024)
    uint4 held[kHeld];
    const uint4* src = (const uint4*)(base + d0);
    if (live && vec) {
#pragma unroll
      for (uint32_t q = 0; q < kHeld; q++)
        if (4 * q < D) held[q] = ld16<kNtStream>(&src[q]);
    }
    copy_tabs();
    if (live) {
      if (vec) {
#pragma unroll
        for (uint32_t q = 0; q < kHeld; q++)
          if (4 * q < D) {
            L[(4 * q) * 64] = held[q].x;
            L[(4 * q + 1) * 64] = held[q].y;
            L[(4 * q + 2) * 64] = held[q].z;
            L[(4 * q + 3) * 64] = held[q].w;
          }
        for (uint32_t q = 4 * kHeld; q < D; q += 4) {  // larger blocks
          const uint4 v = src[q >> 2];
          L[q * 64] = v.x;
          L[(q + 1) * 64] = v.y;
          L[(q + 2) * 64] = v.z;
          L[(q + 3) * 64] = v.w;
        }
      } else {
        // dword j of the block: bits s0 .. s0 + 31 of stream dwords d0 + j and
        // d0 + j + 1; a carry dword past the stream's end (the array's last
        // block only) reads as zero
        uint32_t prev = base[d0];
        for (uint32_t j = 0; j < D; j++) {
          const uint64_t d = d0 + j + 1;
          const uint32_t nxt = region_in_stream(rg, d) ? base[d] : 0u;
          L[j * 64] = __builtin_amdgcn_alignbit(nxt, prev, s0);
          prev = nxt;
        }
        // the block reads as zeros past its last bit (the plane steps rely on it)
        if (g.maxbits & 31) L[(D - 1) * 64] &= (1u << (g.maxbits & 31)) - 1u;
      }
    } else if (wave < g.wave_end) {
      // a lane past the last region block decodes a zero block (its stores are skipped)
      for (uint32_t j = 0; j < D; j++) L[j * 64] = 0;
    }
    if (wave < g.wave_end)
      for (uint32_t j = D; j < D + 5; j++) L[j * 64] = 0;  // the reader's slack rows
  }
  __syncthreads();
  if (wave >= g.wave_end) return;
  wave_lds_sync();
  // Every lane of a live wave decodes (a lane past the last region block reads
  // a zero block); only the stores are guarded.
  Scalar f[N];
  bool coded;  // false only for a wave of zero blocks (decode_block)
  if constexpr (REG) {
    RegReader<false, false> rd;
    rd.lds32 = L;
    rd.lut32 = lut;
    rd.d1d = dtab;
    rd.set_block(blk);
    rd.init(0);
    coded = decode_block<Scalar, DIMS>(f, g.maxbits, rd);
  } else {
    LdsReader<false> rd;
    rd.lds32 = L;
    rd.lut32 = lut;
    rd.d1d = dtab;
    rd.init(0);
    coded = decode_block<Scalar, DIMS>(f, g.maxbits, rd);
  }
  if (!coded) {
#pragma unroll
    for (int i = 0; i < N; i++) f[i] = (Scalar)0;
  }
  if constexpr (!FAST) {
    // the values are final here: without this the inverse transform's last
    // step sinks into the store branch with its operands and its results
    // both live, which spills with 64-bit values
#pragma unroll
    for (int i = 0; i < N; i++) asm volatile("" : "+v"(f[i]));
  }
  if (r < rg.nrb) {
    // the block's position again, from r alone: only r stays live across the
    // decoder (the barrier keeps the compiler from carrying rx, ry, rz over)
    uint32_t r2 = r;
    asm volatile("" : "+v"(r2));
    const RegionBlock sb = region_block<DIMS>(rg, r2);
    if constexpr (FAST)
      scatter<Scalar, DIMS, true>(out, g, BlockPos{sb.rx, sb.ry, sb.rz}, f);
    else
      scatter_region<Scalar, DIMS>(out, rg, sb, f);
  }
}

template <typename Scalar, int DIMS, bool FAST, int REG = 0, int WPG = kDecWaves>
__global__ __launch_bounds__(kLanes * WPG, (occupancy<Scalar, DIMS>::value)) void zfp_decode_region(
    const uint64_t* __restrict__ stream, Geometry g, Region rg, Scalar* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t ctab[chunk_lut_bytes<DIMS>() / 4];  // LDS address 0 (static)
  // 1D: the plane table (Plane1dDecLut, 16 KiB)
  __shared__ __attribute__((aligned(16))) uint16_t dtab[DIMS == 1 ? sizeof(Plane1dDecLut) / 2 : 8];
  zfp_decode_region_body<Scalar, DIMS, FAST, REG>(stream, g, rg, out, ctab, dtab);
}

// The launch of launch_decode_t for a region: the same images, tables,
// workgroup sizes and LDS-budget refusal; no staged row stores (row_stage 0)
// and no plane-loop priority schedule, whose thresholds were measured for
// whole-array launches.
template <typename Scalar, int DIMS>
int launch_decode_region_t(const uint64_t* stream, const Geometry& g0, const Region& rg, bool fast,
                           uint32_t budget, void* out, hipStream_t st) {
  // the kernel's Geometry carries the budget; the stride stays in rg.maxbits
  Geometry g = g0;
  g.maxbits = budget;
  Geometry gg = g;
  const uint32_t nwaves = (rg.nrb + kLanes - 1) / kLanes;
  // the box as an array of its own (the fast row stores)
  gg.nx = rg.ex;
  gg.ny = rg.ey;
  gg.nz = rg.ez;
  gg.wave0 = 0;
  gg.wave_end = nwaves;
  gg.vec_io = (g.maxbits % 2 == 0) && ((uintptr_t)stream % 16 == 0);
  gg.lds_words = ((g.maxbits + 31) / 32 + 5) * 32;  // (dwords per block + 5 slack rows) x 64 lanes
  gg.row_stage = 0;
  const bool reg = DIMS <= 2 && g.maxbits <= 64;
  if (reg) gg.lds_words = 0;
  const size_t kStatic = chunk_lut_bytes<DIMS>() + (DIMS == 1 ? sizeof(Plane1dDecLut) : 16);
  // one wave's image beside the tables must fit the workgroup's LDS budget
  if (gg.lds_words * 8 + kStatic > lds_cap_bytes()) return CUZFP_ERROR_INVALID_ARGUMENT;
  Scalar* d = (Scalar*)out;
  // the row stores exist for the floating-point types only (the C-ABI never
  // asks for them with integers): no integer instantiation of them
  constexpr bool kRows = !traits<Scalar>::is_int;
  if constexpr (DIMS <= 2) {
    if (reg) {
      constexpr int W = DIMS == 1 ? kRegWaves1d : kRegWaves2d;
      const dim3 rgrid((nwaves + W - 1) / W), rblock(kLanes * W);
      if (kRows && fast)
        hipLaunchKernelGGL((zfp_decode_region<Scalar, DIMS, kRows, 64, W>), rgrid, rblock, 0, st, stream, gg, rg, d);
      else
        hipLaunchKernelGGL((zfp_decode_region<Scalar, DIMS, false, 64, W>), rgrid, rblock, 0, st, stream, gg, rg, d);
      const hipError_t e = hipGetLastError();
      t_last_hip = e;
      return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
    }
  }
  const uint32_t wpg = waves_per_group(gg.lds_words, kStatic, kDecWaves);
  const dim3 grid((nwaves + wpg - 1) / wpg), block(kLanes * wpg);
  const size_t lds = (size_t)wpg * gg.lds_words * 8;  // (+ the static chunk tables)
  if (kRows && fast)
    hipLaunchKernelGGL((zfp_decode_region<Scalar, DIMS, kRows>), grid, block, lds, st, stream, gg, rg, d);
  else
    hipLaunchKernelGGL((zfp_decode_region<Scalar, DIMS, false>), grid, block, lds, st, stream, gg, rg, d);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

template <typename Scalar>
int launch_decode_region_type(const Problem& p, const Region& r, const uint64_t* stream, bool fast,
                              uint32_t budget, void* out, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_decode_region_t<Scalar, 1>(stream, p.g, r, fast, budget, out, st);
    case 2: return launch_decode_region_t<Scalar, 2>(stream, p.g, r, fast, budget, out, st);
    default: return launch_decode_region_t<Scalar, 3>(stream, p.g, r, fast, budget, out, st);
  }
}

}  // namespace cuzfp
