// cuzfp_amd/csrc/region_update_kernels.hpp -- in-place update of a sub-box of
// a fixed-rate stream (cuzfp_hip_encode_region): the whole-array coders' block
// encoder and decoder (kernels.hpp, zfp_block.hpp) between a lane-owned
// copy-in and a lane-owned, bit-exact copy-out.
//
// One lane updates one region block (region.hpp), waves run over the region's
// blocks in raster order, as in zfp_decode_region.  Two variants, chosen per
// launch on the host:
//   covered (MERGE = false): every element of every touched block that lies
//     inside the array lies inside the box.  Gather from the box, pad, encode;
//     the old bits are not read.
//   merge (MERGE = true): any other box.  Every lane copies its block's old
//     bits in and decodes them (as zfp_decode_region's general path), replaces
//     the elements inside the box (a two-sided clip, as scatter_region, reading
//     from the box), pads elements outside the array from the merged values by
//     the whole-array encoder's rule (pad_src), and encodes.  Elements of the
//     block outside the box are thus re-encoded from their decoded values.
//
// Block image.  The whole-array encoder's writers assume a wave's blocks are
// contiguous in the stream; here each lane's block starts at its own 64-bit
// bit offset.  The block is coded into the lane's column of a lane-interleaved
// LDS image (64-bit word j at lds[64 j + lane], zeroed; LdsOrWriter with the
// budget `maxbits`, whatever its remainder by 64, and kSlackWords rows for
// what the coder emits past it) and shifted into place on the way out (a
// funnel shift by the block's bit offset in its first dword).  The merge
// variant's decode image is the same LDS, and its decoder tables and encoder
// tables share one static array: the decoder's are loaded first, the
// encoder's over them behind a workgroup barrier once every wave has decoded.
//
// Stores (region_span, region.hpp).  Stream dwords wholly inside the block's
// bit range take plain stores (16-byte ones where maxbits % 128 == 0 and the
// stream is 16-byte aligned).  A dword the block shares with a neighbour --
// another lane's or wave's block of this box, or a block outside it -- is
// updated only by device-scope atomics: atomicAnd with the complement of the
// lane's mask, then atomicOr with its bits.  Two lanes with disjoint masks
// commute in any interleaving, and a lane's own bits never change under
// another lane's update, so the merge variant's copy-in reads shared dwords
// with plain loads.  (The XCDs' L2s are not coherent with each other for
// plain accesses inside one kernel; atomics execute at the memory side.)
// With maxbits % 32 == 0 no atomic is issued.  No access touches a dword at
// or past the stream's end: every dword of a span holds a bit of its block,
// and the copy-in's carry dword is guarded as in the decoder.
//
// Instantiated per scalar type in update_{f32,f64,i32,i64}.hip.
#pragma once
#include "region_kernels.hpp"

namespace cuzfp {

constexpr int kUpdWaves = 4;  // waves a workgroup (fewer when the images do not fit)

// Waves a SIMD the launch bounds ask for.  The merge variant holds the 4^d
// values across a decode and an encode; 3D f32/i32 take looser bounds than the
// whole-array coders' for it and no kernel but the two 3D double ones uses
// scratch.  Those two keep the whole-array double coders' 2 waves a SIMD and
// spill (covered 136 B a lane, merge 260 B; int64 fits): at 1 wave a SIMD
// neither spills, and both measured slower wherever a box fills the device --
// 256^3 at 1024 bits, the whole array through the covered kernel 52.4 us
// against 75.5 us, a 64 x 255 x 255 slab through the merge kernel 51.4 us
// against 73.2 us; 64^3 bricks the same either way.
#ifndef CUZFP_UPD_COVERED64_WAVES  // A/B builds: the variants of 3D 8-byte types
#define CUZFP_UPD_COVERED64_WAVES 2
#endif
#ifndef CUZFP_UPD_MERGE64_WAVES
#define CUZFP_UPD_MERGE64_WAVES 2
#endif
template <typename Scalar, int DIMS, bool MERGE> struct update_occupancy {
  static constexpr int value = DIMS < 3 ? 4 : sizeof(Scalar) == 8 ? (MERGE ? CUZFP_UPD_MERGE64_WAVES : CUZFP_UPD_COVERED64_WAVES) : (MERGE ? 2 : 4);
};

// LDS words (8 bytes) of one wave's image: the encoder's, Wc + kSlackWords
// rows of 64 words, and for the merge variant the decoder's if it is larger
// (dwords per block + 5 slack rows of 64 dwords).
static inline uint32_t update_lds_words(uint32_t maxbits, bool merge) {
  const uint32_t enc = ((maxbits + 63) / 64 + kSlackWords) * 64;
  const uint32_t dec = ((maxbits + 31) / 32 + 5) * 32;
  return merge && dec > enc ? dec : enc;
}

// The static LDS of a kernel: the encoder's tables (the spread tables, in 1D
// the pair table behind them) and, overlaid, the merge variant's decoder
// tables (the chunk tables, in 1D the plane table behind them).
template <int DIMS, bool MERGE>
constexpr size_t update_tab_bytes() {
  constexpr size_t enc = kSpreadTabBytes + (DIMS == 1 ? sizeof(Pair1dLut) : 0);
  constexpr size_t dec = MERGE ? chunk_lut_bytes<DIMS>() + (DIMS == 1 ? sizeof(Plane1dDecLut) : 0) : 0;
  return enc > dec ? enc : dec;
}

// x padded along one axis of w valid values (1 <= w <= 4): pad_src(i, w) for
// i = 1, 2, 3 with compile-time register indices.
template <typename Scalar>
__device__ __forceinline__ void pad4(Scalar& a0, Scalar& a1, Scalar& a2, Scalar& a3, uint32_t w) {
  a1 = w < 2 ? a0 : a1;
  a2 = w < 3 ? a1 : a2;
  a3 = w < 4 ? a0 : a3;
}

// Elements of block `rb` outside the array, from the values inside it
// (separable: along x, then y, then z).
template <typename Scalar, int DIMS>
__device__ __forceinline__ void pad_block(const Geometry& g, const Region& rg, const RegionBlock& rb, Scalar* f) {
  constexpr int NY = DIMS > 1 ? 4 : 1, NZ = DIMS > 2 ? 4 : 1;
  const uint32_t wx = min(4u, g.nx - 4 * (rg.bx0 + rb.rx));
  const uint32_t wy = DIMS > 1 ? min(4u, g.ny - 4 * (rg.by0 + rb.ry)) : 4u;
  const uint32_t wz = DIMS > 2 ? min(4u, g.nz - 4 * (rg.bz0 + rb.rz)) : 4u;
  if (wx < 4) {
#pragma unroll
    for (int r = 0; r < NY * NZ; r++) pad4(f[4 * r], f[4 * r + 1], f[4 * r + 2], f[4 * r + 3], wx);
  }
  if constexpr (DIMS > 1) {
    if (wy < 4) {
#pragma unroll
      for (int z = 0; z < NZ; z++)
#pragma unroll
        for (int x = 0; x < 4; x++)
          pad4(f[16 * z + x], f[16 * z + 4 + x], f[16 * z + 8 + x], f[16 * z + 12 + x], wy);
    }
  }
  if constexpr (DIMS > 2) {
    if (wz < 4) {
#pragma unroll
      for (int i = 0; i < 16; i++) pad4(f[i], f[16 + i], f[32 + i], f[48 + i], wz);
    }
  }
}

// The elements of block `rb` that lie inside the box, read from it (the
// mirror of scatter_region).
template <typename Scalar, int DIMS>
__device__ __forceinline__ void overlay_region(const Scalar* __restrict__ box, const Region& rg,
                                               const RegionBlock& rb, Scalar* f) {
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
      const Scalar* row = box + (int64_t)iz * rg.sz + (int64_t)iy * rg.sy;
#pragma unroll
      for (int x = 0; x < 4; x++) {
        uint32_t ix;
        if (region_clip(gx + x, rg.ox, rg.ex, ix)) f[16 * z + 4 * y + x] = row[(int64_t)ix * rg.sx];
      }
    }
  }
}

// Covered block `rb`: its elements inside the array from the box (whose origin
// is block-aligned), the others padded from them, as gather's general path.
// rows: the box is contiguous, 16-byte aligned and a whole number of blocks.
template <typename Scalar, int DIMS>
__device__ __forceinline__ void gather_region(const Scalar* __restrict__ box, const Geometry& g, const Region& rg,
                                              const RegionBlock& rb, bool rows, Scalar* f) {
  constexpr int NY = DIMS > 1 ? 4 : 1, NZ = DIMS > 2 ? 4 : 1;
  if (rows) {
    const Scalar* p = box + ((size_t)(4 * rb.rz) * rg.ey + 4 * rb.ry) * rg.ex + 4 * rb.rx;
#pragma unroll
    for (int z = 0; z < NZ; z++)
#pragma unroll
      for (int y = 0; y < NY; y++) load_row(p + ((size_t)z * rg.ey + y) * rg.ex, f + 16 * z + 4 * y);
    return;
  }
  const int wx = (int)min(4u, g.nx - 4 * (rg.bx0 + rb.rx));
  const int wy = (int)min(4u, g.ny - 4 * (rg.by0 + rb.ry));
  const int wz = (int)min(4u, g.nz - 4 * (rg.bz0 + rb.rz));
  const Scalar* p = box + (int64_t)(4 * rb.rx) * rg.sx + (int64_t)(4 * rb.ry) * rg.sy + (int64_t)(4 * rb.rz) * rg.sz;
#pragma unroll
  for (int z = 0; z < NZ; z++)
#pragma unroll
    for (int y = 0; y < NY; y++)
#pragma unroll
      for (int x = 0; x < 4; x++)
        f[16 * z + 4 * y + x] = p[(int64_t)pad_src(x, wx) * rg.sx + (int64_t)pad_src(y, wy) * rg.sy +
                                  (int64_t)pad_src(z, wz) * rg.sz];
}

// Dword k of the block image in the lane's column (img: the column's first
// dword; 64-bit word j at dword 128 j), zero from bit maxbits on: the coder
// leaves what it produced past the budget there.
__device__ __forceinline__ uint32_t image_dword(const uint32_t* img, uint32_t k, uint32_t maxbits) {
  const uint32_t v = img[(k >> 1) * 128 + (k & 1)];
  const uint32_t last = maxbits >> 5;
  return k < last ? v : k == last ? v & ((1u << (maxbits & 31)) - 1u) : 0u;
}

// A dword shared with a neighbouring block: the lane's bits alone, by
// device-scope atomics (see the header).
__device__ __forceinline__ void store_shared(uint32_t* p, uint32_t v, uint32_t mask) {
  atomicAnd(p, ~mask);
  atomicOr(p, v & mask);
}

// The lane's coded block -> bits [b * maxbits, (b + 1) * maxbits) of the stream.
__device__ __forceinline__ void store_block(uint32_t* __restrict__ base, const uint64_t* mine, uint32_t b,
                                            uint32_t maxbits, bool vec) {
  if (vec) {
    // maxbits % 128 == 0, 16-byte aligned stream: the block is maxbits / 128
    // aligned 16-byte pieces
    uint4* dst = (uint4*)(base + ((uint64_t)b * maxbits >> 5));
    const uint32_t W = maxbits >> 6;
    for (uint32_t j = 0; j < W; j += 2) {
      uint4 v;
      const uint64_t a0 = mine[j * 64], a1 = mine[(j + 1) * 64];
      __builtin_memcpy(&v.x, &a0, 8);
      __builtin_memcpy(&v.z, &a1, 8);
      st16<false>(&dst[j >> 1], v);
    }
    return;
  }
  const RegionSpan sp = region_span(b, maxbits);
  const uint32_t* img = (const uint32_t*)mine;
  const uint32_t s0 = (uint32_t)((uint64_t)b * maxbits) & 31u;
  // stream dword head + k holds image bits [32 k - s0, 32 k - s0 + 32)
  uint32_t prev = 0, k = 0;
  if (sp.head_mask) {
    prev = image_dword(img, 0, maxbits);
    store_shared(base + sp.head, prev << s0, sp.head_mask);
    k = 1;
  }
  for (uint32_t i = 0; i < sp.nwhole; i++, k++) {
    const uint32_t cur = image_dword(img, k, maxbits);
    base[sp.whole + i] = s0 ? __builtin_amdgcn_alignbit(cur, prev, 32u - s0) : cur;
    prev = cur;
  }
  if (sp.tail_mask) {
    const uint32_t cur = image_dword(img, k, maxbits);
    store_shared(base + sp.tail, s0 ? __builtin_amdgcn_alignbit(cur, prev, 32u - s0) : cur, sp.tail_mask);
  }
}

// g: the array (nx, ny, nz, maxbits) and the launch (wave_end, vec_io: the
// 16-byte stores, lds_words, row_stage: the covered variant's row loads).
template <typename Scalar, int DIMS, bool MERGE>
__global__ __launch_bounds__(kLanes * kUpdWaves, (update_occupancy<Scalar, DIMS, MERGE>::value)) void
zfp_encode_region(const Scalar* __restrict__ box, Geometry g, Region rg, uint64_t* __restrict__ stream) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds_all[];
  __shared__ __attribute__((aligned(16))) uint32_t tabs[update_tab_bytes<DIMS, MERGE>() / 4];
  constexpr int N = 1 << (2 * DIMS);
  const uint32_t wig = wave_in_group();
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + wig;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = wave * kLanes + lane;
  const bool live_wave = wave < g.wave_end;
  const bool live = live_wave && r < rg.nrb;
  uint64_t* lds = lds_all + (size_t)wig * g.lds_words;
  uint64_t* mine = lds + lane;
  uint32_t* base = (uint32_t*)stream;
  const uint32_t W = (g.maxbits + 63) >> 6;  // words of the block image
  Scalar f[N];
  if constexpr (MERGE) {
    // the decoder's tables, the old bits (zfp_decode_region_body's general
    // path: a funnel shift of dword loads from the lane's own bit offset)
    uint32_t* ctab = tabs;
    uint16_t* dtab = (uint16_t*)(tabs + chunk_lut_bytes<DIMS>() / 4);
    constexpr uint32_t kLutEnd = chunk_lut_bytes<DIMS>() / 16;
    for (uint32_t i = threadIdx.x; i < kLutEnd; i += blockDim.x) ((uint4*)ctab)[i] = ((const uint4*)g_chunk_lut.e)[i];
    if constexpr (DIMS == 1)
      for (uint32_t i = threadIdx.x; i < sizeof(Plane1dDecLut) / 16; i += blockDim.x)
        ((uint4*)dtab)[i] = ((const uint4*)g_plane1d_lut.e)[i];
    uint32_t* L = (uint32_t*)lds + lane;
    const uint32_t D = (g.maxbits + 31) >> 5;
    if (live) {
      const RegionBlock rb = region_block<DIMS>(rg, r);
      uint64_t d0;
      uint32_t s0;
      region_block_bits(rb.b, g.maxbits, d0, s0);
      uint32_t prev = base[d0];
      for (uint32_t j = 0; j < D; j++) {
        const uint64_t d = d0 + j + 1;
        const uint32_t nxt = region_in_stream(rg, d) ? base[d] : 0u;
        L[j * 64] = __builtin_amdgcn_alignbit(nxt, prev, s0);
        prev = nxt;
      }
      if (g.maxbits & 31) L[(D - 1) * 64] &= (1u << (g.maxbits & 31)) - 1u;
    } else if (live_wave) {
      for (uint32_t j = 0; j < D; j++) L[j * 64] = 0;
    }
    if (live_wave)
      for (uint32_t j = D; j < D + 5; j++) L[j * 64] = 0;  // the reader's slack rows
    __syncthreads();
    if (live_wave) {
      wave_lds_sync();
      LdsReader<false> rd;
      rd.lds32 = L;
      rd.lut32 = ctab;
      rd.d1d = dtab;
      rd.init(0);
      if (!decode_block<Scalar, DIMS>(f, g.maxbits, rd)) {
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
    __syncthreads();  // every wave has read the decoder's tables for the last time
  }
  // the encoder's tables (over the decoder's) and the zeroed block image
  uint32_t* stab = tabs;
  uint32_t* ptab = tabs + kSpreadTabBytes / 4;
  for (uint32_t i = threadIdx.x; i < kSpreadTabBytes / 16; i += blockDim.x)
    ((uint4*)stab)[i] = ((const uint4*)g_spread_tab.e)[i];
  if constexpr (DIMS == 1)
    for (uint32_t i = threadIdx.x; i < sizeof(Pair1dLut) / 16; i += blockDim.x)
      ((uint4*)ptab)[i] = ((const uint4*)g_pair1d_lut.e)[i];
  if (live_wave)
    for (uint32_t j = 0; j < W + kSlackWords; j++) mine[j * 64] = 0;
  if constexpr (!MERGE) {
    if (live) {
      gather_region<Scalar, DIMS>(box, g, rg, region_block<DIMS>(rg, r), g.row_stage != 0, f);
    } else {
      // a lane past the last region block codes a zero block into its own column
#pragma unroll
      for (int i = 0; i < N; i++) f[i] = (Scalar)0;
    }
  } else {
    if (!live) {
#pragma unroll
      for (int i = 0; i < N; i++) f[i] = (Scalar)0;
    }
  }
  __syncthreads();
  if (!live_wave) return;
  wave_lds_sync();
  {
    LdsOrWriter<false> wr{mine, (lds_spread*)stab, 0, g.maxbits, (P1dPtr)ptab, uniform_const64(0x7fffu)};
    encode_block<Scalar, DIMS>(f, g.maxbits, wr);
  }
  wave_lds_sync();
  if (r < rg.nrb) {
    // the block's position again, from r alone (nothing else stays live
    // across the coder)
    uint32_t r2 = r;
    asm volatile("" : "+v"(r2));
    const RegionBlock sb = region_block<DIMS>(rg, r2);
    store_block(base, mine, sb.b, g.maxbits, (g.maxbits & 127) == 0 && g.vec_io);
  }
}

// covered: every block the box touches is covered (the host's test,
// region_covered); rows: and the box is contiguous, 16-byte aligned and a
// whole number of blocks.
template <typename Scalar, int DIMS>
int launch_encode_region_t(const void* box, const Geometry& g, const Region& rg, bool covered, bool rows,
                           uint64_t* stream, hipStream_t st) {
  Geometry gg = g;
  const uint32_t nwaves = (rg.nrb + kLanes - 1) / kLanes;
  gg.wave0 = 0;
  gg.wave_end = nwaves;
  gg.vec_io = (uintptr_t)stream % 16 == 0;
  gg.lds_words = update_lds_words(g.maxbits, !covered);
  gg.row_stage = covered && rows;
  const size_t kStatic = covered ? update_tab_bytes<DIMS, false>() : update_tab_bytes<DIMS, true>();
  // one wave's image beside the tables must fit the workgroup's LDS budget
  if ((size_t)gg.lds_words * 8 + kStatic > lds_cap_bytes()) return CUZFP_ERROR_INVALID_ARGUMENT;
  const uint32_t wpg = waves_per_group(gg.lds_words, kStatic, kUpdWaves);
  const dim3 grid((nwaves + wpg - 1) / wpg), block(kLanes * wpg);
  const size_t lds = (size_t)wpg * gg.lds_words * 8;
  const Scalar* d = (const Scalar*)box;
  if (covered)
    hipLaunchKernelGGL((zfp_encode_region<Scalar, DIMS, false>), grid, block, lds, st, d, gg, rg, stream);
  else
    hipLaunchKernelGGL((zfp_encode_region<Scalar, DIMS, true>), grid, block, lds, st, d, gg, rg, stream);
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

template <typename Scalar>
int launch_encode_region_type(const Problem& p, const Region& r, const void* box, bool covered, bool rows,
                              uint64_t* stream, hipStream_t st) {
  switch (p.dims) {
    case 1: return launch_encode_region_t<Scalar, 1>(box, p.g, r, covered, rows, stream, st);
    case 2: return launch_encode_region_t<Scalar, 2>(box, p.g, r, covered, rows, stream, st);
    default: return launch_encode_region_t<Scalar, 3>(box, p.g, r, covered, rows, stream, st);
  }
}

}  // namespace cuzfp
