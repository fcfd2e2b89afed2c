// cuzfp_amd/csrc/region.hpp -- index, clip and store-span arithmetic of the
// sub-box decoder and encoder (cuzfp_hip_decode_region, cuzfp_hip_encode_region),
// for host and device: the launcher fills a Region, the kernels
// (region_kernels.hpp, region_update_kernels.hpp) and tests/native/region_map.cpp,
// region_store.cpp read it through the same functions.
//
// The box [ox, ox+ex) x [oy, oy+ey) x [oz, oz+ez) of an array of bx x by x bz
// blocks covers the block columns [ox/4, (ox+ex+3)/4), likewise in y and z:
// rbx x rby x rbz region blocks, numbered in raster order (x fastest).  Fixed
// rate puts global block b at bits [b*maxbits, (b+1)*maxbits) of the stream.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CUZFP_HD __host__ __device__ __forceinline__
#else
#define CUZFP_HD inline
#endif

namespace cuzfp {

struct Region {
  uint32_t bx, by;          // blocks of the whole array along x and y
  uint32_t bx0, by0, bz0;   // the box's first block column
  uint32_t rbx, rby, rbz;   // region blocks (1 along an unused dimension)
  uint32_t nrb;             // rbx * rby * rbz
  uint32_t ox, oy, oz;      // the box's origin (0 along an unused dimension)
  uint32_t ex, ey, ez;      // its extent (1 along an unused dimension)
  uint32_t maxbits;         // bits per block
  // region index -> (rx, ry, rz): q = (n * m) >> s by rbx and by rbx * rby
  // (set_divisor, launch.hpp); divmagic = 0: plain division
  uint32_t drx_m, drx_s, drp_m, drp_s, divmagic;
  uint64_t stream_dwords;   // 2 * ceil(nblocks * maxbits / 64): the whole stream
  int64_t sx, sy, sz;       // element strides of the output box
};

struct RegionBlock {
  uint32_t rx, ry, rz;  // position among the region's blocks
  uint32_t b;           // global block index
};

CUZFP_HD uint32_t region_div(uint32_t n, uint32_t d, uint32_t m, uint32_t s, uint32_t magic) {
  return magic ? (uint32_t)(((uint64_t)n * m) >> s) : n / d;
}

// Region block r (< nrb) -> its position and global block
// b = ((bz0 + rz) * by + by0 + ry) * bx + bx0 + rx.
template <int DIMS>
CUZFP_HD RegionBlock region_block(const Region& g, uint32_t r) {
  RegionBlock p;
  if (DIMS == 1) {
    p.rx = r; p.ry = 0; p.rz = 0;
  } else if (DIMS == 2) {
    p.ry = region_div(r, g.rbx, g.drx_m, g.drx_s, g.divmagic);
    p.rx = r - p.ry * g.rbx; p.rz = 0;
  } else {
    const uint32_t plane = g.rbx * g.rby;
    p.rz = region_div(r, plane, g.drp_m, g.drp_s, g.divmagic);
    const uint32_t q = r - p.rz * plane;
    p.ry = region_div(q, g.rbx, g.drx_m, g.drx_s, g.divmagic);
    p.rx = q - p.ry * g.rbx;
  }
  p.b = ((g.bz0 + p.rz) * g.by + g.by0 + p.ry) * g.bx + g.bx0 + p.rx;
  return p;
}

// Global block b starts at bit `shift` of stream dword `dword`: b * maxbits
// needs 64 bits (b < 2^32, maxbits <= 2^14).
CUZFP_HD void region_block_bits(uint32_t b, uint32_t maxbits, uint64_t& dword, uint32_t& shift) {
  const uint64_t bit = (uint64_t)b * maxbits;
  dword = bit >> 5;
  shift = (uint32_t)bit & 31u;
}

// Dword k of the block image that starts at (dword, shift) takes stream dwords
// dword + k and, as the carry of the funnel shift, dword + k + 1.  The carry
// of the array's last block may lie past the stream's end: region_in_stream
// says whether a dword exists (a missing one reads as zero), region_clamp
// gives an index that is always safe to load.
CUZFP_HD bool region_in_stream(const Region& g, uint64_t d) { return d < g.stream_dwords; }
CUZFP_HD uint64_t region_clamp(const Region& g, uint64_t d) {
  return d < g.stream_dwords ? d : g.stream_dwords - 1;
}

// The stream dwords block b's bits [b*maxbits, (b+1)*maxbits) occupy, for the
// sub-box encoder's stores (region_update_kernels.hpp): a head dword the block
// shares with the block before it (head_mask: the block's bits in it; 0 when
// the block starts on a dword boundary), `nwhole` dwords from `whole` on that
// hold the block's bits only, and a tail dword shared with the block after it
// or with the stream's padding (tail_mask; 0 when the block ends on a dword
// boundary or inside its head dword).  A block of fewer than 32 bits that
// starts on a dword boundary has only a tail.  head, the whole dwords and tail
// are consecutive; every one of them holds a bit of the block, so none is at
// or past the stream's end.
struct RegionSpan {
  uint64_t head, whole, tail;  // dword indices
  uint32_t head_mask, nwhole, tail_mask;
};

CUZFP_HD RegionSpan region_span(uint32_t b, uint32_t maxbits) {
  RegionSpan s;
  uint32_t s0;
  region_block_bits(b, maxbits, s.head, s0);
  const uint64_t end = (uint64_t)b * maxbits + maxbits;
  const uint32_t t = (uint32_t)end & 31u;
  s.tail = end >> 5;
  s.whole = s.head + (s0 ? 1u : 0u);
  s.head_mask = 0;
  if (s0) {
    s.head_mask = ~0u << s0;
    if (s.tail == s.head) s.head_mask &= (1u << t) - 1u;  // the block ends in its head dword
  }
  s.nwhole = s.tail > s.whole ? (uint32_t)(s.tail - s.whole) : 0u;
  s.tail_mask = (t && (s.tail > s.head || !s0)) ? (1u << t) - 1u : 0u;
  return s;
}

// Array coordinate c along an axis with box origin o and extent e: inside the
// box (two-sided: c - o wraps to a large value when c < o) and its offset.
CUZFP_HD bool region_clip(uint32_t c, uint32_t o, uint32_t e, uint32_t& rel) {
  rel = c - o;
  return rel < e;
}

// Element (x, y, z) of region block p -> its offset in the output box, or
// false when the box does not hold it.
CUZFP_HD bool region_out_offset(const Region& g, const RegionBlock& p, uint32_t x, uint32_t y,
                                uint32_t z, int64_t& off) {
  uint32_t ix, iy, iz;
  const bool inx = region_clip(4 * (g.bx0 + p.rx) + x, g.ox, g.ex, ix);
  const bool iny = region_clip(4 * (g.by0 + p.ry) + y, g.oy, g.ey, iy);
  const bool inz = region_clip(4 * (g.bz0 + p.rz) + z, g.oz, g.ez, iz);
  off = (int64_t)ix * g.sx + (int64_t)iy * g.sy + (int64_t)iz * g.sz;
  return inx && iny && inz;
}

}  // namespace cuzfp
