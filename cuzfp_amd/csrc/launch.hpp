// cuzfp_amd/csrc/launch.hpp -- host-side launch interface shared by the
// per-type kernel translation units and the C-ABI (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuzfp_hip.h"
#include "region.hpp"

namespace cuzfp {

constexpr int kLanes = 64;  // blocks per wave64 (one per lane)
constexpr int kMaxDevices = 64;  // per-device caches (launch policy, host pipeline)

struct Geometry {
  uint32_t nx, ny, nz;   // array extent (1 for unused dimensions)
  uint32_t bx, by;       // blocks along x and y
  uint32_t nblocks;      // total blocks
  uint32_t maxbits;      // bits per block
  uint32_t wave0;        // first wave of this launch
  uint32_t wave_end;     // one past its last wave
  uint32_t vec_io;       // stream base 16-byte aligned and maxbits even
  uint32_t lds_words;    // LDS words per wave
  int64_t sx, sy, sz;    // element strides
  // block index -> position without an integer divide: q = (n * m) >> s for
  // n < 2^31 (set_divisor), by bx and by bx * by; divmagic = 0 when nblocks
  // is too large for it (plain division then)
  uint32_t dbx_m, dbx_s, dpl_m, dpl_s, divmagic;
  // 3D double decoder: rows a pass when its row stores are staged through the
  // wave's LDS image (0: stored straight from the lanes), see kernels.hpp
  uint32_t row_stage;
  // 3D LDS-image decoder: workgroups take their waves by decode_wave_of's
  // remap (wave_index.hpp) rather than consecutively
  uint32_t xcd_remap;
};

// q = floor(n / d) = (n * m) >> s for every n < 2^31, with s = 31 + ceil(log2 d)
// and m = ceil(2^s / d) < 2^32: m = (2^s + e) / d with 0 <= e < d, so
// n * m / 2^s = n / d + n e / (d 2^s) and n e < 2^31 * 2^ceil(log2 d) = 2^s
// keeps the error below 1 / d, inside the gap floor(n / d) leaves.
inline void set_divisor(uint32_t d, uint32_t& m, uint32_t& s) {
  uint32_t l = 0;
  while ((1ull << l) < d) l++;
  s = 31 + l;
  m = (uint32_t)(((1ull << s) + d - 1) / d);
}

// The Region of a box inside the array of `g` (make_problem's: extents 1 along
// unused dimensions), origin and extent likewise normalised (0 and 1 along an
// unused dimension), the box inside the array and not empty; strides 0 =
// contiguous out[ez][ey][ex].
inline Region make_region(const Geometry& g, uint32_t ox, uint32_t oy, uint32_t oz, uint32_t ex,
                          uint32_t ey, uint32_t ez, int64_t sx, int64_t sy, int64_t sz) {
  Region r;
  r.bx = g.bx;
  r.by = g.by;
  r.bx0 = ox / 4;
  r.by0 = oy / 4;
  r.bz0 = oz / 4;
  r.rbx = (uint32_t)(((uint64_t)ox + ex + 3) / 4) - r.bx0;
  r.rby = (uint32_t)(((uint64_t)oy + ey + 3) / 4) - r.by0;
  r.rbz = (uint32_t)(((uint64_t)oz + ez + 3) / 4) - r.bz0;
  const uint64_t n = (uint64_t)r.rbx * r.rby * r.rbz;  // <= nblocks
  r.nrb = (uint32_t)n;
  r.ox = ox; r.oy = oy; r.oz = oz;
  r.ex = ex; r.ey = ey; r.ez = ez;
  r.maxbits = g.maxbits;
  set_divisor(r.rbx, r.drx_m, r.drx_s);
  set_divisor(r.rbx * r.rby, r.drp_m, r.drp_s);
  r.divmagic = n < (1ull << 31) ? 1u : 0u;
  r.stream_dwords = (((uint64_t)g.nblocks * g.maxbits + 63) / 64) * 2;
  r.sx = sx ? sx : 1;
  r.sy = sy ? sy : (int64_t)ex;
  r.sz = sz ? sz : (int64_t)ex * ey;
  return r;
}

struct Problem {
  int type;
  unsigned dims;
  Geometry g;
  bool fast_ok;  // contiguous, extents multiple of 4 (aligned base checked per call)
};

extern thread_local int t_last_hip;

template <typename Scalar>
int launch_encode_type(const Problem& p, const void* data, bool fast, uint64_t* stream,
                       uint32_t wave0, uint32_t nwaves, hipStream_t st);
template <typename Scalar>
int launch_decode_type(const Problem& p, const uint64_t* stream, bool fast, void* data,
                       uint32_t wave0, uint32_t nwaves, hipStream_t st);
// The sub-box decoder (region_kernels.hpp): `out` is the box's element (0, 0, 0);
// fast: a block-aligned box into a contiguous, 16-byte aligned `out`.  Blocks
// sit r.maxbits apart in the stream (the stride, p.g.maxbits) and each is
// decoded with `budget` <= r.maxbits bits (cuzfp_hip_decode_region_prefix;
// budget == r.maxbits is cuzfp_hip_decode_region).
template <typename Scalar>
int launch_decode_region_type(const Problem& p, const Region& r, const uint64_t* stream, bool fast,
                              uint32_t budget, void* out, hipStream_t st);

// Every block the box touches is covered: each of its elements that lies
// inside the array lies inside the box.  Along an axis: the origin is a
// multiple of 4 and the far side is one or the array's edge.
inline bool region_covered(const Geometry& g, const Region& r) {
  auto axis = [](uint32_t o, uint32_t e, uint32_t n) { return !(o & 3) && (!((o + e) & 3) || o + e == n); };
  return axis(r.ox, r.ex, g.nx) && axis(r.oy, r.ey, g.ny) && axis(r.oz, r.ez, g.nz);
}

// The sub-box encoder (region_update_kernels.hpp): `box` is the box's element
// (0, 0, 0), strides in the Region; covered: region_covered (else the
// read-modify-write variant); rows: covered, and the box is contiguous,
// 16-byte aligned and a whole number of blocks.
template <typename Scalar>
int launch_encode_region_type(const Problem& p, const Region& r, const void* box, bool covered, bool rows,
                              uint64_t* stream, hipStream_t st);

// cuzfp_hip_truncate (truncate.hip, rerate.hpp): the first m bits of each of
// the nblocks blocks of `src` (M bits apart), packed m apart into `dst`; the
// ranges are disjoint, m <= M.
int launch_truncate(const uint64_t* src, uint64_t* dst, uint32_t nblocks, uint32_t M, uint32_t m, hipStream_t st);

// The variable-rate modes (variable_kernels.hpp).  The workspace holds the
// 64-bit bit offset of every block and the scan's tile sums (variable_tiles).
//   scan: offsets = exclusive sum of lengths; the sum to *total unless null
//   zero: the stream words two waves' segments can share (below cap_words)
//   encode: lengths, *total, and the stream below cap_words (floats only)
//   decode: no load outside [stream, stream + stream_bytes) whatever lengths holds
constexpr uint32_t kVariableScanTile = 1024;  // lengths a scan workgroup
inline uint32_t variable_tiles(uint32_t nblocks) { return (nblocks + kVariableScanTile - 1) / kVariableScanTile; }
int launch_variable_scan(const uint16_t* lengths, uint32_t nblocks, uint64_t* offsets, uint64_t* partials,
                         uint64_t* total, hipStream_t st);
int launch_variable_zero(uint64_t* stream, uint64_t cap_words, const uint64_t* offsets, uint32_t nblocks,
                         const uint64_t* total, hipStream_t st);
template <typename Scalar>
int launch_encode_variable_type(const Problem& p, const void* data, bool fast, uint32_t maxprec, int minexp,
                                uint64_t* stream, uint64_t cap_words, uint16_t* lengths, uint64_t* total,
                                uint64_t* offsets, uint64_t* partials, hipStream_t st);
template <typename Scalar>
int launch_decode_variable_type(const Problem& p, const uint64_t* stream, size_t stream_bytes,
                                const uint16_t* lengths, bool fast, void* out, uint64_t* offsets,
                                uint64_t* partials, hipStream_t st);

// cuzfp_hip_truncate_variable (truncate_variable.hip, rerate_variable.hpp):
// the stream `src` with the index `src_lengths` cut to the mode (new_maxprec,
// new_minexp): lengths, *total, and `dst` below cap_words (cap_words == 0:
// lengths and *total only).  src_offsets and offsets hold nblocks words each,
// partials variable_tiles(nblocks).  No load outside [src, src + src_bytes)
// and src_lengths[0 .. nblocks) whatever src_lengths holds.
int launch_truncate_variable(bool is_double, unsigned dims, const uint64_t* src, size_t src_bytes,
                             const uint16_t* src_lengths, uint32_t nblocks, uint32_t new_maxprec, int new_minexp,
                             uint64_t* dst, uint64_t cap_words, uint16_t* lengths, uint64_t* total,
                             uint64_t* src_offsets, uint64_t* offsets, uint64_t* partials, hipStream_t st);

// The offset index of a variable-rate stream and the sub-box decoder that reads
// it (variable_index.hpp, region_variable_kernels.hpp).
//   index: index[t] = the bit offset of block 64 t, index[T] = the total; the
//          scan's offsets and partials are the variable-rate workspace
//   decode: one launch; `out` is the box's element (0, 0, 0); fast as
//           launch_decode_region_type; no load outside [stream, stream +
//           stream_bytes), lengths[0 .. nblocks) and index[0 .. T) whatever
//           index and lengths hold
int launch_variable_index(const uint16_t* lengths, uint32_t nblocks, uint64_t* index, uint64_t* offsets,
                          uint64_t* partials, hipStream_t st);
template <typename Scalar>
int launch_decode_region_variable_type(const Problem& p, const Region& r, const uint64_t* stream, size_t stream_bytes,
                                       const uint16_t* lengths, const uint64_t* index, bool fast, void* out,
                                       hipStream_t st);

// cuzfp_hip_decode_region_variable_coarse (variable_coarse.hpp,
// region_variable_coarse_kernels.hpp): launch_decode_region_variable_type with
// every block decoded at the target mode (maxprec 1 .. the type's precision,
// minexp), never finer than the stream holds it; one launch, the same bounds.
template <typename Scalar>
int launch_decode_region_variable_coarse_type(const Problem& p, const Region& r, const uint64_t* stream,
                                              size_t stream_bytes, const uint16_t* lengths, const uint64_t* index,
                                              uint32_t maxprec, int minexp, bool fast, void* out, hipStream_t st);

// cuzfp_hip_encode_region_variable (region_variable_update_kernels.hpp): the
// stream `src` with `src_lengths` and `src_index`, the blocks the box touches
// coded anew from `box` at (maxprec, minexp) and every other block copied:
// lengths, *total, the new index unless dst_index is null, and `dst` below
// cap_words.  covered and rows as launch_encode_region_type; offsets holds
// nblocks words, partials variable_tiles(nblocks).  No load outside [src, src +
// src_bytes), src_lengths[0 .. nblocks) and src_index[0 .. T) whatever the two
// hold.
template <typename Scalar>
int launch_encode_region_variable_type(const Problem& p, const Region& r, const void* box, bool covered, bool rows,
                                       uint32_t maxprec, int minexp, const uint64_t* src, size_t src_bytes,
                                       const uint16_t* src_lengths, const uint64_t* src_index, uint64_t* dst,
                                       uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                                       uint64_t* offsets, uint64_t* partials, hipStream_t st);

// cuzfp_hip_extract_region_variable and cuzfp_hip_insert_region_variable
// (region_variable_crop_kernels.hpp): the blocks of the block-aligned box `r`
// moved bit for bit, out of the stream `src` into a stream of their own, or
// from such a stream `box` into a copy of `src`.  Both write lengths, *total,
// the new index unless dst_index is null, and `dst` below cap_words.
//   extract: lengths, dst_index, offsets (r.nrb words) and partials
//            (variable_tiles(r.nrb)) are the box's
//   insert:  they are the array's (nblocks, variable_tiles(nblocks))
// No load outside [src, src + src_bytes), src_lengths[0 .. nblocks), src_index[0
// .. T), [box, box + box_bytes), box_lengths[0 .. r.nrb) and box_index[0 ..
// ceil(r.nrb / 64)) whatever the indices and lengths hold.
template <typename Scalar>
int launch_extract_region_variable_type(unsigned dims, const Region& r, const uint64_t* src, size_t src_bytes,
                                        const uint16_t* src_lengths, const uint64_t* src_index, uint64_t* dst,
                                        uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                                        uint64_t* offsets, uint64_t* partials, hipStream_t st);
template <typename Scalar>
int launch_insert_region_variable_type(const Problem& p, const Region& r, const uint64_t* box, size_t box_bytes,
                                       const uint16_t* box_lengths, const uint64_t* box_index, const uint64_t* src,
                                       size_t src_bytes, const uint16_t* src_lengths, const uint64_t* src_index,
                                       uint64_t* dst, uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index,
                                       uint64_t* total, uint64_t* offsets, uint64_t* partials, hipStream_t st);

// cuzfp_hip_join_variable (join_variable.hip): the streams of the parts of
// `tab` (join_variable.hpp; consecutive runs of the array's blocks in raster
// order) concatenated: lengths, *total, the index unless dst_index is null, and
// `dst` below cap_words (0: none).  bound_words: the words of all parts
// together, which sizes the copy's grid.  offsets holds nblocks words, partials
// variable_tiles(nblocks).  One instantiation for every type and rank.  No load
// outside the parts' [words, words + 4 dwords) and lengths whatever the lengths
// hold.
struct JoinParts;
int launch_join_variable(const JoinParts& tab, uint32_t nblocks, uint64_t bound_words, uint64_t* dst,
                         uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                         uint64_t* offsets, uint64_t* partials, hipStream_t st);

}  // namespace cuzfp
