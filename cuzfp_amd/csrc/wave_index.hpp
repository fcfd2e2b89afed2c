// cuzfp_amd/csrc/wave_index.hpp -- which wave of a launch a decoder workgroup's
// wave slot decodes (plain C++: the kernels and the host tests include it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CUZFP_WI_HD __host__ __device__ __forceinline__
#else
#define CUZFP_WI_HD inline
#endif

namespace cuzfp {

// Workgroup i of a launch runs on XCD i mod kXcds (MI300 / MI355X: the
// dispatcher deals workgroups to the 8 XCDs in turn).
constexpr uint32_t kXcds = 8;

// A launch's wave count allows the remap below: whole rounds of kXcds decoder
// workgroups, each a whole number of encoder workgroups.
CUZFP_WI_HD bool decode_remap_ok(uint32_t nwaves, uint32_t wpg, uint32_t enc_wpg) {
  return enc_wpg != 0 && wpg > enc_wpg && wpg % enc_wpg == 0 && nwaves % (kXcds * wpg) == 0;
}

// The wave (relative to the launch's first) that slot `wig` of decoder
// workgroup `group` decodes; workgroups of `wpg` waves, the encoder's of
// `enc_wpg`.  remap == false: consecutive, group * wpg + wig.  remap (only
// where decode_remap_ok): the workgroup takes the waves of the wpg / enc_wpg
// encoder workgroups of its round of kXcds * wpg waves whose index is its own
// mod kXcds -- the ones that ran on its XCD, so a wave's stream segment is
// read where it was written.  A bijection of the launch's wave slots onto
// themselves either way; a slot of a partial last workgroup (consecutive only)
// maps past the launch's end.
CUZFP_WI_HD uint32_t decode_wave_of(uint32_t group, uint32_t wig, uint32_t wpg, uint32_t enc_wpg, bool remap) {
  if (!remap) return group * wpg + wig;
  const uint32_t x = group % kXcds, q = group / kXcds;
  const uint32_t t = wig / enc_wpg, w = wig % enc_wpg;
  return enc_wpg * (kXcds * ((wpg / enc_wpg) * q + t) + x) + w;
}

}  // namespace cuzfp
