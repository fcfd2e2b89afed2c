// tests/native/variable_coarse_emulate.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The per-lane arithmetic of cuzfp_hip_decode_region_variable_coarse on the
// host: for every block of a host copy of a variable-rate stream, the walk
// truncated_block_length (cuzfp_amd/csrc/rerate_variable.hpp) to the block's
// length L' at the target mode, and the budget variable_coarse_budget
// (cuzfp_amd/csrc/variable_coarse.hpp) the lane decodes with, against the
// column variable_coarse_column_dwords sizes from the target -- the very
// functions every lane of region_variable_coarse_kernels.hpp runs.  The blocks'
// offsets are the running sum of the raw source lengths, which is what the
// index and the lengths of a tile add up to.  tests/test_variable_coarse.py
// checks the budget's bounds over arbitrary bits and decodes the reference's
// streams at L' against CPU zfp 0.5.0's arrays at the target mode.
#include <stddef.h>
#include <stdint.h>

#include "../../cuzfp_amd/csrc/variable_coarse.hpp"

namespace {

// bits [off + pos, off + pos + 64) of the stream; words past its end read as zero
struct HostWindow {
  const uint64_t* w;
  size_t words;
  uint64_t off;
  uint64_t window(unsigned pos) const {
    const uint64_t bit = off + pos;
    const size_t i = (size_t)(bit >> 6);
    const unsigned s = (unsigned)(bit & 63u);
    const uint64_t lo = i < words ? w[i] : 0ull;
    const uint64_t hi = i + 1 < words ? w[i + 1] : 0ull;
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
  }
};

template <typename Scalar, int DIMS>
void blocks(const uint64_t* stream, size_t words, const uint16_t* src_lengths, size_t nblocks, unsigned maxprec,
            int minexp, uint16_t* walked, uint32_t* budget) {
  typedef cuzfp::traits<Scalar> T;
  const uint32_t column_bits = 32u * cuzfp::variable_coarse_column_dwords<Scalar, DIMS>(maxprec);
  const uint32_t longest = cuzfp::variable_longest_block<Scalar, DIMS>();
  uint64_t off = 0;
  for (size_t b = 0; b < nblocks; b++) {
    HostWindow rd{stream, words, off};
    const unsigned w = cuzfp::truncated_block_length<Scalar, DIMS>(rd, src_lengths[b], maxprec, minexp);
    walked[b] = (uint16_t)w;
    budget[b] = cuzfp::variable_coarse_budget(src_lengths[b], w, column_bits, longest, T::ebits);
    off += src_lengths[b];
  }
}

template <typename Scalar>
uint32_t column(int dims, unsigned maxprec) {
  return dims == 1 ? cuzfp::variable_coarse_column_dwords<Scalar, 1>(maxprec)
         : dims == 2 ? cuzfp::variable_coarse_column_dwords<Scalar, 2>(maxprec)
                     : cuzfp::variable_coarse_column_dwords<Scalar, 3>(maxprec);
}

}  // namespace

extern "C" {

// type: 3 float, 4 double; dims 1 .. 3.  walked[b] = L' of block b, budget[b] the
// bits the lane decodes it with.  Returns 0 for arguments it does not know.
int vcoarse_blocks(int type, int dims, const uint64_t* stream, size_t words, const uint16_t* src_lengths,
                   size_t nblocks, unsigned maxprec, int minexp, uint16_t* walked, uint32_t* budget) {
  if ((type != 3 && type != 4) || dims < 1 || dims > 3) return 0;
  if (type == 3) {
    if (dims == 1) blocks<float, 1>(stream, words, src_lengths, nblocks, maxprec, minexp, walked, budget);
    else if (dims == 2) blocks<float, 2>(stream, words, src_lengths, nblocks, maxprec, minexp, walked, budget);
    else blocks<float, 3>(stream, words, src_lengths, nblocks, maxprec, minexp, walked, budget);
  } else {
    if (dims == 1) blocks<double, 1>(stream, words, src_lengths, nblocks, maxprec, minexp, walked, budget);
    else if (dims == 2) blocks<double, 2>(stream, words, src_lengths, nblocks, maxprec, minexp, walked, budget);
    else blocks<double, 3>(stream, words, src_lengths, nblocks, maxprec, minexp, walked, budget);
  }
  return 1;
}

// dwords of a lane's column at the target precision; 0 for arguments it does not know
unsigned vcoarse_column_dwords(int type, int dims, unsigned maxprec) {
  if ((type != 3 && type != 4) || dims < 1 || dims > 3) return 0;
  return type == 3 ? column<float>(dims, maxprec) : column<double>(dims, maxprec);
}

}  // extern "C"
