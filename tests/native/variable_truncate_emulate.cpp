// tests/native/variable_truncate_emulate.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The per-lane function of cuzfp_hip_truncate_variable on the host:
// truncated_block_length (cuzfp_amd/csrc/rerate_variable.hpp), the very
// function the lengths pass of truncate_variable.hip runs on every lane, over
// a 64-bit window on a host copy of the stream.  The blocks' offsets are the
// running sum of the raw source lengths, as the kernels' scan gives them.
// tests/test_variable_truncate.py checks its lengths against CPU zfp 0.5.0's
// at the target mode.
#include <stddef.h>
#include <stdint.h>

#include "../../cuzfp_amd/csrc/rerate_variable.hpp"

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
void lengths(const uint64_t* stream, size_t words, const uint16_t* src_lengths, size_t nblocks, unsigned new_maxprec,
             int new_minexp, uint16_t* out) {
  uint64_t off = 0;
  for (size_t b = 0; b < nblocks; b++) {
    HostWindow rd{stream, words, off};
    out[b] = (uint16_t)cuzfp::truncated_block_length<Scalar, DIMS>(rd, src_lengths[b], new_maxprec, new_minexp);
    off += src_lengths[b];
  }
}

}  // namespace

extern "C" {

// type: 3 float, 4 double; dims 1 .. 3.  Returns 0 for arguments it does not know.
int vtrunc_lengths(int type, int dims, const uint64_t* stream, size_t words, const uint16_t* src_lengths,
                   size_t nblocks, unsigned new_maxprec, int new_minexp, uint16_t* out) {
  if ((type != 3 && type != 4) || dims < 1 || dims > 3) return 0;
  if (type == 3) {
    if (dims == 1) lengths<float, 1>(stream, words, src_lengths, nblocks, new_maxprec, new_minexp, out);
    else if (dims == 2) lengths<float, 2>(stream, words, src_lengths, nblocks, new_maxprec, new_minexp, out);
    else lengths<float, 3>(stream, words, src_lengths, nblocks, new_maxprec, new_minexp, out);
  } else {
    if (dims == 1) lengths<double, 1>(stream, words, src_lengths, nblocks, new_maxprec, new_minexp, out);
    else if (dims == 2) lengths<double, 2>(stream, words, src_lengths, nblocks, new_maxprec, new_minexp, out);
    else lengths<double, 3>(stream, words, src_lengths, nblocks, new_maxprec, new_minexp, out);
  }
  return 1;
}

// the rule of cuzfp_hip_truncate_variable's widening test
int vtrunc_coarsens(unsigned maxprec, int minexp, unsigned new_maxprec, int new_minexp) {
  return cuzfp::variable_mode_coarsens(maxprec, minexp, new_maxprec, new_minexp) ? 1 : 0;
}

}  // extern "C"
