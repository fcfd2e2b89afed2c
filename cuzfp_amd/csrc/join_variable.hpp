// cuzfp_amd/csrc/join_variable.hpp -- the part table of cuzfp_hip_join_variable
// (join_variable.hip): the streams of consecutive runs of blocks, in raster
// order, that the call concatenates into the stream of the whole array.
//
// The table travels by value in the kernel arguments: it is read on the host
// when the call is made, so there is no host-to-device copy, no allocation and
// no synchronisation, and the call can be captured into a graph.  That bounds
// the number of parts: kJoinMaxParts entries are 1804 bytes of the 4 KiB a
// launch may pass.
#pragma once
#include <stdint.h>

namespace cuzfp {

constexpr uint32_t kJoinMaxParts = 64;

struct JoinParts {
  const uint32_t* words[kJoinMaxParts];    // part k's stream, 4-byte aligned
  uint64_t dwords[kJoinMaxParts];          // ... and the whole dwords it holds (bytes / 4)
  const uint16_t* lengths[kJoinMaxParts];  // part k's raw lengths, first[k + 1] - first[k] of them
  uint32_t first[kJoinMaxParts + 1];       // B_k: the result's block that part k begins with; first[nparts] = nblocks
  uint32_t nparts;                         // 1 .. kJoinMaxParts, every part at least one block
  uint32_t longest;                        // the largest block count of a part
};

}  // namespace cuzfp
