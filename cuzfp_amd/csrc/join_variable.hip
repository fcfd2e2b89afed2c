// cuzfp_amd/csrc/join_variable.hip -- cuzfp_hip_join_variable: the
// variable-rate streams of K consecutive runs of blocks (parts: the z-slabs of
// a 3D array, the y-slabs of a 2D one, the x-ranges of a 1D one) concatenated
// into the stream of the whole array.  zfp codes every block on its own and
// writes the blocks back to back in raster order, so the result's bits [O_k,
// O_{k+1}) are part k's bits [0, O_{k+1} - O_k), O_k the offset of the part's
// first block in the result.  Bits are moved, nothing is decoded, and neither
// the scalar type nor the rank matters: one instantiation.
//
//   zfp_join_variable_lengths  the parts' raw lengths, concatenated   -> lengths
//   scan (variable_kernels.hpp) lengths                               -> offsets, total
//   zfp_join_variable_index    offsets[64 t] and the total            -> index
//   zfp_join_variable_copy     built from the output side: a lane owns two
//                              output words and stores them with one 16-byte
//                              store.  For a word it finds the part that holds
//                              the word's first bit -- a binary search over
//                              the K + 1 part offsets in LDS -- and
//                              funnel-shifts the part's dwords into place
//                              (SourceWindow); while the word is not full it
//                              goes on into the next part.
//
// Inside a part the shift (64 w - O_k) mod 32 is the same for every lane and
// neighbouring lanes read neighbouring source dwords.  There is no atomic, no
// zero fill and no segment in LDS: every output word below min(cap_words,
// ceil(total / 64)) is written once and whole by one lane, and no other word
// is written.  A part offset that is a multiple of 64 is the shift 0 of the
// funnel shift, a part of no bits (foreign lengths only) is stepped over, and a
// word can take its bits from up to 64 parts.
//
// The lengths are not trusted.  O_k is the scan of what was just written to
// `lengths`, so the O_k ascend and end at the total whatever the parts'
// lengths hold; a source dword is loaded only behind `d < dwords` of its part
// and reads as zero otherwise; the stores are bounded by the capacity.  With
// lengths that are not the parts' own the stream's words are unspecified, and
// lengths, total and index are still the raw concatenation and its sums.
#include "join_variable.hpp"
#include "kernels.hpp"
#include "source_window.hpp"
#include "variable_index.hpp"

namespace cuzfp {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// blockIdx.y is the part: its table entries are scalar loads of the arguments
__global__ __launch_bounds__(256) void zfp_join_variable_lengths(JoinParts tab, uint16_t* __restrict__ lengths) {
  const uint32_t k = blockIdx.y;
  const uint32_t b0 = tab.first[k], n = tab.first[k + 1] - b0;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < n) lengths[b0 + j] = tab.lengths[k][j];
}

// index[t] = offsets[64 t], t < ntiles; index[ntiles] = the total
__global__ __launch_bounds__(256) void zfp_join_variable_index(const uint64_t* __restrict__ offsets, uint32_t ntiles,
                                                               const uint64_t* __restrict__ total,
                                                               uint64_t* __restrict__ index) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t <= ntiles) index[t] = t < ntiles ? offsets[(uint64_t)t * kIndexTile] : *total;
}

// Output word w < ceil(O[K] / 64).  O[0] = 0 and O[K] > 64 w, so the largest k
// with O[k] <= 64 w has O[k + 1] > 64 w: empty parts at that bit lie before it.
__device__ __forceinline__ uint64_t join_word(uint64_t w, uint32_t K, const uint64_t* O,
                                              const uint32_t* const* W, const uint64_t* D) {
  const uint64_t p = w << 6;
  uint32_t k = 0, hi = K;
  while (hi - k > 1) {
    const uint32_t mid = (k + hi) >> 1;
    if (O[mid] <= p) k = mid; else hi = mid;
  }
  uint64_t v = 0;
  uint32_t have = 0;
  for (;;) {
    const uint64_t pos = p + have;       // O[k] <= pos <= O[k + 1]
    const uint64_t avail = O[k + 1] - pos;
    if (avail) {
      const SourceWindow rd{W[k], D[k], pos - O[k]};
      uint64_t bits = rd.window(0);
      const uint32_t room = 64u - have;
      const uint32_t take = avail < room ? (uint32_t)avail : room;
      if (take < 64) bits &= lowmask(take);
      v |= bits << have;
      have += take;
      if (have == 64) break;
    }
    if (++k == K) break;  // the stream ends inside this word: the pad is zero
  }
  return v;
}

// 256 lanes a workgroup, two words a lane.  The pair begins at an even word of
// the address space, not of the stream, so that the 16-byte store is aligned
// where `dst` is only 8-byte aligned: lane i owns words 2 i - a and 2 i + 1 - a,
// a = 1 where dst is an odd multiple of 8.  A lane with one word inside
// [0, nwords) stores 8 bytes.
__global__ __launch_bounds__(256) void zfp_join_variable_copy(JoinParts tab, const uint64_t* __restrict__ offsets,
                                                              const uint64_t* __restrict__ total,
                                                              uint64_t* __restrict__ dst, uint64_t cap_words) {
  __shared__ uint64_t O[kJoinMaxParts + 1];
  __shared__ const uint32_t* W[kJoinMaxParts];
  __shared__ uint64_t D[kJoinMaxParts];
  const uint32_t K = tab.nparts;
  const uint32_t t = threadIdx.x;
  if (t < K) {
    O[t] = offsets[tab.first[t]];  // first[t] < nblocks: no part is empty of blocks
    W[t] = tab.words[t];
    D[t] = tab.dwords[t];
  } else if (t == K) {
    O[t] = *total;
  }
  __syncthreads();
  const uint64_t swords = (O[K] + 63) >> 6;
  const uint64_t nwords = swords < cap_words ? swords : cap_words;
  const uint64_t a = ((uintptr_t)dst >> 3) & 1u;
  const uint64_t npairs = (nwords + a + 1) >> 1;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + t; i < npairs; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t w1 = 2 * i + 1 - a;  // the pair's second word; the first is w1 - 1
    const bool has0 = w1 >= 1, has1 = w1 < nwords;  // (w1 - 1 < nwords by i < npairs)
    const uint64_t v0 = has0 ? join_word(w1 - 1, K, O, W, D) : 0ull;
    const uint64_t v1 = has1 ? join_word(w1, K, O, W, D) : 0ull;
    if (has0 && has1)
      *(u64x2*)(dst + (w1 - 1)) = u64x2{v0, v1};
    else if (has0)
      dst[w1 - 1] = v0;
    else if (has1)
      dst[w1] = v1;
  }
}

static inline int join_launch_status() {
  const hipError_t e = hipGetLastError();
  t_last_hip = e;
  return e == hipSuccess ? CUZFP_SUCCESS : CUZFP_ERROR_HIP;
}

int launch_join_variable(const JoinParts& tab, uint32_t nblocks, uint64_t bound_words, uint64_t* dst,
                         uint64_t cap_words, uint16_t* lengths, uint64_t* dst_index, uint64_t* total,
                         uint64_t* offsets, uint64_t* partials, hipStream_t st) {
  hipLaunchKernelGGL(zfp_join_variable_lengths, dim3((tab.longest + 255) / 256, tab.nparts), dim3(256), 0, st, tab,
                     lengths);
  int rc = join_launch_status();
  if (rc) return rc;
  rc = launch_variable_scan(lengths, nblocks, offsets, partials, total, st);
  if (rc) return rc;
  if (dst_index) {
    const uint32_t T = variable_index_tiles(nblocks);
    hipLaunchKernelGGL(zfp_join_variable_index, dim3(T / 256 + 1), dim3(256), 0, st, (const uint64_t*)offsets, T,
                       (const uint64_t*)total, dst_index);
    rc = join_launch_status();
    if (rc) return rc;
  }
  // the stream of parts that are what their lengths say has at most bound_words words
  const uint64_t words = cap_words < bound_words ? cap_words : bound_words;
  if (!words) return CUZFP_SUCCESS;  // the size query: lengths, total and index only
  const uint64_t pairs = words / 2 + 1;
  const unsigned grid = (unsigned)std::min<uint64_t>((pairs + 255) / 256, 1u << 24);
  hipLaunchKernelGGL(zfp_join_variable_copy, dim3(grid), dim3(256), 0, st, tab, (const uint64_t*)offsets,
                     (const uint64_t*)total, dst, cap_words);
  return join_launch_status();
}

}  // namespace cuzfp
