// tests/native/variable_emulate.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The variable-rate modes (fixed precision, fixed accuracy) on the host, from
// the functions the HIP kernels of cuzfp_amd/csrc/variable_kernels.hpp run on
// every lane: block_length (the closed-form L_b), encode_block behind a writer
// that stops at L_b, decode_block with a budget of L_b.  Raster, padding and
// the stream layout are restated serially, as tests/native/emulate.cpp does;
// tests/test_variable.py checks the result against CPU zfp 0.5.0's streams.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../cuzfp_amd/csrc/zfp_block.hpp"
#include "host_io.hpp"

namespace {

template <int DIMS>
struct Raster {
  size_t bx, by, bz, nb;
  unsigned nx, ny, nz;
  Raster(unsigned nx_, unsigned ny_, unsigned nz_) : nx(nx_), ny(DIMS > 1 ? ny_ : 1), nz(DIMS > 2 ? nz_ : 1) {
    bx = (nx + 3) / 4;
    by = (ny + 3) / 4;
    bz = (nz + 3) / 4;
    nb = bx * by * bz;
  }
  // element offsets of block b's 4^DIMS positions (padded ones by pad_src) and
  // whether each lies inside the array
  void block(size_t b, long long* off, bool* valid) const {
    constexpr int N = 1 << (2 * DIMS);
    const size_t ix = b % bx, iy = (b / bx) % by, iz = b / (bx * by);
    const int wx = (int)(nx - 4 * ix < 4 ? nx - 4 * ix : 4);
    const int wy = (int)(ny - 4 * iy < 4 ? ny - 4 * iy : 4);
    const int wz = (int)(nz - 4 * iz < 4 ? nz - 4 * iz : 4);
    for (int i = 0; i < N; i++) {
      const int x = i & 3, y = (i >> 2) & 3, z = i >> 4;
      const int px = cuzfp::pad_src(x, wx), py = DIMS > 1 ? cuzfp::pad_src(y, wy) : 0,
                pz = DIMS > 2 ? cuzfp::pad_src(z, wz) : 0;
      off[i] = (long long)(4 * ix + px) + (long long)(4 * iy + py) * nx + (long long)(4 * iz + pz) * nx * ny;
      valid[i] = x < wx && (DIMS < 2 || y < wy) && (DIMS < 3 || z < wz);
    }
  }
};

// lengths[b] for every block; with a stream, the blocks coded back to back
// into it (zeroed here).  Returns the total bit count, or 0 if `words` is too
// small for it.
template <typename Scalar, int DIMS>
uint64_t compress(unsigned nx, unsigned ny, unsigned nz, unsigned maxprec, int minexp, const Scalar* data,
                  uint16_t* lengths, uint64_t* stream, size_t words) {
  constexpr int N = 1 << (2 * DIMS);
  const Raster<DIMS> r(nx, ny, nz);
  long long off[N];
  bool valid[N];
  Scalar f[N];
  uint64_t total = 0;
  for (size_t b = 0; b < r.nb; b++) {
    r.block(b, off, valid);
    for (int i = 0; i < N; i++) f[i] = data[off[i]];
    lengths[b] = (uint16_t)cuzfp::block_length<Scalar, DIMS>(f, maxprec, minexp);
    total += lengths[b];
  }
  if (!stream) return total;
  if (words < (total + 63) / 64) return 0;
  memset(stream, 0, words * 8);
  uint64_t pos = 0;
  for (size_t b = 0; b < r.nb; b++) {
    r.block(b, off, valid);
    // a 1-bit block is coded as the zero block (the kernel zeroes its values)
    for (int i = 0; i < N; i++) f[i] = lengths[b] > 1 ? data[off[i]] : (Scalar)0;
    HostWriter wr{stream, (size_t)pos, (size_t)(pos + lengths[b])};
    cuzfp::encode_block<Scalar, DIMS>(f, 0, wr);
    pos += lengths[b];
  }
  return total;
}

template <typename Scalar, int DIMS>
int decompress(unsigned nx, unsigned ny, unsigned nz, const uint64_t* stream, size_t words,
               const uint16_t* lengths, Scalar* data) {
  constexpr int N = 1 << (2 * DIMS);
  constexpr unsigned kMaxLen = cuzfp::max_block_bits<Scalar, DIMS>(cuzfp::traits<Scalar>::prec);
  const Raster<DIMS> r(nx, ny, nz);
  long long off[N];
  bool valid[N];
  Scalar f[N];
  uint64_t pos = 0;
  for (size_t b = 0; b < r.nb; b++) {
    r.block(b, off, valid);
    // the kernel's sanitised budget (zfp_decode_variable_body)
    unsigned len = lengths[b] < kMaxLen ? lengths[b] : kMaxLen;
    if (len < cuzfp::traits<Scalar>::ebits + 2u) len = 0;
    bool coded = false;
    if (len) {
      HostReader rd{stream, words, (size_t)pos, (size_t)(pos + len)};
      coded = cuzfp::decode_block<Scalar, DIMS>(f, len, rd);
    }
    for (int i = 0; i < N; i++)
      if (valid[i]) data[off[i]] = coded ? f[i] : (Scalar)0;
    pos += lengths[b];
  }
  return 1;
}

}  // namespace

extern "C" {

// type: 3 float, 4 double; ny = nz = 0 for 1D, nz = 0 for 2D
unsigned long long var_compress(int type, unsigned nx, unsigned ny, unsigned nz, unsigned maxprec, int minexp,
                                const void* data, uint16_t* lengths, uint64_t* stream, size_t words) {
  if (type == 3) {
    const float* d = (const float*)data;
    if (nz) return compress<float, 3>(nx, ny, nz, maxprec, minexp, d, lengths, stream, words);
    if (ny) return compress<float, 2>(nx, ny, nz, maxprec, minexp, d, lengths, stream, words);
    return compress<float, 1>(nx, ny, nz, maxprec, minexp, d, lengths, stream, words);
  }
  const double* d = (const double*)data;
  if (nz) return compress<double, 3>(nx, ny, nz, maxprec, minexp, d, lengths, stream, words);
  if (ny) return compress<double, 2>(nx, ny, nz, maxprec, minexp, d, lengths, stream, words);
  return compress<double, 1>(nx, ny, nz, maxprec, minexp, d, lengths, stream, words);
}

int var_decompress(int type, unsigned nx, unsigned ny, unsigned nz, const uint64_t* stream, size_t words,
                   const uint16_t* lengths, void* data) {
  if (type == 3) {
    float* d = (float*)data;
    if (nz) return decompress<float, 3>(nx, ny, nz, stream, words, lengths, d);
    if (ny) return decompress<float, 2>(nx, ny, nz, stream, words, lengths, d);
    return decompress<float, 1>(nx, ny, nz, stream, words, lengths, d);
  }
  double* d = (double*)data;
  if (nz) return decompress<double, 3>(nx, ny, nz, stream, words, lengths, d);
  if (ny) return decompress<double, 2>(nx, ny, nz, stream, words, lengths, d);
  return decompress<double, 1>(nx, ny, nz, stream, words, lengths, d);
}

}  // extern "C"
