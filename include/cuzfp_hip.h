/*
 * include/cuzfp_hip.h -- C-ABI of the MI355X-native zfp fixed-rate codec.
 *
 * This is the drop-in boundary: plain pointers, sizes and a HIP stream, no C++
 * or torch types.  The C++ surface of the reference (`cuZFP::compress`,
 * `cuZFP::decompress`, include/cuZFP.h) is implemented on top of it
 * (cuzfp_amd/csrc/cuZFP.cpp); Python, ctypes, cgo or JNI callers bind it
 * directly.
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * /root/reference/src/cuZFP):
 *
 *   cuzfp_hip_encode  <- internal::encode<T>(dims, maxbits, d_data, d_stream)
 *                        cuZFP.cu:26-64, i.e. encode1launch / encode2launch /
 *                        encode3launch (encode1.cuh:458-526, encode2.cuh:462-528,
 *                        encode3.cuh:428-508) and their kernels.
 *   cuzfp_hip_decode  <- internal::decode<T>(dims, maxbits, d_stream, d_data)
 *                        cuZFP.cu:66-105 -> decode{1,2,3}launch (decode1.cuh:102-145,
 *                        decode2.cuh:141-182, decode3.cuh:217-264).
 *   cuzfp_hip_stream_bytes <- the byte count those launchers return
 *                        (calc_device_mem{1,2,3}d, e.g. encode3.cuh:413-423).
 *   cuzfp_hip_maximum_size <- zfp_stream_maximum_size (zfp_structs.h:222-251).
 *   cuzfp_hip_rate_to_maxbits <- stream_set_rate (zfp_structs.h:46-76).
 *   cuzfp_hip_compress_host / cuzfp_hip_decompress_host <- the host-pointer
 *                        staging of cuZFP::compress / decompress
 *                        (cuZFP.cu:107-170, 174-269), as a pinned, chunked,
 *                        stream-overlapped pipeline.
 *
 * Stream format: bit-exact with zfp 0.5.0 fixed-rate mode (the ground truth of
 * the reference's src/utils/test.py:68-93): 64-bit little-endian words, bits
 * LSB first, block b (raster order z, y, x) at bits [b*maxbits, (b+1)*maxbits),
 * zero padded to a whole word; no header.
 *
 * Unlike the reference (cuZFP.cu:174-269: errors printed, execution continues),
 * every call returns a cuzfp_status.  Device calls are asynchronous on
 * `stream` (0 = the null stream) and never allocate or synchronise, so they
 * can be captured into a hipGraph.
 */
#ifndef CUZFP_HIP_H
#define CUZFP_HIP_H

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUZFP_HIP_ABI_VERSION 1

/* scalar type codes: the reference's zfp_type enum (zfp_structs.h:31-37) */
#define CUZFP_TYPE_INT32 1
#define CUZFP_TYPE_INT64 2
#define CUZFP_TYPE_FLOAT 3
#define CUZFP_TYPE_DOUBLE 4

/* Largest accepted maxbits (bits per block).  Calls with more return
 * CUZFP_ERROR_INVALID_ARGUMENT.  It is far above ZFP_MAX_BITS = 4171
 * (zfp_structs.h:12), the most bits any block can use; beyond that a stream is
 * padding.  The bound keeps one wave's LDS stream image within a gfx950
 * workgroup's LDS (160 KiB, hipDeviceAttributeMaxSharedMemoryPerBlock): the
 * decoder's image at 16384 bits is 129 KiB plus 16 KiB of tables, 145 KiB.  On
 * a device with less LDS per workgroup (e.g. 64 KiB) the launchers check one
 * wave's image plus the tables against the device's budget before launching and
 * return CUZFP_ERROR_INVALID_ARGUMENT for a call that does not fit (3D f32/f64
 * past about 5,980 bits on a 64 KiB device); the environment variable
 * CUZFP_LDS_CAP_BYTES lowers the budget (tests). */
#define CUZFP_MAX_BITS 16384

/* Pinned staging slots of the host-memory pipeline for pageable buffers
 * (callers' default `nstreams` for cuzfp_hip_compress_host / decompress_host). */
#define CUZFP_HOST_STREAMS 4

typedef enum {
  CUZFP_SUCCESS = 0,
  CUZFP_ERROR_INVALID_ARGUMENT = 1, /* bad dims, maxbits or null pointer   */
  CUZFP_ERROR_UNSUPPORTED_TYPE = 2, /* type code not 1..4                   */
  CUZFP_ERROR_BUFFER_TOO_SMALL = 3, /* stream capacity < needed bytes       */
  CUZFP_ERROR_HIP = 4               /* a HIP runtime call failed            */
} cuzfp_status;

int cuzfp_hip_abi_version(void);
const char* cuzfp_hip_status_string(int status);
/* last HIP error seen by this thread (hipSuccess if none) */
int cuzfp_hip_last_hip_error(void);

/* maxbits for `rate` bits/value: floor(4^dims * rate + 0.5), at least 1 + the
 * exponent bits (9 float, 12 double); wra != 0 rounds up to a multiple of 64,
 * which is what the reference's stream_set_rate does for 3D arrays. */
unsigned cuzfp_hip_rate_to_maxbits(double rate, int type, unsigned dims, int wra);

/* Exact compressed size: ceil(blocks * maxbits / 64) * 8.  ny == 0 -> 1D,
 * nz == 0 -> 2D. Returns 0 for invalid arguments. */
size_t cuzfp_hip_stream_bytes(int type, unsigned nx, unsigned ny, unsigned nz, unsigned maxbits);

/* Worst-case buffer size, the reference's zfp_stream_maximum_size. */
size_t cuzfp_hip_maximum_size(int type, unsigned nx, unsigned ny, unsigned nz, unsigned maxbits);

/* Compress a device-resident array into a device-resident stream.
 * Strides are in elements (0 = contiguous a[nz][ny][nx]; negative allowed).
 * *out_bytes (optional) receives cuzfp_hip_stream_bytes(). */
int cuzfp_hip_encode(const void* d_data, int type, unsigned nx, unsigned ny, unsigned nz,
                     long long sx, long long sy, long long sz, unsigned maxbits,
                     uint64_t* d_stream, size_t stream_capacity, size_t* out_bytes,
                     hipStream_t stream);

/* Decompress a device-resident stream into a device-resident array. */
int cuzfp_hip_decode(const uint64_t* d_stream, size_t stream_bytes, int type, unsigned nx,
                     unsigned ny, unsigned nz, long long sx, long long sy, long long sz,
                     unsigned maxbits, void* d_data, hipStream_t stream);

/* Not a reference entry point (callers test CUZFP_HIP_HAS_DECODE_REGION): fixed
 * rate puts block b at bits [b*maxbits, (b+1)*maxbits), so a box decodes from
 * its own blocks alone.
 * Decode the elements [ox, ox+ex) x [oy, oy+ey) x [oz, oz+ez) of the array that
 * d_stream holds (nx, ny, nz, maxbits as for cuzfp_hip_decode) into d_out, an
 * array of extent ex x ey x ez with element strides sx, sy, sz (0 = contiguous
 * out[ez][ey][ex]; negative allowed).  Unused dimensions: origin 0, extent 0.
 * CUZFP_ERROR_INVALID_ARGUMENT for an empty box or one that leaves the array;
 * stream_bytes must cover the whole array's stream. */
#define CUZFP_HIP_HAS_DECODE_REGION 1
int cuzfp_hip_decode_region(const uint64_t* d_stream, size_t stream_bytes, int type,
                            unsigned nx, unsigned ny, unsigned nz, unsigned maxbits,
                            unsigned ox, unsigned oy, unsigned oz,
                            unsigned ex, unsigned ey, unsigned ez,
                            long long sx, long long sy, long long sz,
                            void* d_out, hipStream_t stream);

/* Not a reference entry point (callers test CUZFP_HIP_HAS_ENCODE_REGION): the
 * write half of cuzfp_hip_decode_region.  Write the box [ox, ox+ex) x
 * [oy, oy+ey) x [oz, oz+ez) of new values into the existing stream d_stream of
 * an nx x ny x nz array at maxbits, in place.  d_box is element (0, 0, 0) of
 * the box, an array of extent ex x ey x ez with element strides sx, sy, sz
 * (0 = contiguous box[ez][ey][ex]; negative allowed).  Arguments and status
 * codes are those of cuzfp_hip_decode_region; stream_bytes must cover the whole
 * array's stream.
 *
 * Every block the box touches is re-coded and replaces its bits
 * [b*maxbits, (b+1)*maxbits); every other bit of the stream, the other blocks
 * and the zero padding after the last one, stays exactly as it was.
 *  - A block whose elements inside the array all lie inside the box (a box
 *    that reaches the array's far edge covers that edge's partial blocks) is
 *    coded from the box's values, elements outside the array padded from them
 *    as cuzfp_hip_encode pads.  Its old bits are not read.
 *  - A partially covered block is a read-modify-write: its old bits are
 *    decoded as cuzfp_hip_decode_region decodes them, the elements inside the
 *    box are replaced, and the result is encoded.  THE BLOCK'S OTHER ELEMENTS
 *    ARE RE-ENCODED FROM THEIR DECODED VALUES AND MAY THEREFORE CHANGE WITHIN
 *    THE RATE'S ERROR.  A block-aligned box (or one aligned at its origin and
 *    ending at the array's edges) touches no such block.
 * The result equals encoding the whole array after pasting the box into the
 * stream's decode, restricted to the bits of the box's blocks.
 *
 * Asynchronous on `stream`: one kernel launch, no allocation, no
 * synchronisation; it can be captured into a hipGraph.  d_box must not
 * overlap the stream.  Calls whose boxes share no block may run concurrently
 * (on different streams); calls that share a block must be ordered by the
 * caller.  CUZFP_ERROR_INVALID_ARGUMENT also when one wave's block images and
 * tables exceed the device's LDS per workgroup (see CUZFP_MAX_BITS; on gfx950
 * every maxbits fits). */
#define CUZFP_HIP_HAS_ENCODE_REGION 1
int cuzfp_hip_encode_region(const void* d_box, int type,
                            unsigned nx, unsigned ny, unsigned nz, unsigned maxbits,
                            unsigned ox, unsigned oy, unsigned oz,
                            unsigned ex, unsigned ey, unsigned ez,
                            long long sx, long long sy, long long sz,
                            uint64_t* d_stream, size_t stream_bytes, hipStream_t stream);

/* Not a reference entry point (callers test CUZFP_HIP_HAS_TRUNCATE): lower a
 * stream's rate without decoding it.  zfp's coder is embedded: a block coded
 * with a budget of m bits is the first m bits of the same block coded with any
 * larger budget M.  So the stream of an array at new_maxbits is the stream at
 * maxbits >= new_maxbits with every block cut down to its first new_maxbits
 * bits: store once at a high rate, ship or preview at a lower one.  Unlike
 * decoding and encoding again, this gives the low-rate stream of the ORIGINAL
 * values, bit for bit, and moves no uncompressed data.
 *
 * d_src holds the stream of an nx x ny x nz array of `type` at maxbits (as for
 * cuzfp_hip_decode).  Bits [b*m, (b+1)*m) of d_dst become bits [b*M, b*M + m)
 * of d_src for every block b (M = maxbits, m = new_maxbits); the bits from
 * nblocks*m up to the end of the last 64-bit word become zero, so d_dst is
 * byte-identical to what cuzfp_hip_encode gives at new_maxbits.  Exactly
 * cuzfp_hip_stream_bytes(type, nx, ny, nz, new_maxbits) bytes of d_dst are
 * written -- *out_bytes (optional) receives that count -- and no byte of
 * d_dst past them is touched.  new_maxbits == maxbits is a plain copy.
 *
 * There is no widening: new_maxbits > maxbits is CUZFP_ERROR_INVALID_ARGUMENT.
 * Zero-padding each block up to a higher rate does NOT decode to the same
 * values.  When the budget runs out inside a group scan the decoder still
 * deposits the pending one-bit where it stands; with trailing zeros appended
 * the scan runs on to the end of the bit plane and deposits it elsewhere.
 * new_maxbits has maxbits' lower bound (9 float, 12 double, 1 integer).
 *
 * There is no in-place form either, because blocks would race: the byte
 * ranges [d_src, + stream_bytes at maxbits) and [d_dst, + stream_bytes at
 * new_maxbits) must not overlap (the two addresses are compared on the host;
 * CUZFP_ERROR_INVALID_ARGUMENT, as for a null pointer).  They may be adjacent.
 * CUZFP_ERROR_BUFFER_TOO_SMALL when src_bytes or dst_capacity is less than the
 * respective stream.
 *
 * Asynchronous on `stream`: one kernel launch, no allocation, no
 * synchronisation; it can be captured into a hipGraph.  When both rates are
 * multiples of 64 bits (every 3D stream of cuZFP::compress) whole words move,
 * 16 bytes a lane when both are multiples of 128 and both pointers 16-byte
 * aligned; any other pair is assembled a 64-bit output word a lane. */
#define CUZFP_HIP_HAS_TRUNCATE 1
int cuzfp_hip_truncate(const uint64_t* d_src, size_t src_bytes, int type,
                       unsigned nx, unsigned ny, unsigned nz,
                       unsigned maxbits, unsigned new_maxbits,
                       uint64_t* d_dst, size_t dst_capacity, size_t* out_bytes,
                       hipStream_t stream);

/* Not a reference entry point (callers test CUZFP_HIP_HAS_DECODE_PREFIX):
 * cuzfp_hip_decode_region at a lower rate than the stream's, by the prefix
 * property above.  The blocks of d_stream sit maxbits apart; each is decoded
 * with a budget of prefix_bits <= maxbits.  The result is bit-identical to
 * cuzfp_hip_decode_region at prefix_bits on the stream cuzfp_hip_truncate
 * makes, but no intermediate stream is made and only the first prefix_bits
 * of each of the box's blocks are read.  prefix_bits has maxbits' lower bound
 * (9 float, 12 double, 1 integer); prefix_bits > maxbits is
 * CUZFP_ERROR_INVALID_ARGUMENT (no widening); prefix_bits == maxbits is
 * cuzfp_hip_decode_region.  Every other argument, the status codes and the
 * launch (one kernel, asynchronous, graph-capturable) are
 * cuzfp_hip_decode_region's; stream_bytes must cover the whole stream at
 * maxbits.  A whole-array decode at a lower rate is the box (0, 0, 0) +
 * (nx, ny, nz). */
#define CUZFP_HIP_HAS_DECODE_PREFIX 1
int cuzfp_hip_decode_region_prefix(const uint64_t* d_stream, size_t stream_bytes, int type,
                                   unsigned nx, unsigned ny, unsigned nz,
                                   unsigned maxbits, unsigned prefix_bits,
                                   unsigned ox, unsigned oy, unsigned oz,
                                   unsigned ex, unsigned ey, unsigned ez,
                                   long long sx, long long sy, long long sz,
                                   void* d_out, hipStream_t stream);

/* Not reference entry points (callers test CUZFP_HIP_HAS_VARIABLE): zfp's
 * variable-rate modes, fixed precision (zfp_stream_set_precision) and fixed
 * accuracy (zfp_stream_set_accuracy), float and double only (integer types:
 * CUZFP_ERROR_UNSUPPORTED_TYPE, as zfp 0.5.0's zfp_compress).
 *
 * The stream is byte-identical to CPU zfp 0.5.0's zfp_compress in that mode:
 * the blocks in raster order, back to back without padding, flushed with zero
 * bits to a 64-bit word, no header.  Block b takes lengths[b] bits (uint16,
 * at most 4171); the index `lengths` is a side array the caller keeps with
 * the stream (0.25 bit a value in 3D, 1 in 2D, 4 in 1D) -- it is what lets the
 * decoder start every block in parallel.
 *
 * A mode is the pair (maxprec, minexp):
 *   fixed precision p:  maxprec = p (1 .. 32 float, 1 .. 64 double), minexp = -1074
 *   fixed accuracy tol: maxprec = the type's precision (32 / 64),
 *                       minexp = cuzfp_hip_accuracy_to_minexp(tol)
 *
 * cuzfp_hip_accuracy_to_minexp: zfp_stream_set_accuracy's rule, floor(log2
 *   tolerance) by frexp, or -1074 (ZFP_MIN_EXP) for a tolerance <= 0.
 * cuzfp_hip_variable_maximum_size: the worst-case stream bytes
 *   (zfp_stream_maximum_size in these modes, its header allowance included,
 *   as cuzfp_hip_maximum_size); 0 for invalid arguments.
 * cuzfp_hip_variable_workspace_bytes: bytes of device scratch either call
 *   below needs (the blocks' 64-bit offsets and the scan's partial sums); the
 *   caller owns it (8-byte aligned); 0 for invalid arguments.
 *
 * cuzfp_hip_encode_variable: asynchronous on `stream`, no allocation, no
 *   synchronisation (six kernel launches: lengths, a three-launch scan, a
 *   zero fill, the coder).  Strides as cuzfp_hip_encode.  Writes
 *   d_lengths[0 .. nblocks) and the 64-bit bit count *d_total_bits (both device
 *   memory: the count depends on the data), and the stream's ceil(total / 64)
 *   words, no byte past them and none at or past stream_capacity: if the
 *   stream does not fit, the lengths and the count are still right and the
 *   stream's contents are unspecified (cuzfp_hip_variable_maximum_size bytes
 *   always fit).  maxprec outside 1 .. the type's precision, a null pointer or
 *   a workspace below cuzfp_hip_variable_workspace_bytes:
 *   CUZFP_ERROR_INVALID_ARGUMENT.
 * cuzfp_hip_decode_variable: the same launch properties (a three-launch scan
 *   of the lengths, the decoder).  Block b is decoded from the sum of the
 *   lengths before it with a budget of d_lengths[b] bits; the result is what
 *   zfp_decompress returns in the mode that wrote the stream.  The index is
 *   not trusted: whatever it holds, nothing outside [d_stream, d_stream +
 *   stream_bytes) is read; blocks whose entries are wrong decode to
 *   unspecified values. */
#define CUZFP_HIP_HAS_VARIABLE 1
int cuzfp_hip_accuracy_to_minexp(double tolerance);
size_t cuzfp_hip_variable_maximum_size(int type, unsigned nx, unsigned ny, unsigned nz, unsigned maxprec);
size_t cuzfp_hip_variable_workspace_bytes(int type, unsigned nx, unsigned ny, unsigned nz);
int cuzfp_hip_encode_variable(const void* d_data, int type, unsigned nx, unsigned ny, unsigned nz,
                              long long sx, long long sy, long long sz, unsigned maxprec, int minexp,
                              uint64_t* d_stream, size_t stream_capacity, uint16_t* d_lengths,
                              uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes,
                              hipStream_t stream);
int cuzfp_hip_decode_variable(const uint64_t* d_stream, size_t stream_bytes, const uint16_t* d_lengths,
                              int type, unsigned nx, unsigned ny, unsigned nz,
                              long long sx, long long sy, long long sz, void* d_data,
                              void* d_workspace, size_t workspace_bytes, hipStream_t stream);

/* Not reference entry points (callers test CUZFP_HIP_HAS_VARIABLE_REGION):
 * random access into a variable-rate stream.  cuzfp_hip_decode_variable scans
 * all the lengths on every call and decodes the whole array; with a
 * persistent offset index, built once and kept beside `lengths`, a sub-box is
 * decoded in one launch that reads only the box's blocks.
 *
 * The index is one uint64 per tile of 64 raster-consecutive blocks plus the
 * total, T = ceil(nblocks / 64):
 *   index[t] = sum of lengths[0 .. 64 t)   t = 0 .. T - 1
 *   index[T] = sum of all lengths (the stream's bit count)
 * (the raw uint16 values summed), 8 (T + 1) bytes: a sixteenth of `lengths`.
 * Block b starts at bit index[b / 64] + the sum of lengths[64 (b / 64) .. b).
 *
 * cuzfp_hip_variable_index_bytes: 8 (T + 1); 0 for invalid dimensions and
 *   integer types.
 * cuzfp_hip_variable_index: asynchronous on `stream`, no allocation, no
 *   synchronisation (the three-launch scan into the workspace, one launch that
 *   picks every 64th offset).  d_lengths needs no alignment beyond a
 *   uint16's; d_index and the workspace 8 bytes.  The workspace is
 *   cuzfp_hip_variable_workspace_bytes.  A null or misaligned pointer, a short
 *   index_bytes or workspace: CUZFP_ERROR_INVALID_ARGUMENT before any launch;
 *   integer types CUZFP_ERROR_UNSUPPORTED_TYPE.
 * cuzfp_hip_decode_region_variable: the box origin + extent of the array the
 *   stream holds into d_out, bit for bit the box of cuzfp_hip_decode_variable's
 *   array.  One kernel launch, no workspace, no allocation, no
 *   synchronisation; it can be captured into a graph.  Box, stride and
 *   unused-dimension rules and their status codes are
 *   cuzfp_hip_decode_region's (d_out is the box's element (0, 0, 0), strides 0 =
 *   contiguous out[ez][ey][ex]); a null or misaligned pointer (d_stream 4
 *   bytes, d_index 8) or a short index_bytes: CUZFP_ERROR_INVALID_ARGUMENT.
 *   stream_bytes is the bound of the loads, not checked against the index.
 *   Neither the index nor the lengths are trusted: whatever they hold, nothing
 *   outside [d_stream, d_stream + stream_bytes), d_lengths[0 .. nblocks) and
 *   d_index[0 .. T) is read and nothing outside the box is written; blocks
 *   whose entries are wrong decode to unspecified values. */
#define CUZFP_HIP_HAS_VARIABLE_REGION 1
size_t cuzfp_hip_variable_index_bytes(int type, unsigned nx, unsigned ny, unsigned nz);
int cuzfp_hip_variable_index(const uint16_t* d_lengths, int type, unsigned nx, unsigned ny, unsigned nz,
                             uint64_t* d_index, size_t index_bytes,
                             void* d_workspace, size_t workspace_bytes, hipStream_t stream);
int cuzfp_hip_decode_region_variable(const uint64_t* d_stream, size_t stream_bytes,
                                     const uint16_t* d_lengths, const uint64_t* d_index, size_t index_bytes,
                                     int type, unsigned nx, unsigned ny, unsigned nz,
                                     unsigned ox, unsigned oy, unsigned oz,
                                     unsigned ex, unsigned ey, unsigned ez,
                                     long long sx, long long sy, long long sz, void* d_out, hipStream_t stream);

/* Not reference entry points (callers test CUZFP_HIP_HAS_VARIABLE_TRUNCATE):
 * coarsen a variable-rate stream without recoding -- cuzfp_hip_truncate's
 * counterpart for the variable-rate modes.
 *
 * The rule.  A stream written at the mode (maxprec, minexp) can be cut to
 * (new_maxprec, new_minexp) when new_maxprec <= maxprec and new_minexp >=
 * minexp (anything else is widening and is refused); precision and accuracy
 * modes mix freely under it, e.g. a full-precision stream (maxprec 32 / 64,
 * minexp -1074) can be cut to any tolerance.  The coder is embedded, so every
 * block of the coarser stream is then the first bits of the finer stream's
 * block, up to the end of the planes the coarser mode codes for the block's
 * exponent -- with one exception: a block the coarser mode codes no plane of
 * becomes the one-bit form, the single bit 0, while the finer block starts
 * with a 1.  The result is byte for byte the stream, and the lengths, CPU zfp
 * 0.5.0 writes for the original array at (new_maxprec, new_minexp).  Nothing
 * is decoded: a block's new length is found by walking its bit-plane code,
 * and its prefix is copied.
 *
 * cuzfp_hip_truncate_variable_workspace_bytes: bytes of device scratch the
 *   call needs (both streams' 64-bit block offsets and the scan's partial
 *   sums), 8-byte aligned; 0 for invalid dimensions and integer types.
 * cuzfp_hip_truncate_variable: asynchronous on `stream`, no allocation, no
 *   synchronisation (two three-launch scans, the lengths pass, a zero fill,
 *   the copy pass).  Writes d_lengths[0 .. nblocks), the 64-bit bit count
 *   *d_total_bits, and the new stream's ceil(total / 64) words with zero pad
 *   bits in the last, no byte past them and none at or past dst_capacity: if
 *   the stream does not fit, the lengths and the count are still right and
 *   d_dst's contents are unspecified.  No new length exceeds its block's
 *   source length, so src_bytes always fit.  d_dst == NULL with dst_capacity
 *   == 0 is the size query: lengths and count only.  The source index is not
 *   trusted, by cuzfp_hip_decode_variable's rule: a length is clamped to the
 *   type's longest block, one no coded block can have reads as a zero block,
 *   and whatever d_src_lengths holds, nothing outside [d_src, d_src +
 *   src_bytes) and d_src_lengths[0 .. nblocks) is read and nothing outside the
 *   outputs is written; blocks whose entries are wrong give unspecified bits.
 *   Before any launch: CUZFP_ERROR_UNSUPPORTED_TYPE for integer types;
 *   CUZFP_ERROR_INVALID_ARGUMENT for widening, maxprec or new_maxprec outside
 *   1 .. the type's precision, a null or misaligned pointer (d_src 4 bytes,
 *   the lengths 2, d_dst, d_total_bits and the workspace 8), a workspace below
 *   cuzfp_hip_truncate_variable_workspace_bytes, [d_src, d_src + src_bytes)
 *   overlapping [d_dst, d_dst + dst_capacity), and d_lengths overlapping
 *   d_src_lengths. */
#define CUZFP_HIP_HAS_VARIABLE_TRUNCATE 1
size_t cuzfp_hip_truncate_variable_workspace_bytes(int type, unsigned nx, unsigned ny, unsigned nz);
int cuzfp_hip_truncate_variable(const uint64_t* d_src, size_t src_bytes, const uint16_t* d_src_lengths,
                                int type, unsigned nx, unsigned ny, unsigned nz,
                                unsigned maxprec, int minexp, unsigned new_maxprec, int new_minexp,
                                uint64_t* d_dst, size_t dst_capacity, uint16_t* d_lengths,
                                uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes,
                                hipStream_t stream);

/* Not a reference entry point (callers test
 * CUZFP_HIP_HAS_VARIABLE_DECODE_COARSE): decode a sub-box of a variable-rate
 * stream at a coarser precision or tolerance straight from the fine stream --
 * what cuzfp_hip_decode_region_prefix is to cuzfp_hip_truncate, for the
 * variable-rate modes.  cuzfp_hip_truncate_variable makes the coarser *stream*;
 * this call makes no stream, no lengths and no index, and its work is
 * proportional to the box.
 *
 * The target mode is (maxprec, minexp): precision p is (p, -1074), tolerance t
 * is (the type's 32 / 64, cuzfp_hip_accuracy_to_minexp(t)).  Every block of the
 * box is decoded from the first L' of its bits, L' its length at the target
 * mode, found by walking its bit-plane code as cuzfp_hip_truncate_variable
 * does; a block the target codes no plane of decodes to zeros.  Where the
 * target coarsens the mode that wrote the stream (cuzfp_hip_truncate_variable's
 * rule), the box is bit for bit the box of cuzfp_hip_decode_variable on
 * cuzfp_hip_truncate_variable's output, and of what CPU zfp 0.5.0's
 * zfp_decompress returns for its own stream at the target mode.
 *
 * Never finer than the stream.  The call does not take the mode that wrote the
 * stream, and refuses no target for being finer: the walk ends at the block's
 * own length, so a block decodes from at most the bits the stream holds of it.
 * The result is the array at (the smaller of the two maxprec, the larger of
 * the two minexp); a target at or above the stream's mode gives
 * cuzfp_hip_decode_region_variable's bytes.  Nothing finer than the stream
 * comes out: widening is still not offered.
 *
 * One kernel launch, no workspace, no allocation, no synchronisation; it can be
 * captured into a graph.  The arguments other than the target are
 * cuzfp_hip_decode_region_variable's, with its checks in its order and its
 * status codes; maxprec outside 1 .. the type's precision is
 * CUZFP_ERROR_INVALID_ARGUMENT, integer types CUZFP_ERROR_UNSUPPORTED_TYPE,
 * all before any launch.  Neither the stream, the index nor the lengths are
 * trusted: whatever they hold, nothing outside [d_stream, d_stream +
 * stream_bytes), d_lengths[0 .. nblocks) and d_index[0 .. T) is read and
 * nothing outside the box is written.  The kernel's block image is sized for
 * the longest block a mode with `maxprec` planes writes; a block whose bits
 * walk further than that (arbitrary bits, entries of another stream) is
 * decoded from that many bits and, like any block whose entries are wrong,
 * gives unspecified values. */
#define CUZFP_HIP_HAS_VARIABLE_DECODE_COARSE 1
int cuzfp_hip_decode_region_variable_coarse(const uint64_t* d_stream, size_t stream_bytes,
                                            const uint16_t* d_lengths, const uint64_t* d_index, size_t index_bytes,
                                            int type, unsigned nx, unsigned ny, unsigned nz,
                                            unsigned maxprec, int minexp,
                                            unsigned ox, unsigned oy, unsigned oz,
                                            unsigned ex, unsigned ey, unsigned ez,
                                            long long sx, long long sy, long long sz, void* d_out,
                                            hipStream_t stream);

/* Not reference entry points (callers test
 * CUZFP_HIP_HAS_ENCODE_REGION_VARIABLE): write new values for a sub-box into a
 * variable-rate stream -- cuzfp_hip_encode_region's counterpart for the
 * variable-rate modes.  Block lengths change, so the update is out of place:
 * the call reads the stream, its lengths and its offset index and writes the
 * stream, the lengths, the bit count and (optionally) the index of the updated
 * array.
 *
 * With A the array the source decodes to, M = A with the box replaced by d_box,
 * and E the stream cuzfp_hip_encode_variable writes for M at (maxprec, minexp):
 * a block the box touches is E's block, with E's length; any other block is
 * its bits of the source, unchanged, with its source length; the blocks lie
 * back to back in raster order and the pad to the next 64-bit word is zero
 * (the layout of cuzfp_hip_encode_variable and cuzfp_hip_truncate_variable).
 * A touched block all of whose elements inside the array lie in the box is
 * coded from d_box alone; any other touched block is decoded from its old
 * bits, the box's elements are replaced, elements outside the array are padded
 * by the encoder's rule, and it is coded again -- its other elements are thus
 * re-coded from decoded values, as in cuzfp_hip_encode_region.  A box that is
 * a union of covered blocks, filled with the new array's values, gives byte
 * for byte cuzfp_hip_encode_variable of the new array.  (maxprec, minexp)
 * applies to the touched blocks only and need not be the mode that wrote the
 * rest: the decoders need block boundaries, not the mode.
 *
 * cuzfp_hip_encode_region_variable_workspace_bytes: device scratch of the call
 *   (the new 64-bit block offsets and the scan's partial sums), 8-byte aligned;
 *   0 for invalid dimensions and integer types.
 * cuzfp_hip_encode_region_variable_maximum_size: 8 * ceil((8 * src_bytes +
 *   touched_blocks * B) / 64) bytes, B the most bits a block takes at maxprec
 *   (cuzfp_hip_variable_maximum_size's): a true bound on the result, every
 *   replaced block giving back at least one bit, proportional to the stream
 *   and the box, not to the array.  0 for an invalid argument.
 * cuzfp_hip_encode_region_variable: asynchronous on `stream`, no allocation, no
 *   synchronisation (a copy of the lengths, the lengths pass over the touched
 *   blocks, a three-launch scan, a zero fill, the copy pass over all blocks,
 *   the encode pass over the touched blocks).  d_box is the box's element
 *   (0, 0, 0), sx, sy, sz its element strides (0: contiguous).  d_src_index is
 *   cuzfp_hip_variable_index of d_src_lengths, index_bytes its size.  Writes
 *   d_lengths[0 .. nblocks), *d_total_bits, the result's ceil(total / 64)
 *   words, no byte past them and none at or past dst_capacity (if the stream
 *   does not fit, the lengths, the count and the index are still right and
 *   d_dst's contents are unspecified), and, unless d_index is NULL, the
 *   result's offset index there (index_bytes: the two indices have one size),
 *   equal to cuzfp_hip_variable_index of d_lengths.  The source index and
 *   lengths are not trusted, by the decoders' rule: whatever they hold, nothing
 *   outside [d_src, d_src + src_bytes), d_src_lengths[0 .. nblocks) and
 *   d_src_index[0 .. T) is read and nothing outside the outputs is written;
 *   blocks whose entries are wrong give unspecified bits (the lengths of the
 *   covered blocks are still those of E).
 *   Before any launch: CUZFP_ERROR_UNSUPPORTED_TYPE for integer and unknown
 *   types; CUZFP_ERROR_INVALID_ARGUMENT for invalid dimensions, maxprec outside
 *   1 .. the type's precision, a null pointer (d_index and, with dst_capacity
 *   0, d_dst excepted), a misaligned one (d_src 4 bytes, the lengths 2, the
 *   indices, d_dst, d_total_bits and the workspace 8), the box errors of
 *   cuzfp_hip_decode_region, index_bytes below cuzfp_hip_variable_index_bytes,
 *   a workspace below cuzfp_hip_encode_region_variable_workspace_bytes, [d_src,
 *   d_src + src_bytes) overlapping [d_dst, d_dst + dst_capacity), d_lengths
 *   overlapping d_src_lengths, and d_index overlapping d_src_index. */
#define CUZFP_HIP_HAS_ENCODE_REGION_VARIABLE 1
size_t cuzfp_hip_encode_region_variable_workspace_bytes(int type, unsigned nx, unsigned ny, unsigned nz);
size_t cuzfp_hip_encode_region_variable_maximum_size(int type, unsigned nx, unsigned ny, unsigned nz,
                                                     size_t src_bytes, unsigned ex, unsigned ey, unsigned ez,
                                                     unsigned ox, unsigned oy, unsigned oz, unsigned maxprec);
int cuzfp_hip_encode_region_variable(const void* d_box, long long sx, long long sy, long long sz, int type,
                                     unsigned nx, unsigned ny, unsigned nz, unsigned maxprec, int minexp,
                                     unsigned ox, unsigned oy, unsigned oz,
                                     unsigned ex, unsigned ey, unsigned ez,
                                     const uint64_t* d_src, size_t src_bytes, const uint16_t* d_src_lengths,
                                     const uint64_t* d_src_index, size_t index_bytes,
                                     uint64_t* d_dst, size_t dst_capacity, uint16_t* d_lengths, uint64_t* d_index,
                                     uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes,
                                     hipStream_t stream);

/* Not reference entry points (callers test CUZFP_HIP_HAS_VARIABLE_CROP): crop a
 * box of blocks out of a variable-rate stream into a stream of its own, and
 * paste such a stream into a box of another -- both in the compressed domain.
 * zfp codes every 4^d block on its own, and a block's code depends only on its
 * values and on which of its elements lie inside the array, so both are moves
 * of bits: nothing is decoded, nothing is coded again, the result is exact and
 * no mode is needed.
 *
 * The aligned box.  Both calls take only a box that is aligned: on every used
 * axis origin % 4 == 0, and extent % 4 == 0 or origin + extent == n.  Such a box
 * is a union of whole blocks, and each of them has the same elements inside the
 * box as inside the array.  Any other box is CUZFP_ERROR_INVALID_ARGUMENT;
 * cuzfp_hip_decode_region_variable and cuzfp_hip_encode_region_variable handle
 * partial coverage, by decoding.
 *
 * cuzfp_hip_extract_region_variable: the stream of the sub-array origin +
 *   extent, as a stand-alone stream of an array of shape extent.  Box block r,
 *   in the box's raster order (x fastest), is source block b = ((bz0 + rz) * by +
 *   by0 + ry) * bx + bx0 + rx, copied bit for bit with its raw source length to
 *   d_lengths[r]; the blocks lie back to back and the pad to the next 64-bit
 *   word is zero.  Where the source is cuzfp_hip_encode_variable's (or CPU zfp
 *   0.5.0's) stream of an array A, the result is byte for byte its stream of
 *   A[box] at the same mode.  Unless d_index is NULL the box's offset index,
 *   equal to cuzfp_hip_variable_index of d_lengths, goes there
 *   (dst_index_bytes >= cuzfp_hip_variable_index_bytes of the extent: the box's
 *   index is smaller than the source's).  Asynchronous on `stream`, no
 *   allocation, no synchronisation (a gather of the box's lengths, a
 *   three-launch scan, a zero fill, the copy pass).
 * cuzfp_hip_extract_region_variable_workspace_bytes(type, ex, ey, ez): device
 *   scratch of the call, cuzfp_hip_variable_workspace_bytes of an array of the
 *   box's extent; 0 for invalid dimensions and integer types.
 * cuzfp_hip_extract_region_variable_maximum_size: 8 * ceil(min(8 * src_bytes,
 *   box_blocks * B) / 64) bytes, B the longest block of the type (what
 *   cuzfp_hip_variable_maximum_size counts a block at, at the type's
 *   precision).  0 for an invalid argument, a box that is not aligned included.
 *
 * cuzfp_hip_insert_region_variable: the stream d_src of the array (nx, ny, nz)
 *   with the blocks of the box replaced by those of the stream d_box, out of
 *   place like cuzfp_hip_encode_region_variable.  Block b of the result is box
 *   block r, with d_box_lengths[r], if b lies in the box; otherwise it is its
 *   bits of the source, unchanged, with its source length.  The blocks are
 *   packed back to back with a zero pad.  d_box_index is
 *   cuzfp_hip_variable_index of d_box_lengths (box_index_bytes its size),
 *   d_src_index that of d_src_lengths (index_bytes: the source's and the
 *   result's index have one size).  The box stream must be of the array's
 *   scalar type and rank and hold the box's block count of blocks; the caller
 *   states that and the call cannot check it.  The call knows no modes: a
 *   full-precision brick may be pasted into a fixed-accuracy archive, as the
 *   decoders need block boundaries, not the mode.  Neither input is modified.
 *   Asynchronous on `stream`, no allocation, no synchronisation (a copy of the
 *   source lengths, a scatter of the box lengths, a three-launch scan, a zero
 *   fill, one copy pass over all blocks).
 * cuzfp_hip_insert_region_variable_workspace_bytes(type, nx, ny, nz):
 *   cuzfp_hip_variable_workspace_bytes; 0 for invalid dimensions and integer
 *   types.
 * cuzfp_hip_insert_region_variable_maximum_size(src_bytes, box_bytes): 8 *
 *   ceil((8 * src_bytes + 8 * box_bytes) / 64): every block of the result is
 *   bits of one of the two.
 *
 * Both calls write d_lengths (the box's block count of entries for extract,
 * nblocks for insert), *d_total_bits, the result's ceil(total / 64) words, no
 * byte past them and none at or past dst_capacity (if the stream does not fit,
 * the lengths, the count and the index are still right and d_dst's contents are
 * unspecified), and, unless d_index is NULL, the result's offset index.  d_dst
 * == NULL with dst_capacity == 0 is the size query.  No index and no lengths
 * array is trusted, the source's or the box's, by the decoders' rule: whatever
 * they hold, nothing outside [d_src, d_src + src_bytes), d_src_lengths[0 ..
 * nblocks), d_src_index[0 .. T) and, for insert, [d_box, d_box + box_bytes),
 * d_box_lengths[0 .. box_blocks) and d_box_index[0 .. ceil(box_blocks / 64)) is
 * read and nothing outside the outputs is written; a copied length is clamped
 * to the type's longest block, and blocks whose entries are wrong give
 * unspecified bits.
 * Before any launch: CUZFP_ERROR_UNSUPPORTED_TYPE for integer and unknown
 * types; CUZFP_ERROR_INVALID_ARGUMENT for invalid dimensions, a null pointer
 * (d_index and, with dst_capacity 0, d_dst excepted), a misaligned one (the
 * input streams 4 bytes, the lengths 2, the indices, d_dst, d_total_bits and
 * the workspace 8), the box errors of cuzfp_hip_decode_region, a box that is not
 * aligned, a short index_bytes, box_index_bytes, dst_index_bytes or workspace,
 * and an output that overlaps an input: d_dst an input stream, d_lengths an
 * input's lengths, d_index an input's index. */
#define CUZFP_HIP_HAS_VARIABLE_CROP 1
size_t cuzfp_hip_extract_region_variable_workspace_bytes(int type, unsigned ex, unsigned ey, unsigned ez);
size_t cuzfp_hip_extract_region_variable_maximum_size(int type, unsigned nx, unsigned ny, unsigned nz,
                                                      size_t src_bytes, unsigned ex, unsigned ey, unsigned ez,
                                                      unsigned ox, unsigned oy, unsigned oz);
int cuzfp_hip_extract_region_variable(const uint64_t* d_src, size_t src_bytes, const uint16_t* d_src_lengths,
                                      const uint64_t* d_src_index, size_t index_bytes,
                                      int type, unsigned nx, unsigned ny, unsigned nz,
                                      unsigned ox, unsigned oy, unsigned oz,
                                      unsigned ex, unsigned ey, unsigned ez,
                                      uint64_t* d_dst, size_t dst_capacity, uint16_t* d_lengths,
                                      uint64_t* d_index, size_t dst_index_bytes, uint64_t* d_total_bits,
                                      void* d_workspace, size_t workspace_bytes, hipStream_t stream);
size_t cuzfp_hip_insert_region_variable_workspace_bytes(int type, unsigned nx, unsigned ny, unsigned nz);
size_t cuzfp_hip_insert_region_variable_maximum_size(size_t src_bytes, size_t box_bytes);
int cuzfp_hip_insert_region_variable(const uint64_t* d_box, size_t box_bytes, const uint16_t* d_box_lengths,
                                     const uint64_t* d_box_index, size_t box_index_bytes,
                                     const uint64_t* d_src, size_t src_bytes, const uint16_t* d_src_lengths,
                                     const uint64_t* d_src_index, size_t index_bytes,
                                     int type, unsigned nx, unsigned ny, unsigned nz,
                                     unsigned ox, unsigned oy, unsigned oz,
                                     unsigned ex, unsigned ey, unsigned ez,
                                     uint64_t* d_dst, size_t dst_capacity, uint16_t* d_lengths, uint64_t* d_index,
                                     uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes,
                                     hipStream_t stream);

/* Not a reference entry point (callers test CUZFP_HIP_HAS_VARIABLE_JOIN): the
 * variable-rate streams of K slabs of an array concatenated into the stream of
 * the array, in one pass and in the compressed domain.  zfp codes every block
 * on its own and writes the blocks back to back in raster order, so the stream
 * of an array is the streams of its z-slabs (3D; y-slabs in 2D, x-ranges in 1D)
 * one after the other, bit for bit -- where every slab but the last is a
 * multiple of 4 deep.  A slab's stream ends at an arbitrary bit, so the join is
 * a funnel shift, not a copy.  It is the inverse of
 * cuzfp_hip_extract_region_variable on slabs.
 *
 * parts: a host array of nparts entries, read before the call returns.  Part k
 *   is the stream [d_words, d_words + bytes) (device memory, as
 *   cuzfp_hip_encode_variable wrote it) of nblocks blocks with its raw lengths
 *   d_lengths[0 .. nblocks); the parts hold the result's blocks [B_k, B_{k+1})
 *   in order, B_k the sum of the nblocks before k.  nblocks is a positive
 *   multiple of the blocks in one 4-deep slab of the slowest axis (bx * by in
 *   3D, bx in 2D, 1 in 1D) and the nblocks sum to the array's block count.  The
 *   call takes at most 64 parts: the table travels in the kernel arguments, so
 *   there is no host-to-device copy, no allocation and no synchronisation, and
 *   the call can be captured into a graph.  No index of a part is needed.
 * The result: d_lengths = the parts' lengths concatenated (nblocks entries);
 *   *d_total_bits = their sum; the stream's bits [O_k, O_{k+1}) = part k's bits
 *   [0, O_{k+1} - O_k), O_k the sum of the lengths before block B_k; a zero pad
 *   to the next 64-bit word; unless d_index is NULL, the offset index
 *   (cuzfp_hip_variable_index_bytes of the array), equal to
 *   cuzfp_hip_variable_index of d_lengths.  ceil(total / 64) words are written,
 *   each once, no byte past them and none at or past dst_capacity (if the stream
 *   does not fit, the lengths, the count and the index are still right and
 *   d_dst's contents are unspecified).  d_dst == NULL with dst_capacity == 0 is
 *   the size query.  No part is modified.  Asynchronous on `stream` (a gather of
 *   the lengths, a three-launch scan, the index, one copy pass).
 * cuzfp_hip_join_variable_workspace_bytes: cuzfp_hip_variable_workspace_bytes;
 *   0 for invalid dimensions and integer types.
 * cuzfp_hip_join_variable_maximum_size: 8 * ceil(8 * sum(bytes) / 64): every
 *   bit of the result is a bit of a part.  0 for a NULL table, nparts of 0 or
 *   above 64, or byte counts whose bits would wrap.
 * The lengths are not trusted: whatever they hold, nothing outside the parts'
 *   [d_words, d_words + bytes) and d_lengths[0 .. nblocks) is read, nothing
 *   outside the outputs is written, d_lengths, the total and the index are the
 *   raw concatenation and its sums, and the stream's words are unspecified where
 *   a part's lengths do not belong to it.
 * Before any launch: CUZFP_ERROR_UNSUPPORTED_TYPE for integer and unknown
 *   types; CUZFP_ERROR_INVALID_ARGUMENT for invalid dimensions, a NULL table,
 *   nparts of 0 or above 64, a part whose nblocks is 0 or no whole number of
 *   slabs, nblocks that do not sum to the array's block count, a null pointer
 *   (d_index and, with dst_capacity 0, d_dst excepted), a misaligned one (part
 *   streams 4 bytes, lengths 2, d_dst, d_index, d_total_bits and the workspace
 *   8), a short workspace, and an output (d_dst, d_lengths, d_index,
 *   d_total_bits, the workspace) that overlaps a part's stream or lengths. */
#define CUZFP_HIP_HAS_VARIABLE_JOIN 1
typedef struct {
  const uint64_t* d_words;   /* the part's stream, 4-byte aligned */
  size_t bytes;              /* ... and its size */
  const uint16_t* d_lengths; /* the raw length of each of its blocks */
  unsigned nblocks;          /* how many */
} cuzfp_hip_variable_part;
size_t cuzfp_hip_join_variable_workspace_bytes(int type, unsigned nx, unsigned ny, unsigned nz);
size_t cuzfp_hip_join_variable_maximum_size(const cuzfp_hip_variable_part* parts, unsigned nparts);
int cuzfp_hip_join_variable(const cuzfp_hip_variable_part* parts, unsigned nparts,
                            int type, unsigned nx, unsigned ny, unsigned nz,
                            uint64_t* d_dst, size_t dst_capacity, uint16_t* d_lengths, uint64_t* d_index,
                            uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes, hipStream_t stream);

/* Host-memory end to end: the array and the stream live in
 * host memory; the library moves them in z-slab (3D) / y-slab (2D) / x-range
 * (1D) chunks on three HIP streams -- input copies, kernels, output copies,
 * each in chunk order -- so the copies overlap the kernels and each other
 * (64 MiB chunks between pinned buffers, smaller ones at the pipeline's ends;
 * 8 MiB through `nstreams` pinned staging buffers for pageable ones).
 * Synchronous; contiguous arrays only.  Environment (read per call):
 * CUZFP_HOST_CHUNK_BYTES sets the chunk size, CUZFP_HOST_ORDERED=0 selects
 * round 4's schedule (chunk i's copies and kernel on stream i % nstreams),
 * CUZFP_HOST_ZEROCOPY: 1 (default) compresses a pinned array into a pinned
 * stream in one kernel that loads and stores them over PCIe itself, 2 also
 * lets the decode kernels store to a pinned array, 0 copies everything
 * (capi.hip host_zero_copy has the measurements).  The first call on a device
 * also times which of its streams carry which copies (~15 ms, once).
 *
 * Retention: the first call on a device allocates, and keeps for later calls,
 * device buffers for the array and the stream (grown to the largest call, up
 * to 1 GiB each; larger calls use buffers freed on return), its HIP streams
 * with their events, and (for pageable user buffers) pinned staging buffers of
 * one chunk each (at most 64 MiB apiece).  This memory is outside any
 * framework allocator (e.g. torch's caching allocator).  Calls on one device
 * are serialised; calls on different devices run concurrently. */
int cuzfp_hip_compress_host(const void* h_data, int type, unsigned nx, unsigned ny,
                            unsigned nz, unsigned maxbits, void* h_stream,
                            size_t stream_capacity, size_t* out_bytes, int nstreams);
int cuzfp_hip_decompress_host(const void* h_stream, size_t stream_bytes, int type,
                              unsigned nx, unsigned ny, unsigned nz, unsigned maxbits,
                              void* h_data, int nstreams);

/* Frees the host pipeline's retained buffers, streams and events for `device`
 * (-1: the current device) after its pending work; the next host-pipeline call
 * allocates them again.  Not a reference entry point. */
int cuzfp_hip_release_host_cache(int device);

/* Diagnostic, not a reference entry point: device-to-device copy of `bytes`
 * (a multiple of 16, both pointers 16-byte aligned) with 16-byte non-temporal
 * loads and stores -- the codec's access width and cache policy.  bench.py
 * times it as the achievable-HBM-bandwidth calibrator. */
int cuzfp_hip_copy(const void* d_src, void* d_dst, size_t bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
