"""cuzfp_amd -- MI355X-native zfp fixed-rate codec (drop-in for mclarsen/cuZFP).

The codec is hand-written HIP for gfx950 (``cuzfp_amd/csrc``), exposed through
the C-ABI of ``include/cuzfp_hip.h`` (``lib/libcuzfp_hip.so``) and the
reference's C++ surface ``cuZFP::compress / decompress`` (``lib/libcuZFP.so``).
This module is the Python binding of that C-ABI; PyTorch provides device
memory and streams only.  There is no CPU fallback: every entry point raises
if the HIP library is missing.

Array shapes are numpy/torch order (slowest first): ``(nx,)``, ``(ny, nx)``,
``(nz, ny, nx)`` -- the reference's ``a[nz][ny][nx]`` (zfp_structs.h:42).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

__all__ = [
    "TYPE_INT32", "TYPE_INT64", "TYPE_FLOAT", "TYPE_DOUBLE", "CodecError",
    "library", "library_path", "rate_to_maxbits", "stream_bytes", "maximum_size",
    "encode", "decode", "decode_region", "encode_region", "truncate", "compress_host", "decompress_host", "type_code",
    "encode_variable", "decode_variable", "accuracy_to_minexp", "variable_maximum_size",
    "variable_index", "decode_region_variable", "truncate_variable", "encode_region_variable",
    "extract_region_variable", "insert_region_variable", "join_variable",
]

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")

TYPE_INT32, TYPE_INT64, TYPE_FLOAT, TYPE_DOUBLE = 1, 2, 3, 4
_NP_TYPES = {np.dtype(np.int32): 1, np.dtype(np.int64): 2,
             np.dtype(np.float32): 3, np.dtype(np.float64): 4}
_STATUS = {0: "success", 1: "invalid argument", 2: "unsupported scalar type",
           3: "stream buffer too small", 4: "HIP runtime error"}


class CodecError(RuntimeError):
    """A non-zero cuzfp_status from the C-ABI."""

    def __init__(self, where: str, status: int, hip_error: int = 0):
        msg = f"{where}: {_STATUS.get(status, status)}"
        if status == 4:
            msg += f" (hipError {hip_error})"
        super().__init__(msg)
        self.status = status


class VariablePart(ctypes.Structure):
    """cuzfp_hip_variable_part: one part of `cuzfp_hip_join_variable`."""
    _fields_ = [("d_words", ctypes.c_void_p), ("bytes", ctypes.c_size_t), ("d_lengths", ctypes.c_void_p),
                ("nblocks", ctypes.c_uint)]


_lib = None


def library_path() -> str:
    """The in-tree build; CUZFP_HIP_LIB overrides it (A/B runs of kernel variants)."""
    return os.environ.get("CUZFP_HIP_LIB") or os.path.join(LIB_DIR, "libcuzfp_hip.so")


def library() -> ctypes.CDLL:
    """Load ``libcuzfp_hip.so`` (built by ``cuzfp_amd/build.py``); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"cuzfp_amd: HIP codec library not built ({path}); "
                           "run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(path)
    u, i, sz, vp, ll = ctypes.c_uint, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_longlong
    lib.cuzfp_hip_abi_version.restype = i
    lib.cuzfp_hip_status_string.restype = ctypes.c_char_p
    lib.cuzfp_hip_status_string.argtypes = [i]
    lib.cuzfp_hip_last_hip_error.restype = i
    lib.cuzfp_hip_rate_to_maxbits.restype = u
    lib.cuzfp_hip_rate_to_maxbits.argtypes = [ctypes.c_double, i, u, i]
    lib.cuzfp_hip_stream_bytes.restype = sz
    lib.cuzfp_hip_stream_bytes.argtypes = [i, u, u, u, u]
    lib.cuzfp_hip_maximum_size.restype = sz
    lib.cuzfp_hip_maximum_size.argtypes = [i, u, u, u, u]
    lib.cuzfp_hip_encode.restype = i
    lib.cuzfp_hip_encode.argtypes = [vp, i, u, u, u, ll, ll, ll, u, vp, sz, ctypes.POINTER(sz), vp]
    lib.cuzfp_hip_decode.restype = i
    lib.cuzfp_hip_decode.argtypes = [vp, sz, i, u, u, u, ll, ll, ll, u, vp, vp]
    lib.cuzfp_hip_decode_region.restype = i
    lib.cuzfp_hip_decode_region.argtypes = [vp, sz, i, u, u, u, u, u, u, u, u, u, u, ll, ll, ll, vp, vp]
    lib.cuzfp_hip_decode_region_prefix.restype = i
    lib.cuzfp_hip_decode_region_prefix.argtypes = [vp, sz, i, u, u, u, u, u, u, u, u, u, u, u, ll, ll, ll, vp, vp]
    lib.cuzfp_hip_truncate.restype = i
    lib.cuzfp_hip_truncate.argtypes = [vp, sz, i, u, u, u, u, u, vp, sz, ctypes.POINTER(sz), vp]
    lib.cuzfp_hip_encode_region.restype = i
    lib.cuzfp_hip_encode_region.argtypes = [vp, i, u, u, u, u, u, u, u, u, u, u, ll, ll, ll, vp, sz, vp]
    lib.cuzfp_hip_accuracy_to_minexp.restype = i
    lib.cuzfp_hip_accuracy_to_minexp.argtypes = [ctypes.c_double]
    lib.cuzfp_hip_variable_maximum_size.restype = sz
    lib.cuzfp_hip_variable_maximum_size.argtypes = [i, u, u, u, u]
    lib.cuzfp_hip_variable_workspace_bytes.restype = sz
    lib.cuzfp_hip_variable_workspace_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_encode_variable.restype = i
    lib.cuzfp_hip_encode_variable.argtypes = [vp, i, u, u, u, ll, ll, ll, u, i, vp, sz, vp, vp, vp, sz, vp]
    lib.cuzfp_hip_decode_variable.restype = i
    lib.cuzfp_hip_decode_variable.argtypes = [vp, sz, vp, i, u, u, u, ll, ll, ll, vp, vp, sz, vp]
    lib.cuzfp_hip_variable_index_bytes.restype = sz
    lib.cuzfp_hip_variable_index_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_variable_index.restype = i
    lib.cuzfp_hip_variable_index.argtypes = [vp, i, u, u, u, vp, sz, vp, sz, vp]
    lib.cuzfp_hip_decode_region_variable.restype = i
    lib.cuzfp_hip_decode_region_variable.argtypes = [vp, sz, vp, vp, sz, i, u, u, u, u, u, u, u, u, u, ll, ll, ll,
                                                     vp, vp]
    lib.cuzfp_hip_truncate_variable_workspace_bytes.restype = sz
    lib.cuzfp_hip_decode_region_variable_coarse.restype = i
    lib.cuzfp_hip_decode_region_variable_coarse.argtypes = [vp, sz, vp, vp, sz, i, u, u, u, u, i, u, u, u, u, u, u,
                                                            ll, ll, ll, vp, vp]
    lib.cuzfp_hip_truncate_variable_workspace_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_truncate_variable.restype = i
    lib.cuzfp_hip_truncate_variable.argtypes = [vp, sz, vp, i, u, u, u, u, i, u, i, vp, sz, vp, vp, vp, sz, vp]
    lib.cuzfp_hip_encode_region_variable_workspace_bytes.restype = sz
    lib.cuzfp_hip_encode_region_variable_workspace_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_encode_region_variable_maximum_size.restype = sz
    lib.cuzfp_hip_encode_region_variable_maximum_size.argtypes = [i, u, u, u, sz, u, u, u, u, u, u, u]
    lib.cuzfp_hip_encode_region_variable.restype = i
    lib.cuzfp_hip_encode_region_variable.argtypes = [vp, ll, ll, ll, i, u, u, u, u, i, u, u, u, u, u, u,
                                                     vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp]
    lib.cuzfp_hip_extract_region_variable_workspace_bytes.restype = sz
    lib.cuzfp_hip_extract_region_variable_workspace_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_extract_region_variable_maximum_size.restype = sz
    lib.cuzfp_hip_extract_region_variable_maximum_size.argtypes = [i, u, u, u, sz, u, u, u, u, u, u]
    lib.cuzfp_hip_extract_region_variable.restype = i
    lib.cuzfp_hip_extract_region_variable.argtypes = [vp, sz, vp, vp, sz, i, u, u, u, u, u, u, u, u, u,
                                                      vp, sz, vp, vp, sz, vp, vp, sz, vp]
    lib.cuzfp_hip_insert_region_variable_workspace_bytes.restype = sz
    lib.cuzfp_hip_insert_region_variable_workspace_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_insert_region_variable_maximum_size.restype = sz
    lib.cuzfp_hip_insert_region_variable_maximum_size.argtypes = [sz, sz]
    lib.cuzfp_hip_insert_region_variable.restype = i
    lib.cuzfp_hip_insert_region_variable.argtypes = [vp, sz, vp, vp, sz, vp, sz, vp, vp, sz, i, u, u, u,
                                                     u, u, u, u, u, u, vp, sz, vp, vp, vp, vp, sz, vp]
    lib.cuzfp_hip_join_variable_workspace_bytes.restype = sz
    lib.cuzfp_hip_join_variable_workspace_bytes.argtypes = [i, u, u, u]
    lib.cuzfp_hip_join_variable_maximum_size.restype = sz
    lib.cuzfp_hip_join_variable_maximum_size.argtypes = [ctypes.POINTER(VariablePart), u]
    lib.cuzfp_hip_join_variable.restype = i
    lib.cuzfp_hip_join_variable.argtypes = [ctypes.POINTER(VariablePart), u, i, u, u, u, vp, sz, vp, vp, vp, vp, sz,
                                            vp]
    lib.cuzfp_hip_compress_host.restype = i
    lib.cuzfp_hip_compress_host.argtypes = [vp, i, u, u, u, u, vp, sz, ctypes.POINTER(sz), i]
    lib.cuzfp_hip_decompress_host.restype = i
    lib.cuzfp_hip_decompress_host.argtypes = [vp, sz, i, u, u, u, u, vp, i]
    lib.cuzfp_hip_copy.restype = i
    lib.cuzfp_hip_copy.argtypes = [vp, vp, sz, vp]
    lib.cuzfp_hip_release_host_cache.restype = i
    lib.cuzfp_hip_release_host_cache.argtypes = [i]
    _lib = lib
    return lib


def _check(where: str, rc: int) -> None:
    if rc != 0:
        raise CodecError(where, rc, library().cuzfp_hip_last_hip_error())


def _extents(shape) -> tuple[int, int, int]:
    """(slowest..fastest) shape -> zfp (nx, ny, nz); 0 marks an unused dimension."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 1:
        return shape[0], 0, 0
    if len(shape) == 2:
        return shape[1], shape[0], 0
    if len(shape) == 3:
        return shape[2], shape[1], shape[0]
    raise ValueError("zfp arrays are 1D, 2D or 3D")


def type_code(dtype) -> int:
    """zfp_type code of a numpy or torch dtype."""
    if hasattr(dtype, "is_floating_point"):  # torch.dtype
        import torch
        dtype = {torch.float32: np.float32, torch.float64: np.float64,
                 torch.int32: np.int32, torch.int64: np.int64}.get(dtype)
        if dtype is None:
            raise TypeError("cuzfp_amd supports float32, float64, int32 and int64")
    return _NP_TYPES[np.dtype(dtype)]


def rate_to_maxbits(rate: float, dtype, dims: int, wra: bool = False) -> int:
    """Bits per block for `rate` bits/value (zfp_stream_set_rate; wra rounds to 64)."""
    return int(library().cuzfp_hip_rate_to_maxbits(float(rate), type_code(dtype), dims, int(wra)))


def stream_bytes(shape, dtype, maxbits: int) -> int:
    nx, ny, nz = _extents(shape)
    n = library().cuzfp_hip_stream_bytes(type_code(dtype), nx, ny, nz, maxbits)
    if n == 0:
        raise CodecError("stream_bytes", 1)
    return int(n)


def maximum_size(shape, dtype, maxbits: int) -> int:
    nx, ny, nz = _extents(shape)
    return int(library().cuzfp_hip_maximum_size(type_code(dtype), nx, ny, nz, maxbits))


def _stream_handle(stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _strides(x):
    """Element strides (sx, sy, sz) of a torch tensor in zfp order."""
    st = list(x.stride())[::-1] + [0, 0]
    return st[0], st[1] if x.dim() > 1 else 0, st[2] if x.dim() > 2 else 0


def _broadcast(x) -> bool:
    """True for a view with a zero stride on an axis of extent > 1 (expand /
    broadcast): the C-ABI reads a zero stride as "contiguous default", so such
    a view must not be passed through as it is."""
    return any(st == 0 and n > 1 for st, n in zip(x.stride(), x.shape))


def _check_host_out(out: np.ndarray, shape, dtype, what: str) -> None:
    if not isinstance(out, np.ndarray) or not out.flags.c_contiguous:
        raise ValueError(f"{what}: out must be a C-contiguous numpy array")
    if out.dtype != np.dtype(dtype):
        raise ValueError(f"{what}: out has dtype {out.dtype}, expected {np.dtype(dtype)}")
    if shape is not None and tuple(out.shape) != tuple(int(s) for s in shape):
        raise ValueError(f"{what}: out has shape {out.shape}, expected {tuple(shape)}")


def _materialise(x, stream):
    """A broadcast view (a zero stride means "contiguous" to the C-ABI) made
    contiguous on the launch stream; any other tensor as it is."""
    import torch
    if _broadcast(x):
        # materialise a broadcast view (a zero stride means "contiguous" to the
        # C-ABI) on the launch stream, after the work already queued on torch's
        # current stream.  The copy is allocated on that stream, so the kernel
        # that reads it is ordered before any reuse; the broadcast source was
        # allocated on the current stream and is read on s, so it is recorded
        # there (the caching allocator then waits for s before reusing it).
        cur = torch.cuda.current_stream(x.device)
        s = cur if stream is None else stream
        s.wait_stream(cur)
        src = x
        with torch.cuda.stream(s):
            x = src.contiguous()
        if s != cur:
            src.record_stream(s)
    return x


def encode(x, maxbits: int, out=None, stream=None):
    """Compress a CUDA tensor; returns the stream as an int64 tensor of 64-bit words.

    Bit-exact with zfp 0.5.0 fixed-rate mode (``zfp_compress`` with
    minbits = maxbits).  Asynchronous on `stream` (default: torch's current).
    """
    import torch
    if not x.is_cuda:
        raise ValueError("encode: expects a device tensor (use compress_host for host arrays)")
    x = _materialise(x, stream)
    t = type_code(x.dtype)
    nx, ny, nz = _extents(x.shape)
    nbytes = stream_bytes(x.shape, x.dtype, maxbits)
    if out is None:
        out = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
    sx, sy, sz = _strides(x)
    got = ctypes.c_size_t(0)
    rc = library().cuzfp_hip_encode(x.data_ptr(), t, nx, ny, nz, sx, sy, sz, maxbits,
                                    out.data_ptr(), out.numel() * out.element_size(),
                                    ctypes.byref(got), _stream_handle(stream))
    _check("encode", rc)
    return out


def decode(words, shape, dtype, maxbits: int, out=None, stream=None, prefix_bits=None):
    """Decompress a device stream (int64 words) into a new (or given) CUDA tensor.

    `prefix_bits` (<= maxbits) decodes only the first prefix_bits of each block,
    which sit `maxbits` apart: the array the stream truncated to prefix_bits
    holds (see `truncate`), through `decode_region` with the whole array as
    the box.  None decodes every block in full."""
    import torch
    if prefix_bits is not None:
        shape = tuple(int(s) for s in (shape if out is None else out.shape))
        return decode_region(words, shape, dtype, maxbits, (0,) * len(shape), shape, out=out,
                             stream=stream, prefix_bits=prefix_bits)
    if not words.is_cuda:
        raise ValueError("decode: expects a device stream")
    if out is None:
        out = torch.empty(tuple(shape), dtype=dtype, device=words.device)
    elif _broadcast(out):
        raise ValueError("decode: out is a broadcast view (zero stride); its elements alias each other")
    t = type_code(out.dtype)
    nx, ny, nz = _extents(out.shape)
    sx, sy, sz = _strides(out)
    rc = library().cuzfp_hip_decode(words.data_ptr(), words.numel() * words.element_size(), t,
                                    nx, ny, nz, sx, sy, sz, maxbits, out.data_ptr(),
                                    _stream_handle(stream))
    _check("decode", rc)
    return out


def decode_region(words, shape, dtype, maxbits: int, origin, extent, out=None, stream=None,
                  prefix_bits=None):
    """Decompress the box ``origin .. origin + extent`` (slowest first, like
    `shape`) of the array a device stream holds into a new (or given, possibly
    strided) CUDA tensor of shape `extent`.  Only the box's blocks are read and
    decoded: fixed rate puts block b at bits [b * maxbits, (b + 1) * maxbits).

    `prefix_bits` (<= maxbits) decodes each block from its first prefix_bits
    alone: bit for bit what `decode_region` at prefix_bits gives on
    ``truncate(words, ..., prefix_bits)``, without making that stream."""
    import torch
    shape = tuple(int(s) for s in shape)
    origin = tuple(int(o) for o in origin)
    extent = tuple(int(e) for e in extent)
    nx, ny, nz = _extents(shape)
    if len(origin) != len(shape) or len(extent) != len(shape):
        raise ValueError(f"decode_region: origin {origin} and extent {extent} must have "
                         f"the rank of shape {shape}")
    if any(o < 0 for o in origin) or any(e <= 0 for e in extent):
        raise ValueError("decode_region: origin must be non-negative and extent positive")
    if prefix_bits is not None and prefix_bits > maxbits:
        raise ValueError(f"decode_region: prefix_bits {prefix_bits} exceeds maxbits {maxbits}; a block holds "
                         "no more than maxbits bits")
    if not words.is_cuda:
        raise ValueError("decode_region: expects a device stream")
    if out is None:
        out = torch.empty(extent, dtype=dtype, device=words.device)
    elif _broadcast(out):
        raise ValueError("decode_region: out is a broadcast view (zero stride); its elements alias each other")
    elif tuple(out.shape) != extent:
        raise ValueError(f"decode_region: out has shape {tuple(out.shape)}, expected {extent}")
    ox, oy, oz = _extents(origin)
    ex, ey, ez = _extents(extent)
    sx, sy, sz = _strides(out)
    if prefix_bits is None:
        rc = library().cuzfp_hip_decode_region(words.data_ptr(), words.numel() * words.element_size(),
                                               type_code(out.dtype), nx, ny, nz, maxbits,
                                               ox, oy, oz, ex, ey, ez, sx, sy, sz, out.data_ptr(),
                                               _stream_handle(stream))
    else:
        rc = library().cuzfp_hip_decode_region_prefix(words.data_ptr(), words.numel() * words.element_size(),
                                                      type_code(out.dtype), nx, ny, nz, maxbits, prefix_bits,
                                                      ox, oy, oz, ex, ey, ez, sx, sy, sz, out.data_ptr(),
                                                      _stream_handle(stream))
    _check("decode_region", rc)
    return out


def truncate(words, shape, dtype, maxbits: int, new_maxbits: int, out=None, stream=None):
    """The stream of the same array at `new_maxbits` <= `maxbits` bits a block,
    cut from the device stream `words` (int64 words) at `maxbits` without
    decoding: every block's first new_maxbits bits, packed new_maxbits apart.

    zfp's coder is embedded, so the result is byte for byte what `encode` of the
    original array gives at new_maxbits.  Returns an int64 word tensor
    (allocated when `out` is None; `out` may be longer than the stream, its
    words past the stream are left alone, and it must not overlap `words`).
    Widening is not offered: blocks zero-padded to a higher rate are not the
    same stream as encoding at that rate, and do not decode to the same values."""
    import torch
    if new_maxbits > maxbits:
        raise ValueError(f"truncate: new_maxbits {new_maxbits} exceeds maxbits {maxbits}; widening is not "
                         "supported, zero-padded blocks are not the same stream as encoding at the higher rate")
    if not words.is_cuda:
        raise ValueError("truncate: expects a device stream")
    nx, ny, nz = _extents(shape)
    nbytes = stream_bytes(shape, dtype, new_maxbits)
    if out is None:
        out = torch.empty(nbytes // 8, dtype=torch.int64, device=words.device)
    elif not out.is_cuda or not out.is_contiguous():
        raise ValueError("truncate: out must be a contiguous device tensor")
    got = ctypes.c_size_t(0)
    rc = library().cuzfp_hip_truncate(words.data_ptr(), words.numel() * words.element_size(), type_code(dtype),
                                      nx, ny, nz, maxbits, new_maxbits, out.data_ptr(),
                                      out.numel() * out.element_size(), ctypes.byref(got),
                                      _stream_handle(stream))
    _check("truncate", rc)
    return out


def encode_region(x, words, shape, maxbits: int, origin, stream=None):
    """Write the box `x` (a device tensor whose shape is the box's extent) at
    `origin` (slowest first, like `shape`) into `words`, the device stream of
    an array of `shape` at `maxbits`, in place; returns `words`.

    Only the box's blocks are re-coded; every other bit of the stream stays as
    it was.  A block the box covers (all its elements inside the array lie in
    the box) is coded from `x` alone.  A partially covered block is a
    read-modify-write: it is decoded, the box's elements are replaced and the
    block is encoded again, so its other elements may change within the rate's
    error.  `x` may be strided; a broadcast view (fill the box with a constant)
    is materialised on the launch stream as `encode` does.  Calls whose boxes
    share a block must be ordered by the caller."""
    shape = tuple(int(s) for s in shape)
    origin = tuple(int(o) for o in origin)
    extent = tuple(int(e) for e in getattr(x, "shape", ()))
    nx, ny, nz = _extents(shape)
    if len(origin) != len(shape) or len(extent) != len(shape):
        raise ValueError(f"encode_region: origin {origin} and the box's shape {extent} must have "
                         f"the rank of shape {shape}")
    if any(o < 0 for o in origin) or any(e <= 0 for e in extent):
        raise ValueError("encode_region: origin must be non-negative and the box not empty")
    if any(o + e > n for o, e, n in zip(origin, extent, shape)):
        raise ValueError(f"encode_region: the box {origin} + {extent} leaves the array {shape}")
    if not x.is_cuda or not words.is_cuda:
        raise ValueError("encode_region: expects a device box and a device stream")
    x = _materialise(x, stream)
    ox, oy, oz = _extents(origin)
    ex, ey, ez = _extents(extent)
    sx, sy, sz = _strides(x)
    rc = library().cuzfp_hip_encode_region(x.data_ptr(), type_code(x.dtype), nx, ny, nz, maxbits,
                                           ox, oy, oz, ex, ey, ez, sx, sy, sz, words.data_ptr(),
                                           words.numel() * words.element_size(),
                                           _stream_handle(stream))
    _check("encode_region", rc)
    return words


def accuracy_to_minexp(tolerance: float) -> int:
    """minexp of fixed-accuracy mode at `tolerance` (zfp_stream_set_accuracy:
    floor(log2 tolerance); -1074 for a tolerance <= 0)."""
    return int(library().cuzfp_hip_accuracy_to_minexp(float(tolerance)))


def variable_maximum_size(shape, dtype, maxprec: int) -> int:
    """Worst-case stream bytes of a variable-rate mode with `maxprec` planes a
    block (the precision of fixed-precision mode; the type's 32 / 64 for fixed
    accuracy): zfp_stream_maximum_size, header allowance included."""
    nx, ny, nz = _extents(shape)
    t = type_code(dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError("variable_maximum_size", 2)
    n = library().cuzfp_hip_variable_maximum_size(t, nx, ny, nz, int(maxprec))
    if n == 0:
        raise CodecError("variable_maximum_size", 1)
    return int(n)


def _variable_workspace(t, nx, ny, nz, device, stream, where):
    """The scratch of the variable-rate calls, allocated on the launch stream."""
    import torch
    n = library().cuzfp_hip_variable_workspace_bytes(t, nx, ny, nz)
    if n == 0:
        raise CodecError(where, 2 if t in (TYPE_INT32, TYPE_INT64) else 1)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        return torch.empty((n + 7) // 8, dtype=torch.int64, device=device), n


def encode_variable(x, precision=None, tolerance=None, out=None, stream=None):
    """Compress a CUDA float tensor in one of zfp's variable-rate modes; returns
    ``(words, lengths, nbits)``.

    Exactly one of `precision` (fixed precision: that many bit planes a block,
    1 .. 32 for float32, 1 .. 64 for float64) and `tolerance` (fixed accuracy:
    no value off by more than `tolerance`, as far as the type's precision
    allows; 0 codes every plane above the smallest exponent) must be given.

    The stream is byte-identical to CPU zfp 0.5.0's ``zfp_compress`` after
    ``zfp_stream_set_precision`` / ``zfp_stream_set_accuracy`` (no header).
    `words` is a view of the stream's ceil(nbits / 64) 64-bit words in `out`
    (allocated at the worst-case size, `variable_maximum_size`, when None; a
    shorter `out` is never written past its end, but then holds no valid
    stream if nbits exceeds it -- check nbits).  `lengths` is an int16 tensor
    holding the raw uint16 bit length of every block in raster order: the
    index `decode_variable` needs.  `nbits` is the stream's length in bits.

    The launches are asynchronous on `stream` (default: torch's current), but
    the bit count depends on the data: this function synchronises once with
    that stream to read it back."""
    import torch
    if (precision is None) == (tolerance is None):
        raise ValueError("encode_variable: give exactly one of precision and tolerance")
    if not x.is_cuda:
        raise ValueError("encode_variable: expects a device tensor")
    t = type_code(x.dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError("encode_variable", 2)
    x = _materialise(x, stream)
    type_prec = 32 if t == TYPE_FLOAT else 64
    if precision is not None:
        maxprec, minexp = int(precision), -1074
    else:
        maxprec, minexp = type_prec, accuracy_to_minexp(tolerance)
    if not 1 <= maxprec <= type_prec:
        raise CodecError("encode_variable", 1)
    nx, ny, nz = _extents(x.shape)
    nblocks = 1
    for s in x.shape:
        nblocks *= (int(s) + 3) // 4
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    ws, ws_bytes = _variable_workspace(t, nx, ny, nz, x.device, stream, "encode_variable")
    with torch.cuda.stream(s):
        if out is None:
            out = torch.empty(variable_maximum_size(x.shape, x.dtype, maxprec) // 8, dtype=torch.int64,
                              device=x.device)
        lengths = torch.empty(nblocks, dtype=torch.int16, device=x.device)
        total = torch.empty(1, dtype=torch.int64, device=x.device)
    if not out.is_cuda or not out.is_contiguous() or out.element_size() != 8:
        raise ValueError("encode_variable: out must be a contiguous device tensor of 64-bit words")
    sx, sy, sz = _strides(x)
    rc = library().cuzfp_hip_encode_variable(x.data_ptr(), t, nx, ny, nz, sx, sy, sz, maxprec, minexp,
                                             out.data_ptr(), out.numel() * 8, lengths.data_ptr(),
                                             total.data_ptr(), ws.data_ptr(), ws_bytes, _stream_handle(stream))
    _check("encode_variable", rc)
    with torch.cuda.stream(s):
        nbits = int(total.item())  # the one synchronisation: the count is data dependent
    return out[: min((nbits + 63) // 64, out.numel())], lengths, nbits


def decode_variable(words, lengths, shape, dtype, out=None, stream=None, index=None, precision=None,
                    tolerance=None):
    """Decompress a variable-rate device stream (`words`, 64-bit words) with its
    block index `lengths` (int16 tensor of raw uint16 bits, from
    `encode_variable`) into a new (or given, possibly strided) CUDA tensor:
    bit for bit what ``zfp_decompress`` returns in the mode that wrote the
    stream.  The decoder needs no knowledge of the mode.  Asynchronous on
    `stream`.  An index that does not belong to the stream cannot make the
    decoder read outside `words`; the affected blocks decode to unspecified
    values.

    `index` (from `variable_index`) decodes through `decode_region_variable`
    with the whole array as the box: one launch, no scan of the lengths and no
    workspace.  None scans the lengths on every call.

    One of `precision` and `tolerance` decodes the array at that coarser target
    mode straight from the stream, never finer than the stream holds it: the
    semantics of `decode_region_variable`'s keywords, whose path this takes
    with the whole array as the box.  With `index` that is one launch; with
    ``index=None`` the index is built for the call by `variable_index` (a scan
    of the lengths and its scratch) first.  `truncate_variable` gives the
    coarser *stream*."""
    import torch
    if precision is not None or tolerance is not None:
        shape = tuple(int(s) for s in (shape if out is None else out.shape))
        _coarse_target("decode_variable", dtype if out is None else out.dtype, precision, tolerance)
        if index is None:
            index = variable_index(lengths, shape, dtype if out is None else out.dtype, stream=stream)
        return decode_region_variable(words, lengths, index, shape, dtype, (0,) * len(shape), shape, out=out,
                                      stream=stream, precision=precision, tolerance=tolerance)
    if index is not None:
        shape = tuple(int(s) for s in (shape if out is None else out.shape))
        return decode_region_variable(words, lengths, index, shape, dtype, (0,) * len(shape), shape, out=out,
                                      stream=stream)
    if not words.is_cuda or not lengths.is_cuda:
        raise ValueError("decode_variable: expects a device stream and a device index")
    if lengths.element_size() != 2 or not lengths.is_contiguous() or not words.is_contiguous():
        raise ValueError("decode_variable: lengths must be a contiguous 16-bit tensor, words contiguous")
    if out is None:
        out = torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=words.device)
    elif _broadcast(out):
        raise ValueError("decode_variable: out is a broadcast view (zero stride); its elements alias each other")
    t = type_code(out.dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError("decode_variable", 2)
    nx, ny, nz = _extents(out.shape)
    nblocks = 1
    for s in out.shape:
        nblocks *= (int(s) + 3) // 4
    if lengths.numel() != nblocks:
        raise ValueError(f"decode_variable: lengths has {lengths.numel()} entries, the array has {nblocks} blocks")
    ws, ws_bytes = _variable_workspace(t, nx, ny, nz, words.device, stream, "decode_variable")
    sx, sy, sz = _strides(out)
    rc = library().cuzfp_hip_decode_variable(words.data_ptr(), words.numel() * words.element_size(),
                                             lengths.data_ptr(), t, nx, ny, nz, sx, sy, sz, out.data_ptr(),
                                             ws.data_ptr(), ws_bytes, _stream_handle(stream))
    _check("decode_variable", rc)
    return out


def _block_count(shape) -> int:
    n = 1
    for s in shape:
        n *= (int(s) + 3) // 4
    return n


def variable_index(lengths, shape, dtype, out=None, stream=None):
    """The offset index of a variable-rate stream, from its `lengths` (the
    int16 tensor of `encode_variable`): an int64 tensor of T + 1 entries, T =
    ceil(nblocks / 64), entry t the bit offset of block 64 t and entry T the
    stream's bit count.  It is a sixteenth of `lengths` and is kept with the
    stream: `decode_region_variable` and ``decode_variable(index=)`` find any
    block through it without scanning the lengths.  `lengths` may start at any
    element of a larger tensor (2-byte alignment is enough).  Asynchronous on
    `stream`; the scan's scratch is allocated on that stream."""
    import torch
    if not lengths.is_cuda:
        raise ValueError("variable_index: expects a device index")
    if lengths.element_size() != 2 or not lengths.is_contiguous():
        raise ValueError("variable_index: lengths must be a contiguous 16-bit tensor")
    shape = tuple(int(s) for s in shape)
    nx, ny, nz = _extents(shape)
    t = type_code(dtype)
    n = library().cuzfp_hip_variable_index_bytes(t, nx, ny, nz)
    if n == 0:
        raise CodecError("variable_index", 2 if t in (TYPE_INT32, TYPE_INT64) else 1)
    if lengths.numel() != _block_count(shape):
        raise ValueError(f"variable_index: lengths has {lengths.numel()} entries, the array has "
                         f"{_block_count(shape)} blocks")
    ws, ws_bytes = _variable_workspace(t, nx, ny, nz, lengths.device, stream, "variable_index")
    if out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(lengths.device)):
            out = torch.empty(n // 8, dtype=torch.int64, device=lengths.device)
    elif not out.is_cuda or not out.is_contiguous() or out.element_size() != 8 or out.numel() < n // 8:
        raise ValueError(f"variable_index: out must be a contiguous device tensor of at least {n // 8} 64-bit words")
    rc = library().cuzfp_hip_variable_index(lengths.data_ptr(), t, nx, ny, nz, out.data_ptr(), out.numel() * 8,
                                            ws.data_ptr(), ws_bytes, _stream_handle(stream))
    _check("variable_index", rc)
    return out[: n // 8]


def _coarse_target(where, dtype, precision, tolerance):
    """(maxprec, minexp) of the target of a coarse decode: exactly one of
    `precision` and `tolerance`, checked before anything touches a device."""
    if precision is not None and tolerance is not None:
        raise ValueError(f"{where}: give at most one of precision and tolerance")
    t = type_code(dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError(where, 2)
    return _variable_mode(where, 32 if t == TYPE_FLOAT else 64, precision, tolerance, ("precision", "tolerance"))


def decode_region_variable(words, lengths, index, shape, dtype, origin, extent, out=None, stream=None,
                           precision=None, tolerance=None):
    """Decompress the box ``origin .. origin + extent`` (slowest first, like
    `shape`) of the array a variable-rate device stream holds into a new (or
    given, possibly strided) CUDA tensor of shape `extent`: bit for bit the box
    of `decode_variable`'s array.  `index` is `variable_index` of `lengths`.

    One kernel launch that reads only the box's blocks: no scan, no scratch, no
    allocation when `out` is given, no synchronisation (it can be captured into
    a graph).  Neither `index` nor `lengths` can make the decoder read outside
    `words` or write outside the box; blocks whose entries are wrong decode to
    unspecified values.

    One of `precision` (bit planes a block, 1 .. 32 / 64) and `tolerance` names
    a target mode coarser than the one that wrote the stream, and the box is
    decoded at it straight from the fine stream, still in one launch with no
    scratch: every lane walks its block's bit-plane code to the block's length
    at the target and decodes that prefix, or zeros where the target codes no
    plane of the block.  With a mode as the pair (maxprec, minexp) --
    precision p: (p, -1074); tolerance t: (the type's 32 / 64,
    accuracy_to_minexp(t)) -- and a target that coarsens the stream's mode,
    the result is bit for bit `decode_variable` of `truncate_variable`'s
    output, which is what CPU zfp 0.5.0 decodes from its own stream at the
    target mode.  The call does not take the mode that wrote the stream and
    refuses no target: a block never decodes finer than the stream holds it,
    so the result is the array at (the smaller maxprec, the larger minexp),
    and a target at or above the stream's own mode gives the plain decode.
    Widening is not offered in the sense that nothing finer comes out.
    `truncate_variable` is the way to get the coarser *stream*.  Both None is
    the plain decode; both given is a ValueError."""
    import torch
    target = None
    if precision is not None or tolerance is not None:
        target = _coarse_target("decode_region_variable", dtype if out is None else out.dtype, precision, tolerance)
    shape = tuple(int(s) for s in shape)
    origin = tuple(int(o) for o in origin)
    extent = tuple(int(e) for e in extent)
    nx, ny, nz = _extents(shape)
    if len(origin) != len(shape) or len(extent) != len(shape):
        raise ValueError(f"decode_region_variable: origin {origin} and extent {extent} must have "
                         f"the rank of shape {shape}")
    if any(o < 0 for o in origin) or any(e <= 0 for e in extent):
        raise ValueError("decode_region_variable: origin must be non-negative and extent positive")
    if not words.is_cuda or not lengths.is_cuda or not index.is_cuda:
        raise ValueError("decode_region_variable: expects a device stream and device indices")
    if lengths.element_size() != 2 or not lengths.is_contiguous() or not words.is_contiguous():
        raise ValueError("decode_region_variable: lengths must be a contiguous 16-bit tensor, words contiguous")
    if index.element_size() != 8 or not index.is_contiguous():
        raise ValueError("decode_region_variable: index must be a contiguous tensor of 64-bit words")
    if out is None:
        out = torch.empty(extent, dtype=dtype, device=words.device)
    elif _broadcast(out):
        raise ValueError("decode_region_variable: out is a broadcast view (zero stride); its elements alias "
                         "each other")
    elif tuple(out.shape) != extent:
        raise ValueError(f"decode_region_variable: out has shape {tuple(out.shape)}, expected {extent}")
    t = type_code(out.dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError("decode_region_variable", 2)
    if lengths.numel() != _block_count(shape):
        raise ValueError(f"decode_region_variable: lengths has {lengths.numel()} entries, the array has "
                         f"{_block_count(shape)} blocks")
    ox, oy, oz = _extents(origin)
    ex, ey, ez = _extents(extent)
    sx, sy, sz = _strides(out)
    if target is not None:
        rc = library().cuzfp_hip_decode_region_variable_coarse(
            words.data_ptr(), words.numel() * words.element_size(), lengths.data_ptr(), index.data_ptr(),
            index.numel() * index.element_size(), t, nx, ny, nz, target[0], target[1], ox, oy, oz, ex, ey, ez,
            sx, sy, sz, out.data_ptr(), _stream_handle(stream))
        _check("decode_region_variable", rc)
        return out
    rc = library().cuzfp_hip_decode_region_variable(words.data_ptr(), words.numel() * words.element_size(),
                                                    lengths.data_ptr(), index.data_ptr(),
                                                    index.numel() * index.element_size(), t, nx, ny, nz,
                                                    ox, oy, oz, ex, ey, ez, sx, sy, sz, out.data_ptr(),
                                                    _stream_handle(stream))
    _check("decode_region_variable", rc)
    return out


def _variable_mode(where, type_prec, precision, tolerance, names):
    """(maxprec, minexp) of exactly one of a precision and a tolerance."""
    if (precision is None) == (tolerance is None):
        raise ValueError(f"{where}: give exactly one of {names[0]} and {names[1]}")
    if precision is not None:
        if int(precision) != precision:
            raise ValueError(f"{where}: {names[0]} {precision!r} is not a whole number of bit planes")
        maxprec, minexp = int(precision), -1074
    else:
        maxprec, minexp = type_prec, accuracy_to_minexp(tolerance)
    if not 1 <= maxprec <= type_prec:
        raise CodecError(where, 1)
    return maxprec, minexp


def truncate_variable(words, lengths, shape, dtype, *, from_precision=None, from_tolerance=None,
                      precision=None, tolerance=None, out=None, stream=None, size_only=False):
    """The stream of the same array in a coarser variable-rate mode, cut from
    the device stream `words` with its index `lengths` (both from
    `encode_variable`) without decoding; returns ``(words, lengths, nbits)``
    like `encode_variable`.

    Exactly one of `from_precision` and `from_tolerance` names the mode that
    wrote `words`, exactly one of `precision` and `tolerance` the new mode.
    With a mode as the pair (maxprec, minexp) -- precision p: (p, -1074);
    tolerance t: (the type's 32 / 64, accuracy_to_minexp(t)) -- the new mode
    must have maxprec no higher and minexp no lower than the source's, so a
    full-precision stream can be cut to any precision or tolerance.

    zfp's coder is embedded, so every new block is a prefix of the old one --
    or the single bit 0 where the new mode codes no plane of it -- and the
    result is byte for byte what `encode_variable` of the original array gives
    in the new mode: it feeds `decode_variable`, `variable_index` and
    `decode_region_variable` unchanged.  Widening is not offered: the planes a
    finer mode codes are not in the stream.

    `out` (64-bit words, not overlapping `words`) is allocated at
    `variable_maximum_size` of the new maxprec when None; a shorter `out` is
    never written past its end, but then holds no valid stream if nbits exceeds
    it.  ``size_only=True`` computes the new lengths and the bit count alone and
    returns ``(None, lengths, nbits)``.  An index that does not belong to the
    stream cannot make the call read outside `words` and `lengths` or write
    outside its outputs.  Asynchronous on `stream` except for one
    synchronisation to read the count, as `encode_variable`."""
    import torch
    t = type_code(dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError("truncate_variable", 2)
    type_prec = 32 if t == TYPE_FLOAT else 64
    maxprec, minexp = _variable_mode("truncate_variable", type_prec, from_precision, from_tolerance,
                                     ("from_precision", "from_tolerance"))
    new_maxprec, new_minexp = _variable_mode("truncate_variable", type_prec, precision, tolerance,
                                             ("precision", "tolerance"))
    if new_maxprec > maxprec or new_minexp < minexp:
        raise ValueError(f"truncate_variable: the mode (maxprec {new_maxprec}, minexp {new_minexp}) is finer than the "
                         f"stream's (maxprec {maxprec}, minexp {minexp}); widening is not supported, the planes a "
                         "finer mode codes are not in the stream")
    if size_only and out is not None:
        raise ValueError("truncate_variable: size_only writes no stream; give no out")
    if not words.is_cuda or not lengths.is_cuda:
        raise ValueError("truncate_variable: expects a device stream and a device index")
    if lengths.element_size() != 2 or not lengths.is_contiguous() or not words.is_contiguous():
        raise ValueError("truncate_variable: lengths must be a contiguous 16-bit tensor, words contiguous")
    shape = tuple(int(s) for s in shape)
    nx, ny, nz = _extents(shape)
    nblocks = _block_count(shape)
    if lengths.numel() != nblocks:
        raise ValueError(f"truncate_variable: lengths has {lengths.numel()} entries, the array has {nblocks} blocks")
    n = library().cuzfp_hip_truncate_variable_workspace_bytes(t, nx, ny, nz)
    if n == 0:
        raise CodecError("truncate_variable", 1)
    s = stream if stream is not None else torch.cuda.current_stream(words.device)
    with torch.cuda.stream(s):
        ws = torch.empty((n + 7) // 8, dtype=torch.int64, device=words.device)
        if out is None and not size_only:
            out = torch.empty(variable_maximum_size(shape, dtype, new_maxprec) // 8, dtype=torch.int64,
                              device=words.device)
        new_lengths = torch.empty(nblocks, dtype=torch.int16, device=words.device)
        total = torch.empty(1, dtype=torch.int64, device=words.device)
    if out is not None and (not out.is_cuda or not out.is_contiguous() or out.element_size() != 8):
        raise ValueError("truncate_variable: out must be a contiguous device tensor of 64-bit words")
    rc = library().cuzfp_hip_truncate_variable(words.data_ptr(), words.numel() * words.element_size(),
                                               lengths.data_ptr(), t, nx, ny, nz, maxprec, minexp, new_maxprec,
                                               new_minexp, out.data_ptr() if out is not None else None,
                                               out.numel() * 8 if out is not None else 0, new_lengths.data_ptr(),
                                               total.data_ptr(), ws.data_ptr(), n, _stream_handle(stream))
    _check("truncate_variable", rc)
    with torch.cuda.stream(s):
        nbits = int(total.item())  # the one synchronisation: the count is data dependent
    if out is None:
        return None, new_lengths, nbits
    return out[: min((nbits + 63) // 64, out.numel())], new_lengths, nbits


def encode_region_variable(x, words, lengths, index, shape, origin, *, precision=None, tolerance=None,
                           out=None, stream=None, with_index=False):
    """Write the box `x` (a device float tensor whose shape is the box's extent)
    at `origin` (slowest first, like `shape`) into the array a variable-rate
    device stream holds; returns ``(words, lengths, nbits)`` of the updated
    array like `encode_variable`, or ``(words, lengths, nbits, index)`` with
    ``with_index=True``.  `words`, `lengths` and `index` (`variable_index` of
    `lengths`) are the source and are not changed: block lengths change, so the
    update is out of place.

    Exactly one of `precision` and `tolerance` names the mode the touched
    blocks are coded at.  With A = ``decode_variable(words, lengths)``, M = A
    with the box replaced by `x` and E = ``encode_variable(M, mode)``: a block
    the box touches is E's block with E's length, every other block is its
    source bits and length, unchanged, and the blocks are packed back to back
    as `encode_variable` packs them.  A touched block the box covers (all its
    elements inside the array lie in the box) is coded from `x` alone.  A
    partly covered block is a read-modify-write: it is decoded from its old
    bits, the box's elements are replaced and it is coded again, so its other
    elements are re-coded from their decoded values.  If the box is a union of
    covered blocks and `x` the new array's values there, the result is byte
    for byte `encode_variable` of the new array -- what CPU zfp 0.5.0 writes.

    The mode applies to the touched blocks only and may differ from the mode
    that wrote the rest: a brick of interest can be kept at ``precision=32``
    inside a ``tolerance=1e-2`` archive.  The decoders need only the block
    boundaries and take such a stream as it is; `truncate_variable` assumes one
    mode for the whole stream.

    `x` may be strided; a broadcast view (fill the box with a constant) is
    materialised on the launch stream as `encode_region` does.  `out` (64-bit
    words, not overlapping `words`) is allocated at the call's own worst case
    when None -- the source's bits plus the longest block of the mode for every
    touched block, proportional to the stream and the box rather than the
    array; a shorter `out` is never written past its end, but then holds no
    valid stream if nbits exceeds it.  The new `lengths` is a new int16 tensor;
    ``with_index=True`` also returns the new offset index, equal to
    `variable_index` of the new lengths and written by the pass that places
    the blocks, at no extra launch.  An index that does not belong to the
    stream cannot make the call read outside `words`, `lengths` and `index` or
    write outside its outputs.  Asynchronous on `stream` except for one
    synchronisation to read the count, as `encode_variable`."""
    import torch
    t = type_code(x.dtype)
    # (the mode is checked first, against the precision of the box's element size)
    maxprec, minexp = _variable_mode("encode_region_variable", 32 if t in (TYPE_INT32, TYPE_FLOAT) else 64,
                                     precision, tolerance, ("precision", "tolerance"))
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError("encode_region_variable", 2)
    shape = tuple(int(s) for s in shape)
    origin = tuple(int(o) for o in origin)
    extent = tuple(int(e) for e in getattr(x, "shape", ()))
    nx, ny, nz = _extents(shape)
    if len(origin) != len(shape) or len(extent) != len(shape):
        raise ValueError(f"encode_region_variable: origin {origin} and the box's shape {extent} must have "
                         f"the rank of shape {shape}")
    if any(o < 0 for o in origin) or any(e <= 0 for e in extent):
        raise ValueError("encode_region_variable: origin must be non-negative and the box not empty")
    if any(o + e > n for o, e, n in zip(origin, extent, shape)):
        raise ValueError(f"encode_region_variable: the box {origin} + {extent} leaves the array {shape}")
    if not x.is_cuda or not words.is_cuda or not lengths.is_cuda or not index.is_cuda:
        raise ValueError("encode_region_variable: expects a device box, a device stream and device indices")
    if lengths.element_size() != 2 or not lengths.is_contiguous() or not words.is_contiguous():
        raise ValueError("encode_region_variable: lengths must be a contiguous 16-bit tensor, words contiguous")
    if index.element_size() != 8 or not index.is_contiguous():
        raise ValueError("encode_region_variable: index must be a contiguous tensor of 64-bit words")
    nblocks = _block_count(shape)
    if lengths.numel() != nblocks:
        raise ValueError(f"encode_region_variable: lengths has {lengths.numel()} entries, the array has "
                         f"{nblocks} blocks")
    lib = library()
    n = lib.cuzfp_hip_encode_region_variable_workspace_bytes(t, nx, ny, nz)
    if n == 0:
        raise CodecError("encode_region_variable", 1)
    x = _materialise(x, stream)
    ox, oy, oz = _extents(origin)
    ex, ey, ez = _extents(extent)
    sx, sy, sz = _strides(x)
    src_bytes = words.numel() * words.element_size()
    s = stream if stream is not None else torch.cuda.current_stream(words.device)
    with torch.cuda.stream(s):
        ws = torch.empty((n + 7) // 8, dtype=torch.int64, device=words.device)
        if out is None:
            cap = lib.cuzfp_hip_encode_region_variable_maximum_size(t, nx, ny, nz, src_bytes, ex, ey, ez, ox, oy, oz,
                                                                    maxprec)
            if cap == 0:
                raise CodecError("encode_region_variable", 1)
            out = torch.empty(cap // 8, dtype=torch.int64, device=words.device)
        new_lengths = torch.empty(nblocks, dtype=torch.int16, device=words.device)
        new_index = torch.empty(index.numel(), dtype=torch.int64, device=words.device) if with_index else None
        total = torch.empty(1, dtype=torch.int64, device=words.device)
    if not out.is_cuda or not out.is_contiguous() or out.element_size() != 8:
        raise ValueError("encode_region_variable: out must be a contiguous device tensor of 64-bit words")
    rc = lib.cuzfp_hip_encode_region_variable(
        x.data_ptr(), sx, sy, sz, t, nx, ny, nz, maxprec, minexp, ox, oy, oz, ex, ey, ez,
        words.data_ptr(), src_bytes, lengths.data_ptr(), index.data_ptr(), index.numel() * index.element_size(),
        out.data_ptr(), out.numel() * 8, new_lengths.data_ptr(),
        new_index.data_ptr() if with_index else None, total.data_ptr(), ws.data_ptr(), n, _stream_handle(stream))
    _check("encode_region_variable", rc)
    with torch.cuda.stream(s):
        nbits = int(total.item())  # the one synchronisation: the count is data dependent
    new_words = out[: min((nbits + 63) // 64, out.numel())]
    if with_index:
        return new_words, new_lengths, nbits, new_index[: (nblocks + 63) // 64 + 1]
    return new_words, new_lengths, nbits


def _aligned_box(where, shape, dtype, origin, extent):
    """(type code, shape, origin, extent) of a crop or paste, checked before
    anything touches a device: the dtype, the rank, the box inside the array,
    and the alignment."""
    t = type_code(dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError(where, 2)
    shape = tuple(int(s) for s in shape)
    origin = tuple(int(o) for o in origin)
    extent = tuple(int(e) for e in extent)
    _extents(shape)
    if len(origin) != len(shape) or len(extent) != len(shape):
        raise ValueError(f"{where}: origin {origin} and extent {extent} must have the rank of shape {shape}")
    if any(o < 0 for o in origin) or any(e <= 0 for e in extent):
        raise ValueError(f"{where}: origin must be non-negative and the box not empty")
    if any(o + e > n for o, e, n in zip(origin, extent, shape)):
        raise ValueError(f"{where}: the box {origin} + {extent} leaves the array {shape}")
    if any(o % 4 or (e % 4 and o + e != n) for o, e, n in zip(origin, extent, shape)):
        raise ValueError(f"{where}: the box {origin} + {extent} is not block-aligned in the array {shape} (on every "
                         "axis the origin must be a multiple of 4 and the extent one too, or reach the array's end); "
                         "decode_region_variable / encode_region_variable handle partial coverage, by decoding")
    return t, shape, origin, extent


def _check_variable_stream(where, what, words, lengths, index, nblocks):
    """A stream, its lengths and its index as the crop and paste calls take them."""
    if not words.is_cuda or not lengths.is_cuda or not index.is_cuda:
        raise ValueError(f"{where}: expects a device {what} stream and device indices")
    if lengths.element_size() != 2 or not lengths.is_contiguous() or not words.is_contiguous():
        raise ValueError(f"{where}: {what} lengths must be a contiguous 16-bit tensor, words contiguous")
    if index.element_size() != 8 or not index.is_contiguous():
        raise ValueError(f"{where}: {what} index must be a contiguous tensor of 64-bit words")
    if lengths.numel() != nblocks:
        raise ValueError(f"{where}: {what} lengths has {lengths.numel()} entries, the {what} has {nblocks} blocks")


def extract_region_variable(words, lengths, index, shape, dtype, origin, extent, *, out=None, stream=None,
                            with_index=False):
    """Crop the block-aligned box ``origin .. origin + extent`` (slowest first,
    like `shape`) out of a variable-rate device stream without decoding it;
    returns ``(words, lengths, nbits)`` of a stand-alone stream of an array of
    shape `extent`, like `encode_variable`, or ``(words, lengths, nbits,
    index)`` with ``with_index=True``.  `index` is `variable_index` of
    `lengths`; the source is not changed.

    zfp codes every block on its own, so the box's blocks, copied bit for bit
    and packed back to back in the box's raster order, are byte for byte what
    `encode_variable` -- and CPU zfp 0.5.0 -- writes for the sub-array at the
    mode that wrote the source.  Nothing is decoded or coded again, and no mode
    is needed.  The result feeds `decode_variable`, `variable_index`,
    `decode_region_variable`, `truncate_variable` and `insert_region_variable`
    unchanged.

    The box must be aligned: on every axis the origin a multiple of 4, and the
    extent a multiple of 4 or reaching the array's end.  Any other box is a
    ValueError; `decode_region_variable` decodes such a box.

    `out` (64-bit words, not overlapping `words`) is allocated at the call's
    worst case when None -- the lesser of the source's bits and the type's
    longest block for every block of the box; a shorter `out` is never written
    past its end, but then holds no valid stream if nbits exceeds it.  An index
    that does not belong to the stream cannot make the call read outside
    `words`, `lengths` and `index` or write outside its outputs.  Asynchronous
    on `stream` except for one synchronisation to read the count, as
    `encode_variable`."""
    import torch
    where = "extract_region_variable"
    t, shape, origin, extent = _aligned_box(where, shape, dtype, origin, extent)
    _check_variable_stream(where, "source", words, lengths, index, _block_count(shape))
    nx, ny, nz = _extents(shape)
    ox, oy, oz = _extents(origin)
    ex, ey, ez = _extents(extent)
    lib = library()
    n = lib.cuzfp_hip_extract_region_variable_workspace_bytes(t, ex, ey, ez)
    if n == 0:
        raise CodecError(where, 1)
    nrb = _block_count(extent)
    src_bytes = words.numel() * words.element_size()
    s = stream if stream is not None else torch.cuda.current_stream(words.device)
    with torch.cuda.stream(s):
        ws = torch.empty((n + 7) // 8, dtype=torch.int64, device=words.device)
        if out is None:
            cap = lib.cuzfp_hip_extract_region_variable_maximum_size(t, nx, ny, nz, src_bytes, ex, ey, ez, ox, oy, oz)
            if cap == 0:
                raise CodecError(where, 1)
            out = torch.empty(cap // 8, dtype=torch.int64, device=words.device)
        new_lengths = torch.empty(nrb, dtype=torch.int16, device=words.device)
        new_index = torch.empty((nrb + 63) // 64 + 1, dtype=torch.int64, device=words.device) if with_index else None
        total = torch.empty(1, dtype=torch.int64, device=words.device)
    if not out.is_cuda or not out.is_contiguous() or out.element_size() != 8:
        raise ValueError(f"{where}: out must be a contiguous device tensor of 64-bit words")
    rc = lib.cuzfp_hip_extract_region_variable(
        words.data_ptr(), src_bytes, lengths.data_ptr(), index.data_ptr(), index.numel() * index.element_size(),
        t, nx, ny, nz, ox, oy, oz, ex, ey, ez, out.data_ptr() if out.numel() else None, out.numel() * 8,
        new_lengths.data_ptr(), new_index.data_ptr() if with_index else None,
        new_index.numel() * 8 if with_index else 0, total.data_ptr(), ws.data_ptr(), n, _stream_handle(stream))
    _check(where, rc)
    with torch.cuda.stream(s):
        nbits = int(total.item())  # the one synchronisation: the count is data dependent
    new_words = out[: min((nbits + 63) // 64, out.numel())]
    if with_index:
        return new_words, new_lengths, nbits, new_index
    return new_words, new_lengths, nbits


def insert_region_variable(box_words, box_lengths, box_index, words, lengths, index, shape, dtype, origin, extent, *,
                           out=None, stream=None, with_index=False):
    """Paste the variable-rate device stream of a brick (`box_words`,
    `box_lengths`, `box_index`: a stream of an array of shape `extent`) over
    the block-aligned box ``origin .. origin + extent`` of the array another
    stream (`words`, `lengths`, `index`) holds, without decoding either;
    returns ``(words, lengths, nbits)`` of the updated array like
    `encode_variable`, or ``(words, lengths, nbits, index)`` with
    ``with_index=True``.  Each index is `variable_index` of its lengths.
    Neither input is changed: block lengths change, so the call is out of
    place, like `encode_region_variable`.

    A block inside the box is the brick's block, with the brick's length; every
    other block is its source bits and length; all are packed back to back as
    `encode_variable` packs them.  Pasting ``encode_variable(X, mode)`` gives
    what ``encode_region_variable(X, ..., origin, mode)`` gives on the same
    box, and what `extract_region_variable` cropped goes back byte for byte.

    The brick must be of the archive's dtype and rank -- the caller states that
    and the call cannot check it -- and `box_lengths` must have one entry for
    every block of the box.  The call knows no modes: a ``precision=32`` brick
    may go into a ``tolerance=1e-2`` archive, by the argument of
    `encode_region_variable`: the decoders need the block boundaries, not the
    mode.  The box must be aligned, as for `extract_region_variable`;
    `encode_region_variable` writes any other box, from values.

    Assembling an array from its slabs: the stream of an all-zero array is one
    0 bit a block -- ``nblocks`` lengths of 1, ceil(nblocks / 64) zero words --
    and pasting each slab's stream into it, slab by slab, gives the stream of
    the whole array; `join_variable` does that in one pass for slabs along the
    slowest axis.

    `out` (64-bit words, overlapping neither input) is allocated at the bits of
    both inputs when None; a shorter `out` is never written past its end, but
    then holds no valid stream if nbits exceeds it.  Indices and lengths that do
    not belong to their streams cannot make the call read outside its inputs or
    write outside its outputs.  Asynchronous on `stream` except for one
    synchronisation to read the count, as `encode_variable`."""
    import torch
    where = "insert_region_variable"
    t, shape, origin, extent = _aligned_box(where, shape, dtype, origin, extent)
    nblocks = _block_count(shape)
    _check_variable_stream(where, "source", words, lengths, index, nblocks)
    _check_variable_stream(where, "box", box_words, box_lengths, box_index, _block_count(extent))
    nx, ny, nz = _extents(shape)
    ox, oy, oz = _extents(origin)
    ex, ey, ez = _extents(extent)
    lib = library()
    n = lib.cuzfp_hip_insert_region_variable_workspace_bytes(t, nx, ny, nz)
    if n == 0:
        raise CodecError(where, 1)
    src_bytes = words.numel() * words.element_size()
    box_bytes = box_words.numel() * box_words.element_size()
    s = stream if stream is not None else torch.cuda.current_stream(words.device)
    with torch.cuda.stream(s):
        ws = torch.empty((n + 7) // 8, dtype=torch.int64, device=words.device)
        if out is None:
            cap = lib.cuzfp_hip_insert_region_variable_maximum_size(src_bytes, box_bytes)
            out = torch.empty(cap // 8, dtype=torch.int64, device=words.device)
        new_lengths = torch.empty(nblocks, dtype=torch.int16, device=words.device)
        new_index = torch.empty((nblocks + 63) // 64 + 1, dtype=torch.int64, device=words.device) if with_index else None
        total = torch.empty(1, dtype=torch.int64, device=words.device)
    if not out.is_cuda or not out.is_contiguous() or out.element_size() != 8:
        raise ValueError(f"{where}: out must be a contiguous device tensor of 64-bit words")
    rc = lib.cuzfp_hip_insert_region_variable(
        box_words.data_ptr(), box_bytes, box_lengths.data_ptr(), box_index.data_ptr(),
        box_index.numel() * box_index.element_size(), words.data_ptr(), src_bytes, lengths.data_ptr(),
        index.data_ptr(), index.numel() * index.element_size(), t, nx, ny, nz, ox, oy, oz, ex, ey, ez,
        out.data_ptr() if out.numel() else None, out.numel() * 8, new_lengths.data_ptr(),
        new_index.data_ptr() if with_index else None, total.data_ptr(), ws.data_ptr(), n, _stream_handle(stream))
    _check(where, rc)
    with torch.cuda.stream(s):
        nbits = int(total.item())  # the one synchronisation: the count is data dependent
    new_words = out[: min((nbits + 63) // 64, out.numel())]
    if with_index:
        return new_words, new_lengths, nbits, new_index
    return new_words, new_lengths, nbits


JOIN_MAX_PARTS = 64  # the part table travels in the kernel arguments (kJoinMaxParts)


def join_variable(parts, shape, dtype, out=None, stream=None, with_index=False):
    """Concatenate the variable-rate device streams of the slabs of an array
    into the stream of the array, in one pass and without decoding; returns
    ``(words, lengths, nbits)`` like `encode_variable`, or ``(words, lengths,
    nbits, index)`` with ``with_index=True``.

    `parts` is a sequence of ``(words, lengths)`` or ``(words, lengths,
    nbits)`` tuples as `encode_variable` returns them, in slab order along the
    slowest axis of `shape`: z-slabs of a 3D array, y-slabs of a 2D one,
    x-ranges of a 1D one.  A part's depth follows from its block count; every
    part is a whole number of 4-deep block slabs (so every slab but the last is
    a multiple of 4 deep), and together they are the array.  At most 64 parts.

    zfp codes every block on its own and writes the blocks back to back, so
    the parts' bits laid end to end are byte for byte what `encode_variable` --
    and CPU zfp 0.5.0 -- writes for the whole array at the mode that wrote the
    parts.  No mode and no index of a part is needed; parts of different modes
    join as well, as the decoders need block boundaries, not the mode.  It is
    the inverse of `extract_region_variable` on slabs, and replaces pasting
    slab after slab into an all-zero archive with `insert_region_variable`.

    `out` (64-bit words, overlapping no part) is allocated at the parts' bytes
    when None; a shorter `out` is never written past its end, but then holds no
    valid stream if nbits exceeds it.  Lengths that do not belong to their
    streams cannot make the call read outside the parts or write outside its
    outputs.  Asynchronous on `stream` except for one synchronisation to read
    the count, as `encode_variable`."""
    import torch
    where = "join_variable"
    t = type_code(dtype)
    if t in (TYPE_INT32, TYPE_INT64):
        raise CodecError(where, 2)
    shape = tuple(int(s) for s in shape)
    nx, ny, nz = _extents(shape)
    if any(s <= 0 for s in shape):
        raise ValueError(f"{where}: invalid shape {shape}")
    parts = list(parts)
    if not parts or len(parts) > JOIN_MAX_PARTS:
        raise ValueError(f"{where}: takes 1 to {JOIN_MAX_PARTS} parts, not {len(parts)}")
    nblocks = _block_count(shape)
    slab = _block_count(shape[1:])  # the blocks of one 4-deep slab of the slowest axis
    count = 0
    for k, part in enumerate(parts):
        if len(part) not in (2, 3):
            raise ValueError(f"{where}: part {k} must be (words, lengths) or (words, lengths, nbits)")
        words, lengths = part[0], part[1]
        if not words.is_cuda or not lengths.is_cuda:
            raise ValueError(f"{where}: part {k}: expects a device stream and device lengths")
        if lengths.element_size() != 2 or not lengths.is_contiguous() or not words.is_contiguous():
            raise ValueError(f"{where}: part {k}: lengths must be a contiguous 16-bit tensor, words contiguous")
        if words.element_size() % 4:
            raise ValueError(f"{where}: part {k}: words must be a tensor of 32- or 64-bit words")
        n = lengths.numel()
        if n == 0 or n % slab:
            raise ValueError(f"{where}: part {k} has {n} blocks, no whole number of slabs of {slab} blocks")
        if len(part) == 3 and int(part[2]) > 8 * words.numel() * words.element_size():
            raise ValueError(f"{where}: part {k}: words holds fewer than its {int(part[2])} bits")
        count += n
    if count != nblocks:
        raise ValueError(f"{where}: the parts have {count} blocks, the array {shape} has {nblocks}")
    if out is not None and (not out.is_cuda or not out.is_contiguous() or out.element_size() != 8):
        raise ValueError(f"{where}: out must be a contiguous device tensor of 64-bit words")
    device = parts[0][0].device
    lib = library()
    table = (VariablePart * len(parts))()
    for k, part in enumerate(parts):
        table[k] = VariablePart(part[0].data_ptr(), part[0].numel() * part[0].element_size(), part[1].data_ptr(),
                                part[1].numel())
    n = lib.cuzfp_hip_join_variable_workspace_bytes(t, nx, ny, nz)
    if n == 0:
        raise CodecError(where, 1)
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        ws = torch.empty((n + 7) // 8, dtype=torch.int64, device=device)
        if out is None:
            out = torch.empty(lib.cuzfp_hip_join_variable_maximum_size(table, len(parts)) // 8, dtype=torch.int64,
                              device=device)
        new_lengths = torch.empty(nblocks, dtype=torch.int16, device=device)
        new_index = torch.empty((nblocks + 63) // 64 + 1, dtype=torch.int64, device=device) if with_index else None
        total = torch.empty(1, dtype=torch.int64, device=device)
    rc = lib.cuzfp_hip_join_variable(
        table, len(parts), t, nx, ny, nz, out.data_ptr() if out.numel() else None, out.numel() * 8,
        new_lengths.data_ptr(), new_index.data_ptr() if with_index else None, total.data_ptr(), ws.data_ptr(), n,
        ctypes.c_void_p(s.cuda_stream))
    _check(where, rc)
    with torch.cuda.stream(s):
        nbits = int(total.item())  # the one synchronisation: the count is data dependent
    new_words = out[: min((nbits + 63) // 64, out.numel())]
    if with_index:
        return new_words, new_lengths, nbits, new_index
    return new_words, new_lengths, nbits


def copy(src, dst, stream=None):
    """Device-to-device copy through cuzfp_hip_copy (16-byte non-temporal
    accesses): the bandwidth calibrator bench.py reports beside the codec."""
    for name, t in (("src", src), ("dst", dst)):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"copy: {name} must be a contiguous device tensor")
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() < nbytes:
        raise ValueError("copy: destination too small")
    _check("copy", library().cuzfp_hip_copy(src.data_ptr(), dst.data_ptr(), nbytes, _stream_handle(stream)))
    return dst


def compress_host(a: np.ndarray, maxbits: int, nstreams: int = 4, out: np.ndarray | None = None):
    """Host array -> host stream (uint64 words) through the pinned, overlapped pipeline."""
    a = np.ascontiguousarray(a)
    nx, ny, nz = _extents(a.shape)
    nbytes = stream_bytes(a.shape, a.dtype, maxbits)
    if out is None:
        out = np.empty(nbytes // 8, dtype=np.uint64)
    else:
        _check_host_out(out, None, out.dtype, "compress_host")
        if out.nbytes < nbytes:
            raise ValueError(f"compress_host: out holds {out.nbytes} bytes, the stream needs {nbytes}")
    got = ctypes.c_size_t(0)
    rc = library().cuzfp_hip_compress_host(a.ctypes.data, type_code(a.dtype), nx, ny, nz, maxbits,
                                           out.ctypes.data, out.nbytes, ctypes.byref(got), nstreams)
    _check("compress_host", rc)
    return out


def release_host_cache(device: int = -1) -> None:
    """Free the host pipeline's retained device buffers, pinned staging buffers,
    streams and events (cuzfp_hip_release_host_cache; -1 = the current device)."""
    _check("release_host_cache", library().cuzfp_hip_release_host_cache(device))


def decompress_host(words: np.ndarray, shape, dtype, maxbits: int, nstreams: int = 4,
                    out: np.ndarray | None = None):
    words = np.ascontiguousarray(words)
    if out is None:
        out = np.empty(tuple(shape), dtype=dtype)
    else:
        _check_host_out(out, shape, dtype, "decompress_host")
    nx, ny, nz = _extents(out.shape)
    rc = library().cuzfp_hip_decompress_host(words.ctypes.data, words.nbytes, type_code(out.dtype),
                                             nx, ny, nz, maxbits, out.ctypes.data, nstreams)
    _check("decompress_host", rc)
    return out
