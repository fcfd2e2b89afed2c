"""Variable-rate modes (fixed precision, fixed accuracy): fixture, host emulation
and live fuzz against CPU zfp 0.5.0 (CPU-only; the kernels themselves are
checked in tests/test_variable_gpu.py against the same fixture).

The fixture tests/golden/variable.npz holds, for every case of `cases()`, what
the reference's own library gives: the SHA-256 of the stream of
``zfp_compress`` after ``zfp_stream_set_precision`` / ``zfp_stream_set_accuracy``,
the per-block lengths L_b (the return values of
``zfp_encode_partial_block_strided_*``), the total bit count and the SHA-256 of
``zfp_decompress``'s array.  tests/golden/make_variable_golden.py writes it
from `generate()` below; `test_fixture_is_current` regenerates it in memory
whenever the reference library is there.

tests/native/variable_emulate.cpp runs the per-lane functions of the kernels
(block_length, encode_block behind a writer that stops at L_b, decode_block
with budget L_b) on the host.
"""
import ctypes
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "variable_emulate.cpp")
HDR = os.path.join(ROOT, "cuzfp_amd", "csrc", "zfp_block.hpp")
HOST_IO = os.path.join(ROOT, "tests", "native", "host_io.hpp")
LIB = os.path.join(ROOT, "build", "libcuzfp_varemu.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "variable.npz")
TC = {np.dtype(np.float32): 3, np.dtype(np.float64): 4}
ZFP_MIN_EXP = -1074

# ---------------------------------------------------------------------------
# Cases

# the first three: three or more waves of 64 blocks, the last wave ragged;
# (6, 5, 9) is less than one wave; (13, 22, 38) has partial blocks on every
# axis and room for ordinary values beside the run of zero blocks
SHAPES = [(1000,), (33, 70), (9, 20, 36), (6, 5, 9), (13, 22, 38)]
PRECISIONS = {np.dtype(np.float32): (1, 7, 16, 32), np.dtype(np.float64): (1, 7, 16, 64)}
TOLERANCES = (0.0, 1e-3, 0.05, 1.0, 64.0)
ZERO_RUN = 130  # raster-consecutive all-zero blocks (more than two waves of 1-bit blocks)


def cases():
    """(shape, dtype, mode, parameter), mode "p" (precision) or "a" (accuracy)."""
    out = []
    for shape in SHAPES:
        for dt in (np.float32, np.float64):
            for p in PRECISIONS[np.dtype(dt)]:
                out.append((shape, np.dtype(dt), "p", p))
            for t in TOLERANCES:
                out.append((shape, np.dtype(dt), "a", t))
    return out


def case_id(case):
    shape, dt, mode, par = case
    return f"{'x'.join(map(str, shape))}-{dt.name}-{mode}{par:g}"


def accuracy_to_minexp(tol):
    """zfp_stream_set_accuracy's rule (zfp.c)."""
    if not tol > 0:
        return ZFP_MIN_EXP
    return int(np.frexp(tol)[1]) - 1


def mode_params(case):
    """(maxprec, minexp) of a case."""
    _, dt, mode, par = case
    if mode == "p":
        return int(par), ZFP_MIN_EXP
    return dt.itemsize * 8, accuracy_to_minexp(par)


def nblocks(shape):
    return int(np.prod([(s + 3) // 4 for s in shape]))


def block_ids(shape):
    """Raster index of the block of every element."""
    idx = np.indices(shape)
    nb = [(s + 3) // 4 for s in shape]
    b = np.zeros(shape, np.int64)
    for ax in range(len(shape)):
        b = b * nb[ax] + idx[ax] // 4
    return b


def _values(rng, shape, dtype):
    """The recipe of test_truncate._values (floats)."""
    return (np.cumsum(rng.standard_normal(shape), axis=-1) *
            10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)


def _random_bits(rng, n, dtype):
    """Random sign and mantissa bits under exponents 2^-24 .. 2^-1: every bit
    plane of such a block is dense, which gives near-maximal block lengths."""
    dtype = np.dtype(dtype)
    if dtype.itemsize == 4:
        bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        e = (126 - rng.integers(0, 24, size=n)).astype(np.uint32)
        return ((bits & np.uint32(0x807FFFFF)) | (e << np.uint32(23))).view(np.float32)
    bits = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=n, dtype=np.uint64)
    e = (1022 - rng.integers(0, 24, size=n)).astype(np.uint64)
    return ((bits & np.uint64(0x800FFFFFFFFFFFFF)) | (e << np.uint64(52))).view(np.float64)


_ARRAYS = {}


def array(shape, dtype):
    """The case input: test_truncate's values, overwritten block-wise (raster
    order) with a run of all-zero blocks, a block of 1e-30 (below every
    tolerance, not zero) and two blocks of random bit patterns."""
    key = (tuple(shape), np.dtype(dtype).str)
    if key not in _ARRAYS:
        rng = np.random.default_rng(zlib.crc32(repr(("variable",) + key).encode()))
        a = _values(rng, shape, dtype)
        ids = block_ids(shape)
        nb = nblocks(shape)
        run = ZERO_RUN if nb >= ZERO_RUN + 5 else 2
        a[(ids >= 2) & (ids < 2 + run)] = 0
        a[ids == nb - 3] = 1e-30
        m = ids >= nb - 2
        a[m] = _random_bits(rng, int(m.sum()), dtype)
        assert np.isfinite(a).all()
        a.setflags(write=False)
        _ARRAYS[key] = a
    return _ARRAYS[key]


# ---------------------------------------------------------------------------
# The reference's library (zfp 0.5.0's public API, bound here)

class RefVariable:
    def __init__(self, reference):
        lib = reference.lib
        vp, u, i, sz, d = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
        sig = {
            "zfp_stream_open": (vp, [vp]), "zfp_stream_close": (None, [vp]),
            "stream_open": (vp, [vp, sz]), "stream_close": (None, [vp]),
            "zfp_stream_set_bit_stream": (None, [vp, vp]), "zfp_stream_rewind": (None, [vp]),
            "zfp_stream_flush": (None, [vp]),
            "zfp_stream_set_precision": (u, [vp, u, i]), "zfp_stream_set_accuracy": (d, [vp, d, i]),
            "zfp_stream_maximum_size": (sz, [vp, vp]),
            "zfp_field_1d": (vp, [vp, i, u]), "zfp_field_2d": (vp, [vp, i, u, u]),
            "zfp_field_3d": (vp, [vp, i, u, u, u]), "zfp_field_free": (None, [vp]),
            "zfp_compress": (sz, [vp, vp]), "zfp_decompress": (i, [vp, vp]),
        }
        for t in ("float", "double"):
            sig[f"zfp_encode_partial_block_strided_{t}_1"] = (u, [vp, vp, u, i])
            sig[f"zfp_encode_partial_block_strided_{t}_2"] = (u, [vp, vp, u, u, i, i])
            sig[f"zfp_encode_partial_block_strided_{t}_3"] = (u, [vp, vp, u, u, u, i, i, i])
        for name, (res, args) in sig.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        self.lib = lib

    def _open(self, case, buf):
        _, dt, mode, par = case
        z = self.lib.zfp_stream_open(None)
        bs = self.lib.stream_open(buf.ctypes.data, buf.nbytes)
        self.lib.zfp_stream_set_bit_stream(z, bs)
        if mode == "p":
            self.lib.zfp_stream_set_precision(z, int(par), TC[dt])
        else:
            self.lib.zfp_stream_set_accuracy(z, float(par), TC[dt])
        self.lib.zfp_stream_rewind(z)
        return z, bs

    def _field(self, a):
        t = TC[a.dtype]
        ext = a.shape[::-1]
        f = getattr(self.lib, f"zfp_field_{a.ndim}d")
        return f(a.ctypes.data, t, *ext)

    def maximum_size(self, case):
        shape, dt = case[0], case[1]
        a = np.zeros(shape, dt)
        buf = np.zeros(1, np.uint64)
        z, bs = self._open(case, buf)
        fld = self._field(a)
        n = self.lib.zfp_stream_maximum_size(z, fld)
        self.lib.zfp_field_free(fld)
        self.lib.zfp_stream_close(z)
        self.lib.stream_close(bs)
        return int(n)

    def compress(self, a, case):
        """zfp_compress's stream as uint64 words."""
        a = np.ascontiguousarray(a)
        buf = np.zeros(self.maximum_size(case) // 8 + 1, np.uint64)
        z, bs = self._open(case, buf)
        fld = self._field(a)
        n = self.lib.zfp_compress(z, fld)
        self.lib.zfp_field_free(fld)
        self.lib.zfp_stream_close(z)
        self.lib.stream_close(bs)
        assert n and n % 8 == 0, n
        return buf[: n // 8].copy()

    def decompress(self, words, case):
        shape, dt = case[0], case[1]
        words = np.ascontiguousarray(words, np.uint64)
        buf = np.concatenate([words, np.zeros(2, np.uint64)])
        out = np.zeros(shape, dt)
        z, bs = self._open(case, buf)
        fld = self._field(out)
        ok = self.lib.zfp_decompress(z, fld)
        self.lib.zfp_field_free(fld)
        self.lib.zfp_stream_close(z)
        self.lib.stream_close(bs)
        assert ok
        return out

    def lengths(self, a, case):
        """L_b of every block in raster order: what the block encoder returns."""
        a = np.ascontiguousarray(a)
        dims = a.ndim
        tname = "float" if a.dtype == np.float32 else "double"
        enc = getattr(self.lib, f"zfp_encode_partial_block_strided_{tname}_{dims}")
        buf = np.zeros(self.maximum_size(case) // 8 + 1, np.uint64)
        z, bs = self._open(case, buf)
        ext = a.shape[::-1] + (1,) * (3 - dims)  # (nx, ny, nz)
        st = [s // a.itemsize for s in a.strides[::-1]]
        out = []
        base = a.ctypes.data
        for bz in range(0, ext[2], 4):
            for by in range(0, ext[1], 4):
                for bx in range(0, ext[0], 4):
                    o = [bx, by, bz][:dims]
                    p = base + a.itemsize * sum(oi * si for oi, si in zip(o, st))
                    w = [min(4, ext[k] - o[k]) for k in range(dims)]
                    out.append(enc(z, p, *w, *st))
        self.lib.zfp_stream_close(z)
        self.lib.stream_close(bs)
        return np.array(out, np.uint16)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def generate(reference):
    """The fixture's arrays, from the reference's library."""
    ref = RefVariable(reference)
    names, lens, starts, nbits, ssha, dsha = [], [], [0], [], [], []
    for case in cases():
        a = array(case[0], case[1])
        s = ref.compress(a, case)
        L = ref.lengths(a, case)
        total = int(L.astype(np.uint64).sum())
        assert (total + 63) // 64 == s.size, (case_id(case), total, s.size)
        names.append(case_id(case))
        lens.append(L)
        starts.append(starts[-1] + L.size)
        nbits.append(total)
        ssha.append(sha(s))
        dsha.append(sha(ref.decompress(s, case)))
    return {"names": np.array(names), "lengths": np.concatenate(lens), "starts": np.array(starts, np.int64),
            "nbits": np.array(nbits, np.uint64), "stream_sha": np.stack(ssha), "decoded_sha": np.stack(dsha)}


class Golden:
    def __init__(self, d):
        self.d = {k: d[k] for k in ("names", "lengths", "starts", "nbits", "stream_sha", "decoded_sha")}
        self.index = {str(n): i for i, n in enumerate(self.d["names"])}

    def get(self, case):
        i = self.index[case_id(case)]
        d = self.d
        return {"lengths": d["lengths"][d["starts"][i]: d["starts"][i + 1]], "nbits": int(d["nbits"][i]),
                "stream_sha": d["stream_sha"][i], "decoded_sha": d["decoded_sha"][i]}


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        with np.load(FIXTURE) as z:
            _GOLDEN.append(Golden(z))
    return _GOLDEN[0]


@pytest.fixture(scope="module")
def golden():
    return load_golden()


# ---------------------------------------------------------------------------
# Host emulation

@pytest.fixture(scope="module")
def varemu():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in (SRC, HDR, HOST_IO)):
        subprocess.check_call(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-Wno-unknown-pragmas", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    u, i, vp, sz = ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.var_compress.restype = ctypes.c_ulonglong
    lib.var_compress.argtypes = [i, u, u, u, u, i, vp, vp, vp, sz]
    lib.var_decompress.restype = i
    lib.var_decompress.argtypes = [i, u, u, u, vp, sz, vp, vp]
    return lib


def _ext(shape):
    padded = tuple(shape[::-1]) + (0, 0)
    return padded[0], padded[1], padded[2]


def emu_compress(lib, a, maxprec, minexp):
    """(words, lengths, nbits) of the host emulation."""
    a = np.ascontiguousarray(a)
    nx, ny, nz = _ext(a.shape)
    L = np.zeros(nblocks(a.shape), np.uint16)
    total = lib.var_compress(TC[a.dtype], nx, ny, nz, maxprec, minexp, a.ctypes.data, L.ctypes.data, None, 0)
    words = np.zeros((total + 63) // 64, np.uint64)
    L2 = np.zeros_like(L)
    got = lib.var_compress(TC[a.dtype], nx, ny, nz, maxprec, minexp, a.ctypes.data, L2.ctypes.data,
                           words.ctypes.data, words.size)
    assert got == total and np.array_equal(L, L2)
    return words, L, int(total)


def emu_decompress(lib, words, lengths, shape, dtype):
    nx, ny, nz = _ext(shape)
    out = np.full(shape, np.nan, dtype)
    words = np.ascontiguousarray(words, np.uint64)
    lengths = np.ascontiguousarray(lengths, np.uint16)
    assert lib.var_decompress(TC[np.dtype(dtype)], nx, ny, nz, words.ctypes.data, words.size,
                              lengths.ctypes.data, out.ctypes.data)
    return out


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_emulation_matches_fixture(varemu, golden, case):
    """The closed-form lengths, the stream of the coder stopped at L_b and the
    decode with budget L_b equal the reference's, exactly."""
    g = golden.get(case)
    a = array(case[0], case[1])
    words, L, total = emu_compress(varemu, a, *mode_params(case))
    assert np.array_equal(L, g["lengths"])
    assert total == g["nbits"]
    assert np.array_equal(sha(words), g["stream_sha"])
    d = emu_decompress(varemu, words, L, case[0], case[1])
    assert np.array_equal(sha(d), g["decoded_sha"])


def test_fixture_inputs_reach_the_hard_cases(golden):
    """The recipe does what it is there for: a run of 1-bit blocks longer than
    two waves, a non-zero block below every tolerance, near-maximal lengths."""
    for shape in SHAPES:
        if nblocks(shape) < ZERO_RUN + 5:
            continue
        for dt in (np.float32, np.float64):
            L = golden.get((shape, np.dtype(dt), "a", 1e-3))["lengths"]
            assert (L[2:2 + ZERO_RUN] == 1).all()
            assert L[nblocks(shape) - 3] == 1  # 1e-30 under a tolerance: the one-bit form
            full = golden.get((shape, np.dtype(dt), "p", np.dtype(dt).itemsize * 8))["lengths"]
            assert full[nblocks(shape) - 3] > 1  # ... and a coded block in precision mode
            n = 4 ** len(shape)
            assert full.max() > 0.85 * n * np.dtype(dt).itemsize * 8


def test_fixture_is_current(reference, golden):
    """The committed fixture is what the reference's library gives today."""
    fresh = generate(reference)
    for k, v in fresh.items():
        assert np.array_equal(v, golden.d[k]), k


def test_accuracy_to_minexp():
    """cuzfp_hip_accuracy_to_minexp is zfp_stream_set_accuracy's frexp rule."""
    import cuzfp_amd
    for tol, want in ((0.0, -1074), (-1.0, -1074), (1e-3, -10), (0.05, -5), (1.0, 0), (64.0, 6), (1e-6, -20),
                      (0.5, -1), (0.75, -1), (2.0 ** -30, -30), (3.0, 1)):
        assert cuzfp_amd.accuracy_to_minexp(tol) == want == accuracy_to_minexp(tol), tol


def test_maximum_size(reference):
    """cuzfp_hip_variable_maximum_size is zfp_stream_maximum_size in these modes."""
    import cuzfp_amd
    ref = RefVariable(reference)
    for case in cases():
        assert cuzfp_amd.variable_maximum_size(case[0], case[1], mode_params(case)[0]) == ref.maximum_size(case)
    with pytest.raises(cuzfp_amd.CodecError):
        cuzfp_amd.variable_maximum_size((8, 8), np.int32, 16)
    with pytest.raises(cuzfp_amd.CodecError):
        cuzfp_amd.variable_maximum_size((8, 8), np.float32, 33)


def test_live_fuzz(varemu, reference):
    """Random shapes, modes and parameters (at most 40^3 values) against the
    live library: lengths, stream and decoded array, exactly."""
    ref = RefVariable(reference)
    rng = np.random.default_rng(2024)
    for trial in range(24):
        dims = 1 + trial % 3
        hi = {1: 2000, 2: 120, 3: 40}[dims]
        shape = tuple(int(rng.integers(1, hi + 1)) for _ in range(dims))
        dt = np.dtype(np.float32 if rng.random() < 0.5 else np.float64)
        if rng.random() < 0.5:
            case = (shape, dt, "p", int(rng.integers(1, dt.itemsize * 8 + 1)))
        else:
            case = (shape, dt, "a", float(rng.choice([0.0, 10.0 ** rng.uniform(-8, 3)])))
        kind = trial % 4
        if kind == 0:
            a = _values(rng, shape, dt)
        elif kind == 1:
            a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-40, 30, size=shape)).astype(dt)
        elif kind == 2:
            a = np.where(rng.random(shape) < 0.7, 0, rng.standard_normal(shape)).astype(dt)
        else:
            a = _random_bits(rng, int(np.prod(shape)), dt).reshape(shape)
        a = np.where(np.isfinite(a), a, 0).astype(dt)
        s = ref.compress(a, case)
        words, L, total = emu_compress(varemu, a, *mode_params(case))
        assert np.array_equal(L, ref.lengths(a, case)), case_id(case)
        assert np.array_equal(words, s), case_id(case)
        d = emu_decompress(varemu, words, L, shape, dt)
        assert np.array_equal(d.view(np.uint8), ref.decompress(s, case).view(np.uint8)), case_id(case)
