"""Decoding a variable-rate stream at a coarser mode, the part that needs no
GPU: the per-lane arithmetic of cuzfp_hip_decode_region_variable_coarse on the
host (cuzfp_amd/csrc/variable_coarse.hpp over rerate_variable.hpp), the
semantics pinned to the reference's arrays, the argument checks of the entry
point (every error is a status before any launch) and the Python validation.
The kernel goes through the same corpus in tests/test_variable_coarse_gpu.py.

The rule.  A mode is (maxprec, minexp).  A block of a stream is decoded at a
target mode by decode_block with a budget of L' bits, L' =
truncated_block_length(the block, its source length, the target); L' <= 1 is
the zero block.  Where the target coarsens the stream's mode that is the
decode of the reference's stream at the target mode; in general it is the
array at (the smaller maxprec, the larger minexp).

tests/native/variable_coarse_emulate.cpp runs the walk and the budget function
(variable_coarse_budget: L' clamped to the column the host sizes from the
target) over a host copy of the stream.  Every expectation is the reference's:
the streams, lengths and decoded arrays of test_variable / test_variable_paths'
fixtures (CPU zfp 0.5.0), accepted only on the committed hashes.
"""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import block_zoo as bz
import cuzfp_amd as cz
import test_variable as tv
import test_variable_paths as tp
import test_variable_truncate as tt
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_gpu import ref_of as tv_ref_of  # (a helper: needs no GPU)
from test_variable_paths import F32, F64
from test_variable_truncate import tp_golden, tv_golden  # noqa: F401  (fixtures)

SRC = os.path.join(tv.ROOT, "tests", "native", "variable_coarse_emulate.cpp")
HDRS = [os.path.join(tv.ROOT, "cuzfp_amd", "csrc", h)
        for h in ("variable_coarse.hpp", "rerate_variable.hpp", "variable_index.hpp", "region.hpp", "zfp_block.hpp")]
LIB = os.path.join(tv.ROOT, "build", "libcuzfp_vcoarse.so")
BIG = (13, 22, 38)  # the largest test_variable shape: 240 blocks, ragged waves, partial blocks


@pytest.fixture(scope="module")
def vcoarse():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.check_call(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-Wno-unknown-pragmas", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    u, i, vp, sz = ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.vcoarse_blocks.restype = i
    lib.vcoarse_blocks.argtypes = [i, i, vp, sz, vp, sz, u, i, vp, vp]
    lib.vcoarse_column_dwords.restype = u
    lib.vcoarse_column_dwords.argtypes = [i, i, u]
    return lib


@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


# ---------------------------------------------------------------------------
# The host walk

def host_walk(lib, words, L, dims, dtype, mode):
    """(L', budget) of every block at the target `mode`, on the host."""
    words = np.ascontiguousarray(words, np.uint64)
    L = np.ascontiguousarray(L, np.uint16)
    walked = np.full(L.size, 0xDEAD, np.uint16)
    budget = np.full(L.size, 0xDEADBEEF, np.uint32)
    assert lib.vcoarse_blocks(tv.TC[np.dtype(dtype)], dims, words.ctypes.data, words.size, L.ctypes.data, L.size,
                              mode[0], mode[1], walked.ctypes.data, budget.ctypes.data)
    return walked, budget


def column_bits(dims, dtype, maxprec):
    """The bits of a lane's column at the target precision: the longest block a
    mode with maxprec planes writes (zfp_stream_maximum_size's formula), in
    whole dwords."""
    bits = 1 + tp.ebits(dtype) + 4 ** dims - 1 + 4 ** dims * maxprec
    return 32 * ((bits + 31) // 32)


def coarse_decode(varemu, vcoarse, words, L, shape, dtype, mode):  # noqa: F811
    """The rule on the host: every block's first L' bits (the one-bit form where
    L' is 1), packed back to back, through the emulation's decode_block with a
    budget of L'.  Also checks that the column's clamp does not bind."""
    walked, budget = host_walk(vcoarse, words, L, len(shape), dtype, mode)
    assert np.array_equal(budget, np.where(walked > 1, walked, 0)), "the column is too short for a coded block"
    return tv.emu_decompress(varemu, tt.cut(words, L, walked), walked, shape, dtype), walked


# ---------------------------------------------------------------------------
# The budget function over arbitrary bits

def budget_targets(dtype):
    return [tt.mode_of(dtype, "p", 1), tt.mode_of(dtype, "p", tp.type_prec(dtype)), tt.mode_of(dtype, "a", 0.0),
            tt.mode_of(dtype, "a", 1e38)]


def test_column_dwords(vcoarse):
    """The image height: ceil(max_block_bits(maxprec) / 32), the type's longest
    block at the type's precision; 3D double at p16 is 35 rows."""
    for dt in (F32, F64):
        for dims in (1, 2, 3):
            for p in range(1, tp.type_prec(dt) + 1):
                assert 32 * vcoarse.vcoarse_column_dwords(tv.TC[dt], dims, p) == column_bits(dims, dt, p)
            assert column_bits(dims, dt, tp.type_prec(dt)) == 32 * ((bz.top(dims, dt) + 31) // 32)
    assert vcoarse.vcoarse_column_dwords(4, 3, 16) == 35 and vcoarse.vcoarse_column_dwords(4, 3, 64) == 131
    assert vcoarse.vcoarse_column_dwords(3, 3, 32) == 67


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_budget_bounds_on_arbitrary_bits(vcoarse, dims, dtype):
    """Arbitrary bits under every raw length -- 0, 1, 2 .. ebits + 1 (no block's
    length), ebits + 2 .. the type's longest, and 65535: the budget is 0 or lies
    in [ebits + 2, min(clamped source length, column bits)], and it is 0
    exactly where the source is a zero block or the target codes no plane of
    the block (its exponent field against the target, by zfp's precision())."""
    eb, hi = tp.ebits(dtype), bz.top(dims, dtype)
    lo = eb + 2
    L = np.array([0, 1] + list(range(2, lo)) + list(range(lo, hi + 1)) + [65535], np.int64)
    ebias = {8: 127, 11: 1023}[eb]
    for density in tp.DENSITIES:
        rng = np.random.default_rng(zlib.crc32(repr(("coarse", dims, dtype.str, density)).encode()))
        words = bz.random_stream(rng, 1, int(L.sum()), density)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        off = np.cumsum(L) - L
        clamped = np.minimum(L, hi)
        legal = clamped >= lo
        first = np.where(legal, bits[np.minimum(off, bits.size - 1)], 0)
        e = np.zeros(L.size, np.int64)
        for k in range(eb):
            e += np.where(legal, bits[np.minimum(off + 1 + k, bits.size - 1)].astype(np.int64) << k, 0)
        emax = e - ebias
        reached = {"zero": 0, "coded": 0}
        for mode in budget_targets(dtype):
            walked, budget = host_walk(vcoarse, words, L.astype(np.uint16), dims, dtype, mode)
            budget = budget.astype(np.int64)
            col = column_bits(dims, dtype, mode[0])
            planes = np.minimum(np.maximum(emax - mode[1] + 2 * (dims + 1), 0), mode[0])
            zero = ~legal | (first == 0) | (planes == 0)
            assert np.array_equal(budget == 0, zero), (density, mode)
            assert ((budget == 0) | ((budget >= lo) & (budget <= np.minimum(clamped, col)))).all(), (density, mode)
            assert (budget <= walked).all()
            reached["zero"] += int((legal & (first == 1) & (planes == 0)).sum())
            reached["coded"] += int((budget > 0).sum())
        # the cases the test is for: the clamp to the small image binds (p1), a coded source block the target
        # codes no plane of (a1e38), and coded blocks
        # the cases the test is for: a coded source block the target codes no plane of (a1e38), and coded blocks.
        # (The clamp to the column has not been seen to bind: every bit string is some block's code, so the walk
        # over p planes stays within the longest block of p planes.  All-ones bits reach that length exactly.)
        assert reached["zero"] >= 1 and reached["coded"] >= 1, (density, reached)
    ones = np.full(80, ~np.uint64(0))
    ones[0] = np.uint64((1 << 64) - 1 - (1 << eb))  # the exponent field's top bit clear: a finite exponent
    for p in (1, 2, tp.type_prec(dtype)):
        walked, budget = host_walk(vcoarse, ones, np.array([0xFFFF], np.uint16), dims, dtype, (p, -1074))
        longest = 1 + eb + 4 ** dims - 1 + 4 ** dims * p
        assert int(walked[0]) == int(budget[0]) == longest <= column_bits(dims, dtype, p), (p, walked, budget)


# ---------------------------------------------------------------------------
# The semantics on the reference's streams

BIG_GROUPS = [(BIG, np.dtype(dt)) for dt in (np.float32, np.float64)]


@pytest.mark.parametrize("group", BIG_GROUPS, ids=tt.tv_id)
def test_fixture_arrays(varemu, vcoarse, tv_golden, group):  # noqa: F811
    """13 x 22 x 38: the reference's p = full stream decoded at every mode of the
    case list, its a1e-3 stream at a0.05 and its p16 stream at p7, by the rule,
    is the reference's decode of its own stream at the target mode."""
    shape, dt = group
    pairs = 0
    for src_case, dst_cases in tt.tv_cuts(shape, dt):
        words, L = tv_ref_of(varemu, tv_golden, src_case)[:2]
        for case in dst_cases:
            ref = tv_ref_of(varemu, tv_golden, case)
            got, walked = coarse_decode(varemu, vcoarse, words, L, shape, dt, tv.mode_params(case))
            assert np.array_equal(walked, ref[1]), (tv.case_id(src_case), tv.case_id(case))
            assert tp.same(got, ref[3]), (tv.case_id(src_case), tv.case_id(case))
            pairs += 1
    assert pairs == 9 + 2


@pytest.mark.parametrize("group", tt.TP_GROUPS, ids=tt.tp_id)
def test_paths_arrays(varemu, vcoarse, tp_golden, group):  # noqa: F811
    """The zoo and the ragged zoo (NaN, inf and denormal blocks) from p = full at
    every precision and the tolerance ladder, `three`, and `tiles2d` from the
    emulation's p = full stream: the same."""
    name, dt = group
    shape = tp.array(name, dt).shape
    pairs = 0
    for _, src, dsts in tt.tp_cuts(varemu, tp_golden, name, dt):
        for case, ref in dsts:
            got, walked = coarse_decode(varemu, vcoarse, src[0], src[1], shape, dt, tt.mode_of(dt, case[2], case[3]))
            assert np.array_equal(walked, ref[1]), tp.case_id(case)
            assert tp.same(got, ref[3]), tp.case_id(case)
            pairs += 1
    assert pairs == (tp.type_prec(dt) + len(tp.TOLERANCES) if name in tp.ZOO_NAMES else len(tp.OTHERS[(name, dt)]))


# ---------------------------------------------------------------------------
# Neither mode coarsens the other: the array at (min maxprec, max minexp)

MIXED = ((("a", 1e-3), ("p", 16)), (("p", 16), ("a", 1e-3)))


def mixed_mode(dt, src, dst):
    a, b = tt.mode_of(dt, *src), tt.mode_of(dt, *dst)
    assert not tt.coarsens(a, b) and not tt.coarsens(b, a)
    return min(a[0], b[0]), max(a[1], b[1])


def mixed_expectation(varemu, vcoarse, tv_golden, dt, src, dst):  # noqa: F811
    """(decoded, L') of the source's stream at the target, with L' checked against
    the emulation's lengths at the expert mode (min maxprec, max minexp)."""
    words, L = tv_ref_of(varemu, tv_golden, (BIG, dt) + src)[:2]
    got, walked = coarse_decode(varemu, vcoarse, words, L, BIG, dt, tt.mode_of(dt, *dst))
    ewords, eL, _ = tv.emu_compress(varemu, tv.array(BIG, dt), *mixed_mode(dt, src, dst))
    assert np.array_equal(walked, eL), (dt, src, dst)
    assert np.array_equal(tt.cut(words, L, walked), ewords)
    assert tp.same(got, tv.emu_decompress(varemu, ewords, eL, BIG, dt))
    return got, walked


@pytest.mark.parametrize("dt", [F32, F64], ids=lambda d: d.name)
def test_mixed_pair(varemu, vcoarse, tv_golden, dt):  # noqa: F811
    """An a1e-3 stream decoded at p16 and a p16 stream decoded at a1e-3: the walk
    stops at the first of the target's end and the block's own, so L' is the
    length at (min of the two maxprec, max of the two minexp), and both orders
    give the same array."""
    a = mixed_expectation(varemu, vcoarse, tv_golden, dt, *MIXED[0])
    b = mixed_expectation(varemu, vcoarse, tv_golden, dt, *MIXED[1])
    assert np.array_equal(a[1], b[1]) and tp.same(a[0], b[0])
    # ... which is neither source's own decode
    for src, _ in MIXED:
        assert not tp.same(a[0], tv_ref_of(varemu, tv_golden, (BIG, dt) + src)[3])


@pytest.mark.parametrize("dt", [F32, F64], ids=lambda d: d.name)
def test_mixed_pair_expert_mode_is_the_reference(varemu, reference, dt):  # noqa: F811
    """The emulation's stream at the expert mode (16, minexp of 1e-3) is what the
    reference's library writes after zfp_stream_set_params, and decodes to what
    zfp_decompress returns from it."""
    lib = reference.lib
    ref = tv.RefVariable(reference)
    vp, u, i = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int
    lib.zfp_stream_set_params.restype = i
    lib.zfp_stream_set_params.argtypes = [vp, u, u, u, i]
    maxprec, minexp = mixed_mode(dt, *MIXED[0])
    a = np.ascontiguousarray(tv.array(BIG, dt))
    ewords, eL, total = tv.emu_compress(varemu, a, maxprec, minexp)

    def open_expert(buf):
        z = lib.zfp_stream_open(None)
        bs = lib.stream_open(buf.ctypes.data, buf.nbytes)
        lib.zfp_stream_set_bit_stream(z, bs)
        assert lib.zfp_stream_set_params(z, 0, 4171, maxprec, minexp)  # ZFP_MIN_BITS, ZFP_MAX_BITS
        lib.zfp_stream_rewind(z)
        return z, bs

    buf = np.zeros(ref.maximum_size((BIG, dt, "p", tp.type_prec(dt))) // 8 + 1, np.uint64)
    z, bs = open_expert(buf)
    fld = ref._field(a)
    n = lib.zfp_compress(z, fld)
    lib.zfp_field_free(fld)
    lib.zfp_stream_close(z)
    lib.stream_close(bs)
    assert n == 8 * ewords.size and np.array_equal(buf[: n // 8], ewords)
    out = np.zeros(BIG, dt)
    buf2 = np.concatenate([ewords, np.zeros(2, np.uint64)])
    z, bs = open_expert(buf2)
    fld = ref._field(out)
    assert lib.zfp_decompress(z, fld)
    lib.zfp_field_free(fld)
    lib.zfp_stream_close(z)
    lib.stream_close(bs)
    assert tp.same(out, tv.emu_decompress(varemu, ewords, eL, BIG, dt))


# ---------------------------------------------------------------------------
# Argument checks without a device

def test_argument_errors(libs):
    """Every argument error of cuzfp_hip_decode_region_variable, in the new entry,
    and the target mode's: a status, with pointers that are never dereferenced."""
    lib = cz.library()
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: rejected before any launch
    big = 1 << 30
    ib16 = lib.cuzfp_hip_variable_index_bytes(3, 16, 16, 16)

    def call(stream=buf, nbytes=big, lengths=buf, index=buf, index_bytes=None, t=3, n=(16, 16, 16), maxprec=16,
             minexp=-1074, o=(0, 0, 0), e=(4, 4, 4), out=buf):
        if index_bytes is None:
            index_bytes = lib.cuzfp_hip_variable_index_bytes(3, *n) or ib16
        return lib.cuzfp_hip_decode_region_variable_coarse(stream, nbytes, lengths, index, index_bytes, t, n[0], n[1],
                                                           n[2], maxprec, minexp, o[0], o[1], o[2], e[0], e[1], e[2],
                                                           0, 0, 0, out, None)

    # the target mode: maxprec in 1 .. the type's precision
    assert call(maxprec=0) == 1
    assert call(maxprec=33) == 1
    assert call(t=4, maxprec=65) == 1
    assert call(maxprec=2 ** 32 - 1) == 1
    # an empty box
    assert call(e=(0, 4, 4)) == 1
    assert call(e=(4, 0, 4)) == 1
    assert call(e=(4, 4, 0)) == 1
    # a box that leaves the array (also by wrap-around of origin + extent)
    assert call(o=(13, 0, 0)) == 1
    assert call(o=(0, 16, 0), e=(4, 1, 4)) == 1
    assert call(o=(0, 0, 1), e=(4, 4, 16)) == 1
    assert call(o=(8, 0, 0), e=(2 ** 32 - 4, 4, 4)) == 1
    # an origin or extent for an unused dimension
    assert call(n=(16, 16, 0), o=(0, 0, 1), e=(4, 4, 0)) == 1
    assert call(n=(16, 16, 0), o=(0, 0, 0), e=(4, 4, 1)) == 1
    assert call(n=(16, 0, 0), o=(0, 1, 0), e=(4, 0, 0)) == 1
    assert call(n=(16, 0, 0), o=(0, 0, 0), e=(4, 1, 0)) == 1
    # null pointers
    assert call(stream=None) == 1
    assert call(lengths=None) == 1
    assert call(index=None) == 1
    assert call(out=None) == 1
    # misaligned index, stream and lengths
    assert call(index=ctypes.c_void_p(0x1004)) == 1
    assert call(stream=ctypes.c_void_p(0x1002)) == 1
    assert call(lengths=ctypes.c_void_p(0x1001)) == 1
    # short index_bytes
    assert call(index_bytes=ib16 - 1) == 1
    assert call(index_bytes=8) == 1
    assert call(n=(16, 16, 20), index_bytes=ib16) == 1
    # integer and unknown types (before the mode is looked at), bad dimensions
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2
    assert call(t=1, maxprec=0) == 2
    assert call(n=(16, 0, 16)) == 1
    assert call(n=(0, 0, 0)) == 1
    assert cz.library().cuzfp_hip_abi_version() == 1


def test_python_validation(libs):
    """The keywords' errors come before any tensor is looked at."""
    class NoStream:
        is_cuda = False

    ns = NoStream()
    shape = (16, 16, 16)

    def region(dtype=np.float32, origin=(0, 0, 0), extent=(4, 4, 4), shape=shape, **kw):
        return cz.decode_region_variable(ns, ns, ns, shape, dtype, origin, extent, **kw)

    def whole(dtype=np.float32, **kw):
        return cz.decode_variable(ns, ns, shape, dtype, **kw)

    for f in (region, whole):
        with pytest.raises(ValueError, match="precision and tolerance"):
            f(precision=16, tolerance=1e-3)
        for dtype, p in ((np.float32, 0), (np.float32, 33), (np.float32, -1), (np.float64, 0), (np.float64, 65)):
            with pytest.raises(cz.CodecError) as e:
                f(dtype=dtype, precision=p)
            assert e.value.status == 1
        for p in (7.5, 0.5):
            with pytest.raises(ValueError, match="whole number"):
                f(precision=p)
        for dtype in (np.int32, np.int64):
            for kw in ({"precision": 16}, {"tolerance": 1e-3}):
                with pytest.raises(cz.CodecError) as e:
                    f(dtype=dtype, **kw)
                assert e.value.status == 2
        # a valid target: the existing checks, unchanged (an integral float is a whole number of planes)
        for kw in ({"precision": 16}, {"precision": 32.0}, {"tolerance": 1e-3}, {"tolerance": 0.0}):
            with pytest.raises(ValueError, match="device"):
                f(**kw)
        with pytest.raises(ValueError, match="device"):
            f(dtype=np.float64, precision=64)
    with pytest.raises(ValueError, match="rank"):
        region(origin=(0, 0), precision=16)
    with pytest.raises(ValueError, match="positive"):
        region(extent=(4, 0, 4), tolerance=1.0)
    with pytest.raises(ValueError):
        region(shape=(16,) * 4, origin=(0,) * 4, extent=(4,) * 4, precision=16)
    # decode_variable(index=, precision=) takes the region path, the whole array as the box; without an index
    # it builds one first
    with pytest.raises(ValueError, match="decode_region_variable.*device"):
        whole(index=ns, precision=16)
    with pytest.raises(ValueError, match="variable_index.*device"):
        whole(precision=16)
