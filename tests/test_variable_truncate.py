"""truncate_variable without a GPU: the embedded property on the reference's
own streams, and the per-lane function that finds a block's new length
(cuzfp_amd/csrc/rerate_variable.hpp) on the host (the kernels go through the
same corpus in tests/test_variable_truncate_gpu.py).

A mode is (maxprec, minexp).  A stream at (maxprec, minexp) can be cut to
(maxprec', minexp') when maxprec' <= maxprec and minexp' >= minexp: every
block of the coarser stream is then the first L' bits of the finer stream's
block, or -- when the coarser mode codes no plane of it -- the single bit 0.

Every expectation is the reference's: the streams and lengths of
test_variable / test_variable_paths' fixtures (CPU zfp 0.5.0), which the host
emulation reproduces and `ref_of` accepts only on the committed hashes.  The
corpus:

    test_variable's arrays   five shapes, both types: p = full -> every mode of
                             the case list, a1e-3 -> a0.05, p16 -> p7
    zoo{d}, rag{d}           the block zoo (NaN, inf, denormal blocks), both
                             types: p = full -> every precision and TOLERANCES
    three                    zero, dense, zero waves: p = full -> a1e-3
    tiles2d                  three scan tiles.  Its fixture modes are p16 and
                             a1e-3, neither a cut of the other, so the source
                             is the emulation's p = full stream (no fixture
                             hash of its own); what is asserted is the result,
                             against the fixture's p16 and a1e-3.

tests/native/variable_truncate_emulate.cpp runs truncated_block_length, the
function every lane of the lengths pass runs, over a host copy of the stream.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import block_zoo as bz
import test_variable as tv
import test_variable_paths as tp
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_gpu import ref_of as tv_ref_of  # (a helper: needs no GPU)
from test_variable_paths import F32, F64

SRC = os.path.join(tv.ROOT, "tests", "native", "variable_truncate_emulate.cpp")
HDRS = [os.path.join(tv.ROOT, "cuzfp_amd", "csrc", h) for h in ("rerate_variable.hpp", "zfp_block.hpp")]
LIB = os.path.join(tv.ROOT, "build", "libcuzfp_vtrunc.so")


@pytest.fixture(scope="module")
def vtrunc():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.check_call(["/opt/rocm/llvm/bin/clang++", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-Wno-unknown-pragmas", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    u, i, vp, sz = ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.vtrunc_lengths.restype = i
    lib.vtrunc_lengths.argtypes = [i, i, vp, sz, vp, sz, u, i, vp]
    lib.vtrunc_coarsens.restype = i
    lib.vtrunc_coarsens.argtypes = [u, i, u, i]
    return lib


@pytest.fixture(scope="module")
def tv_golden():
    return tv.load_golden()


@pytest.fixture(scope="module")
def tp_golden():
    return tp.load_golden()


# ---------------------------------------------------------------------------
# The rule and the numpy bit model

def mode_of(dtype, mode, par):
    """(maxprec, minexp) of a precision ("p") or a tolerance ("a")."""
    return tv.mode_params((None, np.dtype(dtype), mode, par))


def coarsens(src, dst):
    """The rule: the mode `dst` is a cut of the mode `src`."""
    return dst[0] <= src[0] and dst[1] >= src[1]


def cut_lengths_ok(L, newL, dtype):
    """What every cut satisfies: a new block is one bit or a prefix of a coded block."""
    L, newL = L.astype(np.int64), newL.astype(np.int64)
    return bool(((newL == 1) | ((newL <= L) & (newL >= tp.ebits(dtype) + 2))).all())


def cut(words, L, newL):
    """The stream `words` with block lengths L cut to the lengths newL: a block
    of one bit becomes the single bit 0, any other the first newL[b] bits of
    source block b; packed back to back, zero padded to a 64-bit word."""
    L, newL = L.astype(np.int64), newL.astype(np.int64)
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
    off = np.cumsum(L) - L
    noff = np.cumsum(newL) - newL
    keep = np.where(newL > 1, newL, 0)
    assert (keep <= L).all()
    start = np.cumsum(keep) - keep
    within = np.arange(int(keep.sum()), dtype=np.int64) - np.repeat(start, keep)
    out = np.zeros((int(newL.sum()) + 63) // 64 * 64, np.uint8)
    out[np.repeat(noff, keep) + within] = bits[np.repeat(off, keep) + within]
    return np.packbits(out, bitorder="little").view(np.uint64)


def emu_lengths(lib, words, L, dims, dtype, mode):
    """truncated_block_length of every block, on the host."""
    words = np.ascontiguousarray(words, np.uint64)
    L = np.ascontiguousarray(L, np.uint16)
    out = np.full(L.size, 0xDEAD, np.uint16)
    assert lib.vtrunc_lengths(tv.TC[np.dtype(dtype)], dims, words.ctypes.data, words.size, L.ctypes.data, L.size,
                              mode[0], mode[1], out.ctypes.data)
    return out


# ---------------------------------------------------------------------------
# Corpus: groups of (id, dtype, dims, source, [(label, target mode, target ref)]), refs being
# (words, lengths, nbits, ...) of a reference

def full(dtype):
    return ("p", tp.type_prec(dtype))


TV_PAIRS = ((("a", 1e-3), (("a", 0.05),)), (("p", 16), (("p", 7),)))  # the pairs beside p = full -> every mode
TV_GROUPS = [(shape, np.dtype(dt)) for shape in tv.SHAPES for dt in (np.float32, np.float64)]
TP_GROUPS = [(name, dt) for name in tp.ZOO_NAMES for dt in (F32, F64)] + \
            [("three", F32), ("three", F64), ("tiles2d", F32), ("tiles2d", F64)]


def tv_cuts(shape, dt):
    """[(source case, [target cases])] of a test_variable array."""
    modes = [c[2:] for c in tv.cases() if c[0] == shape and c[1] == dt]
    out = [((shape, dt) + full(dt), [(shape, dt) + m for m in modes])]
    for src, dsts in TV_PAIRS:
        out.append(((shape, dt) + src, [(shape, dt) + d for d in dsts]))
    return out


_TILES_FULL = {}


def tiles_full(varemu, dt):  # noqa: F811
    """The emulation's p = full stream of tiles2d (no fixture case: see the module's docstring)."""
    key = np.dtype(dt).str
    if key not in _TILES_FULL:
        words, L, total = tv.emu_compress(varemu, tp.array("tiles2d", dt), tp.type_prec(dt), tv.ZFP_MIN_EXP)
        for v in (words, L):
            v.setflags(write=False)
        _TILES_FULL[key] = (words, L, total)
    return _TILES_FULL[key]


def tp_cuts(varemu, golden, name, dt):  # noqa: F811
    """[(source mode, source ref, [(target case, target ref)])] of a test_variable_paths array."""
    if name == "tiles2d":
        src = tiles_full(varemu, dt)
        modes = tp.OTHERS[(name, dt)]
    else:
        src = tp.ref_of(varemu, golden, (name, dt) + full(dt))
        modes = tp.zoo_modes(dt) if name in tp.ZOO_NAMES else tp.OTHERS[(name, dt)]
    return [(full(dt), src, [((name, dt) + m, tp.ref_of(varemu, golden, (name, dt) + m)) for m in modes])]


def tv_id(g):
    return f"{'x'.join(map(str, g[0]))}-{g[1].name}"


def tp_id(g):
    return f"{g[0]}-{np.dtype(g[1]).name}"


# ---------------------------------------------------------------------------
# Tests

def _check_cut(vtrunc, src, dst, dims, dt, mode, cid, stats):
    words, L = src[0], src[1]
    want_words, want_L, want_bits = dst[0], dst[1], dst[2]
    # the property: the reference's coarser stream is the cut of its finer one
    assert cut_lengths_ok(L, want_L, dt), cid
    got = cut(words, L, want_L)
    assert int(want_L.astype(np.int64).sum()) == want_bits and np.array_equal(got, want_words), cid
    # the per-lane function finds the reference's lengths from the finer stream alone
    assert np.array_equal(emu_lengths(vtrunc, words, L, dims, dt, mode), want_L), cid
    stats["one_bit"] += int(((L > 1) & (want_L == 1)).sum())
    stats["same"] += int(((L > 1) & (want_L == L)).sum())
    stats["shorter"] += int(((want_L > 1) & (want_L < L)).sum())
    stats["pairs"] += 1


@pytest.mark.parametrize("group", TV_GROUPS, ids=tv_id)
def test_cut_fixture_arrays(varemu, vtrunc, tv_golden, group):  # noqa: F811
    """test_variable's arrays: p = full to every mode of the case list, a1e-3 ->
    a0.05 and p16 -> p7.  The reference's coarser stream is the cut of its finer
    one, and truncated_block_length gives the reference's lengths.  The corpus
    reaches what it is for: a coded block that becomes one bit (the 1e-30 block
    under a tolerance), one that stays whole, one that gets shorter."""
    shape, dt = group
    stats = {"one_bit": 0, "same": 0, "shorter": 0, "pairs": 0}
    for src_case, dst_cases in tv_cuts(shape, dt):
        src = tv_ref_of(varemu, tv_golden, src_case)
        for case in dst_cases:
            assert coarsens(tv.mode_params(src_case), tv.mode_params(case))
            _check_cut(vtrunc, src, tv_ref_of(varemu, tv_golden, case), len(shape), dt, tv.mode_params(case),
                       (tv.case_id(src_case), tv.case_id(case)), stats)
    assert stats["one_bit"] >= 1 and stats["same"] >= 1 and stats["shorter"] >= 1, stats
    assert stats["pairs"] == 9 + 2  # every mode of the case list from p = full, and the two pairs beside them


@pytest.mark.parametrize("group", TP_GROUPS, ids=tp_id)
def test_cut_paths_arrays(varemu, vtrunc, tp_golden, group):  # noqa: F811
    """The zoo (every precision and tolerance from p = full; tolerance 1e38 makes
    every finite block one bit), `three` and `tiles2d`, the same way."""
    name, dt = group
    dims = tp.array(name, dt).ndim
    stats = {"one_bit": 0, "same": 0, "shorter": 0, "pairs": 0}
    for src_mode, src, dsts in tp_cuts(varemu, tp_golden, name, dt):
        for case, dst in dsts:
            mode = mode_of(dt, case[2], case[3])
            assert coarsens(mode_of(dt, *src_mode), mode)
            _check_cut(vtrunc, src, dst, dims, dt, mode, tp.case_id(case), stats)
            if name in tp.ZOO_NAMES and case[2:] == ("a", 1e38):
                classes = np.array(bz.zoo(dims, dt)[1]) if name.startswith("zoo") else None
                if classes is not None:
                    small = ~np.isin(classes, ("huge", "nan_block", "nan_zeros", "noise_inf", "noise_nan_ninf"))
                    assert (dst[1][small] == 1).all() and ((src[1] > 1) & small).sum() > 64
    assert stats["shorter"] >= 1, (tp_id(group), stats)
    # tiles2d is there for its three scan tiles.  Its only fixture modes are p16 and a1e-3: none of its coded
    # blocks lies below that tolerance, so no target takes one to one bit; and from p64 every coded block of the
    # float64 array gets shorter at both.  Those two are left to every other array of the corpus.
    assert stats["one_bit"] >= 1 or name == "tiles2d", (tp_id(group), stats)
    assert stats["same"] >= 1 or (name, dt) == ("tiles2d", F64), (tp_id(group), stats)
    # every fixture mode of the array was a target
    want_pairs = tp.type_prec(dt) + len(tp.TOLERANCES) if name in tp.ZOO_NAMES else len(tp.OTHERS[(name, dt)])
    assert stats["pairs"] == want_pairs, (tp_id(group), stats)


def test_rule(vtrunc):
    """variable_mode_coarsens, the C-ABI's widening test, is the rule."""
    modes = [(p, tv.ZFP_MIN_EXP) for p in (1, 7, 16, 32)] + [(32, tv.accuracy_to_minexp(t)) for t in (1e-3, 1.0, 64.0)]
    for a in modes:
        for b in modes:
            assert bool(vtrunc.vtrunc_coarsens(a[0], a[1], b[0], b[1])) == coarsens(a, b), (a, b)
    assert coarsens((32, -1074), (32, -10)) and not coarsens((32, -10), (32, -1074))
    assert coarsens((16, -1074), (7, -1074)) and not coarsens((7, -1074), (16, -1074))
    assert not coarsens((16, -1074), (32, -10))  # a precision stream cannot become a tolerance stream


RANDOM_TARGETS = (("p", 1), ("p", 7), ("p", None), ("a", 1e-3), ("a", 1.0), ("a", 1e38))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_arbitrary_bits_terminate_within_the_source(vtrunc, dims, dtype):
    """Streams no encoder wrote, with lengths no encoder writes among them: the
    walk ends, and a new length is 1 (0 for a source length of 0) or at most the
    source length clamped to the type's longest block; a source length no coded
    block can have gives the zero block."""
    lo, hi = tp.ebits(dtype) + 2, bz.top(dims, dtype)
    for kind in tp.RANDOM_SHAPES:
        for density in tp.DENSITIES:
            for illegal in (False, True):
                words, L = tp.random_stream(dims, dtype, kind, density, illegal)
                clamped = np.minimum(L.astype(np.int64), hi)
                for mode, par in RANDOM_TARGETS:
                    m = mode_of(dtype, mode, tp.type_prec(dtype) if par is None else par)
                    got = emu_lengths(vtrunc, words, L, dims, dtype, m).astype(np.int64)
                    assert (got <= clamped).all() and (got >= 1).all(), (kind, density, illegal, mode, par)
                    assert (got[clamped < lo] == 1).all()
                    assert ((got == 1) | (got >= lo)).all()
                    if par is None:
                        # every plane of the type: a block whose flag is set runs to the end of its code or its length
                        first = np.unpackbits(words.view(np.uint8), bitorder="little")[np.cumsum(L.astype(np.int64)) - L]
                        assert (got[(first == 0)] == 1).all()
    # a length of 0 reads nothing and gives nothing; all-ones words at the longest length: a walk of group tests
    z = emu_lengths(vtrunc, np.zeros(4, np.uint64), np.array([0, 5, 0, 40], np.uint16), dims, dtype, (1, -1074))
    assert z.tolist() == [0, 1, 0, 1]
    ones = np.full(80, ~np.uint64(0))
    got = emu_lengths(vtrunc, ones, np.array([0xFFFF], np.uint16), dims, dtype, (tp.type_prec(dtype), -1074))
    assert lo <= int(got[0]) <= hi
