"""The variable-rate coders on hard blocks, at every precision, on streams no
encoder wrote and on arrays larger than one scan tile: the corpus and the
checks that need no GPU (the kernels go through the same corpus in
tests/test_variable_paths_gpu.py).

The fixture tests/golden/variable_paths.npz holds, for every case of `cases()`,
what the reference's own library (CPU zfp 0.5.0) gives: the SHA-256 of
``zfp_compress``'s stream, the SHA-256 of the uint16 block lengths, the total
bit count and the SHA-256 of ``zfp_decompress``'s array -- hashes only.
tests/golden/make_variable_golden.py writes it from `generate()` below;
`test_fixture_is_current` regenerates it in memory whenever the reference
library is there.  The bytes themselves come from the host emulation
(tests/native/variable_emulate.cpp), accepted only on those hashes (`ref_of`).

The cases:

    zoo{d}, rag{d}   tests/block_zoo.py's 256-block zoo and its ragged zoo rotated
                     by one (NaN, inf, denormals, -0.0, single-element and huge
                     blocks; a zero lane in a dense wave), at every precision of
                     the type and at TOLERANCES
    tiles2d          (131, 259): 33 x 65 = 2145 blocks, three scan tiles of 1024,
                     partial blocks on both far edges
    scan1d           263 205 blocks (float32): 258 scan tiles, so the scan of the
                     tile sums takes a second trip of 256, with a ragged tile and
                     a ragged wave after it
    zeros*           all-zero arrays of 1, 63, 64, 65, 128 and 4160 blocks (1D)
                     and of 128 blocks (3D): a wave of 64 one-bit blocks is one
                     stream word exactly
    three            64 zero blocks, 64 dense blocks, 64 zero blocks

A block of a variable-rate stream is a fixed-rate block at maxbits = its
length, so the oracle's restatement of the fixed-rate decoder, applied to
every block alone, is a second decoder reference; `test_random_streams_two_references`
shows that it and the emulation agree on arbitrary bits at arbitrary lengths,
which is what the GPU tests of such streams lean on.

The `test_reach_*` tests state, from the reference's lengths alone, that the
inputs get where the GPU tests need them.
"""
import os
import zlib

import numpy as np
import pytest

import block_zoo as bz
import test_variable as tv
from test_variable import varemu  # noqa: F401  (fixture)

FIXTURE = os.path.join(tv.ROOT, "tests", "golden", "variable_paths.npz")
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
TOLERANCES = (0.0, 1e-320, 1e-40, 1e-12, 1e-3, 1.0, 1e10, 1e38)
SCAN_TILE = 1024  # kScanTile of csrc/variable_kernels.hpp
SCAN_TRIP = 256  # tile sums a trip of variable_scan_partials (kScanThreads)
# 256 * 1024 + 1024 + 37 blocks, the last one partial: the least that gives the scan of the tile sums a second
# trip and leaves a whole tile, a ragged tile and a ragged wave behind it
SCAN1D_BLOCKS = SCAN_TRIP * SCAN_TILE + SCAN_TILE + 37
SCAN1D_SHAPE = (4 * SCAN1D_BLOCKS - 2,)
TILES2D_SHAPE = (131, 259)
ZERO_BLOCKS_1D = (1, 63, 64, 65, 128, 4096 + 64)
ZEROS3D_SHAPE = (8, 16, 64)  # 2 x 4 x 16 = 128 blocks
SEEDS = {"tiles2d": 7, "scan1d": 11}


def type_prec(dt):
    return np.dtype(dt).itemsize * 8


def ebits(dt):
    return {4: 8, 8: 11}[np.dtype(dt).itemsize]


# ---------------------------------------------------------------------------
# Arrays

def _runs(shape, dtype, seed, cross=None):
    """test_variable's values with runs of all-zero blocks of several lengths
    (one of them a whole wave, one across block `cross`) and blocks of random
    bit patterns scattered by block index: lengths from 1 to near the type's
    longest all along the array."""
    rng = np.random.default_rng(seed)
    a = tv._values(rng, shape, dtype)
    ids = tv.block_ids(shape)
    nb = tv.nblocks(shape)
    zero = np.zeros(nb, bool)
    nruns = max(6, nb // 700)
    for s, n in zip(rng.integers(0, nb, nruns), rng.choice([1, 2, 3, 7, 63, 64, 65, 130, 200], nruns)):
        zero[s: s + n] = True
    wave = int(rng.integers(1, nb // 64 - 1))
    zero[64 * wave - 3: 64 * wave + 64 + 5] = True  # a whole wave and a little on either side
    if cross is not None:
        zero[cross - 37: cross + 100] = True
    dense = rng.choice(nb, max(4, nb // 97), replace=False)
    dense = dense[~zero[dense]]
    a[zero[ids]] = 0
    m = np.isin(ids, dense)
    a[m] = tv._random_bits(rng, int(m.sum()), dtype)
    assert np.isfinite(a).all()
    return a


_ARRAYS = {}


def array(name, dtype):
    """The input of a case by name: made once, read only."""
    dtype = np.dtype(dtype)
    key = (name, dtype.str)
    if key not in _ARRAYS:
        if name.startswith("zoo"):
            a = bz.zoo(int(name[3:]), dtype)[0]
        elif name.startswith("rag"):
            d = int(name[3:])
            a = bz.zoo(d, dtype, shape=bz.RAGGED[d], rotate=1)[0]
        elif name == "tiles2d":
            a = _runs(TILES2D_SHAPE, dtype, SEEDS[name])
        elif name == "scan1d":
            a = _runs(SCAN1D_SHAPE, dtype, SEEDS[name], cross=SCAN_TRIP * SCAN_TILE)
        elif name == "zeros3d":
            a = np.zeros(ZEROS3D_SHAPE, dtype)
        elif name.startswith("zeros"):
            a = np.zeros((4 * int(name[5:]),), dtype)
        elif name == "three":
            rng = np.random.default_rng(zlib.crc32(repr(("three", dtype.str)).encode()))
            a = np.zeros(4 * 192, dtype)
            a[256:512] = tv._random_bits(rng, 256, dtype)
        else:
            raise ValueError(name)
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        _ARRAYS[key] = a
    return _ARRAYS[key]


# ---------------------------------------------------------------------------
# Cases: (array name, dtype, mode, parameter), mode "p" (precision) or "a" (accuracy)

def zoo_modes(dtype):
    return [("p", p) for p in range(1, type_prec(dtype) + 1)] + [("a", t) for t in TOLERANCES]


ZOO_NAMES = tuple(f"{kind}{d}" for d in (1, 2, 3) for kind in ("zoo", "rag"))
ZERO_ARRAYS = tuple((f"zeros{n}", F32) for n in ZERO_BLOCKS_1D) + (("zeros3d", F64),)
PAIR = (("p", 16), ("a", 1e-3))
# (name, dtype) -> modes of the arrays beside the zoo
OTHERS = {("tiles2d", F32): PAIR, ("tiles2d", F64): PAIR,
          ("scan1d", F32): (("p", 32), ("a", 1e-3)),
          ("three", F32): (("p", 32), ("a", 1e-3)), ("three", F64): (("p", 64), ("a", 1e-3))}
OTHERS.update({k: PAIR for k in ZERO_ARRAYS})


def groups():
    """(name, dtype, modes) of every array of the corpus."""
    out = [(name, dt, tuple(zoo_modes(dt))) for name in ZOO_NAMES for dt in (F32, F64)]
    return out + [(name, dt, modes) for (name, dt), modes in OTHERS.items()]


def cases():
    return [(name, dt, mode, par) for name, dt, modes in groups() for mode, par in modes]


def case_id(case):
    name, dt, mode, par = case
    return f"{name}-{np.dtype(dt).name}-{mode}{par:g}"


def group_id(g):
    return f"{g[0]}-{np.dtype(g[1]).name}"


def tv_case(case):
    """The case in test_variable's form (shape first)."""
    return (array(case[0], case[1]).shape,) + tuple(case[1:])


def kw(case):
    return {"precision": case[3]} if case[2] == "p" else {"tolerance": case[3]}


def column_words(dims, dtype, maxprec):
    """variable_column_words of csrc/variable_kernels.hpp: the words of a
    column of the encoder's image, the longest block of the mode (1D: of the
    type)."""
    if dims == 1:
        maxprec = type_prec(dtype)
    bits = 1 + ebits(dtype) + 4 ** dims - 1 + 4 ** dims * maxprec
    return (bits + 63) // 64


# ---------------------------------------------------------------------------
# Fixture

KEYS = ("names", "nbits", "stream_sha", "lengths_sha", "decoded_sha")


def generate(reference):
    """The fixture's arrays, from the reference's library."""
    ref = tv.RefVariable(reference)
    names, nbits, ssha, lsha, dsha = [], [], [], [], []
    for case in cases():
        a = array(case[0], case[1])
        c = tv_case(case)
        s = ref.compress(a, c)
        L = ref.lengths(a, c)
        total = int(L.astype(np.uint64).sum())
        assert (total + 63) // 64 == s.size, (case_id(case), total, s.size)
        names.append(case_id(case))
        nbits.append(total)
        ssha.append(tv.sha(s))
        lsha.append(tv.sha(L))
        dsha.append(tv.sha(ref.decompress(s, c)))
    return {"names": np.array(names), "nbits": np.array(nbits, np.uint64), "stream_sha": np.stack(ssha),
            "lengths_sha": np.stack(lsha), "decoded_sha": np.stack(dsha)}


class Golden:
    def __init__(self, d):
        self.d = {k: d[k] for k in KEYS}
        self.index = {str(n): i for i, n in enumerate(self.d["names"])}

    def get(self, case):
        i = self.index[case_id(case)]
        return {k: self.d[k][i] for k in KEYS[1:]}


_GOLDEN = []


def load_golden():
    if not _GOLDEN:
        with np.load(FIXTURE) as z:
            _GOLDEN.append(Golden(z))
    return _GOLDEN[0]


@pytest.fixture(scope="module")
def golden():
    return load_golden()


_REF = {}


def ref_of(varemu, golden, case):  # noqa: F811
    """(words, lengths, nbits, decoded) of the reference for a case: the host
    emulation's, accepted only on the fixture's hashes; computed once, read
    only."""
    key = case_id(case)
    if key not in _REF:
        g = golden.get(case)
        a = array(case[0], case[1])
        words, L, total = tv.emu_compress(varemu, a, *tv.mode_params(tv_case(case)))
        assert total == int(g["nbits"]), key
        assert np.array_equal(tv.sha(L), g["lengths_sha"]), key
        assert np.array_equal(tv.sha(words), g["stream_sha"]), key
        d = tv.emu_decompress(varemu, words, L, a.shape, a.dtype)
        assert np.array_equal(tv.sha(d), g["decoded_sha"]), key
        for v in (words, L, d):
            v.setflags(write=False)
        _REF[key] = (words, L, total, d)
    return _REF[key]


def want_index(L):
    """index[t] = sum of lengths[0 .. 64 t), index[T] = the total, in uint64."""
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(L.astype(np.uint64), dtype=np.uint64)])
    return np.concatenate([c[:-1][::64], c[-1:]])


# ---------------------------------------------------------------------------
# Streams no encoder wrote

DENSITIES = (0.5, 0.05, 0.95)
RANDOM_SHAPES = {"aligned": bz.SHAPES, "ragged": bz.RAGGED}


def random_stream(dims, dtype, kind, density, illegal=False):
    """(words, lengths) of a stream of arbitrary bits for RANDOM_SHAPES[kind][dims]:
    lengths from {1} and [ebits + 2, top], about a tenth of them 1, with top,
    ebits + 2 and 1 forced present.  `illegal` replaces an eighth of the others
    by lengths no encoder writes: 2 .. ebits + 1 and top + 1 .. 65535, the four
    ends included.  The stream holds the sum of the raw lengths."""
    dtype = np.dtype(dtype)
    shape = RANDOM_SHAPES[kind][dims]
    n = bz.nblocks(shape)
    rng = np.random.default_rng(zlib.crc32(repr(("random", dims, dtype.str, kind, density, illegal)).encode()))
    lo, hi = ebits(dtype) + 2, bz.top(dims, dtype)
    L = rng.integers(lo, hi + 1, size=n)
    L[rng.random(n) < 0.1] = 1
    order = rng.permutation(n)
    L[order[:3]] = (hi, lo, 1)
    if illegal:
        bad = order[3: 3 + n // 8]
        L[bad[::2]] = rng.integers(2, lo, size=bad[::2].size)
        L[bad[1::2]] = rng.integers(hi + 1, 65536, size=bad[1::2].size)
        L[bad[:4]] = (2, hi + 1, lo - 1, 65535)
    total = int(L.sum())
    words = bz.random_stream(rng, 1, total, density)
    return words, L.astype(np.uint16)


def restatement_decode(restatement, words, L, shape, dtype):
    """Every block decoded alone by the oracle's fixed-rate restatement at
    maxbits = its length, pasted in raster order and cropped to `shape`.  A
    one-bit block is the format's zero block whatever the bit (zfp writes it
    only for one; its decoder then reads nothing more), and fixed rate has no
    maxbits that low, so the restatement is not asked.  Lengths no encoder
    writes follow the decoders' documented rule (zfp_decode_variable_body):
    2 .. ebits + 1 is a zero block too, a length above the type's longest block
    decodes as the longest, and the next block starts after the raw length."""
    dims = len(shape)
    lo, hi = ebits(dtype) + 2, bz.top(dims, dtype)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    off = np.concatenate([[0], np.cumsum(L.astype(np.int64))])
    blocks = []
    for b in range(L.size):
        n = min(int(L[b]), hi)
        if n < lo:
            blocks.append(np.zeros((4,) * dims, dtype))
            continue
        chunk = np.zeros((n + 63) // 64 * 64, np.uint8)
        chunk[:n] = bits[off[b]: off[b] + n]
        w = np.packbits(chunk, bitorder="little").view(np.uint64)
        blocks.append(restatement.decompress(w, (4,) * dims, dtype, n))
    a = bz.assemble(blocks, tuple((s + 3) // 4 for s in shape))
    return np.ascontiguousarray(a[tuple(slice(0, s) for s in shape)])


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------------------
# Tests

def test_case_count():
    c = cases()
    assert len(c) == 696 and len({case_id(x) for x in c}) == 696
    assert sum(1 for x in c if x[0] in ZOO_NAMES) == 2 * 3 * (32 + 64 + 2 * len(TOLERANCES))


@pytest.mark.parametrize("group", groups(), ids=group_id)
def test_emulation_matches_fixture(varemu, golden, group):  # noqa: F811
    """Lengths, stream and decoded array of the host emulation are the
    reference library's, non-finite blocks included (`ref_of` asserts the
    hashes)."""
    name, dt, modes = group
    for mode, par in modes:
        words, L, total, d = ref_of(varemu, golden, (name, dt, mode, par))
        assert L.size == tv.nblocks(array(name, dt).shape) and words.size == (total + 63) // 64
        assert d.shape == array(name, dt).shape


def test_fixture_is_current(reference, golden):
    """The committed fixture is what the reference's library gives today."""
    fresh = generate(reference)
    for k, v in fresh.items():
        assert np.array_equal(v, golden.d[k]), k


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_random_streams_two_references(varemu, restatement, dims, dtype):  # noqa: F811
    """Arbitrary bits at arbitrary legal lengths: every block decoded alone by
    the restatement of the fixed-rate decoder at maxbits = its length equals
    the emulation of the variable-rate decoder, byte for byte; and with
    illegal lengths among them, under the documented rule for those."""
    for kind in RANDOM_SHAPES:
        shape = RANDOM_SHAPES[kind][dims]
        for density in DENSITIES:
            for illegal in (False, True):
                words, L = random_stream(dims, dtype, kind, density, illegal)
                a = restatement_decode(restatement, words, L, shape, dtype)
                b = tv.emu_decompress(varemu, words, L, shape, dtype)
                assert same(a, b), (kind, density, illegal)


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_reach_random_streams(dims, dtype):
    """The drawn lengths: the longest and the shortest coded block and the
    one-bit block are there, about a tenth are one bit; the illegal variant
    has both kinds with their ends and keeps the legal ends."""
    lo, hi = ebits(dtype) + 2, bz.top(dims, dtype)
    for kind in RANDOM_SHAPES:
        n = bz.nblocks(RANDOM_SHAPES[kind][dims])
        for density in DENSITIES:
            words, L = random_stream(dims, dtype, kind, density)
            assert L.size == n and words.size == (int(L.astype(np.int64).sum()) + 63) // 64
            assert ((L == 1) | ((L >= lo) & (L <= hi))).all()
            assert {1, lo, hi} <= set(L.tolist())
            assert 0.04 * n < (L == 1).sum() < 0.2 * n
            assert len(set((np.cumsum(L.astype(np.int64)) % 32).tolist())) > 24  # the dword phases of an offset
            ones = np.unpackbits(words.view(np.uint8)).mean()
            assert abs(ones - density) < 0.02
            words, L = random_stream(dims, dtype, kind, density, illegal=True)
            short, long_ = (L >= 2) & (L < lo), L > hi
            assert {2, lo - 1} <= set(L[short].tolist()) and {hi + 1, 65535} <= set(L[long_].tolist())
            assert short.sum() >= n // 20 and long_.sum() >= n // 20
            assert {1, lo, hi} <= set(L.tolist())
            assert words.size * 64 >= int(L.astype(np.int64).sum())


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_reach_zoo(varemu, golden, dims, dtype):  # noqa: F811
    """What the zoo sweep is there for, from the reference's lengths."""
    prec = type_prec(dtype)
    # the encoder's column height takes every value up to the type's over the precision sweep
    W = [column_words(dims, dtype, p) for p in range(1, prec + 1)]
    top_words = (bz.top(dims, dtype) + 63) // 64
    if dims == 1:
        assert set(W) == {top_words}
    else:
        assert set(W) == set(range(column_words(dims, dtype, 1), top_words + 1)) and len(set(W)) > 1
    name = f"zoo{dims}"
    classes = np.array(bz.zoo(dims, dtype)[1])
    assert (classes[:64] == "zero").all() and set(classes[128:192]) == set(bz.FLOAT_CLASSES)
    rows_seen = set()
    for mode, par in zoo_modes(dtype):
        L = ref_of(varemu, golden, (name, dtype, mode, par))[1].astype(np.int64)
        assert (L[:64] == 1).all()  # the zero wave: one word
        maxprec = par if mode == "p" else prec
        assert L.max() <= 1 + ebits(dtype) + 4 ** dims - 1 + 4 ** dims * maxprec
        for w in range(4):
            wmax = int(L[64 * w: 64 * w + 64].max())
            cw = column_words(dims, dtype, maxprec)
            rows_seen.add(cw if dims == 1 else min(cw, (wmax + 63) // 64))
        if (mode, par) in (("p", prec), ("a", 0.0)):
            # lanes of one wave stop in different rows of the image: every class, and dense with a zero lane
            for w in (2, 3):
                lw = L[64 * w: 64 * w + 64]
                assert lw.max() - lw.min() > 64, (mode, par, w)
            assert L[192 + bz.ZERO_LANE] == 1 and L[192:256].max() > 0.85 * 4 ** dims * prec
            assert L.max() > 0.95 * bz.top(dims, dtype)  # a lane that fills its column
        if mode == "a" and par >= 1e10:
            # p == 0 on non-zero data: one bit a block, whatever it holds, unless its exponent passes the tolerance
            big = np.isin(classes, ("huge", "nan_block", "nan_zeros", "noise_inf", "noise_nan_ninf"))
            assert (L[~big] == 1).all() and (classes[~big] == "noise").sum() > 64
    # `rows` of zfp_encode_variable (before the slack): 1D columns are always whole; in 2D and 3D every value from
    # one word to the longest block there is (no block of real values reaches the worst case of a 3D column)
    if dims == 1:
        assert rows_seen == {top_words}
    else:
        assert rows_seen == set(range(1, max(rows_seen) + 1)) and max(rows_seen) >= top_words - 2
    # the ragged zoo rotated by one: a partial last wave, the classes in wave 1, the zero lane in wave 2
    rag = np.array(bz.zoo(dims, dtype, shape=bz.RAGGED[dims], rotate=1)[1])
    assert rag.size % 64 and set(rag[64:128]) == set(bz.FLOAT_CLASSES) and rag[128 + bz.ZERO_LANE - 1] == "zero"
    L = ref_of(varemu, golden, (f"rag{dims}", dtype, "p", prec))[1]
    assert L[128 + bz.ZERO_LANE - 1] == 1 and (L[192:] == 1).all()


def _wave_edges(L):
    """Per wave: its first bit offset, its end offset, whether it holds a coded block."""
    c = np.concatenate([[0], np.cumsum(L.astype(np.int64))])
    nw = (L.size + 63) // 64
    start = c[:-1][::64]
    end = c[np.minimum(64 * (np.arange(nw) + 1), L.size)]
    coded = np.array([(L[64 * w: 64 * w + 64] > 1).any() for w in range(nw)])
    return start, end, coded


def test_reach_tiles(varemu, golden):  # noqa: F811
    """tiles2d: three scan tiles; scan1d: more than SCAN_TRIP tiles, a ragged
    tile and wave, a zero run across the trip edge, an all-zero wave, lengths
    from 1 to near the longest on either side of the edge, and coded waves
    whose segment starts, and ends, on a word boundary."""
    a = array("tiles2d", F32)
    assert a.shape[0] % 4 and a.shape[1] % 4 and tv.nblocks(a.shape) == 33 * 65
    assert (tv.nblocks(a.shape) + SCAN_TILE - 1) // SCAN_TILE == 3
    for dt in (F32, F64):
        for mode, par in PAIR:
            L = ref_of(varemu, golden, ("tiles2d", dt, mode, par))[1]
            assert L.min() == 1 and (L[SCAN_TILE:2 * SCAN_TILE] > 1).any() and (L[2 * SCAN_TILE:] > 1).any()
            assert any((L[64 * w: 64 * w + 64] == 1).all() for w in range(L.size // 64))
    nb = tv.nblocks(SCAN1D_SHAPE)
    edge = SCAN_TRIP * SCAN_TILE
    assert nb == SCAN1D_BLOCKS and SCAN1D_SHAPE[0] % 4
    ntiles = (nb + SCAN_TILE - 1) // SCAN_TILE
    assert ntiles == 258 > SCAN_TRIP and nb % SCAN_TILE and nb % 64
    for mode, par in OTHERS[("scan1d", F32)]:
        L = ref_of(varemu, golden, ("scan1d", F32, mode, par))[1]
        assert (L[edge - 30: edge + 90] == 1).all()  # a run of zero blocks across the second trip's first tile
        for part in (L[:edge], L[edge:]):
            assert part.min() == 1 and part.max() > (0.85 * 4 * 32 if mode == "p" else 64)
        start, end, coded = _wave_edges(L)
        assert (~coded).any()
        assert (coded & (start % 64 == 0))[1:].any(), "no coded wave starts a word"
        assert (coded & (end % 64 == 0)).any(), "no coded wave ends a word"
        assert (coded & (start % 64 != 0) & (end % 64 != 0)).any()
        assert int(end[-1]) > 2 ** 24


def test_reach_word_boundaries(varemu, golden):  # noqa: F811
    """All-zero arrays: 64 k blocks are k whole words, every segment aligned at
    both ends; 63 and 65 blocks leave the last word open or shared.  The
    three-wave array: the dense wave starts on a word."""
    for name, dt in ZERO_ARRAYS:
        nb = tv.nblocks(array(name, dt).shape)
        for mode, par in PAIR:
            words, L, total, _ = ref_of(varemu, golden, (name, dt, mode, par))
            assert (L == 1).all() and total == nb and not words.any()
            start, end, _ = _wave_edges(L)
            if nb % 64 == 0:
                assert (start % 64 == 0).all() and (end % 64 == 0).all() and words.size == nb // 64
            else:
                assert end[-1] % 64 != 0
    assert sorted(tv.nblocks(array(n, d).shape) for n, d in ZERO_ARRAYS) == [1, 63, 64, 65, 128, 128, 4160]
    for dt in (F32, F64):
        for mode, par in OTHERS[("three", dt)]:
            L = ref_of(varemu, golden, ("three", dt, mode, par))[1]
            start, end, coded = _wave_edges(L)
            assert coded.tolist() == [False, True, False] and start[1] == 64 and end[2] - start[2] == 64
            assert (L[64:128] > 64).all() if mode == "p" else (L[64:128] > 1).sum() > 48
