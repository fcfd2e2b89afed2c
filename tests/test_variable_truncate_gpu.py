"""truncate_variable on the GPU: a variable-rate stream cut to a coarser mode,
against the reference's own stream, lengths and bit count at that mode (the
corpus and the references of tests/test_variable_truncate.py: CPU zfp 0.5.0's
bytes, through the host emulation accepted only on the fixtures' hashes).

The `zeros*` arrays and `tiles2d` have no p = full case in the fixture, so their
source is the emulation's p = full stream, which no committed hash vouches for;
what is asserted is the result, against the fixture's modes through `ref_of`
(a wrong source could not cut to the hashed target).

Every comparison is of bytes.  Every `out` is filled with all-ones words first:
the copy pass ORs into the words two waves share, so a missed clear or a stray
OR shows, and the words after the stream must still hold the fill.
"""
import ctypes

import numpy as np
import pytest

import block_zoo as bz
import test_variable as tv
import test_variable_paths as tp
import test_variable_truncate as tt
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_gpu import CANARY, _dev, _lengths, _tdtype, _words
from test_variable_gpu import ref_of as tv_ref_of
from test_variable_paths import F32, F64
from test_variable_paths_gpu import _same
from test_variable_region_gpu import _box
from test_variable_truncate import tp_golden, tv_golden, vtrunc  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = -1  # all-ones words
BIG = (13, 22, 38)  # the largest test_variable shape: 240 blocks, ragged waves, partial blocks
ICANARY = int(np.uint64(CANARY).astype(np.int64))


def from_kw(mode):
    return {"from_precision": mode[1]} if mode[0] == "p" else {"from_tolerance": mode[1]}


def to_kw(mode):
    return {"precision": mode[1]} if mode[0] == "p" else {"tolerance": mode[1]}


class Source:
    """A reference stream on the device, uploaded once."""

    def __init__(self, cuda, ref, shape, dt, mode):
        self.words, self.L = ref[0], ref[1]
        self.w = _dev(self.words.view(np.int64), cuda)
        self.l = _dev(self.L.view(np.int16), cuda)
        self.shape, self.dt, self.mode = tuple(shape), np.dtype(dt), mode

    def cut(self, mode, **kw):
        import cuzfp_amd
        return cuzfp_amd.truncate_variable(self.w, self.l, self.shape, _tdtype(self.dt), **from_kw(self.mode),
                                           **to_kw(mode), **kw)


def check_cut(src, mode, ref, cid=None):
    """The cut into an all-ones `out` of the worst-case size: the bit count, the
    lengths, the stream's words, and the fill after them.  Returns the result."""
    import torch
    import cuzfp_amd
    maxprec = tt.mode_of(src.dt, *mode)[0]
    full = cuzfp_amd.variable_maximum_size(src.shape, src.dt, maxprec) // 8
    nwords = ref[0].size
    assert full >= nwords
    buf = torch.full((full,), FILL, dtype=torch.int64, device=src.w.device)
    words, lengths, nbits = src.cut(mode, out=buf)
    cid = cid or (src.mode, mode)
    assert nbits == ref[2], cid
    assert np.array_equal(_lengths(lengths), ref[1]), cid
    assert words.data_ptr() == buf.data_ptr() and np.array_equal(_words(words), ref[0]), cid
    assert bool((buf[nwords:] == FILL).all()), cid
    return words, lengths, nbits


# ---------------------------------------------------------------------------
# The fixture cases of test_variable

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_fixture_cases(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """13 x 22 x 38: p = full to every mode of the case list (itself included:
    the identity), a1e-3 -> a0.05, a1, a64 and p16 -> p7, p1: words, lengths
    and bit count are the reference's at the target mode."""
    modes = [c[2:] for c in tv.cases() if c[0] == BIG and c[1] == dtype]
    cuts = [(tt.full(dtype), modes), (("a", 1e-3), [("a", 0.05), ("a", 1.0), ("a", 64.0)]),
            (("p", 16), [("p", 7), ("p", 1)])]
    for src_mode, targets in cuts:
        src = Source(cuda, tv_ref_of(varemu, tv_golden, (BIG, dtype) + src_mode), BIG, dtype, src_mode)
        for mode in targets:
            assert tt.coarsens(tt.mode_of(dtype, *src_mode), tt.mode_of(dtype, *mode))
            check_cut(src, mode, tv_ref_of(varemu, tv_golden, (BIG, dtype) + mode))


@pytest.mark.parametrize("case", [(BIG, np.dtype(dt)) + m for dt in (np.float32, np.float64)
                                  for m in (("p", 16), ("a", 1e-3), ("a", 0.0))], ids=tv.case_id)
def test_identity(cuda, varemu, tv_golden, case):  # noqa: F811
    """The same mode in and out gives the same bytes."""
    ref = tv_ref_of(varemu, tv_golden, case)
    check_cut(Source(cuda, ref, case[0], case[1], case[2:]), case[2:], ref)


# ---------------------------------------------------------------------------
# The zoo

@pytest.mark.parametrize("group", [g for g in tp.groups() if g[0] in tp.ZOO_NAMES], ids=tp.group_id)
def test_zoo(cuda, varemu, tp_golden, group):  # noqa: F811
    """256 blocks with NaN, inf, denormal, single-element and huge blocks and a
    zero lane in a dense wave: p = full to every precision and every tolerance
    of the ladder (1e38: every finite block becomes one bit)."""
    name, dt, modes = group
    a = tp.array(name, dt)
    src_mode = tt.full(dt)
    src = Source(cuda, tp.ref_of(varemu, tp_golden, (name, dt) + src_mode), a.shape, dt, src_mode)
    for mode in modes:
        case = (name, dt) + mode
        check_cut(src, mode, tp.ref_of(varemu, tp_golden, case), tp.case_id(case))


# ---------------------------------------------------------------------------
# Word and wave edges, scan tiles

EDGES = [(f"zeros{n}", F32) for n in (63, 64, 65, 128)] + [("zeros3d", F64), ("three", F32), ("three", F64),
                                                            ("tiles2d", F32), ("tiles2d", F64)]


@pytest.mark.parametrize("name,dtype", EDGES, ids=lambda v: v if isinstance(v, str) else v.name)
def test_word_and_wave_edges(cuda, varemu, tp_golden, name, dtype):  # noqa: F811
    """All-zero arrays (a wave of 64 one-bit blocks is exactly one word; 63 and
    65 blocks leave the last word open or shared), zero / dense / zero waves,
    and three scan tiles.  The zero arrays and tiles2d have no p = full fixture
    case: their source is the emulation's p = full stream, the targets the
    fixture's modes."""
    a = tp.array(name, dtype)
    src_mode = tt.full(dtype)
    if src_mode in tp.OTHERS[(name, dtype)]:
        ref = tp.ref_of(varemu, tp_golden, (name, dtype) + src_mode)
    else:
        words, L, total = tv.emu_compress(varemu, a, tp.type_prec(dtype), tv.ZFP_MIN_EXP)
        ref = (words, L, total)
    src = Source(cuda, ref, a.shape, dtype, src_mode)
    for mode in tp.OTHERS[(name, dtype)]:
        case = (name, dtype) + mode
        check_cut(src, mode, tp.ref_of(varemu, tp_golden, case), tp.case_id(case))


def test_second_scan_trip(cuda, varemu, tp_golden):  # noqa: F811
    """263 205 blocks in 1D, p32 -> a1e-3: both scans take a second trip, with a
    ragged tile and a ragged wave after it.  One call."""
    a = tp.array("scan1d", F32)
    src = Source(cuda, tp.ref_of(varemu, tp_golden, ("scan1d", F32, "p", 32)), a.shape, F32, ("p", 32))
    check_cut(src, ("a", 1e-3), tp.ref_of(varemu, tp_golden, ("scan1d", F32, "a", 1e-3)))


# ---------------------------------------------------------------------------
# Composition, round trip

def test_composition(cuda, varemu, tv_golden, tp_golden):  # noqa: F811
    """p64 -> p32 -> p16 equals p16: on the zoo (where p32 is a fixture mode
    too) and on 13 x 22 x 38."""
    import cuzfp_amd
    import torch
    a = tp.array("zoo3", F64)
    src = Source(cuda, tp.ref_of(varemu, tp_golden, ("zoo3", F64, "p", 64)), a.shape, F64, ("p", 64))
    w32, l32, _ = check_cut(src, ("p", 32), tp.ref_of(varemu, tp_golden, ("zoo3", F64, "p", 32)))
    ref16 = tp.ref_of(varemu, tp_golden, ("zoo3", F64, "p", 16))
    w16, l16, n16 = cuzfp_amd.truncate_variable(w32, l32, a.shape, torch.float64, from_precision=32,
                                                precision=16)
    assert n16 == ref16[2] and np.array_equal(_lengths(l16), ref16[1]) and np.array_equal(_words(w16), ref16[0])
    src = Source(cuda, tv_ref_of(varemu, tv_golden, (BIG, F64, "p", 64)), BIG, F64, ("p", 64))
    w32, l32, _ = src.cut(("p", 32))
    ref16 = tv_ref_of(varemu, tv_golden, (BIG, F64, "p", 16))
    w16, l16, n16 = cuzfp_amd.truncate_variable(w32, l32, BIG, torch.float64, from_precision=32, precision=16)
    assert n16 == ref16[2] and np.array_equal(_lengths(l16), ref16[1]) and np.array_equal(_words(w16), ref16[0])


@pytest.mark.parametrize("case", [(BIG, np.dtype(dt)) + m for dt in (np.float32, np.float64)
                                  for m in (("p", 7), ("a", 1e-3), ("a", 64.0))], ids=tv.case_id)
def test_round_trip(cuda, varemu, tv_golden, case):  # noqa: F811
    """The result feeds the decoders unchanged: decode_variable gives the target
    case's decoded array (the fixture's decoded_sha), and variable_index plus
    decode_region_variable of an interior box agrees with it."""
    import cuzfp_amd
    shape, dt = case[0], case[1]
    td = _tdtype(dt)
    src_mode = tt.full(dt)
    src = Source(cuda, tv_ref_of(varemu, tv_golden, (shape, dt) + src_mode), shape, dt, src_mode)
    words, lengths, nbits = src.cut(case[2:])
    ref = tv_ref_of(varemu, tv_golden, case)
    got = cuzfp_amd.decode_variable(words, lengths, shape, td)
    assert np.array_equal(tv.sha(got.cpu().numpy()), tv_golden.get(case)["decoded_sha"])
    assert _same(got, ref[3])
    idx = cuzfp_amd.variable_index(lengths, shape, td)
    assert np.array_equal(idx.cpu().numpy().view(np.uint64), tp.want_index(ref[1]))
    origin, extent = (1, 2, 3), (10, 17, 30)  # interior, unaligned at both ends on every axis
    assert all(o % 4 and (o + e) % 4 and o + e < n for o, e, n in zip(origin, extent, shape))
    box = cuzfp_amd.decode_region_variable(words, lengths, idx, shape, td, origin, extent)
    assert _same(box, ref[3][_box(origin, extent)])


# ---------------------------------------------------------------------------
# Capacity, tail, size query, streams

@pytest.mark.parametrize("case", [(BIG, np.dtype(dt)) + m for dt in (np.float32, np.float64)
                                  for m in (("p", 16), ("a", 1e-3))], ids=tv.case_id)
def test_capacity_and_tail(cuda, varemu, tv_golden, case):  # noqa: F811
    """`out` one word too short: nothing at or past the capacity changes, the
    lengths and the bit count are still right.  A long `out`: the words after
    the stream keep their canary.  size_only: the lengths and the count of the
    full call, no stream."""
    import torch
    shape, dt = case[0], case[1]
    src_mode = tt.full(dt)
    src = Source(cuda, tv_ref_of(varemu, tv_golden, (shape, dt) + src_mode), shape, dt, src_mode)
    ref = tv_ref_of(varemu, tv_golden, case)
    nwords = ref[0].size
    buf = torch.full((nwords + 8,), ICANARY, dtype=torch.int64, device=cuda)
    words, lengths, nbits = src.cut(case[2:], out=buf[: nwords - 1])
    assert nbits == ref[2] and np.array_equal(_lengths(lengths), ref[1])
    assert words.numel() == nwords - 1
    assert bool((buf[nwords - 1:] == ICANARY).all())
    buf = torch.full((nwords + 100,), ICANARY, dtype=torch.int64, device=cuda)
    words, lengths, nbits = src.cut(case[2:], out=buf)
    assert nbits == ref[2] and np.array_equal(_lengths(lengths), ref[1]) and np.array_equal(_words(words), ref[0])
    assert bool((buf[nwords:] == ICANARY).all())
    none, l2, n2 = src.cut(case[2:], size_only=True)
    assert none is None and n2 == nbits and np.array_equal(_lengths(l2), ref[1])


def test_non_default_stream(cuda, varemu, tv_golden):  # noqa: F811
    """On a stream of its own; the source stream and the source lengths are
    unchanged afterwards."""
    import torch
    src = Source(cuda, tv_ref_of(varemu, tv_golden, (BIG, F32, "p", 32)), BIG, F32, ("p", 32))
    ref = tv_ref_of(varemu, tv_golden, (BIG, F32, "a", 1e-3))
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    words, lengths, nbits = src.cut(("a", 1e-3), stream=s)
    s.synchronize()
    assert nbits == ref[2] and np.array_equal(_lengths(lengths), ref[1]) and np.array_equal(_words(words), ref[0])
    assert np.array_equal(_words(src.w), src.words) and np.array_equal(_lengths(src.l), src.L)


# ---------------------------------------------------------------------------
# Streams no encoder wrote, an index that is not the stream's

class Raw:
    """The C-ABI on buffers with canaries on both sides of every output."""
    PAD = 64

    def __init__(self, cuda, words, L, shape, dt, cap_words):
        import torch
        import cuzfp_amd
        self.lib = cuzfp_amd.library()
        self.t = tv.TC[np.dtype(dt)]
        self.ext = cuzfp_amd._extents(shape)
        self.n = L.size
        self.w = _dev(np.ascontiguousarray(words).view(np.int64), cuda)
        self.l = _dev(np.ascontiguousarray(L).view(np.int16), cuda)
        self.cap = cap_words
        self.dst = torch.full((cap_words + 2 * self.PAD,), ICANARY, dtype=torch.int64, device=cuda)
        self.len = torch.full((self.n + 2 * self.PAD,), 0x5A5A, dtype=torch.int16, device=cuda)
        self.total = torch.full((3,), ICANARY, dtype=torch.int64, device=cuda)
        self.need = self.lib.cuzfp_hip_truncate_variable_workspace_bytes(self.t, *self.ext)
        assert self.need >= 8 * (2 * self.n + 1)
        self.ws = torch.full((self.need // 8 + self.PAD,), ICANARY, dtype=torch.int64, device=cuda)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(self, src_mode, mode, **over):
        a = {"src": self.w.data_ptr(), "src_bytes": self.w.numel() * 8, "src_len": self.l.data_ptr(), "t": self.t,
             "dst": self.dst[self.PAD:].data_ptr(), "cap": self.cap * 8, "len": self.len[self.PAD:].data_ptr(),
             "total": self.total[1:].data_ptr(), "ws": self.ws.data_ptr(), "ws_bytes": self.need}
        a.update(over)
        return self.lib.cuzfp_hip_truncate_variable(a["src"], a["src_bytes"], a["src_len"], a["t"], *self.ext,
                                                    src_mode[0], src_mode[1], mode[0], mode[1], a["dst"], a["cap"],
                                                    a["len"], a["total"], a["ws"], a["ws_bytes"], self.st)

    def canaries_intact(self):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        return (bool((self.dst[:P] == ICANARY).all()) and bool((self.dst[P + self.cap:] == ICANARY).all()) and
                bool((self.len[:P] == 0x5A5A).all()) and bool((self.len[P + self.n:] == 0x5A5A).all()) and
                int(self.total[0]) == ICANARY and int(self.total[2]) == ICANARY and
                bool((self.ws[self.need // 8:] == ICANARY).all()))

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return (bool((self.dst == ICANARY).all()) and bool((self.len == 0x5A5A).all()) and
                bool((self.total == ICANARY).all()))

    def result(self):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        L = self.len[P: P + self.n].cpu().numpy().view(np.uint16)
        return self.dst[P: P + self.cap].cpu().numpy().view(np.uint64), L, int(self.total[1])


def _valid_case_is_exact(cuda, varemu, tv_golden):  # noqa: F811
    src = Source(cuda, tv_ref_of(varemu, tv_golden, (BIG, F64, "p", 64)), BIG, F64, ("p", 64))
    check_cut(src, ("a", 1e-3), tv_ref_of(varemu, tv_golden, (BIG, F64, "a", 1e-3)))


def test_index_of_all_ones(cuda, varemu, tv_golden):  # noqa: F811
    """Source lengths of 65535 throughout: every length is clamped to the type's
    longest block and every stream load is behind the stream_bytes bound, so
    nothing can fault by construction.  Success; the canaries around `out`, the
    lengths, the count and the workspace are intact; every new length is at
    most the clamped source length and the total is their sum; the source is
    unchanged; a valid case run afterwards is exact."""
    shape = (9, 20, 36)
    words, L, _, _ = tv_ref_of(varemu, tv_golden, (shape, F64, "p", 64))
    top = bz.top(3, F64)
    bad = np.full(L.size, 0xFFFF, np.uint16)
    for mode in ((64, -1074), (64, -10)):
        raw = Raw(cuda, words, bad, shape, F64, (L.size * top + 63) // 64 + 1)
        assert raw.call((64, -1074), mode) == 0
        assert raw.canaries_intact()
        _, newL, total = raw.result()
        assert (newL.astype(np.int64) <= top).all() and total == int(newL.astype(np.int64).sum())
        assert np.array_equal(_words(raw.w), words) and (_lengths(raw.l) == 0xFFFF).all()
    _valid_case_is_exact(cuda, varemu, tv_golden)


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_random_streams(cuda, varemu, vtrunc, tv_golden, dims, dtype):  # noqa: F811
    """Arbitrary bits at arbitrary lengths.  With legal lengths the new lengths
    are the host walk's (the same function on the host) and the stream is the
    numpy cut at those lengths.  With lengths no encoder writes among them
    (2 .. ebits + 1, above the longest block up to 65535): success, canaries
    intact, every new length at most the clamped source length, the total
    their sum.  A valid case run afterwards is exact."""
    top = bz.top(dims, dtype)
    prec = tp.type_prec(dtype)
    shape = tp.RANDOM_SHAPES["ragged"][dims]
    for density in tp.DENSITIES:
        words, L = tp.random_stream(dims, dtype, "ragged", density, illegal=False)
        for mode in ((prec, -1074), (7, -1074), (prec, -10)):
            raw = Raw(cuda, words, L, shape, dtype, words.size + 1)
            assert raw.call((prec, -1074), mode) == 0
            assert raw.canaries_intact()
            got, newL, total = raw.result()
            wantL = tt.emu_lengths(vtrunc, words, L, dims, dtype, mode)
            assert np.array_equal(newL, wantL), (density, mode)
            want = tt.cut(words, L, wantL)
            assert total == int(wantL.astype(np.int64).sum()) and np.array_equal(got[: want.size], want), (density, mode)
            assert (got[want.size:] == np.uint64(CANARY)).all(), (density, mode)
        words, L = tp.random_stream(dims, dtype, "ragged", density, illegal=True)
        clamped = np.minimum(L.astype(np.int64), top)
        for mode in ((prec, -1074), (prec, -10)):
            raw = Raw(cuda, words, L, shape, dtype, (int(clamped.sum()) + 63) // 64 + 1)
            assert raw.call((prec, -1074), mode) == 0
            assert raw.canaries_intact()
            _, newL, total = raw.result()
            assert (newL.astype(np.int64) <= clamped).all() and total == int(newL.astype(np.int64).sum()), density
            assert np.array_equal(_words(raw.w), words) and np.array_equal(_lengths(raw.l), L)
    _valid_case_is_exact(cuda, varemu, tv_golden)


# ---------------------------------------------------------------------------
# Arguments

def test_argument_errors(cuda, varemu, tv_golden):  # noqa: F811
    import torch
    import cuzfp_amd
    shape = (6, 5, 9)
    words, L, _, _ = tv_ref_of(varemu, tv_golden, (shape, F32, "p", 16))
    w, l = _dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda)

    def cut(**kw):
        return cuzfp_amd.truncate_variable(w, l, shape, torch.float32, **kw)

    # widening in either component, with a message in the spirit of truncate's
    for kw in ({"from_precision": 16, "precision": 17}, {"from_tolerance": 1e-3, "tolerance": 1e-4},
               {"from_precision": 16, "tolerance": 1e-3}, {"from_tolerance": 1e-3, "precision": 32},
               {"from_tolerance": 1e-3, "tolerance": 0.0}):
        with pytest.raises(ValueError, match="widening is not supported"):
            cut(**kw)
    # both or neither of a pair
    for kw in ({"precision": 7}, {"from_precision": 16}, {}, {"from_precision": 16, "from_tolerance": 1.0, "precision": 7},
               {"from_precision": 16, "precision": 7, "tolerance": 1.0}):
        with pytest.raises(ValueError, match="exactly one"):
            cut(**kw)
    for kw in ({"from_precision": 16, "precision": 7.9}, {"from_precision": 16.5, "precision": 7}):
        with pytest.raises(ValueError, match="whole number"):
            cut(**kw)
    with pytest.raises(cuzfp_amd.CodecError) as e:
        cuzfp_amd.truncate_variable(w, l, shape, torch.int32, from_precision=16, precision=7)
    assert e.value.status == 2
    for kw in ({"from_precision": 16, "precision": 0}, {"from_precision": 33, "precision": 7},
               {"from_precision": 0, "precision": 0}):
        with pytest.raises(cuzfp_amd.CodecError) as e:
            cut(**kw)
        assert e.value.status == 1
    got = cut(from_precision=16, precision=7)
    ref = tv_ref_of(varemu, tv_golden, (shape, F32, "p", 7))
    assert got[2] == ref[2] and np.array_equal(_words(got[0]), ref[0])

    # the C-ABI itself: every refusal comes before any launch (the outputs keep their canaries)
    raw = Raw(cuda, words, L, shape, F32, words.size + 4)
    src, ok = (16, -1074), (7, -1074)
    assert raw.call(src, (17, -1074)) == 1 and raw.call((32, -10), (32, -11)) == 1  # widening
    assert raw.call(src, (32, -10)) == 1
    assert raw.call(src, ok, t=1) == 2 and raw.call(src, ok, t=2) == 2  # integer types
    assert raw.call((0, -1074), (0, -1074)) == 1 and raw.call((33, -1074), ok) == 1 and raw.call(src, (0, -1074)) == 1
    assert raw.call((32, -1074), (33, -1074)) == 1
    assert raw.call(src, ok, ws_bytes=raw.need - 1) == 1  # a workspace one byte short
    assert raw.call(src, ok, dst=raw.w.data_ptr(), cap=8) == 1  # overlapping source and destination
    assert raw.call(src, ok, dst=raw.w.data_ptr() + 8 * (words.size - 1), cap=16) == 1
    assert raw.call(src, ok, len=raw.l.data_ptr()) == 1  # aliased lengths
    assert raw.call(src, ok, len=raw.l.data_ptr() + 2 * (L.size - 1)) == 1
    for name in ("src", "src_len", "len", "total", "ws"):  # null pointers
        assert raw.call(src, ok, **{name: None}) == 1, name
    assert raw.call(src, ok, dst=None) == 1  # no destination, yet a capacity
    for name, by in (("src", 2), ("src_len", 1), ("len", 1), ("dst", 4), ("total", 4), ("ws", 4)):  # misaligned
        a = {"src": raw.w, "src_len": raw.l, "len": raw.len, "dst": raw.dst, "total": raw.total, "ws": raw.ws}[name]
        assert raw.call(src, ok, **{name: a.data_ptr() + by}) == 1, name
    assert raw.lib.cuzfp_hip_truncate_variable_workspace_bytes(1, 9, 5, 6) == 0
    assert raw.untouched()
    # ... and the same buffers with nothing wrong: the size query, then the cut
    assert raw.call(src, ok, dst=None, cap=0) == 0
    assert raw.canaries_intact()
    _, newL, total = raw.result()
    assert total == ref[2] and np.array_equal(newL, ref[1]) and bool((raw.dst == ICANARY).all())
    assert raw.call(src, ok) == 0
    assert raw.canaries_intact()
    got, newL, total = raw.result()
    assert total == ref[2] and np.array_equal(newL, ref[1]) and np.array_equal(got[: ref[0].size], ref[0])
    assert (got[ref[0].size:] == np.uint64(CANARY)).all()
