"""The variable-rate kernels on the corpus of tests/test_variable_paths.py:
the block zoo at every precision and a ladder of tolerances, streams of
arbitrary bits at arbitrary lengths, arrays of several scan tiles and of more
than 256, and arrays whose wave segments start and end on stream words.

Reference data is the host emulation's, accepted only when its SHA-256 equal
the fixture's (test_variable_paths.ref_of), so they are CPU zfp 0.5.0's bytes;
for the streams no encoder wrote, the references are the emulation and the
oracle's restatement of the fixed-rate decoder applied to every block alone
(tests/test_variable_paths.py shows the two agree).  Every comparison is of
bytes.  Every `out` the encoder gets is filled with all-ones words first: the
encoder ORs into the words two waves share, so a missed clear or a stray OR
shows; the words after the stream must still hold the fill.

What each test's inputs reach is asserted from the reference's lengths in
tests/test_variable_paths.py (`test_reach_*`), without a GPU.
"""
import numpy as np
import pytest

import test_variable as tv
import test_variable_paths as tp
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_paths import F32, F64, golden  # noqa: F401  (fixture)
from test_variable_gpu import CANARY, _dev, _lengths, _tdtype, _words
from test_variable_region_gpu import _box, boxes

pytestmark = pytest.mark.gpu

FILL = -1  # all-ones words


def _same(t, want):
    return tp.same(t.cpu().numpy(), want)


def _check_encode(x, case, ref):
    """encode_variable into an all-ones `out` of the worst-case size: the bit
    count, the lengths, the stream's words, and the fill after them."""
    import torch
    import cuzfp_amd
    maxprec = tv.mode_params(tp.tv_case(case))[0]
    full = cuzfp_amd.variable_maximum_size(tuple(x.shape), case[1], maxprec) // 8
    nwords = ref[0].size
    assert full >= nwords
    buf = torch.full((full,), FILL, dtype=torch.int64, device=x.device)
    words, lengths, nbits = cuzfp_amd.encode_variable(x, out=buf, **tp.kw(case))
    cid = tp.case_id(case)
    assert nbits == ref[2], cid
    assert np.array_equal(_lengths(lengths), ref[1]), cid
    assert words.data_ptr() == buf.data_ptr() and np.array_equal(_words(words), ref[0]), cid
    assert bool((buf[nwords:] == FILL).all()), cid


def _check_decode(cuda, case, ref, box, own_index=True):
    """The reference's stream through decode_variable with the scan, with the
    index of variable_index (itself against numpy's), and one box of it."""
    import cuzfp_amd
    words, L, _, want = ref
    td = _tdtype(case[1])
    shape = want.shape
    cid = tp.case_id(case)
    w, l = _dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda)
    assert _same(cuzfp_amd.decode_variable(w, l, shape, td), want), cid
    idx = cuzfp_amd.variable_index(l, shape, td)
    assert np.array_equal(idx.cpu().numpy().view(np.uint64), tp.want_index(L)), cid
    assert _same(cuzfp_amd.decode_variable(w, l, shape, td, index=idx), want), cid
    origin, extent = box
    got = cuzfp_amd.decode_region_variable(w, l, idx, shape, td, origin, extent)
    assert _same(got, want[_box(origin, extent)]), (cid, box)


def _interior(shape):
    """An interior box unaligned on every axis (test_variable_region_gpu.boxes)."""
    origin, extent = boxes(tuple(shape))[2]
    assert all(o % 4 and (o + e) % 4 and o + e < s for o, e, s in zip(origin, extent, shape)), (shape, origin, extent)
    return origin, extent


# ---------------------------------------------------------------------------
# 2.1 the zoo at every precision and on the tolerance ladder

@pytest.mark.parametrize("group", [g for g in tp.groups() if g[0] in tp.ZOO_NAMES], ids=tp.group_id)
def test_zoo(cuda, varemu, golden, group):  # noqa: F811
    """NaN, inf, denormal, -0.0, single-element and huge blocks, a zero lane in
    a dense wave: every mode's stream, lengths and count are the reference's,
    and the reference's stream decodes to the reference's array (NaN payloads
    as bytes) by the scan, by the index and as a box.  test_reach_zoo: the
    column height W takes every value, lanes of a wave stop in different
    rows, whole waves are one word."""
    name, dt, modes = group
    a = tp.array(name, dt)
    x = _dev(a, cuda)
    box = _interior(a.shape)
    for mode, par in modes:
        case = (name, dt, mode, par)
        ref = tp.ref_of(varemu, golden, case)
        _check_encode(x, case, ref)
        _check_decode(cuda, case, ref, box)


# ---------------------------------------------------------------------------
# 2.2 streams of arbitrary bits with arbitrary lengths

_RANDOM = {}


def _random_ref(varemu, restatement, dims, dtype, kind, density, illegal):  # noqa: F811
    """(words, lengths, expected array): the emulation's decode, which must equal
    the per-block restatement decode (for illegal lengths under the documented
    rule, test_variable_paths.restatement_decode); made once."""
    key = (dims, np.dtype(dtype).str, kind, density, illegal)
    if key not in _RANDOM:
        shape = tp.RANDOM_SHAPES[kind][dims]
        words, L = tp.random_stream(dims, dtype, kind, density, illegal)
        want = tv.emu_decompress(varemu, words, L, shape, dtype)
        assert tp.same(want, tp.restatement_decode(restatement, words, L, shape, dtype))
        for v in (words, L, want):
            v.setflags(write=False)
        _RANDOM[key] = (words, L, want)
    return _RANDOM[key]


@pytest.mark.parametrize("kind", list(tp.RANDOM_SHAPES))
@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_random_streams(cuda, varemu, restatement, dims, dtype, kind):  # noqa: F811
    """Bits no encoder wrote (plane steps cut mid-group at any length, exponent
    fields of every value) at lengths 1, ebits + 2 .. the type's longest:
    decode_variable, and decode_region_variable with numpy's index on the
    whole array and on an unaligned box, equal the per-block restatement
    decode and the emulation."""
    import cuzfp_amd
    shape = tp.RANDOM_SHAPES[kind][dims]
    td = _tdtype(dtype)
    origin, extent = _interior(shape)
    zero = (0,) * dims
    for density in tp.DENSITIES:
        words, L, want = _random_ref(varemu, restatement, dims, dtype, kind, density, False)
        w, l = _dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda)
        idx = _dev(tp.want_index(L).view(np.int64), cuda)
        assert _same(cuzfp_amd.decode_variable(w, l, shape, td), want), density
        assert _same(cuzfp_amd.decode_region_variable(w, l, idx, shape, td, zero, shape), want), density
        got = cuzfp_amd.decode_region_variable(w, l, idx, shape, td, origin, extent)
        assert _same(got, want[_box(origin, extent)]), density


@pytest.mark.parametrize("kind", list(tp.RANDOM_SHAPES))
@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_random_streams_illegal_lengths(cuda, varemu, restatement, dims, dtype, kind):  # noqa: F811
    """The same with an eighth of the lengths in 2 .. ebits + 1 (a zero block)
    and above the type's longest block (clamped), offsets advancing by the raw
    lengths: the decoded values are the emulation's, the canaries after the
    stream and around a strided `out` are intact, the stream is unchanged."""
    import torch
    import cuzfp_amd
    shape = tp.RANDOM_SHAPES[kind][dims]
    td = _tdtype(dtype)
    origin, extent = _interior(shape)
    canary = int(np.uint64(CANARY).astype(np.int64))
    inner = tuple(slice(1, 2 * s + 1, 2) for s in shape)
    for density in tp.DENSITIES:
        words, L, want = _random_ref(varemu, restatement, dims, dtype, kind, density, True)
        buf = torch.full((words.size + 64,), canary, dtype=torch.int64, device=cuda)
        buf[: words.size] = _dev(words.view(np.int64), cuda)
        w, l = buf[: words.size], _dev(L.view(np.int16), cuda)
        idx = _dev(tp.want_index(L).view(np.int64), cuda)
        big = torch.full(tuple(2 * s + 1 for s in shape), -7.0, dtype=td, device=cuda)
        cuzfp_amd.decode_variable(w, l, shape, td, out=big[inner])
        assert _same(big[inner], want), density
        outer = big.clone()
        outer[inner] = -7.0
        assert bool((outer == -7.0).all()), density
        big.fill_(-7.0)
        cuzfp_amd.decode_region_variable(w, l, idx, shape, td, (0,) * dims, shape, out=big[inner])
        assert _same(big[inner], want), density
        outer = big.clone()
        outer[inner] = -7.0
        assert bool((outer == -7.0).all()), density
        got = cuzfp_amd.decode_region_variable(w, l, idx, shape, td, origin, extent)
        assert _same(got, want[_box(origin, extent)]), density
        assert bool((buf[words.size:] == canary).all())
        assert np.array_equal(_words(buf[: words.size]), words)


# ---------------------------------------------------------------------------
# 2.3 more than one scan tile, more than 256 tiles

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_three_scan_tiles(cuda, varemu, golden, dtype):  # noqa: F811
    """(131, 259), 2145 blocks: the offsets of the second and third scan tile
    reach the coders (test_reach_tiles)."""
    a = tp.array("tiles2d", dtype)
    x = _dev(a, cuda)
    for mode, par in tp.OTHERS[("tiles2d", dtype)]:
        case = ("tiles2d", dtype, mode, par)
        ref = tp.ref_of(varemu, golden, case)
        _check_encode(x, case, ref)
        _check_decode(cuda, case, ref, _interior(a.shape))


def test_second_scan_trip(cuda, varemu, golden):  # noqa: F811
    """263 205 blocks in 1D: variable_scan_partials takes a second trip, with a
    ragged tile and a ragged wave after it; the box straddles block 262 144
    (test_reach_tiles: a zero run across it, coded waves that start and end
    on stream words)."""
    a = tp.array("scan1d", F32)
    x = _dev(a, cuda)
    edge = 4 * tp.SCAN_TRIP * tp.SCAN_TILE
    box = ((edge - 301,), (703,))
    for mode, par in tp.OTHERS[("scan1d", F32)]:
        case = ("scan1d", F32, mode, par)
        ref = tp.ref_of(varemu, golden, case)
        _check_encode(x, case, ref)
        _check_decode(cuda, case, ref, box)


# ---------------------------------------------------------------------------
# 2.4 segments on word boundaries by construction

@pytest.mark.parametrize("name,dtype", list(tp.ZERO_ARRAYS) + [("three", F32), ("three", F64)],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_word_boundaries(cuda, varemu, golden, name, dtype):  # noqa: F811
    """All-zero arrays (a wave of 64 one-bit blocks is one word: sh0 == 0, the
    segment closed at its end, the total a multiple of 64 or one off it) and
    zero / dense / zero waves, into all-ones words (test_reach_word_boundaries)."""
    a = tp.array(name, dtype)
    x = _dev(a, cuda)
    n = a.shape[-1]
    box = tuple((0,) * (a.ndim - 1)) + (min(1, n - 1),), tuple(a.shape[:-1]) + (max(1, n - 2),)
    for mode, par in tp.OTHERS[(name, dtype)]:
        case = (name, dtype, mode, par)
        ref = tp.ref_of(varemu, golden, case)
        _check_encode(x, case, ref)
        _check_decode(cuda, case, ref, box)
