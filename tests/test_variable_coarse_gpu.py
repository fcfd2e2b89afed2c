"""Decoding a variable-rate stream at a coarser mode on the GPU:
decode_region_variable / decode_variable with `precision=` or `tolerance=`
(cuzfp_hip_decode_region_variable_coarse) against the reference's own decode at
the target mode -- the corpus and the references of
tests/test_variable_coarse.py: CPU zfp 0.5.0's arrays, through the host
emulation accepted only on the fixtures' hashes.

The `zeros*` arrays and `tiles2d` have no p = full case in the fixture, so their
source is the emulation's p = full stream; what is asserted is the result,
against the fixture's modes.  Every comparison is of bytes; every `out` is
filled beforehand, so a block the kernel skipped shows.
"""
import ctypes

import numpy as np
import pytest

import test_variable as tv
import test_variable_coarse as tc
import test_variable_paths as tp
import test_variable_truncate as tt
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_coarse import BIG, vcoarse  # noqa: F401  (fixture)
from test_variable_gpu import CANARY, _dev, _tdtype
from test_variable_gpu import ref_of as tv_ref_of
from test_variable_paths import F32, F64
from test_variable_region_gpu import _box, _same
from test_variable_truncate import tp_golden, tv_golden  # noqa: F401  (fixtures)
from test_variable_truncate_gpu import from_kw, to_kw

pytestmark = pytest.mark.gpu

ICANARY = int(np.uint64(CANARY).astype(np.int64))
INTERIOR = ((1, 2, 3), (10, 17, 30))  # unaligned on every axis
ALIGNED = ((4, 8, 12), (8, 12, 24))  # whole blocks: the row stores


class Stream:
    """A stream on the device, uploaded once, with the index numpy gives."""

    def __init__(self, cuda, words, L, shape, dt):
        self.shape, self.dt, self.td = tuple(shape), np.dtype(dt), _tdtype(dt)
        self.w = _dev(np.ascontiguousarray(words).view(np.int64), cuda)
        self.l = _dev(np.ascontiguousarray(L).view(np.int16), cuda)
        self.idx = _dev(tp.want_index(L).view(np.int64), cuda)

    def box(self, origin, extent, mode, **kw):
        import cuzfp_amd
        return cuzfp_amd.decode_region_variable(self.w, self.l, self.idx, self.shape, self.td, origin, extent,
                                                **to_kw(mode), **kw)

    def whole(self, mode, **kw):
        import cuzfp_amd
        return cuzfp_amd.decode_variable(self.w, self.l, self.shape, self.td, index=self.idx, **to_kw(mode), **kw)


def check_target(src, mode, want, boxes=(), cid=None):
    cid = cid or (src.shape, src.dt.name, mode)
    got = src.whole(mode)
    assert tuple(got.shape) == src.shape and _same(got, want), cid
    for origin, extent in boxes:
        got = src.box(origin, extent, mode)
        assert tuple(got.shape) == tuple(extent) and _same(got, want[_box(origin, extent)]), (cid, origin, extent)


def rows_differ(L, dtype):
    """Some wave of 64 raster-consecutive blocks has coded blocks that end in
    different rows of the image."""
    rows = np.where(L > 1, (L.astype(np.int64) + 31) // 32, 0)
    for w in range(0, rows.size, 64):
        r = rows[w: w + 64]
        if np.unique(r[r > 0]).size > 1:
            return True
    return False


# ---------------------------------------------------------------------------
# The fixture cases of test_variable

def fixture_cuts(dtype):
    modes = [c[2:] for c in tv.cases() if c[0] == BIG and c[1] == dtype]
    return [(tt.full(dtype), modes), (("a", 1e-3), [("a", 0.05), ("a", 1.0), ("a", 64.0)]),
            (("p", 16), [("p", 7), ("p", 1)])]


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_fixture_cases(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """13 x 22 x 38, the reference's p = full stream at every mode of the case
    list (itself included), its a1e-3 stream at a0.05, a1, a64 and its p16
    stream at p7, p1: the whole array, an interior unaligned box and a
    block-aligned box are the reference's decode at the target mode."""
    for src_mode, targets in fixture_cuts(dtype):
        ref = tv_ref_of(varemu, tv_golden, (BIG, dtype) + src_mode)
        src = Stream(cuda, ref[0], ref[1], BIG, dtype)
        for mode in targets:
            assert tt.coarsens(tt.mode_of(dtype, *src_mode), tt.mode_of(dtype, *mode))
            check_target(src, mode, tv_ref_of(varemu, tv_golden, (BIG, dtype) + mode)[3], (INTERIOR, ALIGNED),
                         (src_mode, mode))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_fixture_cases_own_stream(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """The same from our own encoder's streams and variable_index's index."""
    import cuzfp_amd
    x = _dev(tv.array(BIG, dtype), cuda)
    td = _tdtype(dtype)
    for src_mode, targets in fixture_cuts(dtype):
        w, l, _ = cuzfp_amd.encode_variable(x, **to_kw(src_mode))
        idx = cuzfp_amd.variable_index(l, BIG, td)
        for mode in targets:
            want = tv_ref_of(varemu, tv_golden, (BIG, dtype) + mode)[3]
            got = cuzfp_amd.decode_variable(w, l, BIG, td, index=idx, **to_kw(mode))
            assert _same(got, want), (src_mode, mode)
            for origin, extent in (INTERIOR, ALIGNED):
                got = cuzfp_amd.decode_region_variable(w, l, idx, BIG, td, origin, extent, **to_kw(mode))
                assert _same(got, want[_box(origin, extent)]), (src_mode, mode, origin)


# ---------------------------------------------------------------------------
# The zoo

@pytest.mark.parametrize("group", [g for g in tp.groups() if g[0] in tp.ZOO_NAMES], ids=tp.group_id)
def test_zoo(cuda, varemu, tp_golden, group):  # noqa: F811
    """NaN, inf, denormal, single-element and huge blocks and a zero lane in a
    dense wave: p = full at every precision (the image takes every height) and
    every tolerance of the ladder (1e38: every finite block is one bit)."""
    name, dt, modes = group
    a = tp.array(name, dt)
    ref = tp.ref_of(varemu, tp_golden, (name, dt) + tt.full(dt))
    src = Stream(cuda, ref[0], ref[1], a.shape, dt)
    assert len(modes) == tp.type_prec(dt) + len(tp.TOLERANCES)
    ragged = 0
    for mode in modes:
        case = (name, dt) + mode
        want = tp.ref_of(varemu, tp_golden, case)
        check_target(src, mode, want[3], cid=tp.case_id(case))
        ragged += rows_differ(want[1], dt)
    assert ragged >= 1, "no wave of the corpus has lanes that stop in different rows"


# ---------------------------------------------------------------------------
# Word and wave edges, offsets past block 2^18

EDGES = [(f"zeros{n}", F32) for n in (63, 64, 65, 128)] + [("zeros3d", F64), ("three", F32), ("three", F64),
                                                            ("tiles2d", F32), ("tiles2d", F64)]


@pytest.mark.parametrize("name,dtype", EDGES, ids=lambda v: v if isinstance(v, str) else v.name)
def test_edges(cuda, varemu, tp_golden, name, dtype):  # noqa: F811
    """All-zero arrays (nothing but one-bit blocks: no lane reads the stream),
    zero / dense / zero waves, and three scan tiles of ragged blocks, from
    p = full at the fixture's modes."""
    a = tp.array(name, dtype)
    src_mode = tt.full(dtype)
    if src_mode in tp.OTHERS[(name, dtype)]:
        words, L = tp.ref_of(varemu, tp_golden, (name, dtype) + src_mode)[:2]
    else:
        words, L, _ = tv.emu_compress(varemu, a, tp.type_prec(dtype), tv.ZFP_MIN_EXP)
    if words.size == 0:
        words = np.zeros(1, np.uint64)
    src = Stream(cuda, words, L, a.shape, dtype)
    lo = tuple(min(1, s - 1) for s in a.shape)
    inner = (lo, tuple(max(1, s - 3) for s in a.shape))
    for mode in tp.OTHERS[(name, dtype)]:
        case = (name, dtype) + mode
        check_target(src, mode, tp.ref_of(varemu, tp_golden, case)[3], (inner,), tp.case_id(case))


def test_box_across_block_262144(cuda, varemu, tp_golden):  # noqa: F811
    """scan1d, 263 205 blocks, p32 at a1e-3: one box across block 262 144, where
    the index entries have long passed 2^22 bits."""
    a = tp.array("scan1d", F32)
    ref = tp.ref_of(varemu, tp_golden, ("scan1d", F32, "p", 32))
    want = tp.ref_of(varemu, tp_golden, ("scan1d", F32, "a", 1e-3))[3]
    src = Stream(cuda, ref[0], ref[1], a.shape, F32)
    origin, extent = (4 * 262144 - 1001,), (2003,)
    got = src.box(origin, extent, ("a", 1e-3))
    assert _same(got, want[_box(origin, extent)])


# ---------------------------------------------------------------------------
# Against truncate_variable; identity; never finer than the stream

CROSS = [(BIG, np.dtype(dt), src, dst) for dt in (np.float32, np.float64)
         for src, dst in ((None, ("a", 1e-3)), (("a", 1e-3), ("a", 1.0)), (("p", 16), ("p", 7)))]


@pytest.mark.parametrize("case", CROSS, ids=lambda c: f"{c[1].name}-{c[2]}-{c[3]}")
def test_equals_decode_of_truncated(cuda, varemu, tv_golden, case):  # noqa: F811
    """The coarse decode is decode_variable of truncate_variable's output."""
    import cuzfp_amd
    shape, dt, src_mode, mode = case
    src_mode = src_mode or tt.full(dt)
    ref = tv_ref_of(varemu, tv_golden, (shape, dt) + src_mode)
    src = Stream(cuda, ref[0], ref[1], shape, dt)
    w2, l2, _ = cuzfp_amd.truncate_variable(src.w, src.l, shape, src.td, **from_kw(src_mode), **to_kw(mode))
    want = cuzfp_amd.decode_variable(w2, l2, shape, src.td).cpu().numpy()
    check_target(src, mode, want, (INTERIOR,))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_identity_and_never_finer(cuda, varemu, vcoarse, tv_golden, dtype):  # noqa: F811
    """A target equal to the stream's mode, p = type on a p16 stream and
    tolerance 0 on an a1e-3 stream are the plain decode; an a1e-3 stream at p16
    and a p16 stream at a1e-3 are the array at (16, minexp of 1e-3)."""
    import cuzfp_amd
    full = tt.full(dtype)
    for src_mode, mode in ((("p", 16), ("p", 16)), (("a", 1e-3), ("a", 1e-3)), (full, full), (("p", 16), full),
                           (("a", 1e-3), ("a", 0.0)), (("a", 1e-3), full), (("p", 1), ("a", 0.0))):
        ref = tv_ref_of(varemu, tv_golden, (BIG, dtype) + src_mode)
        src = Stream(cuda, ref[0], ref[1], BIG, dtype)
        for origin, extent in (((0, 0, 0), BIG), INTERIOR, ALIGNED):
            plain = cuzfp_amd.decode_region_variable(src.w, src.l, src.idx, BIG, src.td, origin, extent)
            assert _same(plain, ref[3][_box(origin, extent)])
            assert _same(src.box(origin, extent, mode), ref[3][_box(origin, extent)]), (src_mode, mode, origin)
    for src_mode, mode in tc.MIXED:
        want, _ = tc.mixed_expectation(varemu, vcoarse, tv_golden, dtype, src_mode, mode)
        ref = tv_ref_of(varemu, tv_golden, (BIG, dtype) + src_mode)
        check_target(Stream(cuda, ref[0], ref[1], BIG, dtype), mode, want, (INTERIOR, ALIGNED), (src_mode, mode))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_decode_variable_without_index(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """decode_variable(precision=) builds the index itself when none is given."""
    import cuzfp_amd
    ref = tv_ref_of(varemu, tv_golden, (BIG, dtype) + tt.full(dtype))
    src = Stream(cuda, ref[0], ref[1], BIG, dtype)
    for mode in (("p", 7), ("a", 1e-3)):
        got = cuzfp_amd.decode_variable(src.w, src.l, BIG, src.td, **to_kw(mode))
        assert _same(got, src.whole(mode).cpu().numpy())
        assert _same(got, tv_ref_of(varemu, tv_golden, (BIG, dtype) + mode)[3])


# ---------------------------------------------------------------------------
# Mechanics

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_strided_out_and_stream(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """Into a strided view of a filled parent on a non-default stream: the box
    changes and nothing else."""
    import torch
    ref = tv_ref_of(varemu, tv_golden, (BIG, dtype) + tt.full(dtype))
    want = tv_ref_of(varemu, tv_golden, (BIG, dtype, "a", 1e-3))[3]
    src = Stream(cuda, ref[0], ref[1], BIG, dtype)
    origin, extent = INTERIOR
    big = torch.full(tuple(2 * e + 3 for e in extent), -7.0, dtype=src.td, device=cuda)
    sl = tuple(slice(2, 2 + 2 * e, 2) for e in extent)
    view = big[sl]
    assert not view.is_contiguous()
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    src.box(origin, extent, ("a", 1e-3), out=view, stream=s)
    s.synchronize()
    got = big.cpu().numpy()
    assert tp.same(got[sl], want[_box(origin, extent)])
    mask = np.ones(got.shape, bool)
    mask[sl] = False
    assert np.all(got[mask] == -7.0)


def test_graph_capture(cuda, varemu, tv_golden):  # noqa: F811
    """One coarse decode captured into a graph and replayed twice gives the
    eager call's bytes (no allocation or synchronisation inside the call)."""
    import torch
    ref = tv_ref_of(varemu, tv_golden, (BIG, F32, "p", 32))
    want = tv_ref_of(varemu, tv_golden, (BIG, F32, "a", 1e-3))[3]
    src = Stream(cuda, ref[0], ref[1], BIG, F32)
    origin, extent = INTERIOR
    eager = src.box(origin, extent, ("a", 1e-3))
    out = torch.zeros(extent, dtype=torch.float32, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        src.box(origin, extent, ("a", 1e-3), out=out)
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, eager.cpu().numpy())
    assert _same(eager, want[_box(origin, extent)])


def test_tail_and_canaries(cuda, varemu, tv_golden):  # noqa: F811
    """A box inside a larger tensor, and the whole array into the head of a
    longer one: everything around the box keeps its fill."""
    import torch
    import cuzfp_amd
    ref = tv_ref_of(varemu, tv_golden, (BIG, F64, "p", 64))
    want = tv_ref_of(varemu, tv_golden, (BIG, F64, "p", 7))[3]
    src = Stream(cuda, ref[0], ref[1], BIG, F64)
    for origin, extent in (INTERIOR, ALIGNED):
        big = torch.full(tuple(e + 2 for e in extent), -7.0, dtype=torch.float64, device=cuda)
        inner = tuple(slice(1, 1 + e) for e in extent)
        src.box(origin, extent, ("p", 7), out=big[inner])
        assert _same(big[inner], want[_box(origin, extent)])
        outer = big.clone()
        outer[inner] = -7.0
        assert (outer == -7.0).all()
    n = int(np.prod(BIG))
    flat = torch.full((n + 64,), -7.0, dtype=torch.float64, device=cuda)
    cuzfp_amd.decode_variable(src.w, src.l, BIG, torch.float64, index=src.idx, precision=7, out=flat[:n].view(BIG))
    assert _same(flat[:n].view(BIG), want) and (flat[n:] == -7.0).all()


# ---------------------------------------------------------------------------
# Untrusted input

def _canaried(cuda, words):
    import torch
    buf = torch.full((words.size + 64,), ICANARY, dtype=torch.int64, device=cuda)
    buf[: words.size] = _dev(words.view(np.int64), cuda)
    return buf


def _decode_in_canaries(cuda, buf, nwords, l, idx, shape, td, origin, extent, mode):
    """The call into a box inside a filled tensor; the stream's canaries and the
    fill around the box must be intact.  Returns the box."""
    import torch
    import cuzfp_amd
    big = torch.full(tuple(e + 2 for e in extent), -7.0, dtype=td, device=cuda)
    inner = tuple(slice(1, 1 + e) for e in extent)
    cuzfp_amd.decode_region_variable(buf[:nwords], l, idx, shape, td, origin, extent, out=big[inner], **to_kw(mode))
    torch.cuda.synchronize()
    assert (buf[nwords:] == ICANARY).all()
    outer = big.clone()
    outer[inner] = -7.0
    assert (outer == -7.0).all()
    return big[inner]


def test_bad_index(cuda, varemu, tv_golden):  # noqa: F811
    """test_variable_region_gpu.test_bad_index for the coarse entry: lengths of
    65535 and index entries that point past the stream and near 2^64, at p1
    (the smallest image), a tolerance and p64.  The walk loads every dword
    behind the stream's bound and ends at the clamped length, the budget is
    clamped to the column, and the copy-in is the existing decoder's: nothing
    can fault by construction.  Success, the canaries intact, the stream
    unchanged, and the good index decodes correctly afterwards."""
    import torch
    shape = (9, 20, 36)
    words, L, _, _ = tv_ref_of(varemu, tv_golden, (shape, F64, "p", 64))
    buf = _canaried(cuda, words)
    bad_l = torch.full((L.size,), -1, dtype=torch.int16, device=cuda)  # 0xffff
    T = (L.size + 63) // 64
    bad = np.array([64 * words.size - 100, 64 * words.size + 7, 2 ** 64 - 5000, 2 ** 64 - 1][: T + 1], np.uint64)
    assert bad.size == T + 1
    ones = np.full(T + 1, 2 ** 64 - 1, np.uint64)
    origin, extent = (1, 3, 5), (7, 13, 22)
    good_l, good_idx = _dev(L.view(np.int16), cuda), _dev(tp.want_index(L).view(np.int64), cuda)
    for mode in (("p", 1), ("a", 1e-3), ("p", 64)):
        for l, idx in ((bad_l, bad), (bad_l, ones), (good_l, ones), (bad_l, tp.want_index(L))):
            _decode_in_canaries(cuda, buf, words.size, l, _dev(idx.view(np.int64), cuda), shape, torch.float64, origin,
                                extent, mode)
        assert np.array_equal(buf[: words.size].cpu().numpy().view(np.uint64), words)
    want = tv_ref_of(varemu, tv_golden, (shape, F64, "a", 1e-3))[3]
    got = _decode_in_canaries(cuda, buf, words.size, good_l, good_idx, shape, torch.float64, origin, extent,
                              ("a", 1e-3))
    assert _same(got, want[_box(origin, extent)])


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_random_streams(cuda, varemu, vcoarse, tv_golden, dims, dtype):  # noqa: F811
    """Arbitrary bits at arbitrary lengths, at p1 (the smallest image), p = type
    and a tolerance.  With legal lengths the result is the emulation's decode at
    the host walk's lengths (the same functions on the host).  With lengths no
    encoder writes among them (2 .. ebits + 1, above the longest block up to
    65535): success and the canaries intact; the values are unspecified.  A
    valid case run afterwards is exact."""
    prec = tp.type_prec(dtype)
    shape = tp.RANDOM_SHAPES["ragged"][dims]
    td = _tdtype(dtype)
    whole = ((0,) * dims, shape)
    inner = (tuple(min(1, s - 1) for s in shape), tuple(max(1, s - 3) for s in shape))
    for density in tp.DENSITIES:
        words, L = tp.random_stream(dims, dtype, "ragged", density, illegal=False)
        buf = _canaried(cuda, words)
        l, idx = _dev(L.view(np.int16), cuda), _dev(tp.want_index(L).view(np.int64), cuda)
        for mode in (("p", 1), ("p", prec), ("a", 1e-3)):
            walked, budget = tc.host_walk(vcoarse, words, L, dims, dtype, tt.mode_of(dtype, *mode))
            assert np.array_equal(budget, np.where(walked > 1, walked, 0))
            want = tv.emu_decompress(varemu, tt.cut(words, L, walked), walked, shape, dtype)
            for origin, extent in (whole, inner):
                got = _decode_in_canaries(cuda, buf, words.size, l, idx, shape, td, origin, extent, mode)
                assert _same(got, want[_box(origin, extent)]), (density, mode, origin)
        words, L = tp.random_stream(dims, dtype, "ragged", density, illegal=True)
        buf = _canaried(cuda, words)
        l, idx = _dev(L.view(np.int16), cuda), _dev(tp.want_index(L).view(np.int64), cuda)
        for mode in (("p", 1), ("p", prec)):
            _decode_in_canaries(cuda, buf, words.size, l, idx, shape, td, whole[0], whole[1], mode)
        assert np.array_equal(buf[: words.size].cpu().numpy().view(np.uint64), words)
    ref = tv_ref_of(varemu, tv_golden, (BIG, F64, "p", 64))
    check_target(Stream(cuda, ref[0], ref[1], BIG, F64), ("a", 1e-3), tv_ref_of(varemu, tv_golden, (BIG, F64, "a", 1e-3))[3])


# ---------------------------------------------------------------------------
# Arguments

def test_argument_errors(cuda):
    """The C-ABI's checks with real buffers -- nothing is launched on an error --
    and the Python checks that need a device tensor."""
    import torch
    import cuzfp_amd
    lib = cuzfp_amd.library()
    n = (16, 16, 20)  # 80 blocks: T = 2
    ib = lib.cuzfp_hip_variable_index_bytes(3, *n)
    assert ib == 24
    lengths = torch.full((80,), 1, dtype=torch.int16, device=cuda)
    index = torch.tensor([0, 64, 80], dtype=torch.int64, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    words = torch.zeros(2, dtype=torch.int64, device=cuda)
    out = torch.full((4, 4, 4), -7.0, dtype=torch.float32, device=cuda)

    def dec(index_bytes=ib, t=3, maxprec=16, minexp=-1074, e=(4, 4, 4)):
        return lib.cuzfp_hip_decode_region_variable_coarse(words.data_ptr(), 16, lengths.data_ptr(), index.data_ptr(),
                                                           index_bytes, t, n[0], n[1], n[2], maxprec, minexp, 4, 4, 4,
                                                           e[0], e[1], e[2], 0, 0, 0, out.data_ptr(), st)

    assert dec(index_bytes=ib - 1) == 1 and dec(t=2) == 2 and dec(t=1, maxprec=0) == 2
    assert dec(maxprec=0) == 1 and dec(maxprec=33) == 1 and dec(e=(4, 4, 17)) == 1 and dec(e=(0, 4, 4)) == 1
    torch.cuda.synchronize()
    assert (out == -7.0).all()  # nothing was launched
    assert dec() == 0 and dec(maxprec=1) == 0 and dec(maxprec=32, minexp=100) == 0  # 80 one-bit blocks: zeros
    torch.cuda.synchronize()
    assert (out == 0).all()
    shape = (20, 16, 16)
    origin, extent = (0, 0, 0), (4, 4, 4)
    with pytest.raises(ValueError, match="precision and tolerance"):
        cuzfp_amd.decode_region_variable(words, lengths, index, shape, torch.float32, origin, extent, precision=16,
                                         tolerance=1.0)
    with pytest.raises(ValueError, match="shape"):
        cuzfp_amd.decode_region_variable(words, lengths, index, shape, torch.float32, origin, extent, precision=16,
                                         out=torch.zeros((4, 4, 5), device=cuda))
    with pytest.raises(ValueError, match="entries"):
        cuzfp_amd.decode_region_variable(words, lengths[:79], index, shape, torch.float32, origin, extent,
                                         tolerance=1.0)
    with pytest.raises(ValueError, match="entries"):
        cuzfp_amd.decode_variable(words, lengths[:79], shape, torch.float32, precision=16)
    for kw in ({"precision": 0}, {"precision": 33}):
        with pytest.raises(cuzfp_amd.CodecError) as e:
            cuzfp_amd.decode_region_variable(words, lengths, index, shape, torch.float32, origin, extent, **kw)
        assert e.value.status == 1
    with pytest.raises(cuzfp_amd.CodecError) as e:  # a short index
        cuzfp_amd.decode_region_variable(words, lengths, index[:2], shape, torch.float32, origin, extent, precision=16)
    assert e.value.status == 1
    with pytest.raises(cuzfp_amd.CodecError) as e:  # the dtype of `out` decides
        cuzfp_amd.decode_region_variable(words, lengths, index, shape, torch.float32, origin, extent, precision=16,
                                         out=torch.zeros(extent, dtype=torch.int32, device=cuda))
    assert e.value.status == 2
    got = cuzfp_amd.decode_variable(words, lengths, shape, torch.float32, tolerance=1.0)
    assert tuple(got.shape) == shape and (got == 0).all()
