"""extract_region_variable / insert_region_variable without a GPU: the host
model of the two calls, the claim they rest on, the raw C-ABI's argument errors
and size functions, and the Python wrappers' validation.

The model.  zfp codes every block on its own, so the blocks of a block-aligned
box, packed back to back in the box's raster order, are the stream of the
sub-array (`model_extract`), and a stream of the box's blocks replaces the
box's blocks of another stream block for block (`model_insert`: `splice` of
test_variable_region_update with the box stream re-indexed from box order to
archive order).  Both are numpy on bit arrays.  The claim is checked against
the host emulation of test_variable (`varemu`, which the fixture hashes vouch
for), not against the code under test; tests/test_variable_crop_gpu.py compares
the device calls with the model.
"""
import ctypes

import numpy as np
import pytest

import block_zoo as bz
import cuzfp_amd as cz
import test_variable as tv
import test_variable_region_update as ru
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_paths import F32, F64

SHAPES = [(13, 22, 38), (33, 70), (1000,), (6, 5, 9)]
MODES = ru._modes


def aligned_boxes(shape):
    """The aligned boxes of test_variable_region_update, the whole array, and,
    for the 240-block array, a 120-block box whose x-rows of 5 blocks end in
    the middle of a wave."""
    out = list(ru.ALIGNED[shape]) + [((0,) * len(shape), tuple(shape))]
    if shape == (13, 22, 38):
        out.append(((0, 0, 0), (13, 22, 20)))
    return out


def is_aligned(shape, origin, extent):
    return all(o % 4 == 0 and (e % 4 == 0 or o + e == n) for o, e, n in zip(origin, extent, shape))


# ---------------------------------------------------------------------------
# The model

def box_blocks(shape, origin, extent):
    """Archive block index of every box block, in the box's raster order."""
    t = ru.touched_blocks(shape, origin, extent)
    return np.flatnonzero(t)  # raster order of the archive restricted to the box is the box's raster order


def _pack(parts, L):
    bits = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    nbits = int(L.astype(np.int64).sum())
    assert bits.size == nbits
    pad = np.zeros(-nbits % 64, np.uint8)
    return np.packbits(np.concatenate([bits, pad]), bitorder="little").view(np.uint64), L.astype(np.uint16), nbits


def model_extract(words, L, shape, origin, extent):
    """(words', L', nbits) of the box's blocks, back to back."""
    src, so = ru._bits(words), ru._offsets(L)
    ids = box_blocks(shape, origin, extent)
    return _pack([src[so[b]: so[b] + L[b]] for b in ids], L[ids])


def model_insert(bwords, bL, words, L, shape, origin, extent):
    """(words', L', nbits): block b is box block r where the box holds b, else the source's."""
    ids = box_blocks(shape, origin, extent)
    assert bL.size == ids.size
    # the box stream in archive order: a stream with the box's blocks at their archive places
    # and empty blocks elsewhere, which splice takes the touched blocks from
    bits, bo = ru._bits(bwords), ru._offsets(bL)
    LE = np.zeros(L.size, np.uint16)
    LE[ids] = bL
    parts = [bits[bo[r]: bo[r] + bL[r]] for r in range(ids.size)]
    wordsE = _pack(parts, bL)[0]  # ids ascend, so archive order is box order
    touched = np.zeros(L.size, bool)
    touched[ids] = True
    return ru.splice(words, L, wordsE, LE, touched)


def test_box_blocks_is_region_block_order():
    """b = ((bz0 + rz) * by + by0 + ry) * bx + bx0 + rx, x fastest."""
    shape, origin, extent = (13, 22, 38), (8, 16, 32), (5, 6, 6)
    bz_, by, bx = 4, 6, 10
    want = [((2 + rz) * by + 4 + ry) * bx + 8 + rx for rz in range(2) for ry in range(2) for rx in range(2)]
    assert box_blocks(shape, origin, extent).tolist() == want
    assert box_blocks((1000,), (100,), (256,)).tolist() == list(range(25, 89))
    assert box_blocks(shape, (0, 0, 0), (13, 22, 20)).size == 120


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_extract_is_the_stream_of_the_subarray(varemu, shape, dtype):  # noqa: F811
    """The claim the feature rests on: model_extract(stream of A, box) is
    emu_compress(A[box], mode) in words, lengths and bit count."""
    a = tv.array(shape, dtype)
    for mode in MODES(dtype):
        words, L, _ = tv.emu_compress(varemu, a, *ru.mode_of(dtype, mode))
        for origin, extent in aligned_boxes(shape):
            assert is_aligned(shape, origin, extent)
            want = tv.emu_compress(varemu, a[ru.box_slices(origin, extent)], *ru.mode_of(dtype, mode))
            got = model_extract(words, L, shape, origin, extent)
            assert got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), \
                (mode, origin, extent)


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_round_trips_in_the_model(varemu, shape, dtype):  # noqa: F811
    """insert(extract(S, box), S, box) == S and extract(insert(B, S, box), box)
    == B, B the stream of other values at another mode."""
    a = tv.array(shape, dtype)
    mode = MODES(dtype)[2]
    S = tv.emu_compress(varemu, a, *ru.mode_of(dtype, mode))
    for origin, extent in aligned_boxes(shape):
        E = model_extract(S[0], S[1], shape, origin, extent)
        back = model_insert(E[0], E[1], S[0], S[1], shape, origin, extent)
        assert back[2] == S[2] and np.array_equal(back[1], S[1]) and np.array_equal(back[0], S[0]), origin
        B = tv.emu_compress(varemu, ru.other_values(extent, dtype, origin), *ru.mode_of(dtype, MODES(dtype)[0]))
        P = model_insert(B[0], B[1], S[0], S[1], shape, origin, extent)
        E2 = model_extract(P[0], P[1], shape, origin, extent)
        assert E2[2] == B[2] and np.array_equal(E2[1], B[1]) and np.array_equal(E2[0], B[0]), origin
        # ... and the paste is the stream of the array with the box replaced, where the modes agree
        a2 = a.copy()
        a2[ru.box_slices(origin, extent)] = ru.other_values(extent, dtype, origin)
        B3 = tv.emu_compress(varemu, a2[ru.box_slices(origin, extent)], *ru.mode_of(dtype, mode))
        P3 = model_insert(B3[0], B3[1], S[0], S[1], shape, origin, extent)
        W3 = tv.emu_compress(varemu, a2, *ru.mode_of(dtype, mode))
        assert P3[2] == W3[2] and np.array_equal(P3[1], W3[1]) and np.array_equal(P3[0], W3[0]), origin


# ---------------------------------------------------------------------------
# Argument checks without a device

@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def _at(p, by):
    return ctypes.c_void_p(p.value + by)


UNALIGNED = [  # (n, origin, extent): one axis at a time, origin then extent
    ((16, 16, 16), (1, 0, 0), (4, 4, 4)), ((16, 16, 16), (0, 2, 0), (4, 4, 4)), ((16, 16, 16), (0, 0, 3), (4, 4, 4)),
    ((16, 16, 16), (0, 0, 0), (3, 4, 4)), ((16, 16, 16), (0, 0, 0), (4, 5, 4)), ((16, 16, 16), (0, 0, 0), (4, 4, 6)),
    ((18, 16, 16), (12, 0, 0), (5, 4, 4)),  # stops one short of the ragged end
    ((18, 16, 16), (13, 0, 0), (5, 4, 4)),  # reaches the end from an unaligned origin
    ((16, 18, 0), (0, 2, 0), (4, 16, 0)), ((16, 18, 0), (0, 0, 0), (2, 4, 0)),
    ((18, 0, 0), (2, 0, 0), (16, 0, 0)), ((18, 0, 0), (0, 0, 0), (6, 0, 0))]


def test_extract_argument_errors(libs):
    """Every argument error of cuzfp_hip_extract_region_variable: a status, with
    pointers that are never dereferenced."""
    lib = cz.library()
    assert lib.cuzfp_hip_abi_version() == 1
    P = {k: ctypes.c_void_p(0x100000 * (i + 1)) for i, k in enumerate(
        ("src", "src_len", "src_index", "dst", "len", "index", "total", "ws"))}
    ib16 = lib.cuzfp_hip_variable_index_bytes(3, 16, 16, 16)

    def call(t=3, n=(16, 16, 16), o=(0, 0, 0), e=(8, 8, 8), src_bytes=4096, index_bytes=None, cap=8192,
             dib=None, ws_bytes=None, **over):
        p = dict(P)
        p.update(over)
        if index_bytes is None:
            index_bytes = lib.cuzfp_hip_variable_index_bytes(3, *n) or ib16
        if dib is None:
            dib = lib.cuzfp_hip_variable_index_bytes(3, *e) or ib16
        if ws_bytes is None:
            ws_bytes = lib.cuzfp_hip_extract_region_variable_workspace_bytes(3, *e) or 1 << 16
        return lib.cuzfp_hip_extract_region_variable(
            p["src"], src_bytes, p["src_len"], p["src_index"], index_bytes, t, *n, *o, *e,
            p["dst"], cap, p["len"], p["index"], dib, p["total"], p["ws"], ws_bytes, None)

    # unaligned boxes, one axis at a time, in origin and in extent
    for n, o, e in UNALIGNED:
        assert call(n=n, o=o, e=e) == 1, (n, o, e)
    # null pointers (the box's index may be null; that call would launch and is not made here)
    for name in ("src", "src_len", "src_index", "len", "total", "ws"):
        assert call(**{name: None}) == 1, name
    assert call(dst=None) == 1  # no destination, yet a capacity
    # misaligned pointers: the stream 4 bytes, the lengths 2, the rest 8
    for name, by in (("src", 2), ("src_len", 1), ("len", 1), ("src_index", 4), ("index", 4), ("dst", 4),
                     ("total", 4), ("ws", 4)):
        assert call(**{name: _at(P[name], by)}) == 1, name
    # a short source index, a short index of the box (8 blocks: 16 bytes), a short workspace (8 + 1 words)
    assert call(index_bytes=ib16 - 1) == 1 and call(n=(16, 16, 20), e=(8, 8, 8), index_bytes=ib16) == 1
    assert call(dib=15) == 1 and call(dib=0) == 1
    assert call(e=(16, 16, 16), dib=lib.cuzfp_hip_variable_index_bytes(3, 16, 16, 16) - 8) == 1
    assert call(ws_bytes=8 * 9 - 1) == 1 and call(ws_bytes=0) == 1
    # an empty box, a box that leaves the array (also by wrap-around), unused dimensions
    assert call(e=(0, 8, 8)) == 1 and call(e=(8, 0, 8)) == 1 and call(e=(8, 8, 0)) == 1
    assert call(o=(12, 0, 0), e=(8, 4, 4)) == 1 and call(o=(16, 0, 0), e=(4, 4, 4)) == 1
    assert call(o=(8, 0, 0), e=(2 ** 32 - 4, 4, 4)) == 1
    assert call(n=(16, 16, 0), o=(0, 0, 4), e=(4, 4, 0)) == 1 and call(n=(16, 16, 0), e=(4, 4, 4)) == 1
    assert call(n=(16, 0, 0), o=(0, 4, 0), e=(4, 0, 0)) == 1 and call(n=(16, 0, 0), e=(4, 4, 0)) == 1
    # an output overlapping an input: the streams, the lengths (64 and 8 blocks), the indices (2 words each)
    assert call(dst=P["src"]) == 1 and call(dst=_at(P["src"], 4096 - 8)) == 1
    assert call(dst=ctypes.c_void_p(P["src"].value - 8192 + 8)) == 1
    assert call(len=P["src_len"]) == 1 and call(len=_at(P["src_len"], 126)) == 1
    assert call(len=ctypes.c_void_p(P["src_len"].value - 14)) == 1
    assert call(index=P["src_index"]) == 1 and call(index=_at(P["src_index"], 8)) == 1
    # integer and unknown types (before anything else is looked at), bad dimensions
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2 and call(t=0) == 2
    assert call(t=1, src=None, o=(1, 0, 0)) == 2
    assert call(n=(16, 0, 16)) == 1 and call(n=(0, 0, 0)) == 1


def test_insert_argument_errors(libs):
    """The same for cuzfp_hip_insert_region_variable."""
    lib = cz.library()
    P = {k: ctypes.c_void_p(0x100000 * (i + 1)) for i, k in enumerate(
        ("box", "box_len", "box_index", "src", "src_len", "src_index", "dst", "len", "index", "total", "ws"))}
    ib16 = lib.cuzfp_hip_variable_index_bytes(3, 16, 16, 16)
    ws16 = lib.cuzfp_hip_insert_region_variable_workspace_bytes(3, 16, 16, 16)
    assert ib16 == 16 and ws16 == 8 * (64 + 1)

    def call(t=3, n=(16, 16, 16), o=(0, 0, 0), e=(8, 8, 8), box_bytes=1024, bib=16, src_bytes=4096, index_bytes=None,
             cap=8192, ws_bytes=None, **over):
        p = dict(P)
        p.update(over)
        if index_bytes is None:
            index_bytes = lib.cuzfp_hip_variable_index_bytes(3, *n) or ib16
        if ws_bytes is None:
            ws_bytes = lib.cuzfp_hip_insert_region_variable_workspace_bytes(3, *n) or ws16
        return lib.cuzfp_hip_insert_region_variable(
            p["box"], box_bytes, p["box_len"], p["box_index"], bib, p["src"], src_bytes, p["src_len"],
            p["src_index"], index_bytes, t, *n, *o, *e, p["dst"], cap, p["len"], p["index"], p["total"], p["ws"],
            ws_bytes, None)

    for n, o, e in UNALIGNED:
        assert call(n=n, o=o, e=e) == 1, (n, o, e)
    for name in ("box", "box_len", "box_index", "src", "src_len", "src_index", "len", "total", "ws"):
        assert call(**{name: None}) == 1, name
    assert call(dst=None) == 1
    for name, by in (("box", 2), ("src", 2), ("box_len", 1), ("src_len", 1), ("len", 1), ("box_index", 4),
                     ("src_index", 4), ("index", 4), ("dst", 4), ("total", 4), ("ws", 4)):
        assert call(**{name: _at(P[name], by)}) == 1, name
    # a short index of the box (8 blocks: 16 bytes; 4096 blocks: 65 words) or of the source, a short workspace
    assert call(bib=15) == 1 and call(bib=0) == 1
    assert call(n=(64, 64, 64), e=(64, 64, 64), bib=8 * 65 - 1, box_bytes=8) == 1
    assert call(index_bytes=ib16 - 1) == 1 and call(n=(16, 16, 20), index_bytes=ib16) == 1
    assert call(ws_bytes=ws16 - 1) == 1 and call(ws_bytes=0) == 1
    assert call(e=(0, 8, 8)) == 1 and call(e=(8, 0, 8)) == 1 and call(e=(8, 8, 0)) == 1
    assert call(o=(12, 0, 0), e=(8, 4, 4)) == 1 and call(o=(8, 0, 0), e=(2 ** 32 - 4, 4, 4)) == 1
    assert call(n=(16, 16, 0), e=(4, 4, 4)) == 1 and call(n=(16, 0, 0), o=(0, 4, 0), e=(4, 0, 0)) == 1
    # the output stream over either input stream, the lengths over either lengths, the index over either index
    assert call(dst=P["src"]) == 1 and call(dst=_at(P["src"], 4096 - 8)) == 1
    assert call(dst=P["box"]) == 1 and call(dst=_at(P["box"], 1024 - 8)) == 1
    assert call(dst=ctypes.c_void_p(P["box"].value - 8192 + 8)) == 1
    assert call(len=P["src_len"]) == 1 and call(len=_at(P["src_len"], 126)) == 1
    assert call(len=P["box_len"]) == 1 and call(len=_at(P["box_len"], 14)) == 1
    assert call(len=ctypes.c_void_p(P["box_len"].value - 126)) == 1
    assert call(index=P["src_index"]) == 1 and call(index=_at(P["src_index"], 8)) == 1
    assert call(index=P["box_index"]) == 1 and call(index=_at(P["box_index"], 8)) == 1
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2 and call(t=0) == 2
    assert call(t=2, box=None, o=(1, 0, 0)) == 2
    assert call(n=(16, 0, 16)) == 1 and call(n=(0, 0, 0)) == 1


def test_size_functions(libs):
    lib = cz.library()
    ews = lib.cuzfp_hip_extract_region_variable_workspace_bytes
    iws = lib.cuzfp_hip_insert_region_variable_workspace_bytes
    for t in (3, 4):
        assert ews(t, 16, 8, 8) == 8 * (16 + 1)  # the box's blocks and one scan tile
        assert ews(t, 6, 6, 5) == 8 * (8 + 1)  # a box at the ragged end: ceil(e / 4) blocks an axis
        assert ews(t, 256, 0, 0) == 8 * (64 + 1)
        assert ews(t, 259, 131, 0) == 8 * (65 * 33 + 3)  # three scan tiles
        assert iws(t, 38, 22, 13) == 8 * (240 + 1) == lib.cuzfp_hip_variable_workspace_bytes(t, 38, 22, 13)
        assert iws(t, 1000, 0, 0) == 8 * (250 + 1)
    for ws in (ews, iws):
        assert ws(1, 16, 16, 16) == 0 and ws(2, 16, 16, 16) == 0 and ws(9, 16, 16, 16) == 0
        assert ws(3, 0, 0, 0) == 0 and ws(3, 16, 0, 16) == 0

    emx = lib.cuzfp_hip_extract_region_variable_maximum_size

    def want(dt, dims, src_bytes, blocks):
        return 8 * ((min(8 * src_bytes, blocks * bz.top(dims, dt)) + 63) // 64)

    assert bz.top(3, F64) == 4171 and bz.top(1, F32) == 9 + 3 + 128
    # (type, n, src_bytes, e, o)
    assert emx(3, 38, 22, 13, 100000, 16, 8, 8, 12, 8, 4) == want(F32, 3, 100000, 16)  # the box's blocks bound it
    assert emx(3, 38, 22, 13, 1000, 16, 8, 8, 12, 8, 4) == 1000  # the source's bits do
    assert emx(3, 38, 22, 13, 1001, 16, 8, 8, 12, 8, 4) == 1008
    assert emx(4, 38, 22, 13, 10 ** 6, 6, 6, 5, 32, 16, 8) == want(F64, 3, 10 ** 6, 8)
    assert emx(4, 38, 22, 13, 10 ** 9, 38, 22, 13, 0, 0, 0) == want(F64, 3, 10 ** 9, 240)
    assert emx(4, 70, 33, 0, 10 ** 6, 20, 12, 0, 16, 8, 0) == want(F64, 2, 10 ** 6, 15)
    assert emx(3, 1000, 0, 0, 10 ** 6, 256, 0, 0, 100, 0, 0) == want(F32, 1, 10 ** 6, 64)
    assert emx(3, 1000, 0, 0, 0, 256, 0, 0, 100, 0, 0) == 0  # (an empty source has nothing to crop)
    # invalid: types, dimensions, the box, alignment
    ok = (1000, 4, 4, 4, 0, 0, 0)
    assert emx(1, 38, 22, 13, *ok) == 0 and emx(9, 38, 22, 13, *ok) == 0
    assert emx(3, 0, 0, 0, *ok) == 0 and emx(3, 38, 0, 13, *ok) == 0
    assert emx(3, 38, 22, 13, 1000, 0, 4, 4, 0, 0, 0) == 0  # empty
    assert emx(3, 38, 22, 13, 1000, 4, 4, 4, 36, 0, 0) == 0  # leaves the array
    assert emx(3, 38, 22, 13, 1000, 2 ** 32 - 4, 4, 4, 8, 0, 0) == 0  # ... by wrap-around
    assert emx(3, 38, 22, 0, 1000, 4, 4, 4, 0, 0, 0) == 0  # an extent for an unused dimension
    assert emx(3, 38, 22, 13, 1000, 4, 4, 4, 2, 0, 0) == 0 and emx(3, 38, 22, 13, 1000, 4, 6, 4, 0, 0, 0) == 0
    assert emx(3, 38, 22, 13, 1000, 2, 4, 4, 36, 0, 0) == want(F32, 3, 1000, 1)  # aligned by reaching the end

    imx = lib.cuzfp_hip_insert_region_variable_maximum_size
    assert imx(0, 0) == 0 and imx(8, 0) == 8 and imx(4, 4) == 8 and imx(4, 5) == 16
    assert imx(1000, 24) == 1024 and imx(1001, 24) == 1032
    assert imx(2 ** 60, 8) == 0 and imx(8, 2 ** 60) == 0  # 8 * bytes would wrap


# ---------------------------------------------------------------------------
# The wrappers' validation

class Fake:
    """What a wrapper may look at of a tensor before it needs a device."""

    def __init__(self, n=0, size=8, cuda=True, contiguous=True):
        self.is_cuda, self._n, self._size, self._c = cuda, n, size, contiguous

    def numel(self):
        return self._n

    def element_size(self):
        return self._size

    def is_contiguous(self):
        return self._c


def test_python_validation(libs):
    """The dtype, the rank, the box and its alignment, then the tensors, before
    anything touches a device."""
    assert "extract_region_variable" in cz.__all__ and "insert_region_variable" in cz.__all__
    shape = (16, 16, 16)
    w, l64, i2 = Fake(100), Fake(64, 2), Fake(2)
    bl8 = Fake(8, 2)

    def ext(words=w, lengths=l64, index=i2, shape=shape, dtype=np.float32, origin=(0, 0, 0), extent=(8, 8, 8), **kw):
        return cz.extract_region_variable(words, lengths, index, shape, dtype, origin, extent, **kw)

    def ins(bw=w, bl=bl8, bi=i2, words=w, lengths=l64, index=i2, shape=shape, dtype=np.float32, origin=(0, 0, 0),
            extent=(8, 8, 8), **kw):
        return cz.insert_region_variable(bw, bl, bi, words, lengths, index, shape, dtype, origin, extent, **kw)

    for f in (ext, ins):
        # integer dtypes, before the rank
        for dtype in (np.int32, np.int64):
            with pytest.raises(cz.CodecError) as e:
                f(dtype=dtype, origin=(0, 0))
            assert e.value.status == 2
        # a rank mismatch
        for origin, extent in (((0, 0), (8, 8, 8)), ((0, 0, 0), (8, 8)), ((0,), (8,))):
            with pytest.raises(ValueError, match="rank"):
                f(origin=origin, extent=extent)
        with pytest.raises(ValueError):
            f(shape=(16,) * 4, origin=(0,) * 4, extent=(8,) * 4)
        with pytest.raises(ValueError, match="non-negative"):
            f(origin=(0, -4, 0))
        with pytest.raises(ValueError, match="not empty"):
            f(extent=(8, 0, 8))
        with pytest.raises(ValueError, match="leaves the array"):
            f(origin=(12, 0, 0))
        # boxes that are not aligned; the message names the calls that decode
        for n, o, e in UNALIGNED:
            rank = 3 if n[2] else 2 if n[1] else 1
            with pytest.raises(ValueError, match="decode_region_variable / encode_region_variable"):
                f(shape=n[:rank][::-1], origin=o[:rank][::-1], extent=e[:rank][::-1])
        # ... and only then the tensors: host tensors, wrong widths, non-contiguous ones, wrong counts
        with pytest.raises(ValueError, match="device"):
            f(words=Fake(100, cuda=False))
        with pytest.raises(ValueError, match="device"):
            f(lengths=Fake(64, 2, cuda=False))
        with pytest.raises(ValueError, match="device"):
            f(index=Fake(2, cuda=False))
        with pytest.raises(ValueError, match="16-bit"):
            f(lengths=Fake(64, 4))
        with pytest.raises(ValueError, match="contiguous"):
            f(lengths=Fake(64, 2, contiguous=False))
        with pytest.raises(ValueError, match="contiguous"):
            f(words=Fake(100, contiguous=False))
        with pytest.raises(ValueError, match="64-bit"):
            f(index=Fake(2, 4))
        with pytest.raises(ValueError, match="64-bit"):
            f(index=Fake(2, contiguous=False))
        with pytest.raises(ValueError, match="63 entries.*64 blocks"):
            f(lengths=Fake(63, 2))
    # the box stream of the paste
    with pytest.raises(ValueError, match="device box"):
        ins(bw=Fake(10, cuda=False))
    with pytest.raises(ValueError, match="device box"):
        ins(bi=Fake(2, cuda=False))
    with pytest.raises(ValueError, match="box lengths.*16-bit"):
        ins(bl=Fake(8, 8))
    with pytest.raises(ValueError, match="box index.*64-bit"):
        ins(bi=Fake(2, 2))
    for n in (7, 9, 64):
        with pytest.raises(ValueError, match=f"box lengths has {n} entries, the box has 8 blocks"):
            ins(bl=Fake(n, 2))
    # a box at the ragged end counts ceil(extent / 4) blocks an axis
    with pytest.raises(ValueError, match="box lengths has 8 entries, the box has 4 blocks"):
        ins(shape=(13, 22, 38), lengths=Fake(240, 2), index=Fake(5), origin=(8, 16, 32), extent=(5, 6, 4))
