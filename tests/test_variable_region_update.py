"""encode_region_variable without a GPU: the host model of the call, the raw
C-ABI's argument errors, and the Python wrapper's validation.

The model.  With A = decode(words, L), M = A with the box replaced, and E the
stream of M at the call's mode, the result keeps every block the box does not
touch bit for bit (its source bits, its source length), takes E's block and
length for every touched block, and packs them back to back in raster order
with a zero pad to the next 64-bit word.  `splice` is that in numpy on bit
arrays; `model` builds A, M and E with the host emulation of test_variable
(`varemu`, which the fixture hashes vouch for).  Neither uses the code under
test; tests/test_variable_region_update_gpu.py compares the device call with
them.
"""
import ctypes
import zlib

import numpy as np
import pytest

import cuzfp_amd as cz
import test_variable as tv
import test_variable_paths as tp
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_paths import F32, F64

SHAPES = [(13, 22, 38), (33, 70), (1000,)]


def full(dt):
    return ("p", tp.type_prec(dt))


def mode_of(dt, mode):
    """(maxprec, minexp) of ("p", precision) or ("a", tolerance)."""
    return tv.mode_params((None, np.dtype(dt)) + tuple(mode))


# ---------------------------------------------------------------------------
# The model

def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little")


def _offsets(L):
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(L.astype(np.int64))])


def touched_blocks(shape, origin, extent):
    """Raster-order mask of the blocks the box intersects."""
    nb = [(s + 3) // 4 for s in shape]
    m = np.ones(nb, bool)
    for ax, (o, e) in enumerate(zip(origin, extent)):
        k = np.arange(nb[ax])
        on = (k >= o // 4) & (k < (o + e + 3) // 4)
        m &= on.reshape([-1 if i == ax else 1 for i in range(len(nb))])
    return m.reshape(-1)


def splice(words, L, wordsE, LE, touched):
    """(words', L', nbits): block b is E's where touched[b], else the source's."""
    src, new = _bits(words), _bits(wordsE)
    so, eo = _offsets(L), _offsets(LE)
    Lp = np.where(touched, LE, L).astype(np.uint16)
    parts = []
    for b in range(L.size):
        parts.append(new[eo[b]: eo[b] + LE[b]] if touched[b] else src[so[b]: so[b] + L[b]])
    bits = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    nbits = int(Lp.astype(np.int64).sum())
    assert bits.size == nbits
    pad = np.zeros(-nbits % 64, np.uint8)
    return np.packbits(np.concatenate([bits, pad]), bitorder="little").view(np.uint64), Lp, nbits


def box_slices(origin, extent):
    return tuple(slice(o, o + e) for o, e in zip(origin, extent))


def model(varemu, words, L, shape, dt, origin, x, mode):  # noqa: F811
    """The expected (words', L', nbits) of the update, and M."""
    A = tv.emu_decompress(varemu, words, L, shape, dt)
    M = A.copy()
    M[box_slices(origin, x.shape)] = x
    wordsE, LE, _ = tv.emu_compress(varemu, M, *mode_of(dt, mode))
    return splice(words, L, wordsE, LE, touched_blocks(shape, origin, x.shape)) + (M,)


def other_values(shape, dtype, tag):
    """Values unlike tv.array's, with a zero block among them where there is room."""
    rng = np.random.default_rng(zlib.crc32(repr(("update", tag, tuple(shape), np.dtype(dtype).str)).encode()))
    x = tv._values(rng, shape, dtype)
    if all(s >= 8 for s in shape):
        x[tuple(slice(4, 8) for _ in shape)] = 0
    return x


# block-aligned boxes: interior, and reaching the array's ragged end on every axis
ALIGNED = {(13, 22, 38): [((4, 8, 12), (8, 8, 16)), ((8, 16, 32), (5, 6, 6)), ((0, 0, 0), (4, 4, 4))],
           (33, 70): [((8, 16), (12, 20)), ((32, 64), (1, 6))],
           (1000,): [((100,), (256,)), ((996,), (4,))],
           (6, 5, 9): [((0, 0, 4), (4, 4, 4)), ((4, 4, 8), (2, 1, 1))]}


def _modes(dt):
    return (("p", 16), full(dt), ("a", 1e-3))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_splice_on_emulation(varemu, shape, dtype):  # noqa: F811
    """An aligned box overwritten gives a'; splice(stream(a), stream(a'),
    touched) is stream(a') byte for byte, lengths and bit count included."""
    a = tv.array(shape, dtype)
    for mode in _modes(dtype):
        words, L, _ = tv.emu_compress(varemu, a, *mode_of(dtype, mode))
        for origin, extent in ALIGNED[shape]:
            a2 = a.copy()
            a2[box_slices(origin, extent)] = other_values(extent, dtype, origin)
            w2, L2, n2 = tv.emu_compress(varemu, a2, *mode_of(dtype, mode))
            t = touched_blocks(shape, origin, extent)
            assert 0 < t.sum() < t.size
            got = splice(words, L, w2, L2, t)
            assert got[2] == n2 and np.array_equal(got[1], L2) and np.array_equal(got[0], w2), (mode, origin)
            # ... and the untouched blocks of the two streams were equal to begin with
            assert np.array_equal(L[~t], L2[~t])


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_splice_on_live_reference(reference, shape, dtype):
    """The same on CPU zfp 0.5.0's own streams and lengths."""
    ref = tv.RefVariable(reference)
    a = tv.array(shape, dtype)
    for mode in _modes(dtype):
        case = (shape, dtype) + mode
        words, L = ref.compress(a, case), ref.lengths(a, case)
        for origin, extent in ALIGNED[shape]:
            a2 = a.copy()
            a2[box_slices(origin, extent)] = other_values(extent, dtype, origin)
            w2, L2 = ref.compress(a2, case), ref.lengths(a2, case)
            got = splice(words, L, w2, L2, touched_blocks(shape, origin, extent))
            assert got[2] == int(L2.astype(np.int64).sum())
            assert np.array_equal(got[1], L2) and np.array_equal(got[0], w2), (mode, origin)


def test_touched_blocks():
    t = touched_blocks((13, 22, 38), (3, 4, 7), (2, 1, 2)).reshape(4, 6, 10)
    want = np.zeros((4, 6, 10), bool)
    want[0:2, 1:2, 1:3] = True
    assert np.array_equal(t, want)
    assert touched_blocks((1000,), (0,), (1000,)).all()
    assert touched_blocks((33, 70), (32, 69), (1, 1)).sum() == 1


# ---------------------------------------------------------------------------
# Argument checks without a device

@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def test_argument_errors(libs):
    """Every argument error of cuzfp_hip_encode_region_variable: a status, with
    pointers that are never dereferenced."""
    lib = cz.library()
    assert lib.cuzfp_hip_abi_version() == 1
    P = {k: ctypes.c_void_p(0x100000 * (i + 1)) for i, k in enumerate(
        ("box", "src", "src_len", "src_index", "dst", "len", "index", "total", "ws"))}
    ib16 = lib.cuzfp_hip_variable_index_bytes(3, 16, 16, 16)
    ws16 = lib.cuzfp_hip_encode_region_variable_workspace_bytes(3, 16, 16, 16)
    assert ib16 == 8 * 2 and ws16 == 8 * (64 + 1)

    def call(t=3, n=(16, 16, 16), maxprec=16, minexp=-1074, o=(0, 0, 0), e=(4, 4, 4), src_bytes=4096,
             index_bytes=None, cap=8192, ws_bytes=None, **over):
        p = dict(P)
        p.update(over)
        if index_bytes is None:
            index_bytes = lib.cuzfp_hip_variable_index_bytes(3, *n) or ib16
        if ws_bytes is None:
            ws_bytes = lib.cuzfp_hip_encode_region_variable_workspace_bytes(3, *n) or ws16
        return lib.cuzfp_hip_encode_region_variable(
            p["box"], 0, 0, 0, t, n[0], n[1], n[2], maxprec, minexp, o[0], o[1], o[2], e[0], e[1], e[2],
            p["src"], src_bytes, p["src_len"], p["src_index"], index_bytes, p["dst"], cap, p["len"], p["index"],
            p["total"], p["ws"], ws_bytes, None)

    def at(name, by):
        return ctypes.c_void_p(P[name].value + by)

    # null pointers (the destination index may be null; that call has nothing else wrong and
    # would launch, so it is not made here)
    for name in ("box", "src", "src_len", "src_index", "len", "total", "ws"):
        assert call(**{name: None}) == 1, name
    assert call(dst=None) == 1  # no destination, yet a capacity
    # a misaligned stream, lengths or index (and the other 8-byte outputs)
    for name, by in (("src", 2), ("src_len", 1), ("len", 1), ("src_index", 4), ("index", 4), ("dst", 4),
                     ("total", 4), ("ws", 4)):
        assert call(**{name: at(name, by)}) == 1, name
    # short index_bytes or workspace
    assert call(index_bytes=ib16 - 1) == 1 and call(index_bytes=8) == 1
    assert call(n=(16, 16, 20), index_bytes=ib16) == 1
    assert call(ws_bytes=ws16 - 1) == 1 and call(ws_bytes=0) == 1
    # maxprec outside 1 .. 32 or 1 .. 64
    assert call(maxprec=0) == 1 and call(maxprec=33) == 1 and call(maxprec=2 ** 32 - 1) == 1
    assert call(t=4, maxprec=0) == 1 and call(t=4, maxprec=65) == 1
    # an empty box
    assert call(e=(0, 4, 4)) == 1 and call(e=(4, 0, 4)) == 1 and call(e=(4, 4, 0)) == 1
    # a box that leaves the array, also by wrap-around of origin + extent
    assert call(o=(13, 0, 0)) == 1
    assert call(o=(0, 16, 0), e=(4, 1, 4)) == 1
    assert call(o=(0, 0, 1), e=(4, 4, 16)) == 1
    assert call(o=(8, 0, 0), e=(2 ** 32 - 4, 4, 4)) == 1
    assert call(o=(2 ** 32 - 4, 0, 0), e=(8, 4, 4)) == 1
    # an origin or extent given for an unused dimension
    assert call(n=(16, 16, 0), o=(0, 0, 1), e=(4, 4, 0)) == 1
    assert call(n=(16, 16, 0), o=(0, 0, 0), e=(4, 4, 1)) == 1
    assert call(n=(16, 0, 0), o=(0, 1, 0), e=(4, 0, 0)) == 1
    assert call(n=(16, 0, 0), o=(0, 0, 0), e=(4, 1, 0)) == 1
    # source and destination streams that overlap
    assert call(dst=P["src"]) == 1
    assert call(dst=at("src", 4096 - 8)) == 1
    assert call(dst=ctypes.c_void_p(P["src"].value - 8192 + 8)) == 1
    # the two lengths arrays overlapping (64 blocks: 128 bytes), and the two indices
    assert call(len=P["src_len"]) == 1
    assert call(len=at("src_len", 126)) == 1
    assert call(len=ctypes.c_void_p(P["src_len"].value - 126)) == 1
    assert call(index=P["src_index"]) == 1
    assert call(index=at("src_index", 8)) == 1
    # integer and unknown types (before anything else is looked at), bad dimensions
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2 and call(t=0) == 2
    assert call(t=1, maxprec=0, box=None) == 2
    assert call(n=(16, 0, 16)) == 1 and call(n=(0, 0, 0)) == 1


def test_size_queries(libs):
    lib = cz.library()
    ws = lib.cuzfp_hip_encode_region_variable_workspace_bytes
    for t in (3, 4):
        assert ws(t, 38, 22, 13) == 8 * (240 + 1)
        assert ws(t, 259, 131, 0) == 8 * (65 * 33 + 3)  # three scan tiles
        assert ws(t, 1000, 0, 0) == 8 * (250 + 1)
        assert ws(t, 38, 22, 13) == lib.cuzfp_hip_variable_workspace_bytes(t, 38, 22, 13)
    assert ws(1, 16, 16, 16) == 0 and ws(2, 16, 16, 16) == 0 and ws(9, 16, 16, 16) == 0
    assert ws(3, 0, 0, 0) == 0 and ws(3, 16, 0, 16) == 0

    mx = lib.cuzfp_hip_encode_region_variable_maximum_size

    def want(dt, dims, src_bytes, touched, maxprec):
        n = 4 ** dims
        block = min(1 + tp.ebits(dt) + n - 1 + n * maxprec, 4171)
        return 8 * ((8 * src_bytes + touched * block + 63) // 64)

    # (type, n, src_bytes, e, o, maxprec) -> touched blocks
    assert mx(3, 38, 22, 13, 1000, 4, 4, 4, 0, 0, 0, 16) == want(F32, 3, 1000, 1, 16)
    assert mx(3, 38, 22, 13, 1000, 2, 1, 2, 7, 4, 3, 32) == want(F32, 3, 1000, 4, 32)  # x 7..8 and z 3..4 straddle
    assert mx(4, 38, 22, 13, 8, 38, 22, 13, 0, 0, 0, 64) == want(F64, 3, 8, 240, 64)  # 4171 a block
    assert want(F64, 3, 0, 1, 64) == 8 * ((4171 + 63) // 64)
    assert mx(4, 70, 33, 0, 0, 5, 5, 0, 3, 3, 0, 7) == want(F64, 2, 0, 4, 7)
    assert mx(3, 1000, 0, 0, 24, 1000, 0, 0, 0, 0, 0, 1) == want(F32, 1, 24, 250, 1)
    # invalid: types, dimensions, maxprec, the box
    ok = (1000, 4, 4, 4, 0, 0, 0)
    assert mx(1, 38, 22, 13, *ok, 16) == 0 and mx(9, 38, 22, 13, *ok, 16) == 0
    assert mx(3, 0, 0, 0, *ok, 16) == 0 and mx(3, 38, 0, 13, *ok, 16) == 0
    assert mx(3, 38, 22, 13, *ok, 0) == 0 and mx(3, 38, 22, 13, *ok, 33) == 0 and mx(4, 38, 22, 13, *ok, 65) == 0
    assert mx(3, 38, 22, 13, 1000, 0, 4, 4, 0, 0, 0, 16) == 0  # empty
    assert mx(3, 38, 22, 13, 1000, 4, 4, 4, 36, 0, 0, 16) == 0  # leaves the array
    assert mx(3, 38, 22, 13, 1000, 2 ** 32 - 4, 4, 4, 8, 0, 0, 16) == 0  # ... by wrap-around
    assert mx(3, 38, 22, 0, 1000, 4, 4, 1, 0, 0, 0, 16) == 0  # an extent for an unused dimension
    assert mx(3, 38, 22, 0, 1000, 4, 4, 0, 0, 0, 1, 16) == 0


class FakeBox:
    """What the wrapper may look at before it needs a device."""
    is_cuda = False

    def __init__(self, shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), dtype


def test_python_validation(libs):
    """The order of the errors: the mode, the integer dtypes, the rank, the
    origin and the box, and only then the tensors."""
    class NoStream:
        is_cuda = False

    ns = NoStream()
    shape = (16, 16, 16)
    assert "encode_region_variable" in cz.__all__

    def call(box=(4, 4, 4), dtype=np.float32, origin=(0, 0, 0), shape=shape, **kw):
        return cz.encode_region_variable(FakeBox(box, dtype), ns, ns, ns, shape, origin, **kw)

    # the mode, before everything else (a wrong rank and an integer box behind it)
    for kw in ({}, {"precision": 16, "tolerance": 1e-3}):
        with pytest.raises(ValueError, match="exactly one"):
            call(**kw)
        with pytest.raises(ValueError, match="exactly one"):
            call(origin=(0, 0), dtype=np.int32, **kw)
    for p in (7.5, 0.5):
        with pytest.raises(ValueError, match="whole number"):
            call(precision=p, origin=(0, 0))
    for dtype, p in ((np.float32, 0), (np.float32, 33), (np.float32, -1), (np.float64, 0), (np.float64, 65)):
        with pytest.raises(cz.CodecError) as e:
            call(dtype=dtype, precision=p, origin=(0, 0))
        assert e.value.status == 1
    # integer dtypes, before the rank
    for dtype in (np.int32, np.int64):
        for kw in ({"precision": 16}, {"tolerance": 1e-3}):
            with pytest.raises(cz.CodecError) as e:
                call(dtype=dtype, origin=(0, 0), **kw)
            assert e.value.status == 2
    # rank, origin, box
    for box, origin in (((4, 4, 4), (0, 0)), ((4, 4), (0, 0, 0)), ((4,), (0,)), ((4,) * 4, (0,) * 4)):
        with pytest.raises(ValueError, match="rank"):
            call(box=box, origin=origin, precision=16)
    with pytest.raises(ValueError):
        call(box=(4,) * 4, origin=(0,) * 4, shape=(16,) * 4, tolerance=1.0)
    with pytest.raises(ValueError, match="non-negative"):
        call(origin=(0, -1, 0), precision=16)
    with pytest.raises(ValueError, match="not empty"):
        call(box=(4, 0, 4), tolerance=1e-3)
    with pytest.raises(ValueError, match="leaves the array"):
        call(origin=(0, 13, 0), precision=16)
    with pytest.raises(ValueError, match="leaves the array"):
        call(box=(17, 4, 4), precision=16)
    # ... and only then the tensors
    for kw in ({"precision": 16}, {"precision": 32.0}, {"tolerance": 1e-3}, {"tolerance": 0.0}):
        with pytest.raises(ValueError, match="device"):
            call(**kw)
    with pytest.raises(ValueError, match="device"):
        call(dtype=np.float64, precision=64, with_index=True)
