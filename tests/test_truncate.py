"""Lowering a stream's rate without recoding (truncate / cuzfp_hip_truncate)
and decoding at a lower rate than the stream's (prefix_bits /
cuzfp_hip_decode_region_prefix).

zfp's coder is embedded: a block coded with a budget of m bits is the first m
bits of the same block coded with any larger budget M.  So every expectation
here is exact bytes from the CPU oracle at the lower rate (R:
oracle.restatement) -- nothing is recomputed, there are no tolerances:

    truncate(R.compress(a, M), M -> m)       == R.compress(a, m)
    decode(R.compress(a, M), prefix_bits=m)  == R.decompress(R.compress(a, m), m)

test_prefix_property_golden checks the property itself on the reference's own
streams (tests/golden/streams.npz) with a numpy bit model, without the library.
test_prefix_property_zoo checks it on the block zoo (tests/block_zoo.py), whose
streams the zoo cases here decode.  For a stream of arbitrary bits, which no
encoder wrote, the expectations are the definition itself (_cpu_truncate) and
the oracle's decode of the stream so truncated.
Every GPU case makes a fresh device copy of the source stream, one call,
synchronises and compares whole buffers.
"""
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import block_zoo as bz
import cuzfp_amd as cz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
gpu = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
_ARRAYS = {}
_STREAMS = {}


def _floor(dtype):
    """The least maxbits of a type: 1 + the exponent bits of a float."""
    return {np.dtype(np.float32): 9, np.dtype(np.float64): 12}.get(np.dtype(dtype), 1)


def _values(rng, shape, dtype):
    """The recipe of test_region_update._values."""
    if np.dtype(dtype).kind == "f":
        return (np.cumsum(rng.standard_normal(shape), axis=-1) *
                10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)
    lim = 2 ** 26 if np.dtype(dtype).itemsize == 4 else 2 ** 28
    return rng.integers(-lim, lim, size=shape).astype(dtype)


def _array(shape, dtype):
    key = (shape, np.dtype(dtype).str)
    if key not in _ARRAYS:
        rng = np.random.default_rng(zlib.crc32(repr(("truncate",) + key).encode()))
        a = _values(rng, shape, dtype)
        a.setflags(write=False)
        _ARRAYS[key] = a
    return _ARRAYS[key]


def _stream(restatement, shape, dtype, mb, zoo=False):
    """The oracle's stream of _array(shape, dtype), or of the block zoo of that
    shape, at mb: computed once, read only."""
    key = (shape, np.dtype(dtype).str, mb, zoo)
    if key not in _STREAMS:
        s = restatement.compress(bz.zoo(len(shape), dtype, shape)[0] if zoo else _array(shape, dtype), mb)
        s.setflags(write=False)
        _STREAMS[key] = s
    return _STREAMS[key]


def _nblocks(shape):
    return int(np.prod([(n + 3) // 4 for n in shape]))


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[np.dtype(dtype)]


def _words(stream, dev, offset=0):
    """A fresh device copy of a stream; offset 1: its base 8 bytes off a
    16-byte boundary (as test_region_update._update(base_offset=1))."""
    import torch
    w = torch.from_numpy(np.ascontiguousarray(stream).view(np.int64).copy()).to(dev)
    if offset:
        buf = torch.zeros(len(stream) + 1, dtype=torch.int64, device=dev)
        buf[1:] = w
        w = buf[1:]
    assert w.data_ptr() % 16 == 8 * offset
    return w


def _box(origin, extent):
    return tuple(slice(o, o + e) for o, e in zip(origin, extent))


def _same_bytes(got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    return got.nbytes == want.nbytes and np.array_equal(got.view(np.uint8).ravel(), want.view(np.uint8).ravel())


def _cpu_truncate(stream, nblocks, M, m):
    """The definition, a bit at a time: output bit b*m + i = source bit b*M + i
    for i < m, zero padded to a whole 64-bit word."""
    bits = np.unpackbits(np.ascontiguousarray(stream).view(np.uint8), bitorder="little")
    pos = (np.arange(nblocks, dtype=np.int64)[:, None] * M + np.arange(m, dtype=np.int64)[None, :]).ravel()
    out = np.zeros((nblocks * m + 63) // 64 * 64, np.uint8)
    out[:nblocks * m] = bits[pos]
    return np.packbits(out, bitorder="little").view(np.uint64)


# ---------------------------------------------------------------------------
# GPU: truncate

GENERAL_PAIRS = [(33, 1), (17, 9), (64, 63), (65, 64), (100, 33), (200, 100), (1280, 100), (4200, 1000)]
WORD_PAIRS = [(192, 64), (512, 256), (1280, 512), (1280, 128), (2048, 1920), (512, 512)]


def _pairs(dtype):
    """(M, m) with m raised to the type's floor where needed."""
    out = []
    for M, m in GENERAL_PAIRS + WORD_PAIRS:
        m = max(m, _floor(dtype))
        assert m <= M
        out.append((M, m))
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(37,), (18, 37), (21, 18, 37)], ids=str)
def test_truncate_equals_lower_rate_encode(cuda, restatement, shape, dtype):
    """Partial blocks and a last word that is not full; pairs of the general
    path (a 64-bit output word a lane) and of the word path (both rates
    multiples of 64, 16 bytes a lane when both are multiples of 128)."""
    import torch
    for M, m in _pairs(dtype):
        src = _words(_stream(restatement, shape, dtype, M), cuda)
        out = cz.truncate(src, shape, dtype, M, m)
        torch.cuda.synchronize()
        assert out.dtype == torch.int64 and out.numel() * 8 == cz.stream_bytes(shape, dtype, m)
        assert _same_bytes(out.cpu().numpy(), _stream(restatement, shape, dtype, m)), (M, m)


def _rate_maxbits(rate, dtype, dims):
    """zfp's stream_set_rate without word alignment (cuzfp_hip_rate_to_maxbits)."""
    return max(int(np.floor(4 ** dims * rate + 0.5)), _floor(dtype) if np.dtype(dtype).kind == "f" else 0)


def _golden_pairs():
    """(name, shape, dtype, higher stream, M, lower stream, m) for every pair of
    rates of a field of tests/golden/streams.npz whose maxbits, from the rate,
    are what the stored sizes imply and are not clamped up to the type's floor
    (the lowest 1D rates are)."""
    streams = {k.replace("__", "/"): v for k, v in np.load(os.path.join(GOLDEN, "streams.npz")).items()}
    cases = json.load(open(os.path.join(GOLDEN, "golden.json")))["cases"]
    fields = {}
    for name, s in streams.items():
        if not name.startswith("fields/"):
            continue
        rec = cases[name]
        shape, dtype = tuple(rec["shape"]), np.dtype(rec["dtype"])
        mb = _rate_maxbits(rec["rate"], dtype, len(shape))
        if mb != 4 ** len(shape) * rec["rate"] or len(s) != (_nblocks(shape) * mb + 63) // 64:
            continue
        assert mb == rec["maxbits"]
        fields.setdefault((name.split("/")[1], shape, dtype.str), []).append((mb, s))
    out = []
    for (field, shape, dtype), rates in sorted(fields.items()):
        rates.sort(key=lambda r: -r[0])
        for i, (M, hi) in enumerate(rates):
            for m, lo in rates[i + 1:]:
                out.append((f"{field}/{M}->{m}", shape, np.dtype(dtype), hi, M, lo, m))
    return out


@gpu
def test_truncate_reference_golden_pairs(cuda):
    """The reference zfp's own streams: the higher-rate one, truncated, is the
    stored lower-rate one."""
    import torch
    pairs = _golden_pairs()
    assert len(pairs) == 22
    for name, shape, dtype, hi, M, lo, m in pairs:
        assert M == cz.rate_to_maxbits(M / 4 ** len(shape), dtype, len(shape))
        assert m == cz.rate_to_maxbits(m / 4 ** len(shape), dtype, len(shape))
        out = cz.truncate(_words(hi, cuda), shape, dtype, M, m)
        torch.cuda.synchronize()
        assert _same_bytes(out.cpu().numpy(), lo), name


SENTINEL = 0x5A5A5A5A5A5A5A5A


@gpu
@pytest.mark.parametrize("M,m", [(512, 256), (100, 33)])
def test_truncate_many_waves_bases_bounds(cuda, restatement, M, m):
    """4096 blocks; source and destination bases at 0 and 8 mod 16 (the 16-byte
    moves need both at 0); a destination 64 words too long keeps its sentinel
    past the stream, and out_bytes is the stream's size."""
    import torch
    shape, dtype = (64, 64, 64), np.float32
    want = _stream(restatement, shape, dtype, m)
    need = cz.stream_bytes(shape, dtype, m)
    assert need == want.nbytes
    for so in (0, 1):
        for do in (0, 1):
            src = _words(_stream(restatement, shape, dtype, M), cuda, so)
            buf = torch.full((do + need // 8 + 64,), SENTINEL, dtype=torch.int64, device=cuda)
            dst = buf[do:]
            assert dst.data_ptr() % 16 == 8 * do
            got = ctypes.c_size_t(0)
            rc = cz.library().cuzfp_hip_truncate(src.data_ptr(), src.numel() * 8, 3, 64, 64, 64, M, m,
                                                 dst.data_ptr(), dst.numel() * 8, ctypes.byref(got), None)
            assert rc == 0
            torch.cuda.synchronize()
            assert got.value == need
            host = buf.cpu().numpy()
            assert _same_bytes(host[do:do + need // 8], want), (so, do)
            assert np.all(host[:do] == SENTINEL) and np.all(host[do + need // 8:] == SENTINEL), (so, do)
            # the same through the Python entry with `out`
            buf.fill_(SENTINEL)
            out = cz.truncate(src, shape, dtype, M, m, out=dst)
            torch.cuda.synchronize()
            assert out.data_ptr() == dst.data_ptr()
            assert _same_bytes(buf.cpu().numpy(), host)


@gpu
def test_truncate_64bit_positions(cuda):
    """Positions past bit 2^32: 1D f32 at 16384 bits a block, 262144 zero blocks
    and then 67 coded ones (as test_update_64bit_stream_offsets).  To 8192
    (word path) the source crosses bit 2^32; to 16383 (general path) the output
    crosses it too, at block 262161.  lead * m is a multiple of 64 in both, so
    the output's tail is the CPU truncation of the 67-block sub-stream."""
    import torch
    M, lead, tail = 16384, 262144, 67
    nblocks = lead + tail
    shape = (4 * nblocks,)
    rng = np.random.default_rng(64)
    small = rng.standard_normal(4 * tail).astype(np.float32)
    sw = cz.encode(torch.from_numpy(small).to(cuda), M)
    assert sw.numel() == tail * 256
    words = torch.zeros(nblocks * 256, dtype=torch.int64, device=cuda)  # just over 512 MiB
    words[lead * 256:] = sw
    torch.cuda.synchronize()
    sub = sw.cpu().numpy().view(np.uint64)
    for m in (8192, 16383):
        assert lead * m % 64 == 0
        out = cz.truncate(words, shape, np.float32, M, m)
        torch.cuda.synchronize()
        assert out.numel() == (nblocks * m + 63) // 64
        assert int(torch.count_nonzero(out[:lead * m // 64])) == 0
        assert _same_bytes(out[lead * m // 64:].cpu().numpy(), _cpu_truncate(sub, tail, M, m)), m
        del out


@gpu
def test_truncate_graph_capture(cuda, restatement):
    """One call captured into a graph; the destination is cleared before each
    of two replays, and each gives the eager call's bytes."""
    import torch
    shape, dtype, M, m = (21, 18, 37), np.float32, 100, 33
    src = _words(_stream(restatement, shape, dtype, M), cuda)
    eager = cz.truncate(src, shape, dtype, M, m)
    torch.cuda.synchronize()
    assert _same_bytes(eager.cpu().numpy(), _stream(restatement, shape, dtype, m))
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cz.truncate(src, shape, dtype, M, m, out=out)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same_bytes(out.cpu().numpy(), eager.cpu().numpy())


# ---------------------------------------------------------------------------
# GPU: prefix decode

SHAPE3 = (21, 18, 37)  # 6 x 5 x 10 blocks, partial on every far edge
BOXES3 = [((1, 2, 3), (14, 9, 30)),     # unaligned on every side
          ((4, 4, 8), (12, 8, 24)),     # block-aligned interior (the row-store path)
          ((17, 15, 33), (4, 3, 4))]    # the far corner, with the stream's last block
SHAPE2 = (30, 275)
BOXES2 = [((1, 3), (20, 200)), ((4, 8), (12, 64)), ((27, 271), (3, 4))]
SHAPE1 = (1203,)
BOXES1 = [((3,), (1000,)), ((8,), (640,)), ((1199,), (4,))]


def _check_prefix(cuda, restatement, shape, dtype, M, m, boxes, zoo=False, source=None):
    """`source`: a stream at M to decode instead of the oracle's; the expected
    value is then the oracle's decode of its CPU truncation to m."""
    import torch
    td = _torch_dtype(dtype)
    if source is None:
        source = _stream(restatement, shape, dtype, M, zoo)
        lower = _stream(restatement, shape, dtype, m, zoo)
    else:
        lower = _cpu_truncate(source, _nblocks(shape), M, m)
    want = restatement.decompress(lower, shape, dtype, m)
    words = _words(source, cuda)
    for origin, extent in boxes:
        got = cz.decode_region(words, shape, td, M, origin, extent, prefix_bits=m)
        torch.cuda.synchronize()
        assert tuple(got.shape) == tuple(extent)
        assert _same_bytes(got.cpu().numpy(), want[_box(origin, extent)]), (M, m, origin, extent)
    # the whole array through decode
    full = cz.decode(words, shape, td, M, prefix_bits=m)
    torch.cuda.synchronize()
    assert tuple(full.shape) == shape
    assert _same_bytes(full.cpu().numpy(), want), (M, m)


@gpu
@pytest.mark.parametrize("M,m", [(1280, 100), (512, 256), (100, 33), (512, 128)])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_prefix_decode_3d(cuda, restatement, dtype, M, m):
    """(512, 256), (512, 128): 16-byte copy-in under a 16-byte stride; (1280,
    100): dword loads under one; (100, 33): blocks that straddle dwords."""
    _check_prefix(cuda, restatement, SHAPE3, dtype, M, m, BOXES3)


@gpu
@pytest.mark.parametrize("M,m", [(128, 64), (100, 33), (64, 17), (200, 100)])
@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.float64, np.int64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dims", [1, 2])
def test_prefix_decode_1d_2d(cuda, restatement, dims, dtype, M, m):
    """(128, 64), (100, 33): the register path (budget <= 64) under a stride
    that alone would take the LDS image; (64, 17): both register-sized; (200,
    100): the LDS image."""
    shape, boxes = (SHAPE1, BOXES1) if dims == 1 else (SHAPE2, BOXES2)
    _check_prefix(cuda, restatement, shape, dtype, M, m, boxes)


# The zoo (64 blocks along x: a box of whole x-rows of blocks is a box of whole
# waves): the whole array, the zero wave alone, whole waves 1 and 2, an
# unaligned box through waves 2 and 3, the zero block of wave 3.
ZOO_PAIRS = [(512, 100), (100, 33), (128, 64)]
ZOO_BOXES = {
    1: [((0,), (1024,)), ((0,), (256,)), ((256,), (512,)), ((515,), (400,)), ((768 + 68,), (4,))],
    2: [((0, 0), (16, 256)), ((0, 0), (4, 256)), ((4, 0), (8, 256)), ((9, 5), (6, 200)), ((12, 68), (4, 4))],
    3: [((0, 0, 0), (4, 16, 256)), ((0, 0, 0), (4, 4, 256)), ((0, 4, 0), (4, 8, 256)), ((1, 9, 5), (2, 6, 200)),
        ((0, 12, 68), (4, 4, 4))],
}


@gpu
@pytest.mark.parametrize("M,m", ZOO_PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_prefix_decode_and_truncate_zoo(cuda, restatement, dims, dtype, M, m):
    """Zero blocks beside coded ones, a wave of zero blocks, NaN, inf, -0.0,
    denormal and huge blocks, decoded at a lower rate than the stream's
    (test_prefix_property_zoo holds the property), and truncated to it."""
    import torch
    shape = bz.SHAPES[dims]
    _check_prefix(cuda, restatement, shape, dtype, M, m, ZOO_BOXES[dims], zoo=True)
    out = cz.truncate(_words(_stream(restatement, shape, dtype, M, True), cuda), shape, dtype, M, m)
    torch.cuda.synchronize()
    assert _same_bytes(out.cpu().numpy(), _stream(restatement, shape, dtype, m, True)), (M, m)


RANDOM_PAIRS = {1: [(128, 64), (100, 33), (64, 17), (200, 100)], 2: [(128, 64), (100, 33), (64, 17), (200, 100)],
                3: [(1280, 100), (512, 256), (100, 33)]}


@gpu
@pytest.mark.parametrize("density", [0.5, 0.05, 0.95])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_prefix_decode_and_truncate_random_streams(cuda, restatement, dims, dtype, density):
    """Streams that are not encoder output, on the shapes and boxes above:
    truncate against its definition (_cpu_truncate, no oracle), prefix decode
    against the oracle's decode of the stream so truncated."""
    import torch
    shape, boxes = {1: (SHAPE1, BOXES1), 2: (SHAPE2, BOXES2), 3: (SHAPE3, BOXES3)}[dims]
    rng = np.random.default_rng(zlib.crc32(f"random/{dims}/{np.dtype(dtype).str}/{density}".encode()))
    for M, m in RANDOM_PAIRS[dims]:
        s = bz.random_stream(rng, _nblocks(shape), M, density)
        out = cz.truncate(_words(s, cuda), shape, dtype, M, m)
        torch.cuda.synchronize()
        assert _same_bytes(out.cpu().numpy(), _cpu_truncate(s, _nblocks(shape), M, m)), (M, m)
        _check_prefix(cuda, restatement, shape, dtype, M, m, boxes, source=s)


@gpu
def test_prefix_equal_to_maxbits_and_strided_out(cuda, restatement):
    """prefix_bits == maxbits is decode_region's output; a step-2 `out` view
    takes the box and leaves the sentinel everywhere else."""
    import torch
    shape, dtype = SHAPE3, np.float32
    for M in (100, 512):
        words = _words(_stream(restatement, shape, dtype, M), cuda)
        for origin, extent in BOXES3:
            a = cz.decode_region(words, shape, torch.float32, M, origin, extent)
            b = cz.decode_region(words, shape, torch.float32, M, origin, extent, prefix_bits=M)
            torch.cuda.synchronize()
            assert _same_bytes(a.cpu().numpy(), b.cpu().numpy()), (M, origin, extent)
    M, m = 512, 100
    origin, extent = BOXES3[0]
    want = restatement.decompress(_stream(restatement, shape, dtype, m), shape, dtype, m)[_box(origin, extent)]
    words = _words(_stream(restatement, shape, dtype, M), cuda)
    dst = torch.full((30, 20, 64), -7.0, dtype=torch.float32, device=cuda)
    sl = (slice(1, 29, 2), slice(2, 20, 2), slice(3, 63, 2))
    out = cz.decode_region(words, shape, torch.float32, M, origin, extent, out=dst[sl], prefix_bits=m)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert out.data_ptr() == dst[sl].data_ptr()
    assert _same_bytes(got[sl], want)
    mask = np.ones(got.shape, bool)
    mask[sl] = False
    assert np.all(got[mask] == -7.0)


# ---------------------------------------------------------------------------
# CPU: argument checks (no launches), the position arithmetic, the property


@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def test_truncate_argument_errors(libs):
    lib = cz.library()
    base = 0x100000  # never dereferenced: every call is rejected before any launch
    big = 1 << 30
    need_src = cz.stream_bytes((16, 16, 16), np.float32, 512)
    need_dst = cz.stream_bytes((16, 16, 16), np.float32, 256)

    def call(src=base, src_bytes=big, t=3, n=(16, 16, 16), mb=512, new=256, dst=base + (1 << 24), cap=big):
        got = ctypes.c_size_t(0)
        return lib.cuzfp_hip_truncate(ctypes.c_void_p(src) if src else None, src_bytes, t, n[0], n[1], n[2], mb,
                                      new, ctypes.c_void_p(dst) if dst else None, cap, ctypes.byref(got), None)

    # widening, and a rate below the type's floor
    assert call(new=513) == 1
    assert call(mb=100, new=101) == 1
    assert call(new=8) == 1
    assert call(t=4, new=11) == 1
    assert call(t=1, new=0) == 1
    assert call(t=2, new=0) == 1
    # null pointers
    assert call(src=None) == 1
    assert call(dst=None) == 1
    # what make_problem rejects: type, dims, maxbits
    assert call(t=9) == 2
    assert call(n=(16, 0, 16)) == 1
    assert call(n=(0, 0, 0)) == 1
    assert call(mb=8, new=8) == 1
    assert call(mb=16385) == 1
    # overlapping ranges [src, + stream_bytes(M)) and [dst, + stream_bytes(m)):
    # rejected whatever the capacities say
    assert call(dst=base) == 1                      # in place
    assert call(dst=base + need_src - 8) == 1       # the source's last word
    assert call(dst=base - need_dst + 8) == 1       # the destination's last word
    assert call(dst=base + 8, cap=need_dst - 8) == 1
    # adjacent ranges pass the overlap check: they get as far as the size
    # checks, which these calls fail
    assert call(dst=base + need_src, cap=need_dst - 8) == 3
    assert call(dst=base - need_dst, cap=need_dst - 8) == 3
    assert call(dst=base + need_src, src_bytes=need_src - 8) == 3
    # short buffers
    assert call(src_bytes=need_src - 8) == 3
    assert call(cap=need_dst - 8) == 3
    assert call(src_bytes=100, n=(16, 16, 0), mb=100, new=33) == 3


def test_prefix_argument_errors(libs):
    lib = cz.library()
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: rejected before any launch
    big = 1 << 30

    def call(stream=buf, nbytes=big, t=3, n=(16, 16, 16), mb=512, pb=256, o=(0, 0, 0), e=(4, 4, 4), out=buf):
        return lib.cuzfp_hip_decode_region_prefix(stream, nbytes, t, n[0], n[1], n[2], mb, pb, o[0], o[1], o[2],
                                                  e[0], e[1], e[2], 0, 0, 0, out, None)

    # prefix_bits above maxbits or below the type's floor
    assert call(pb=513) == 1
    assert call(pb=8) == 1
    assert call(t=4, pb=11) == 1
    assert call(t=1, pb=0) == 1
    # the rules of cuzfp_hip_decode_region
    assert call(e=(0, 4, 4)) == 1
    assert call(o=(13, 0, 0)) == 1
    assert call(n=(16, 16, 0), o=(0, 0, 1), e=(4, 4, 0)) == 1
    assert call(stream=None) == 1
    assert call(out=None) == 1
    assert call(t=9) == 2
    assert call(n=(16, 0, 16)) == 1
    assert call(mb=8, pb=8) == 1
    assert call(mb=16385) == 1
    # the stream must cover the whole array at maxbits, not at prefix_bits
    assert call(nbytes=cz.stream_bytes((16, 16, 16), np.float32, 512) - 8) == 3
    assert call(nbytes=cz.stream_bytes((16, 16, 16), np.float32, 256)) == 3


def test_truncate_python_errors(libs):
    class NoTensor:  # the checks come before any tensor is looked at
        is_cuda = False

    with pytest.raises(ValueError, match="widening"):
        cz.truncate(NoTensor(), (16, 16, 16), np.float32, 256, 512)
    with pytest.raises(ValueError, match="device"):
        cz.truncate(NoTensor(), (16, 16, 16), np.float32, 512, 256)
    with pytest.raises(ValueError, match="prefix_bits"):
        cz.decode_region(NoTensor(), (16, 16, 16), np.float32, 256, (0, 0, 0), (4, 4, 4), prefix_bits=512)
    assert "truncate" in cz.__all__


def test_rerate_position_arithmetic(tmp_path):
    """tests/native/rerate_map.cpp over csrc/rerate.hpp: every output word,
    assembled by the functions the kernels call, equals a bit-at-a-time loop,
    for every 1 <= m <= M <= 130 and a few large pairs; the index functions
    hold at word indices around 2^26 and 2^40."""
    exe = str(tmp_path / "rerate_map")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "rerate_map.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr


def test_prefix_property_golden():
    """The property the GPU expectations rest on, on the reference zfp's own
    streams and without the library: the per-block m-bit prefix of the stream
    at M is the stream at m, for all 22 counted pairs of the golden fields."""
    pairs = _golden_pairs()
    assert len(pairs) == 22
    for name, shape, dtype, hi, M, lo, m in pairs:
        assert _same_bytes(_cpu_truncate(hi, _nblocks(shape), M, m), lo), name


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_prefix_property_zoo(restatement, dims, dtype):
    """The same property on the block zoo, for the pairs its GPU cases use:
    _cpu_truncate(R.compress(zoo, M), M -> m) == R.compress(zoo, m), zero, NaN,
    inf, denormal and huge blocks included."""
    shape = bz.SHAPES[dims]
    a, _ = bz.zoo(dims, dtype)
    for M, m in ZOO_PAIRS:
        hi, lo = restatement.compress(a, M), restatement.compress(a, m)
        assert _same_bytes(_cpu_truncate(hi, _nblocks(shape), M, m), lo), (M, m)
