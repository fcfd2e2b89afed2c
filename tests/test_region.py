"""Random-access decode of a sub-box of a fixed-rate stream (decode_region /
cuzfp_hip_decode_region).

The expected value of every GPU case is the box cut out of the CPU oracle's
decode of the whole array, compared bit for bit.  The stream is the oracle's
of a smooth field, of the block zoo (tests/block_zoo.py: zero blocks beside
coded ones, a wave of zero blocks, NaN, inf, denormal and huge blocks) or
arbitrary bits that no encoder wrote.
The argument checks and the host program over csrc/region.hpp need no GPU.
"""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import block_zoo as bz
import cuzfp_amd as cz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

_REF = {}


def _reference(restatement, shape, dtype, mb):
    """(array, oracle stream, oracle decode) of a case: computed once, read only."""
    key = (shape, np.dtype(dtype).str, mb)
    if key not in _REF:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        if np.dtype(dtype).kind == "f":
            a = (np.cumsum(rng.standard_normal(shape), axis=-1) *
                 10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)
        else:
            a = rng.integers(-2 ** 30, 2 ** 30, size=shape).astype(dtype)
        ref = restatement.compress(a, mb)
        want = restatement.decompress(ref, shape, dtype, mb)
        for v in (a, ref, want):
            v.setflags(write=False)
        _REF[key] = (a, ref, want)
    return _REF[key]


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[np.dtype(dtype)]


def _words(ref, dev):
    import torch
    return torch.from_numpy(ref.view(np.int64).copy()).to(dev)


def _box(origin, extent):
    return tuple(slice(o, o + e) for o, e in zip(origin, extent))


def _same_bytes(got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _check_boxes(cuda, restatement, shape, dtype, mb, boxes, reference=None):
    """`reference`: the (array, stream, oracle decode) to use instead of _reference's."""
    import torch
    _, ref, want = reference or _reference(restatement, shape, dtype, mb)
    words = _words(ref, cuda)
    td = _torch_dtype(dtype)
    for origin, extent in boxes:
        got = cz.decode_region(words, shape, td, mb, origin, extent)
        torch.cuda.synchronize()
        assert tuple(got.shape) == tuple(extent)
        assert _same_bytes(got.cpu().numpy(), want[_box(origin, extent)]), (origin, extent)
    # the whole-array box is the first: it also equals the whole-array decoder
    full = cz.decode(words, shape, td, mb)
    whole = cz.decode_region(words, shape, td, mb, boxes[0][0], boxes[0][1])
    torch.cuda.synchronize()
    assert _same_bytes(whole.cpu().numpy(), full.cpu().numpy())


SHAPE3 = (21, 18, 37)  # 6 x 5 x 10 blocks, partial on every far edge
BOXES3 = [((0, 0, 0), (21, 18, 37)),    # the whole array
          ((5, 6, 7), (1, 1, 1)),       # one interior element
          ((1, 2, 3), (14, 9, 30)),     # unaligned on every side
          ((4, 4, 8), (12, 8, 24)),     # block-aligned interior (the row-store path)
          ((17, 15, 33), (4, 3, 4)),    # the far corner, with the stream's last block
          ((8, 0, 0), (4, 18, 37))]     # a one-block-thick z slab


def _cases3():
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        for mb in (64, 100, 512, 1280) + ((1024,) if np.dtype(dtype).itemsize == 8 else ()):
            yield pytest.param(dtype, mb, id=f"{np.dtype(dtype).name}-{mb}")


@gpu
@pytest.mark.parametrize("dtype,mb", list(_cases3()))
def test_region_3d(cuda, restatement, dtype, mb):
    """maxbits 64: word-aligned blocks; 100: blocks that straddle dwords; 512,
    1024: 16-byte loads; 1280: a block beyond the 8 held pieces."""
    _check_boxes(cuda, restatement, SHAPE3, dtype, mb, BOXES3)


SHAPE2 = (30, 275)  # 8 x 69 blocks
BOXES2 = [((0, 0), (30, 275)), ((5, 7), (1, 1)), ((1, 3), (20, 200)), ((4, 8), (12, 64)),
          ((27, 271), (3, 4)), ((8, 0), (4, 275))]
SHAPE1 = (1203,)    # 301 blocks, the last one partial
BOXES1 = [((0,), (1203,)), ((7,), (1,)), ((3,), (1000,)), ((8,), (640,)), ((1199,), (4,)),
          ((8,), (4,))]


@gpu
@pytest.mark.parametrize("mb", [17, 32, 33, 64, 128, 200])
@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.float64, np.int64])
@pytest.mark.parametrize("dims", [1, 2])
def test_region_1d_2d(cuda, restatement, dims, dtype, mb):
    """maxbits <= 64: the register reader with a per-lane base (17: several
    blocks a dword); above: the LDS image."""
    shape, boxes = (SHAPE1, BOXES1) if dims == 1 else (SHAPE2, BOXES2)
    _check_boxes(cuda, restatement, shape, dtype, mb, boxes)


# The zoo: 64 blocks along x, so a box of whole x-rows of blocks is a box of
# whole waves.  Wave 0 holds zero blocks only, wave 3 one zero block at lane
# ZERO_LANE (x = 4 * 17 = 68) among dense noise.
ZOO_BOXES = {
    1: [((0,), (1024,)),            # the whole array
        ((0,), (256,)),             # the zero wave alone
        ((256,), (512,)),           # whole waves 1 and 2
        ((515,), (400,)),           # unaligned, through waves 2 and 3
        ((768 + 68,), (4,))],       # the zero block of wave 3
    2: [((0, 0), (16, 256)), ((0, 0), (4, 256)), ((4, 0), (8, 256)), ((9, 5), (6, 200)), ((12, 68), (4, 4))],
    3: [((0, 0, 0), (4, 16, 256)), ((0, 0, 0), (4, 4, 256)), ((0, 4, 0), (4, 8, 256)), ((1, 9, 5), (2, 6, 200)),
        ((0, 12, 68), (4, 4, 4))],
}
_ZOO_REF = {}


def _zoo_reference(restatement, dims, dtype, mb):
    key = (dims, np.dtype(dtype).str, mb)
    if key not in _ZOO_REF:
        a, names = bz.zoo(dims, dtype)
        assert names[0] == names[63] == names[192 + bz.ZERO_LANE] == "zero"
        ref = restatement.compress(a, mb)
        want = restatement.decompress(ref, a.shape, dtype, mb)
        for v in (ref, want):
            v.setflags(write=False)
        _ZOO_REF[key] = (a, ref, want)
    return _ZOO_REF[key]


def _zoo_cases():
    for dims in (1, 2, 3):
        for dtype in bz.DTYPES:
            for mb in ((33,) if dims < 3 else ()) + (64, 100, 512):
                yield pytest.param(dims, dtype, mb, id=f"{dims}d-{np.dtype(dtype).name}-{mb}")


@gpu
@pytest.mark.parametrize("dims,dtype,mb", list(_zoo_cases()))
def test_region_zoo(cuda, restatement, dims, dtype, mb):
    """decode_block returning false (a wave of zero blocks) inside the region
    kernels, a zero block beside coded ones, and blocks of NaN, inf, -0.0,
    denormal and huge values; 33: the register reader."""
    ref = _zoo_reference(restatement, dims, dtype, mb)
    # the premise: the zero wave decodes to +0, the box that holds it alone too
    origin, extent = ZOO_BOXES[dims][1]
    assert not ref[2][_box(origin, extent)].view(np.uint8).any()
    _check_boxes(cuda, restatement, bz.SHAPES[dims], dtype, mb, ZOO_BOXES[dims], reference=ref)


@gpu
@pytest.mark.parametrize("density", [0.5, 0.05, 0.95])
@pytest.mark.parametrize("dtype", bz.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_region_random_streams(cuda, restatement, dims, dtype, density):
    """Streams that are not encoder output: arbitrary bits through the region
    copy-in (the funnel shift from a per-lane bit offset, the last-dword mask,
    the slack rows) into LdsReader<false> and RegReader<false, false>, whose
    budget-cut and past-the-end cases encoder output rarely reaches."""
    shape, boxes = {1: (SHAPE1, BOXES1), 2: (SHAPE2, BOXES2), 3: (SHAPE3, BOXES3)}[dims]
    rng = np.random.default_rng(zlib.crc32(f"random/{dims}/{np.dtype(dtype).str}/{density}".encode()))
    for mb in ((17, 33, 64, 200) if dims < 3 else (100, 512)):
        s = bz.random_stream(rng, bz.nblocks(shape), mb, density)
        want = restatement.decompress(s, shape, dtype, mb)
        _check_boxes(cuda, restatement, shape, dtype, mb, boxes, reference=(None, s, want))


@gpu
def test_region_many_waves(cuda, restatement):
    """6 x 9 x 21 = 1134 region blocks: 18 waves, the last one partial, in runs
    of 21 blocks (no divisor of 64)."""
    _check_boxes(cuda, restatement, (24, 40, 100), np.float32, 256,
                 [((0, 0, 0), (24, 40, 100)), ((3, 5, 6), (18, 30, 80))])


@gpu
@pytest.mark.parametrize("mb", [100, 512])
def test_region_unaligned_stream_base(cuda, restatement, mb):
    """A stream that starts 8 bytes off a 16-byte boundary takes the dword
    loads at every maxbits."""
    import torch
    _, ref, want = _reference(restatement, SHAPE3, np.float32, mb)
    buf = torch.zeros(len(ref) + 1, dtype=torch.int64, device=cuda)
    buf[1:] = _words(ref, cuda)
    words = buf[1:]
    assert words.data_ptr() % 16 == 8
    for origin, extent in BOXES3:
        got = cz.decode_region(words, SHAPE3, torch.float32, mb, origin, extent)
        torch.cuda.synchronize()
        assert _same_bytes(got.cpu().numpy(), want[_box(origin, extent)]), (origin, extent)


@gpu
def test_region_strided_destinations(cuda, restatement):
    """A step-2 view through decode_region, a reversed view through the C-ABI
    with a hand-made base pointer; everything outside the view keeps the
    sentinel."""
    import torch
    mb = 100
    _, ref, want = _reference(restatement, SHAPE3, np.float32, mb)
    words = _words(ref, cuda)
    origin, extent = (1, 2, 3), (14, 9, 30)
    box = want[_box(origin, extent)]
    # step 2 on every axis, inside a larger sentinel-filled tensor
    dst = torch.full((30, 20, 64), -7.0, dtype=torch.float32, device=cuda)
    sl = (slice(1, 29, 2), slice(2, 20, 2), slice(3, 63, 2))
    out = cz.decode_region(words, SHAPE3, torch.float32, mb, origin, extent, out=dst[sl])
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert out.data_ptr() == dst[sl].data_ptr()
    assert _same_bytes(got[sl], box)
    mask = np.ones(got.shape, bool)
    mask[sl] = False
    assert np.all(got[mask] == -7.0)
    # reversed on y and x (negative strides), step 2 on x
    host = np.full((16, 12, 70), -7.0, np.float32)
    nsl = (slice(1, 15), slice(10, 1, -1), slice(65, 5, -2))
    view = host[nsl]
    assert view.shape == extent
    st = tuple(s // 4 for s in view.strides[::-1])
    assert st[0] < 0 and st[1] < 0
    off = (view.__array_interface__["data"][0] - host.__array_interface__["data"][0]) // 4
    dst = torch.from_numpy(host).to(cuda)
    rc = cz.library().cuzfp_hip_decode_region(
        words.data_ptr(), words.numel() * 8, 3, SHAPE3[2], SHAPE3[1], SHAPE3[0], mb,
        origin[2], origin[1], origin[0], extent[2], extent[1], extent[0], st[0], st[1], st[2],
        dst.data_ptr() + 4 * off, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert _same_bytes(got[nsl], box)
    mask = np.ones(got.shape, bool)
    mask[nsl] = False
    assert np.all(got[mask] == -7.0)
    # a broadcast view is rejected, as in decode
    with pytest.raises(ValueError):
        cz.decode_region(words, SHAPE3, torch.float32, mb, origin, extent,
                         out=torch.zeros((1, 9, 30), device=cuda).expand(14, 9, 30))


@gpu
def test_region_64bit_stream_offsets(cuda, restatement):
    """Blocks past bit 2^32 of the stream: 1D f32 at 16384 bits a block, 262144
    zero blocks (which decode to zeros) and then 67 coded ones.  Block 262144
    starts at bit 2^32 exactly: a 32-bit bit offset reads block 0."""
    import torch
    mb, lead, tail = 16384, 262144, 67
    nblocks = lead + tail
    rng = np.random.default_rng(64)
    small = rng.standard_normal(4 * tail).astype(np.float32)
    sw = cz.encode(torch.from_numpy(small).to(cuda), mb)
    assert sw.numel() == tail * 256
    words = torch.zeros(nblocks * 256, dtype=torch.int64, device=cuda)  # just over 512 MiB
    words[lead * 256:] = sw  # blocks are 256 words each and position independent
    want = restatement.decompress(sw.cpu().numpy().view(np.uint64), small.shape, np.float32, mb)
    got = cz.decode_region(words, (4 * nblocks,), torch.float32, mb, (4 * lead,), (4 * tail,))
    zeros = cz.decode_region(words, (4 * nblocks,), torch.float32, mb, (4 * lead - 8,), (8,))
    torch.cuda.synchronize()
    assert _same_bytes(got.cpu().numpy(), want)
    assert _same_bytes(zeros.cpu().numpy(), np.zeros(8, np.float32))


@gpu
def test_region_graph_capture(cuda, restatement):
    """One region decode captured into a graph and replayed twice gives the
    eager call's bytes (no allocation or synchronisation inside the call)."""
    import torch
    mb = 100
    _, ref, want = _reference(restatement, SHAPE3, np.float32, mb)
    words = _words(ref, cuda)
    origin, extent = (1, 2, 3), (14, 9, 30)
    eager = cz.decode_region(words, SHAPE3, torch.float32, mb, origin, extent)
    out = torch.zeros(extent, dtype=torch.float32, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cz.decode_region(words, SHAPE3, torch.float32, mb, origin, extent, out=out)
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert _same_bytes(out.cpu().numpy(), eager.cpu().numpy())
    assert _same_bytes(eager.cpu().numpy(), want[_box(origin, extent)])


# ---------------------------------------------------------------------------
# CPU: argument checks (no launches) and the index arithmetic


@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def test_region_argument_errors(libs):
    lib = cz.library()
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: rejected before any launch
    big = 1 << 30

    def call(stream=buf, nbytes=big, t=3, n=(16, 16, 16), mb=512, o=(0, 0, 0), e=(4, 4, 4), out=buf):
        return lib.cuzfp_hip_decode_region(stream, nbytes, t, n[0], n[1], n[2], mb, o[0], o[1], o[2],
                                           e[0], e[1], e[2], 0, 0, 0, out, None)

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
    assert call(out=None) == 1
    # what make_problem rejects: type, dims, maxbits
    assert call(t=9) == 2
    assert call(n=(16, 0, 16)) == 1
    assert call(n=(0, 0, 0)) == 1
    assert call(mb=8) == 1
    assert call(mb=16385) == 1
    # a stream shorter than the whole array's
    need = cz.stream_bytes((16, 16, 16), np.float32, 512)
    assert call(nbytes=need - 8) == 3
    assert call(nbytes=100, n=(16, 16, 0), o=(0, 0, 0), e=(4, 4, 0)) == 3


def test_region_rank_mismatch(libs):
    class NoStream:  # the rank check comes before the stream is looked at
        is_cuda = False

    for origin, extent in (((0, 0), (4, 4, 4)), ((0, 0, 0), (4, 4)), ((0,), (4,)), ((0, 0, 0, 0), (4, 4, 4, 4))):
        with pytest.raises(ValueError, match="rank"):
            cz.decode_region(NoStream(), (16, 16, 16), np.float32, 512, origin, extent)
    with pytest.raises(ValueError):
        cz.decode_region(NoStream(), (16, 16, 16, 16), np.float32, 512, (0,) * 4, (4,) * 4)
    assert "decode_region" in cz.__all__


def test_region_index_map(tmp_path):
    """tests/native/region_map.cpp over csrc/region.hpp: every box of every
    shape up to 9 x 9 x 9 is covered exactly once, block bit offsets equal
    b * maxbits in 128-bit arithmetic, no load reaches the stream's end."""
    exe = str(tmp_path / "region_map")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "region_map.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
