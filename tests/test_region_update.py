"""In-place update of a sub-box of a fixed-rate stream (encode_region /
cuzfp_hip_encode_region).

Every GPU case starts from a fresh device copy of the old stream, makes one
call, synchronises and compares the whole stream's bytes with

    splice(old, R.compress(paste(R.decompress(old), box, new)), blocks_of(box))

computed on the CPU (R: oracle.restatement; splice copies the bit ranges of
the box's blocks from the second stream into the first).  The old stream is
the oracle's of a smooth field, of the block zoo (tests/block_zoo.py), or
arbitrary bits that no encoder wrote; the formula is the same.  The argument checks
and the host program over csrc/region.hpp need no GPU.
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


def _values(rng, shape, dtype):
    """Floats as test_region._reference; int32 from +-2^26 and int64 from
    +-2^28, so that re-encoding decoded values cannot overflow the oracle's
    integer transform (see _reference's assertion)."""
    if np.dtype(dtype).kind == "f":
        return (np.cumsum(rng.standard_normal(shape), axis=-1) *
                10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)
    lim = 2 ** 26 if np.dtype(dtype).itemsize == 4 else 2 ** 28
    return rng.integers(-lim, lim, size=shape).astype(dtype)


def _reference(restatement, shape, dtype, mb):
    """(old stream, its oracle decode, an array of new values) of a case:
    computed once, read only."""
    key = (shape, np.dtype(dtype).str, mb)
    if key not in _REF:
        rng = np.random.default_rng(zlib.crc32(repr(("update",) + key).encode()))
        a = _values(rng, shape, dtype)
        new = _values(rng, shape, dtype)
        old = restatement.compress(a, mb)
        dec = restatement.decompress(old, shape, dtype, mb)
        if np.dtype(dtype).kind == "i":
            # a factor of 4 below the transform's range: 2^29 for int32; int64
            # values of +-2^28 decode to 0.78 * 2^30 at 64 bits a block, far
            # inside the 64-bit transform's range, so 2^61 there
            bound = 2 ** 29 if np.dtype(dtype).itemsize == 4 else 2 ** 61
            assert np.abs(dec.astype(np.int64)).max() < bound
        for v in (old, dec, new):
            v.setflags(write=False)
        _REF[key] = (old, dec, new)
    return _REF[key]


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[np.dtype(dtype)]


def _words(stream, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(stream).view(np.int64).copy()).to(dev)


def _dev(values, dev):
    """A device tensor of (a writable copy of) a numpy array."""
    import torch
    return torch.from_numpy(np.array(values)).to(dev)


def _box(origin, extent):
    return tuple(slice(o, o + e) for o, e in zip(origin, extent))


def _same_bytes(got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    return got.nbytes == want.nbytes and np.array_equal(got.view(np.uint8).ravel(), want.view(np.uint8).ravel())


def _blocks_of(shape, origin, extent):
    """Global indices of the blocks the box touches (raster order, x fastest)."""
    nb = [(n + 3) // 4 for n in shape]
    axes = [np.arange(o // 4, (o + e + 3) // 4) for o, e in zip(origin, extent)]
    idx = np.zeros((), np.int64)
    for n, ax in zip(nb, axes):
        idx = idx[..., None] * n + ax
    return idx.ravel()


def _bits(stream):
    return np.unpackbits(np.ascontiguousarray(stream).view(np.uint8), bitorder="little")


def _splice(old, new, blocks, mb):
    """`old` with bits [b * mb, (b + 1) * mb) of `new` for every b in blocks."""
    assert old.shape == new.shape
    ob, nb = _bits(old), _bits(new)
    pos = (blocks[:, None] * mb + np.arange(mb)[None, :]).ravel()
    ob[pos] = nb[pos]
    return np.packbits(ob, bitorder="little").view(np.uint64)


def _expect(restatement, old, dec, shape, dtype, mb, origin, box_values):
    pasted = np.array(dec)
    pasted[_box(origin, box_values.shape)] = box_values
    return _splice(old, restatement.compress(pasted, mb), _blocks_of(shape, origin, box_values.shape), mb)


def _update(cuda, old, shape, dtype, mb, origin, box_values, base_offset=0):
    """One encode_region call on a fresh device copy of `old`; the stream's bytes after."""
    import torch
    if base_offset:
        buf = torch.zeros(len(old) + 1, dtype=torch.int64, device=cuda)
        buf[1:] = _words(old, cuda)
        words = buf[1:]
        assert words.data_ptr() % 16 == 8
    else:
        words = _words(old, cuda)
    x = _dev(box_values, cuda)
    out = cz.encode_region(x, words, shape, mb, origin)
    torch.cuda.synchronize()
    assert out.data_ptr() == words.data_ptr()
    return words.cpu().numpy().view(np.uint64)


def _check_boxes(cuda, restatement, shape, dtype, mb, boxes, base_offset=0, reference=None):
    """`reference`: the (old stream, its oracle decode, new values) to use
    instead of _reference's."""
    old, dec, new = reference or _reference(restatement, shape, dtype, mb)
    for origin, extent in boxes:
        vals = new[_box(origin, extent)]
        want = _expect(restatement, old, dec, shape, dtype, mb, origin, vals)
        got = _update(cuda, old, shape, dtype, mb, origin, vals, base_offset)
        assert _same_bytes(got, want), (origin, extent)


SHAPE3 = (21, 18, 37)  # 6 x 5 x 10 blocks, partial on every far edge
BOXES3 = [((0, 0, 0), (21, 18, 37)),    # the whole array
          ((5, 6, 7), (1, 1, 1)),       # one interior element
          ((1, 2, 3), (14, 9, 30)),     # unaligned on every side
          ((4, 4, 8), (12, 8, 24)),     # block-aligned interior: the covered variant
          ((17, 15, 33), (4, 3, 4)),    # the far corner: merge, padding, the stream's last block
          ((16, 16, 32), (5, 2, 5)),    # aligned origin reaching every far edge: covered, with padding
          ((8, 0, 0), (4, 18, 37))]     # a one-block-thick z slab
ALIGNED3 = BOXES3[3]


def _cases3():
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        for mb in (64, 100, 512, 1280) + ((1024,) if np.dtype(dtype).itemsize == 8 else ()):
            yield pytest.param(dtype, mb, id=f"{np.dtype(dtype).name}-{mb}")


@gpu
@pytest.mark.parametrize("dtype,mb", list(_cases3()))
def test_update_3d(cuda, restatement, dtype, mb):
    """maxbits 64: whole dwords only; 100: blocks that share dwords (atomics);
    512, 1024: 16-byte stores; 1280: a larger image."""
    import torch
    _check_boxes(cuda, restatement, SHAPE3, dtype, mb, BOXES3)
    old, dec, new = _reference(restatement, SHAPE3, dtype, mb)
    td = _torch_dtype(dtype)
    # the whole-array box also equals the whole-array encoder
    whole = _update(cuda, old, SHAPE3, dtype, mb, (0, 0, 0), new)
    full = cz.encode(_dev(new, cuda), mb)
    torch.cuda.synchronize()
    assert _same_bytes(whole, full.cpu().numpy())
    # the block-aligned box reads back through decode_region
    origin, extent = ALIGNED3
    vals = new[_box(origin, extent)]
    want = _expect(restatement, old, dec, SHAPE3, dtype, mb, origin, vals)
    words = _words(old, cuda)
    cz.encode_region(_dev(vals, cuda), words, SHAPE3, mb, origin)
    back = cz.decode_region(words, SHAPE3, td, mb, origin, extent)
    torch.cuda.synchronize()
    assert _same_bytes(back.cpu().numpy(), restatement.decompress(want, SHAPE3, dtype, mb)[_box(origin, extent)])


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
def test_update_1d_2d(cuda, restatement, dims, dtype, mb):
    """17: several blocks a dword, every store an atomic; 32, 64: no atomics;
    33: a one-bit carry; 128: 16-byte stores; 200: head, whole dwords and tail."""
    shape, boxes = (SHAPE1, BOXES1) if dims == 1 else (SHAPE2, BOXES2)
    _check_boxes(cuda, restatement, shape, dtype, mb, boxes)


# The zoo (64 blocks along x: a box of whole x-rows of blocks is a box of whole
# waves; wave 0 holds zero blocks only).
ZOO_BOXES = {
    1: [((256,), (512,)),           # block-aligned, waves 1 and 2: covered
        ((515,), (400,)),           # unaligned, through waves 2 and 3: merge
        ((0,), (256,)),             # the zero wave alone, covered
        ((3,), (250,))],            # inside the zero wave, unaligned: merge over decoded zero blocks
    2: [((4, 64), (8, 128)), ((9, 5), (6, 200)), ((0, 0), (4, 256)), ((1, 3), (2, 250))],
    3: [((0, 4, 64), (4, 8, 128)), ((1, 9, 5), (2, 6, 200)), ((0, 0, 0), (4, 4, 256)), ((1, 1, 3), (2, 2, 250))],
}
_ZOO_REF = {}


def _zoo_reference(restatement, dims, dtype, mb, rotate):
    key = (dims, np.dtype(dtype).str, mb, rotate)
    if key not in _ZOO_REF:
        a, _ = bz.zoo(dims, dtype)
        new, _ = bz.zoo(dims, dtype, rotate=rotate)
        old = restatement.compress(a, mb)
        dec = restatement.decompress(old, a.shape, dtype, mb)
        for v in (old, dec):
            v.setflags(write=False)
        _ZOO_REF[key] = (old, dec, new)
    return _ZOO_REF[key]


def _zoo_cases():
    for dims in (1, 2, 3):
        for dtype in (np.float32, np.float64):
            for mb in ((33,) if dims < 3 else ()) + (64, 100, 512):
                yield pytest.param(dims, dtype, mb, id=f"{dims}d-{np.dtype(dtype).name}-{mb}")


@gpu
@pytest.mark.parametrize("rotate", [1, 2])
@pytest.mark.parametrize("dims,dtype,mb", list(_zoo_cases()))
def test_update_zoo(cuda, restatement, dims, dtype, mb, rotate):
    """The old stream is the zoo's, the new values a zoo with its recipes moved
    `rotate` waves up: 1 puts noise over the zero wave and every class (zeros,
    NaN, inf) over coded noise blocks; 2 puts every class over the zero wave --
    the merge then decodes all zeros (decode_block returns false) and the box
    brings NaN -- and zeros over the every-class wave.  Floats only: the paste
    of a decoded integer zoo can leave the range in which the oracle's integer
    transform does not overflow; integer types keep the recipe of _values."""
    _check_boxes(cuda, restatement, bz.SHAPES[dims], dtype, mb, ZOO_BOXES[dims],
                 reference=_zoo_reference(restatement, dims, dtype, mb, rotate))


@gpu
@pytest.mark.parametrize("density", [0.5, 0.05, 0.95])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_update_random_old_stream(cuda, restatement, dims, dtype, density):
    """An old stream of arbitrary bits, which no encoder wrote: the merge
    decodes it (up to 60 % of the values +-inf at density 0.95, never NaN),
    pastes and re-encodes; the oracle does the same and is repeatable on it.
    float32 and float64 only: arbitrary decoded integers overflow the oracle's
    integer transform (see _values), so this one case has no integer form."""
    shape, boxes = {1: (SHAPE1, BOXES1), 2: (SHAPE2, BOXES2), 3: (SHAPE3, BOXES3)}[dims]
    rng = np.random.default_rng(zlib.crc32(f"random/{dims}/{np.dtype(dtype).str}/{density}".encode()))
    for mb in ((33, 200) if dims < 3 else (100,)):
        old = bz.random_stream(rng, bz.nblocks(shape), mb, density)
        dec = restatement.decompress(old, shape, dtype, mb)
        assert not np.isnan(dec).any()
        new = _values(rng, shape, dtype)
        _check_boxes(cuda, restatement, shape, dtype, mb, boxes, reference=(old, dec, new))


@gpu
@pytest.mark.parametrize("mb", [256, 100])
def test_update_many_waves(cuda, restatement, mb):
    """Up to 6 x 10 x 25 = 1500 region blocks, 24 waves; full-width rows, whose
    runs abut across lanes and waves (shared dwords at 100 bits)."""
    _check_boxes(cuda, restatement, (24, 40, 100), np.float32, mb,
                 [((0, 0, 0), (24, 40, 100)), ((3, 5, 6), (18, 30, 80)), ((3, 5, 0), (18, 30, 100))])


@gpu
@pytest.mark.parametrize("mb", [100, 1280])
def test_update_keeps_neighbours_bits(cuda, restatement, mb):
    """An old stream of all-one bits (legal for a block-aligned box, which
    decodes nothing): every bit outside the box's blocks is still one -- an
    oracle stream's zero tails would hide a cleared neighbour bit -- and the
    box's blocks are the oracle's."""
    old, dec, new = _reference(restatement, SHAPE3, np.float32, mb)
    origin, extent = ALIGNED3
    vals = new[_box(origin, extent)]
    nblocks = 6 * 5 * 10
    ones = _bits(np.zeros_like(old))
    ones[:nblocks * mb] = 1  # the final word's padding stays zero
    ones = np.packbits(ones, bitorder="little").view(np.uint64)
    blocks = _blocks_of(SHAPE3, origin, extent)
    # a covered block's code depends on the box's values alone
    pasted = np.array(dec)
    pasted[_box(origin, extent)] = vals
    want = _splice(ones, restatement.compress(pasted, mb), blocks, mb)
    got = _update(cuda, ones, SHAPE3, np.float32, mb, origin, vals)
    outside = np.ones(nblocks * mb, bool)
    outside[(blocks[:, None] * mb + np.arange(mb)[None, :]).ravel()] = False
    gb = _bits(got)
    assert gb[:nblocks * mb][outside].all()
    assert not gb[nblocks * mb:].any()
    assert _same_bytes(got, want)


@gpu
@pytest.mark.parametrize("mb", [100, 512])
def test_update_unaligned_stream_base(cuda, restatement, mb):
    """A stream that starts 8 bytes off a 16-byte boundary takes dword stores
    at every maxbits."""
    _check_boxes(cuda, restatement, SHAPE3, np.float32, mb, BOXES3, base_offset=8)


@gpu
def test_update_strided_sources(cuda, restatement):
    """A step-2 view through encode_region, a view reversed on y and x through
    the C-ABI with a hand-made base pointer, a broadcast constant box: each
    gives the contiguous call's stream."""
    import torch
    mb = 100
    old, dec, new = _reference(restatement, SHAPE3, np.float32, mb)
    origin, extent = (1, 2, 3), (14, 9, 30)
    vals = np.ascontiguousarray(new[_box(origin, extent)])
    want = _expect(restatement, old, dec, SHAPE3, np.float32, mb, origin, vals)
    contiguous = _update(cuda, old, SHAPE3, np.float32, mb, origin, vals)
    assert _same_bytes(contiguous, want)
    # step 2 on every axis, inside a larger sentinel-filled tensor
    host = np.full((30, 20, 64), -7.0, np.float32)
    sl = (slice(1, 29, 2), slice(2, 20, 2), slice(3, 63, 2))
    host[sl] = vals
    src = torch.from_numpy(host).to(cuda)
    words = _words(old, cuda)
    cz.encode_region(src[sl], words, SHAPE3, mb, origin)
    torch.cuda.synchronize()
    assert _same_bytes(words.cpu().numpy(), contiguous)
    # reversed on y and x (negative strides), step 2 on x
    host = np.full((16, 12, 70), -7.0, np.float32)
    nsl = (slice(1, 15), slice(10, 1, -1), slice(65, 5, -2))
    host[nsl] = vals
    view = host[nsl]
    assert view.shape == extent
    st = tuple(s // 4 for s in view.strides[::-1])
    assert st[0] < 0 and st[1] < 0
    off = (view.__array_interface__["data"][0] - host.__array_interface__["data"][0]) // 4
    src = torch.from_numpy(host).to(cuda)
    words = _words(old, cuda)
    rc = cz.library().cuzfp_hip_encode_region(
        src.data_ptr() + 4 * off, 3, SHAPE3[2], SHAPE3[1], SHAPE3[0], mb,
        origin[2], origin[1], origin[0], extent[2], extent[1], extent[0], st[0], st[1], st[2],
        words.data_ptr(), words.numel() * 8, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert _same_bytes(words.cpu().numpy(), contiguous)
    # fill the box with a constant: a broadcast (zero-stride) view
    const = np.full(extent, 2.5, np.float32)
    want = _expect(restatement, old, dec, SHAPE3, np.float32, mb, origin, const)
    words = _words(old, cuda)
    cz.encode_region(torch.full((1, 1, 1), 2.5, dtype=torch.float32, device=cuda).expand(*extent),
                     words, SHAPE3, mb, origin)
    torch.cuda.synchronize()
    assert _same_bytes(words.cpu().numpy(), _update(cuda, old, SHAPE3, np.float32, mb, origin, const))
    assert _same_bytes(words.cpu().numpy(), want)


@gpu
def test_update_64bit_stream_offsets(cuda, restatement):
    """Blocks past bit 2^32 of the stream: 1D f32 at 16384 bits a block, 262144
    zero blocks and then 67.  Block 262144 starts at bit 2^32 exactly: a 32-bit
    bit offset writes block 0."""
    import torch
    mb, lead, tail = 16384, 262144, 67
    nblocks = lead + tail
    shape = (4 * nblocks,)
    rng = np.random.default_rng(64)
    small = rng.standard_normal(4 * tail).astype(np.float32)
    sw = cz.encode(torch.from_numpy(small).to(cuda), mb)
    assert sw.numel() == tail * 256
    words = torch.zeros(nblocks * 256, dtype=torch.int64, device=cuda)  # just over 512 MiB
    cz.encode_region(torch.from_numpy(small).to(cuda), words, shape, mb, (4 * lead,))
    torch.cuda.synchronize()
    assert torch.equal(words[lead * 256:], sw)
    assert int(torch.count_nonzero(words[:lead * 256])) == 0
    # one unaligned update of 4 elements over the blocks lead - 1 and lead,
    # against the CPU expectation on that two-block sub-stream (blocks are
    # position independent)
    sub = slice((lead - 1) * 256, (lead + 1) * 256)
    old = words[sub].cpu().numpy().view(np.uint64)
    after = words[(lead + 1) * 256:].clone()
    vals = rng.standard_normal(4).astype(np.float32)
    dec = restatement.decompress(old, (8,), np.float32, mb)
    want = _expect(restatement, old, dec, (8,), np.float32, mb, (2,), vals)
    cz.encode_region(torch.from_numpy(vals).to(cuda), words, shape, mb, (4 * lead - 2,))
    torch.cuda.synchronize()
    assert _same_bytes(words[sub].cpu().numpy(), want)
    assert int(torch.count_nonzero(words[:(lead - 1) * 256])) == 0
    assert torch.equal(words[(lead + 1) * 256:], after)


@gpu
def test_update_graph_capture(cuda, restatement):
    """One block-aligned update captured into a graph; the stream is restored
    before each of two replays, and each gives the eager call's bytes (no
    allocation or synchronisation inside the call)."""
    import torch
    mb = 100
    old, dec, new = _reference(restatement, SHAPE3, np.float32, mb)
    origin, extent = ALIGNED3
    vals = np.ascontiguousarray(new[_box(origin, extent)])
    eager = _update(cuda, old, SHAPE3, np.float32, mb, origin, vals)
    assert _same_bytes(eager, _expect(restatement, old, dec, SHAPE3, np.float32, mb, origin, vals))
    x = torch.from_numpy(vals).to(cuda)
    keep = _words(old, cuda)
    words = keep.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cz.encode_region(x, words, SHAPE3, mb, origin)
    for _ in range(2):
        words.copy_(keep)
        g.replay()
        torch.cuda.synchronize()
        assert _same_bytes(words.cpu().numpy(), eager)


# ---------------------------------------------------------------------------
# CPU: argument checks (no launches) and the span arithmetic


@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def test_update_argument_errors(libs):
    lib = cz.library()
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: rejected before any launch
    big = 1 << 30

    def call(box=buf, t=3, n=(16, 16, 16), mb=512, o=(0, 0, 0), e=(4, 4, 4), stream=buf, nbytes=big):
        return lib.cuzfp_hip_encode_region(box, t, n[0], n[1], n[2], mb, o[0], o[1], o[2],
                                           e[0], e[1], e[2], 0, 0, 0, stream, nbytes, None)

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
    assert call(box=None) == 1
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


def test_update_python_errors(libs):
    class NoTensor:  # the checks come before any tensor is looked at
        is_cuda = False

        def __init__(self, shape=()):
            self.shape = shape

    words = NoTensor()
    shape = (16, 16, 16)
    for box, origin in (((4, 4), (0, 0, 0)), ((4, 4, 4), (0, 0)), ((4,), (0,)), ((4,) * 4, (0,) * 4)):
        with pytest.raises(ValueError, match="rank"):
            cz.encode_region(NoTensor(box), words, shape, 512, origin)
    with pytest.raises(ValueError, match="non-negative"):
        cz.encode_region(NoTensor((4, 4, 4)), words, shape, 512, (0, -1, 0))
    for box, origin in (((4, 4, 4), (13, 0, 0)), ((4, 17, 4), (0, 0, 0)), ((4, 4, 4), (0, 0, 16))):
        with pytest.raises(ValueError, match="leaves"):
            cz.encode_region(NoTensor(box), words, shape, 512, origin)
    assert "encode_region" in cz.__all__


def test_update_store_spans(tmp_path):
    """tests/native/region_store.cpp over csrc/region.hpp: the head mask, whole
    dwords and tail mask of a block cover exactly its bits, are disjoint from
    its neighbours' and stay inside the stream."""
    exe = str(tmp_path / "region_store")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "region_store.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
