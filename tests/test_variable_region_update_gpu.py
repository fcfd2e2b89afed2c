"""encode_region_variable on the GPU against the host model of
tests/test_variable_region_update.py: A, M and E from the host emulation
(`varemu`, vouched for by the fixture hashes), spliced in numpy.  The source
streams are the reference's (through `ref_of`, accepted on the fixture's
hashes) wherever the fixture has the case, the emulation's otherwise.

Every comparison is of bytes.  The raw C-ABI runs on buffers with canaries on
both sides of the stream, the lengths, the index, the count and the workspace;
the wrapper's `out` is filled with all-ones words first, and what lies past the
result must still hold the fill.
"""
import ctypes

import numpy as np
import pytest

import block_zoo as bz
import test_variable as tv
import test_variable_paths as tp
import test_variable_region_update as ru
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_gpu import CANARY, _dev, _lengths, _tdtype, _words
from test_variable_gpu import ref_of as tv_ref_of
from test_variable_paths import F32, F64, want_index
from test_variable_truncate import tp_golden, tv_golden  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = -1  # all-ones words
ICANARY = int(np.uint64(CANARY).astype(np.int64))
BIG = (13, 22, 38)  # 240 blocks: four waves, the last ragged; partial blocks on every axis
SHAPES = [BIG, (33, 70), (1000,), (6, 5, 9)]
SRC_MODES = [("p", 16), ("a", 1e-3)]


def kw_of(mode):
    return {"precision": mode[1]} if mode[0] == "p" else {"tolerance": mode[1]}


def source(varemu, tv_golden, shape, dt, mode):  # noqa: F811
    """(words, L) of tv.array(shape, dt) at `mode`: the reference's where the fixture has the case."""
    if mode[0] == "p" and mode[1] in tv.PRECISIONS[np.dtype(dt)] or mode[0] == "a" and mode[1] in tv.TOLERANCES:
        ref = tv_ref_of(varemu, tv_golden, (tuple(shape), np.dtype(dt)) + tuple(mode))
        return ref[0], ref[1]
    words, L, _ = tv.emu_compress(varemu, tv.array(shape, dt), *ru.mode_of(dt, mode))
    return words, L


class Raw:
    """The C-ABI on buffers with canaries on both sides of every output."""
    PAD = 64

    def __init__(self, cuda, words, L, shape, dt, cap_words=None, index=None, touched=None, maxprec=None):
        import torch
        import cuzfp_amd
        self.cuda = cuda
        self.lib = cuzfp_amd.library()
        self.t = tv.TC[np.dtype(dt)]
        self.ext = cuzfp_amd._extents(shape)
        self.n = L.size
        self.T = (self.n + 63) // 64
        self.w = _dev(np.ascontiguousarray(words).view(np.int64), cuda)
        self.l = _dev(np.ascontiguousarray(L).view(np.int16), cuda)
        idx = want_index(L) if index is None else index
        self.i = _dev(np.ascontiguousarray(idx).view(np.int64), cuda)
        if cap_words is None:  # the whole array at the type's longest block: every call fits
            cap_words = words.size + (self.n * bz.top(len(shape), np.dtype(dt)) + 63) // 64
        self.cap = cap_words
        P = self.PAD
        self.dst = torch.full((cap_words + 2 * P,), ICANARY, dtype=torch.int64, device=cuda)
        self.len = torch.full((self.n + 2 * P,), 0x5A5A, dtype=torch.int16, device=cuda)
        self.idx = torch.full((self.T + 1 + 2 * P,), ICANARY, dtype=torch.int64, device=cuda)
        self.total = torch.full((3,), ICANARY, dtype=torch.int64, device=cuda)
        self.need = self.lib.cuzfp_hip_encode_region_variable_workspace_bytes(self.t, *self.ext)
        assert self.need >= 8 * (self.n + 1)
        self.ws = torch.full((self.need // 8 + P,), ICANARY, dtype=torch.int64, device=cuda)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(self, x, origin, mode, with_index=True):
        """x: a device tensor of the box; mode: (maxprec, minexp)."""
        import cuzfp_amd
        P = self.PAD
        o = cuzfp_amd._extents(origin)
        e = cuzfp_amd._extents(x.shape)
        sx, sy, sz = cuzfp_amd._strides(x)
        return self.lib.cuzfp_hip_encode_region_variable(
            x.data_ptr(), sx, sy, sz, self.t, *self.ext, mode[0], mode[1], *o, *e,
            self.w.data_ptr(), self.w.numel() * 8, self.l.data_ptr(), self.i.data_ptr(), self.i.numel() * 8,
            self.dst[P:].data_ptr(), self.cap * 8, self.len[P:].data_ptr(),
            self.idx[P:].data_ptr() if with_index else None, self.total[1:].data_ptr(), self.ws.data_ptr(),
            self.need, self.st)

    def canaries_intact(self, with_index=True):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        ok = (bool((self.dst[:P] == ICANARY).all()) and bool((self.dst[P + self.cap:] == ICANARY).all()) and
              bool((self.len[:P] == 0x5A5A).all()) and bool((self.len[P + self.n:] == 0x5A5A).all()) and
              int(self.total[0]) == ICANARY and int(self.total[2]) == ICANARY and
              bool((self.ws[self.need // 8:] == ICANARY).all()))
        if with_index:
            return ok and bool((self.idx[:P] == ICANARY).all()) and bool((self.idx[P + self.T + 1:] == ICANARY).all())
        return ok and bool((self.idx == ICANARY).all())

    def result(self):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        L = self.len[P: P + self.n].cpu().numpy().view(np.uint16)
        return (self.dst[P: P + self.cap].cpu().numpy().view(np.uint64), L, int(self.total[1]),
                self.idx[P: P + self.T + 1].cpu().numpy().view(np.uint64))

    def source_unchanged(self, words, L):
        return np.array_equal(_words(self.w), words) and np.array_equal(_lengths(self.l), L)


def check_raw(cuda, varemu, words, L, shape, dt, origin, x, mode, with_index=True, cid=None):  # noqa: F811
    """One call of the C-ABI against the model: the count, the lengths, the
    stream's words and the canary after them, the index.  Returns the model."""
    want = ru.model(varemu, words, L, shape, dt, origin, x, mode)
    raw = Raw(cuda, words, L, shape, dt)
    cid = cid or (shape, np.dtype(dt).name, mode, origin, x.shape)
    assert raw.call(_dev(x, cuda), origin, ru.mode_of(dt, mode), with_index) == 0, cid
    assert raw.canaries_intact(with_index), cid
    got, newL, total, idx = raw.result()
    assert total == want[2], cid
    assert np.array_equal(newL, want[1]), cid
    assert np.array_equal(got[: want[0].size], want[0]), cid
    assert (got[want[0].size:] == np.uint64(CANARY)).all(), cid
    if with_index:
        assert np.array_equal(idx, want_index(want[1])), cid
    assert raw.source_unchanged(words, L), cid
    return want


def update(cuda, words, L, shape, dt, origin, x, mode, **kw):
    """The wrapper on a host stream and a host box."""
    import cuzfp_amd
    xd = x if hasattr(x, "is_cuda") else _dev(x, cuda)
    return cuzfp_amd.encode_region_variable(xd, _dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda),
                                            _dev(want_index(L).view(np.int64), cuda), shape, origin, **kw_of(mode),
                                            **kw)


def check_wrapper(cuda, got, want, buf=None):
    words, lengths, nbits = got[:3]
    assert nbits == want[2]
    assert np.array_equal(_lengths(lengths), want[1])
    assert np.array_equal(_words(words), want[0])
    if len(got) > 3:
        assert np.array_equal(got[3].cpu().numpy().view(np.uint64), want_index(want[1]))
    if buf is not None:
        assert words.data_ptr() == buf.data_ptr() and bool((buf[want[0].size:] == FILL).all())


# ---------------------------------------------------------------------------
# Boxes

def boxes(shape):
    """(origin, extent): one element; one aligned block; an unaligned box inside
    one block; a box across the wave boundary at block 64 (where the array has
    one); the far corner with the array's last, ragged block on every axis,
    from an unaligned origin; one-element-thick slabs on each axis; the whole
    array."""
    n = len(shape)
    nb = [(s + 3) // 4 for s in shape]
    out = [(tuple(s // 2 for s in shape), (1,) * n),
           (tuple(4 * (b // 2) for b in nb), tuple(min(4, s - 4 * (b // 2)) for s, b in zip(shape, nb))),
           (tuple(4 * (b // 2) + 1 if s - 4 * (b // 2) >= 3 else 4 * (b // 2) for s, b in zip(shape, nb)),
            tuple(2 if s - 4 * (b // 2) >= 3 else 1 for s, b in zip(shape, nb)))]
    if int(np.prod(nb)) > 65:
        pos = [int(p) for p in np.unravel_index(63, nb)]  # block 63 and its right neighbour, block 64
        assert pos[-1] + 1 < nb[-1]
        o = [min(4 * p + 1, s - 2) for p, s in zip(pos, shape)]
        o[-1] = 4 * pos[-1] + 2
        out.append((tuple(o), (2,) * (n - 1) + (4,)))
    out.append((tuple(max(0, s - 6) for s in shape), tuple(min(6, s) for s in shape)))
    for ax in range(n):
        out.append((tuple(shape[k] // 2 + 1 if k == ax else 0 for k in range(n)),
                    tuple(1 if k == ax else shape[k] for k in range(n))))
    out.append(((0,) * n, tuple(shape)))
    for o, e in out:
        assert all(0 <= a and b >= 1 and a + b <= s for a, b, s in zip(o, e, shape)), (shape, o, e)
    return out


@pytest.mark.parametrize("mode", SRC_MODES, ids=lambda m: f"{m[0]}{m[1]:g}")
@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_boxes(cuda, varemu, tv_golden, shape, dtype, mode):  # noqa: F811
    """Every box of `boxes`, in the stream's own mode, with and without the
    index: words, lengths, bit count and index are the model's."""
    words, L = source(varemu, tv_golden, shape, dtype, mode)
    for k, (origin, extent) in enumerate(boxes(shape)):
        check_raw(cuda, varemu, words, L, shape, dtype, origin, ru.other_values(extent, dtype, origin), mode,
                  with_index=k % 2 == 0)


@pytest.mark.parametrize("mode", SRC_MODES, ids=lambda m: f"{m[0]}{m[1]:g}")
@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identity(cuda, varemu, tv_golden, shape, dtype, mode):  # noqa: F811
    """The whole array as the box, the original data, the stream's mode: the
    source stream byte for byte."""
    import torch
    import cuzfp_amd
    words, L = source(varemu, tv_golden, shape, dtype, mode)
    nbits = int(L.astype(np.int64).sum())
    cap = cuzfp_amd.library().cuzfp_hip_encode_region_variable_maximum_size(
        tv.TC[dtype], *cuzfp_amd._extents(shape), words.nbytes, *cuzfp_amd._extents(shape), 0, 0, 0,
        ru.mode_of(dtype, mode)[0])
    buf = torch.full((cap // 8,), FILL, dtype=torch.int64, device=cuda)
    got = update(cuda, words, L, shape, dtype, (0,) * len(shape), tv.array(shape, dtype), mode, out=buf,
                 with_index=True)
    check_wrapper(cuda, got, (words, L, nbits), buf)


@pytest.mark.parametrize("mode", SRC_MODES, ids=lambda m: f"{m[0]}{m[1]:g}")
@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_covered_update_equals_reference(cuda, varemu, tv_golden, shape, dtype, mode):  # noqa: F811
    """A block-aligned box of new values a'[box]: the result is the stream of
    a' -- which the model gives too."""
    a = tv.array(shape, dtype)
    words, L = source(varemu, tv_golden, shape, dtype, mode)
    for origin, extent in ru.ALIGNED[shape]:
        a2 = a.copy()
        x = ru.other_values(extent, dtype, origin)
        a2[ru.box_slices(origin, extent)] = x
        ref = tv.emu_compress(varemu, a2, *ru.mode_of(dtype, mode))
        want = check_raw(cuda, varemu, words, L, shape, dtype, origin, x, mode)
        assert want[2] == ref[2] and np.array_equal(want[1], ref[1]) and np.array_equal(want[0], ref[0])


# ---------------------------------------------------------------------------
# Length changes across word and wave edges, scan tiles

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_dense_over_the_zero_run_and_zeros_over_dense(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """tv.array has 130 one-bit zero blocks from block 2 on (a wave of them is
    one word).  Dense values over a part of the run lengthen blocks inside it;
    zeros over dense blocks shorten them to one bit."""
    rng = np.random.default_rng(5)
    for shape, dense_box, zero_box in (((1000,), ((101,), (299,)), ((600,), (203,))),
                                       (BIG, ((0, 4, 0), (4, 18, 38)), ((8, 0, 0), (4, 22, 38))),
                                       (BIG, ((0, 5, 3), (3, 9, 30)), ((7, 1, 2), (5, 20, 33)))):
        words, L = source(varemu, tv_golden, shape, dtype, tp.PAIR[0])
        t = ru.touched_blocks(shape, *dense_box)
        assert (L[t] == 1).sum() >= 20
        x = tv._random_bits(rng, int(np.prod(dense_box[1])), dtype).reshape(dense_box[1])
        want = check_raw(cuda, varemu, words, L, shape, dtype, dense_box[0], x, ru.full(dtype))
        assert want[2] > int(L.astype(np.int64).sum()) + 50 * t.sum()  # (a dense 1D float block is up to 140 bits)
        t = ru.touched_blocks(shape, *zero_box)
        want = check_raw(cuda, varemu, words, L, shape, dtype, zero_box[0], np.zeros(zero_box[1], dtype), tp.PAIR[0])
        covered = all(o % 4 == 0 and ((o + e) % 4 == 0 or o + e == n) for o, e, n in zip(*zero_box, shape))
        if covered:
            assert (want[1][t] == 1).all() and (L[t] > 1).any()


@pytest.mark.parametrize("name,dtype,block", [("zeros64", F32, 31), ("zeros65", F32, 32), ("zeros65", F32, 64),
                                              ("three", F32, 32), ("three", F64, 63), ("three", F64, 64)])
def test_one_dense_block_in_the_middle(cuda, varemu, name, dtype, block):  # noqa: F811
    """All-zero waves (64 one-bit blocks are one word; 65 leave a word open):
    one block replaced by a dense block, which moves everything after it."""
    a = tp.array(name, dtype)
    rng = np.random.default_rng(block)
    for mode in tp.PAIR:
        words, L, _ = tv.emu_compress(varemu, a, *ru.mode_of(dtype, mode))
        x = tv._random_bits(rng, 4, dtype)
        want = check_raw(cuda, varemu, words, L, a.shape, dtype, (4 * block,), x, ru.full(dtype))
        assert want[1][block] > 64
        # ... and back: zeros over it again give the source stream
        if L[block] == 1:
            got = update(cuda, want[0], want[1], a.shape, dtype, (4 * block,), np.zeros(4, dtype), mode)
            check_wrapper(cuda, got, (words, L, int(L.astype(np.int64).sum())))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_more_than_one_scan_tile(cuda, varemu, dtype):  # noqa: F811
    """tiles2d: 33 x 65 = 2145 blocks, three scan tiles; a box whose blocks
    straddle the tile boundary at block 1024 (row 15, column 49)."""
    a = tp.array("tiles2d", dtype)
    mode = tp.PAIR[0]
    words, L, _ = tv.emu_compress(varemu, a, *ru.mode_of(dtype, mode))
    origin, extent = (4 * 14 + 1, 4 * 40 + 2), (10, 60)
    t = ru.touched_blocks(a.shape, origin, extent)
    assert t[1023] and t[1024] and t[:1024].any() and t[1024:].any()
    check_raw(cuda, varemu, words, L, a.shape, dtype, origin, ru.other_values(extent, dtype, "tiles"), mode)
    check_raw(cuda, varemu, words, L, a.shape, dtype, (60, 0), ru.other_values((4, 259), dtype, "row"), mode)


# ---------------------------------------------------------------------------
# Another mode for the box, composition with the other calls

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_a_different_mode_for_the_box(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """A full-precision brick in a tolerance 1e-2 stream and a p7 brick in a
    full-precision stream: the model's stream, and decode_variable of it is
    the emulation's decode of the model, inside and outside the box."""
    import cuzfp_amd
    for src_mode, box_mode in ((("a", 1e-2), ru.full(dtype)), (ru.full(dtype), ("p", 7))):
        words, L = source(varemu, tv_golden, BIG, dtype, src_mode)
        for origin, extent in (((4, 8, 12), (8, 8, 16)), ((3, 5, 9), (7, 11, 20))):
            x = ru.other_values(extent, dtype, origin)
            want = check_raw(cuda, varemu, words, L, BIG, dtype, origin, x, box_mode)
            got = update(cuda, words, L, BIG, dtype, origin, x, box_mode)
            check_wrapper(cuda, got, want)
            dec = cuzfp_amd.decode_variable(got[0], got[1], BIG, _tdtype(dtype)).cpu().numpy()
            ref = tv.emu_decompress(varemu, want[0], want[1], BIG, dtype)
            assert np.array_equal(dec.view(np.uint8), ref.view(np.uint8))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_result_feeds_the_other_calls(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """variable_index of the new lengths is the returned index; the updated box
    and an untouched box decode to the emulation's; truncate_variable of the
    result is the splice of the two streams at the coarser mode."""
    import cuzfp_amd
    td = _tdtype(dtype)
    mode, coarse = ru.full(dtype), ("p", 7)
    words, L = source(varemu, tv_golden, BIG, dtype, mode)
    origin, extent = (4, 8, 12), (8, 8, 16)
    x = ru.other_values(extent, dtype, origin)
    want = ru.model(varemu, words, L, BIG, dtype, origin, x, mode)
    w, l, nbits, idx = update(cuda, words, L, BIG, dtype, origin, x, mode, with_index=True)
    check_wrapper(cuda, (w, l, nbits, idx), want)
    assert np.array_equal(cuzfp_amd.variable_index(l, BIG, td).cpu().numpy(), idx.cpu().numpy())
    ref = tv.emu_decompress(varemu, want[0], want[1], BIG, dtype)
    for o, e in ((origin, extent), ((0, 0, 0), (4, 8, 12)), ((1, 2, 3), (10, 17, 30))):
        got = cuzfp_amd.decode_region_variable(w, l, idx, BIG, td, o, e).cpu().numpy()
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref[ru.box_slices(o, e)]).view(np.uint8))
    cw, cl, cn = cuzfp_amd.truncate_variable(w, l, BIG, td, from_precision=mode[1], precision=coarse[1])
    src7 = source(varemu, tv_golden, BIG, dtype, coarse)
    e7 = tv.emu_compress(varemu, want[3], *ru.mode_of(dtype, coarse))
    want7 = ru.splice(src7[0], src7[1], e7[0], e7[1], ru.touched_blocks(BIG, origin, extent))
    check_wrapper(cuda, (cw, cl, cn), want7)


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_two_updates_in_sequence(cuda, varemu, tv_golden, dtype):  # noqa: F811
    import cuzfp_amd
    mode = ("a", 1e-3)
    words, L = source(varemu, tv_golden, BIG, dtype, mode)
    o1, x1 = (0, 3, 5), ru.other_values((13, 6, 20), dtype, 1)
    o2, x2 = (8, 4, 16), ru.other_values((5, 12, 8), dtype, 2)  # overlaps the first
    m1 = ru.model(varemu, words, L, BIG, dtype, o1, x1, mode)
    m2 = ru.model(varemu, m1[0], m1[1], BIG, dtype, o2, x2, ("p", 16))
    w, l, n, idx = update(cuda, words, L, BIG, dtype, o1, x1, mode, with_index=True)
    check_wrapper(cuda, (w, l, n, idx), m1)
    got = cuzfp_amd.encode_region_variable(_dev(x2, cuda), w, l, idx, BIG, o2, precision=16, with_index=True)
    check_wrapper(cuda, got, m2)


# ---------------------------------------------------------------------------
# Strided and broadcast boxes, another stream

def test_strided_broadcast_and_stream(cuda, varemu, tv_golden):  # noqa: F811
    import torch
    mode = ("p", 16)
    words, L = source(varemu, tv_golden, BIG, F32, mode)
    origin, extent = (2, 4, 7), (9, 10, 21)
    x = ru.other_values(extent, F32, "strided")
    want = ru.model(varemu, words, L, BIG, F32, origin, x, mode)
    # a sliced view: every other element along x of every other row of a larger tensor
    # (torch has no negative strides; test_negative_stride_through_the_c_abi has those)
    big = torch.zeros((9, 20, 42), dtype=torch.float32, device=cuda)
    view = big[:, 1::2, ::2]
    view.copy_(_dev(x, cuda))
    assert view.stride() == (840, 84, 2)
    check_wrapper(cuda, update(cuda, words, L, BIG, F32, origin, view, mode, with_index=True), want)
    t = _dev(np.ascontiguousarray(x.transpose(2, 1, 0)), cuda).permute(2, 1, 0)  # a permuted view
    assert not t.is_contiguous()
    check_wrapper(cuda, update(cuda, words, L, BIG, F32, origin, t, mode), want)
    # a broadcast view: fill the box with a constant
    fill = torch.full((1,), 2.5, dtype=torch.float32, device=cuda).expand(extent)
    wantc = ru.model(varemu, words, L, BIG, F32, origin, np.full(extent, 2.5, np.float32), mode)
    check_wrapper(cuda, update(cuda, words, L, BIG, F32, origin, fill, mode), wantc)
    # a stream of its own
    s = torch.cuda.Stream(device=cuda)
    xd = _dev(x, cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    got = update(cuda, words, L, BIG, F32, origin, xd, mode, stream=s, with_index=True)
    gotc = update(cuda, words, L, BIG, F32, origin, fill, mode, stream=s)
    s.synchronize()
    check_wrapper(cuda, got, want)
    check_wrapper(cuda, gotc, wantc)


def test_negative_stride_through_the_c_abi(cuda, varemu, tv_golden):  # noqa: F811
    """Element strides below zero: the box pointer is its element (0, 0, 0)."""
    mode = ("a", 1e-3)
    words, L = source(varemu, tv_golden, (33, 70), F64, mode)
    origin, extent = (5, 9), (20, 33)
    x = ru.other_values(extent, F64, "neg")
    want = ru.model(varemu, words, L, (33, 70), F64, origin, x, mode)
    raw = Raw(cuda, words, L, (33, 70), F64)
    rev = _dev(np.ascontiguousarray(x[::-1, ::-1]), cuda)  # element (i, j) of the box at rev[19 - i, 32 - j]

    class View:  # what Raw.call reads of a tensor
        shape = extent

        def data_ptr(self):
            return rev.data_ptr() + 8 * (20 * 33 - 1)

        def stride(self):
            return (-33, -1)

        def dim(self):
            return 2

    assert raw.call(View(), origin, ru.mode_of(F64, mode)) == 0
    assert raw.canaries_intact()
    got, newL, total, idx = raw.result()
    assert total == want[2] and np.array_equal(newL, want[1]) and np.array_equal(got[: want[0].size], want[0])


# ---------------------------------------------------------------------------
# Capacity

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_capacity(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """`out` one word short: nothing at or past its end is written, the lengths
    and the count are the full call's.  The default allocation holds the
    result at the bound of ..._maximum_size."""
    import torch
    import cuzfp_amd
    mode = ("p", 16)
    words, L = source(varemu, tv_golden, BIG, dtype, mode)
    origin, extent = (3, 5, 9), (7, 11, 20)
    x = ru.other_values(extent, dtype, origin)
    want = ru.model(varemu, words, L, BIG, dtype, origin, x, ru.full(dtype))
    nwords = want[0].size
    buf = torch.full((nwords + 8,), ICANARY, dtype=torch.int64, device=cuda)
    w, l, n, idx = update(cuda, words, L, BIG, dtype, origin, x, ru.full(dtype), out=buf[: nwords - 1],
                          with_index=True)
    assert n == want[2] and np.array_equal(_lengths(l), want[1]) and w.numel() == nwords - 1
    assert np.array_equal(idx.cpu().numpy().view(np.uint64), want_index(want[1]))
    assert bool((buf[nwords - 1:] == ICANARY).all())
    assert np.array_equal(_words(w)[: nwords - 2], want[0][: nwords - 2])
    # the default allocation
    touched = int(ru.touched_blocks(BIG, origin, extent).sum())
    bound = cuzfp_amd.library().cuzfp_hip_encode_region_variable_maximum_size(
        tv.TC[dtype], *cuzfp_amd._extents(BIG), words.nbytes, *cuzfp_amd._extents(extent),
        *cuzfp_amd._extents(origin), tp.type_prec(dtype))
    assert bound == 8 * ((8 * words.nbytes + touched * bz.top(3, dtype) + 63) // 64) and bound >= 8 * nwords
    got = update(cuda, words, L, BIG, dtype, origin, x, ru.full(dtype))
    check_wrapper(cuda, got, want)
    assert got[0]._base is not None and got[0]._base.numel() * 8 == bound


# ---------------------------------------------------------------------------
# An index that is not the stream's

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_bad_index(cuda, varemu, tv_golden, dtype):  # noqa: F811
    """Source lengths of 65535 throughout, lengths no encoder writes, an index
    of zeros, an index of huge offsets.  Every source length is clamped and
    every source dword is loaded behind the stream_bytes bound, every store is
    behind the capacity, so nothing can fault by construction: the call
    returns, the canaries around every output hold, and the new lengths of the
    touched blocks -- covered ones, coded from the box alone -- are the
    model's.  A valid case run afterwards is exact."""
    words, L = source(varemu, tv_golden, BIG, dtype, ("p", 16))
    mode = ("p", 16)
    origin, extent = (4, 8, 12), (8, 8, 16)
    x = ru.other_values(extent, dtype, origin)
    t = ru.touched_blocks(BIG, origin, extent)
    M = np.zeros(BIG, dtype)
    M[ru.box_slices(origin, extent)] = x
    LE = tv.emu_compress(varemu, M, *ru.mode_of(dtype, mode))[1]  # covered blocks: from the box alone
    rng = np.random.default_rng(3)
    illegal = np.where(rng.random(L.size) < 0.5, rng.integers(2, tp.ebits(dtype) + 2, L.size), L).astype(np.uint16)
    illegal[::7] = 40000
    bads = [(np.full(L.size, 0xFFFF, np.uint16), None), (illegal, None),
            (L, np.zeros((L.size + 63) // 64 + 1, np.uint64)),
            (L, np.full((L.size + 63) // 64 + 1, (1 << 63) + 12345, np.uint64)),
            (np.full(L.size, 0xFFFF, np.uint16), np.full((L.size + 63) // 64 + 1, 2 ** 64 - 1, np.uint64))]
    for badL, badI in bads:
        for o, xx in ((origin, x), ((3, 5, 9), ru.other_values((7, 11, 20), dtype, "merge"))):
            raw = Raw(cuda, words, badL, BIG, dtype, index=badI, cap_words=words.size + 64)
            assert raw.call(_dev(xx, cuda), o, ru.mode_of(dtype, mode)) == 0
            assert raw.canaries_intact()
            _, newL, total, idx = raw.result()
            assert total == int(newL.astype(np.int64).sum())
            assert np.array_equal(idx, want_index(newL))
            if o == origin:
                assert np.array_equal(newL[t], LE[t])
                assert np.array_equal(newL[~t], badL[~t])
            assert raw.source_unchanged(words, badL)
    check_raw(cuda, varemu, words, L, BIG, dtype, origin, x, mode)
