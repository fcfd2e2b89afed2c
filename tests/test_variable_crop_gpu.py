"""extract_region_variable / insert_region_variable on the GPU against the host
model of tests/test_variable_crop.py (`model_extract`, `model_insert`: numpy on
bit arrays, the source streams from the host emulation `varemu`, which the
fixture hashes vouch for) and against the device calls they replace.

Every comparison is of bytes.  The raw C-ABI runs on buffers with canaries on
both sides of the stream, the lengths, the index, the count and the workspace
(`Raw`, after test_variable_region_update_gpu's); the wrappers' `out` is filled
with all-ones words first, and what lies past the result must still hold the
fill.
"""
import ctypes

import numpy as np
import pytest

import test_variable as tv
import test_variable_crop as vc
import test_variable_paths as tp
import test_variable_region_update as ru
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_gpu import CANARY, _dev, _lengths, _tdtype, _words
from test_variable_paths import F32, F64, want_index
from test_variable_region_update_gpu import FILL, ICANARY, kw_of

pytestmark = pytest.mark.gpu

BIG = (13, 22, 38)  # 240 blocks: four waves, the last ragged; partial blocks on every axis
_SRC = {}


def source(varemu, shape, dt, mode, a=None):  # noqa: F811
    """(words, L, nbits) of tv.array(shape, dt) at `mode` from the host emulation; computed once, read only."""
    if a is not None:
        return tv.emu_compress(varemu, a, *ru.mode_of(dt, mode))
    key = (tuple(shape), np.dtype(dt).str, tuple(mode))
    if key not in _SRC:
        _SRC[key] = tv.emu_compress(varemu, tv.array(shape, dt), *ru.mode_of(dt, mode))
    return _SRC[key]


def same(got, want):
    return got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


class Raw:
    """Either call of the C-ABI on buffers with canaries on both sides of every
    output.  box=None: extract from (words, L); else insert box = (words, L) of
    the brick into (words, L)."""
    PAD = 64

    def __init__(self, cuda, words, L, shape, dt, origin, extent, box=None, cap_words=None, index=None,
                 box_index=None):
        import torch
        import cuzfp_amd
        self.lib = cuzfp_amd.library()
        self.t = tv.TC[np.dtype(dt)]
        self.ext = cuzfp_amd._extents(shape)
        self.o, self.e = cuzfp_amd._extents(origin), cuzfp_amd._extents(extent)
        self.paste = box is not None
        self.nrb = int(ru.touched_blocks(shape, origin, extent).sum())
        self.w = _dev(np.ascontiguousarray(words).view(np.int64), cuda)
        self.l = _dev(np.ascontiguousarray(L).view(np.int16), cuda)
        self.i = _dev(np.ascontiguousarray(want_index(L) if index is None else index).view(np.int64), cuda)
        if self.paste:
            self.bw = _dev(np.ascontiguousarray(box[0]).view(np.int64), cuda)
            self.bl = _dev(np.ascontiguousarray(box[1]).view(np.int16), cuda)
            self.bi = _dev(np.ascontiguousarray(want_index(box[1]) if box_index is None else box_index).view(np.int64),
                           cuda)
            self.n = L.size
            self.need = self.lib.cuzfp_hip_insert_region_variable_workspace_bytes(self.t, *self.ext)
            bound = self.lib.cuzfp_hip_insert_region_variable_maximum_size(words.nbytes, box[0].nbytes)
            assert bound == 8 * ((8 * words.nbytes + 8 * box[0].nbytes + 63) // 64)
        else:
            self.n = self.nrb
            self.need = self.lib.cuzfp_hip_extract_region_variable_workspace_bytes(self.t, *self.e)
            bound = self.lib.cuzfp_hip_extract_region_variable_maximum_size(self.t, *self.ext, words.nbytes, *self.e,
                                                                            *self.o)
        assert self.need >= 8 * (self.n + 1) and bound > 0
        self.T = (self.n + 63) // 64
        self.cap = bound // 8 if cap_words is None else cap_words
        P = self.PAD
        self.dst = torch.full((self.cap + 2 * P,), ICANARY, dtype=torch.int64, device=cuda)
        self.len = torch.full((self.n + 2 * P,), 0x5A5A, dtype=torch.int16, device=cuda)
        self.idx = torch.full((self.T + 1 + 2 * P,), ICANARY, dtype=torch.int64, device=cuda)
        self.total = torch.full((3,), ICANARY, dtype=torch.int64, device=cuda)
        self.ws = torch.full((self.need // 8 + P,), ICANARY, dtype=torch.int64, device=cuda)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(self, with_index=True, query=False):
        P = self.PAD
        dst, cap = (None, 0) if query else (self.dst[P:].data_ptr(), self.cap * 8)
        idx = self.idx[P:].data_ptr() if with_index else None
        src = (self.w.data_ptr(), self.w.numel() * 8, self.l.data_ptr(), self.i.data_ptr(), self.i.numel() * 8)
        if self.paste:
            return self.lib.cuzfp_hip_insert_region_variable(
                self.bw.data_ptr(), self.bw.numel() * 8, self.bl.data_ptr(), self.bi.data_ptr(), self.bi.numel() * 8,
                *src, self.t, *self.ext, *self.o, *self.e, dst, cap, self.len[P:].data_ptr(), idx,
                self.total[1:].data_ptr(), self.ws.data_ptr(), self.need, self.st)
        return self.lib.cuzfp_hip_extract_region_variable(
            *src, self.t, *self.ext, *self.o, *self.e, dst, cap, self.len[P:].data_ptr(), idx, 8 * (self.T + 1),
            self.total[1:].data_ptr(), self.ws.data_ptr(), self.need, self.st)

    def canaries_intact(self, with_index=True, query=False):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        ok = (bool((self.dst[:P] == ICANARY).all()) and bool((self.dst[P + self.cap:] == ICANARY).all()) and
              bool((self.len[:P] == 0x5A5A).all()) and bool((self.len[P + self.n:] == 0x5A5A).all()) and
              int(self.total[0]) == ICANARY and int(self.total[2]) == ICANARY and
              bool((self.ws[self.need // 8:] == ICANARY).all()))
        if query:
            ok = ok and bool((self.dst == ICANARY).all())
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

    def inputs_unchanged(self, words, L, box=None):
        ok = np.array_equal(_words(self.w), words) and np.array_equal(_lengths(self.l), L)
        if box is not None:
            ok = ok and np.array_equal(_words(self.bw), box[0]) and np.array_equal(_lengths(self.bl), box[1])
        return ok


def check_raw(cuda, want, words, L, shape, dt, origin, extent, box=None, with_index=True, cid=None):
    """One call of the C-ABI against the model's (words, L, nbits): the count,
    the lengths, the stream's words and the canary after them, the index."""
    raw = Raw(cuda, words, L, shape, dt, origin, extent, box=box)
    cid = cid or (shape, np.dtype(dt).name, origin, extent, box is not None)
    assert raw.cap >= want[0].size, cid
    assert raw.call(with_index) == 0, cid
    assert raw.canaries_intact(with_index), cid
    got, newL, total, idx = raw.result()
    assert total == want[2], cid
    assert np.array_equal(newL, want[1]), cid
    assert np.array_equal(got[: want[0].size], want[0]), cid
    assert (got[want[0].size:] == np.uint64(CANARY)).all(), cid
    if with_index:
        assert np.array_equal(idx, want_index(want[1])), cid
    assert raw.inputs_unchanged(words, L, box), cid


def dev_stream(cuda, s, index=None):
    """(words, lengths, index) of a host stream on the device."""
    return (_dev(s[0].view(np.int64), cuda), _dev(s[1].view(np.int16), cuda),
            _dev((want_index(s[1]) if index is None else index).view(np.int64), cuda))


def check_wrapper(got, want, buf=None):
    words, lengths, nbits = got[:3]
    assert nbits == want[2]
    assert np.array_equal(_lengths(lengths), want[1])
    assert np.array_equal(_words(words), want[0])
    if len(got) > 3:
        assert np.array_equal(got[3].cpu().numpy().view(np.uint64), want_index(want[1]))
    if buf is not None:
        assert words.data_ptr() == buf.data_ptr() and bool((buf[want[0].size:] == FILL).all())


# ---------------------------------------------------------------------------
# Every aligned box of the CPU file, both calls, against the model

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", vc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_boxes(cuda, varemu, shape, dtype):  # noqa: F811
    """Crop equals model_extract, paste (of a brick of other values, coded at
    another mode) equals model_insert: words, lengths, count and index, with
    and without the index; the inputs unchanged, the canaries intact."""
    modes = vc.MODES(dtype)
    for m, mode in enumerate(modes):
        words, L, _ = source(varemu, shape, dtype, mode)
        for k, (origin, extent) in enumerate(vc.aligned_boxes(shape)):
            want = vc.model_extract(words, L, shape, origin, extent)
            check_raw(cuda, want, words, L, shape, dtype, origin, extent, with_index=(k + m) % 2 == 0)
            B = source(varemu, extent, dtype, modes[(m + 1) % 3], a=ru.other_values(extent, dtype, origin))
            want = vc.model_insert(B[0], B[1], words, L, shape, origin, extent)
            check_raw(cuda, want, words, L, shape, dtype, origin, extent, box=B, with_index=(k + m) % 2 == 1)


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_wrappers(cuda, varemu, dtype):  # noqa: F811
    """The Python calls with an all-ones `out`: the model's bytes, the fill
    after them; the default allocation; a stream of its own."""
    import torch
    import cuzfp_amd
    td = _tdtype(dtype)
    mode = ("a", 1e-3)
    S = source(varemu, BIG, dtype, mode)
    d = dev_stream(cuda, S)
    for origin, extent in (((0, 0, 0), (13, 22, 20)), ((8, 16, 32), (5, 6, 6)), ((0, 0, 0), BIG)):
        want = vc.model_extract(S[0], S[1], BIG, origin, extent)
        buf = torch.full((want[0].size + 9,), FILL, dtype=torch.int64, device=cuda)
        got = cuzfp_amd.extract_region_variable(*d, BIG, td, origin, extent, out=buf, with_index=True)
        check_wrapper(got, want, buf)
        check_wrapper(cuzfp_amd.extract_region_variable(*d, BIG, td, origin, extent), want)
        B = source(varemu, extent, dtype, ("p", 16), a=ru.other_values(extent, dtype, origin))
        wantp = vc.model_insert(B[0], B[1], S[0], S[1], BIG, origin, extent)
        buf = torch.full((wantp[0].size + 9,), FILL, dtype=torch.int64, device=cuda)
        b = dev_stream(cuda, B)
        gotp = cuzfp_amd.insert_region_variable(*b, *d, BIG, td, origin, extent, out=buf, with_index=True)
        check_wrapper(gotp, wantp, buf)
        check_wrapper(cuzfp_amd.insert_region_variable(*b, *d, BIG, td, origin, extent), wantp)
        # the crop pasted back over the pasted stream gives the source again
        back = cuzfp_amd.insert_region_variable(got[0], got[1], got[3], gotp[0], gotp[1], gotp[3], BIG, td, origin,
                                                extent, with_index=True)
        check_wrapper(back, S)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    origin, extent = (4, 8, 12), (8, 8, 16)
    got = cuzfp_amd.extract_region_variable(*d, BIG, td, origin, extent, stream=s, with_index=True)
    back = cuzfp_amd.insert_region_variable(got[0], got[1], got[3], *d, BIG, td, origin, extent, stream=s)
    s.synchronize()
    check_wrapper(got, vc.model_extract(S[0], S[1], BIG, origin, extent))
    check_wrapper(back, S)
    with pytest.raises(ValueError, match="decode_region_variable / encode_region_variable"):
        cuzfp_amd.extract_region_variable(*d, BIG, td, (4, 8, 12), (8, 8, 15))


# ---------------------------------------------------------------------------
# Against the device code the two calls replace

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("shape", vc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_existing_device_code(cuda, shape, dtype):
    """Crop equals encode_variable of the box of the array; paste of
    encode_variable(X, mode) equals encode_region_variable(X, ..., origin, mode)
    in stream, lengths, count and index; decoding the pasted stream gives X
    inside the box and the old array outside it, bit for bit."""
    import torch
    import cuzfp_amd
    td = _tdtype(dtype)
    a = tv.array(shape, dtype)
    x = _dev(a, cuda)
    for mode in (("p", 16), ("a", 1e-3)):
        kw = kw_of(mode)
        w, l, nbits = cuzfp_amd.encode_variable(x, **kw)
        idx = cuzfp_amd.variable_index(l, shape, td)
        old = cuzfp_amd.decode_variable(w, l, shape, td)
        for origin, extent in vc.aligned_boxes(shape):
            sl = ru.box_slices(origin, extent)
            cw, cl, cn, ci = cuzfp_amd.extract_region_variable(w, l, idx, shape, td, origin, extent, with_index=True)
            ew, el, en = cuzfp_amd.encode_variable(x[sl].contiguous(), **kw)
            assert cn == en and torch.equal(cl, el) and torch.equal(cw, ew), (mode, origin)
            assert torch.equal(ci, cuzfp_amd.variable_index(el, extent, td)), (mode, origin)
            X = _dev(ru.other_values(extent, dtype, origin), cuda)
            bw, bl, _ = cuzfp_amd.encode_variable(X, **kw)
            bi = cuzfp_amd.variable_index(bl, extent, td)
            pw, pl, pn, pi = cuzfp_amd.insert_region_variable(bw, bl, bi, w, l, idx, shape, td, origin, extent,
                                                              with_index=True)
            uw, ul, un, ui = cuzfp_amd.encode_region_variable(X, w, l, idx, shape, origin, with_index=True, **kw)
            assert pn == un and torch.equal(pl, ul) and torch.equal(pw, uw) and torch.equal(pi, ui), (mode, origin)
            dec = cuzfp_amd.decode_variable(pw, pl, shape, td)
            want = old.clone()
            want[sl] = cuzfp_amd.decode_variable(bw, bl, extent, td)
            it = torch.int32 if dtype == F32 else torch.int64
            assert torch.equal(dec.view(it), want.view(it)), (mode, origin)


# ---------------------------------------------------------------------------
# Shared words, long blocks

def test_shared_words(cuda, varemu):  # noqa: F811
    """A float32 (16, 16, 64) array of zeros except for its first block, at
    tolerance 1e-3: every block but one is a single bit, so a wave's segment is
    64 bits at an odd offset and each destination word holds bits of two
    waves."""
    shape, mode = (16, 16, 64), ("a", 1e-3)
    a = np.zeros(shape, F32)
    a[:4, :4, :4] = np.random.default_rng(11).uniform(1, 2, (4, 4, 4))
    S = source(varemu, shape, F32, mode, a=a)
    assert S[1].size == 256 and S[1][0] > 1 and S[1][0] % 64 and (S[1][1:] == 1).all()
    for origin, extent in (((0, 0, 0), shape), ((0, 0, 0), (16, 16, 32)), ((0, 0, 4), (16, 16, 60))):
        check_raw(cuda, vc.model_extract(S[0], S[1], shape, origin, extent), S[0], S[1], shape, F32, origin, extent)
    # a two-wave box (8 of the 16 blocks of every x-row) into the middle: touched and untouched
    # lanes alternate inside the shared words; the brick has dense blocks among one-bit ones
    origin, extent = (0, 0, 16), (16, 16, 32)
    x = np.zeros(extent, F32)
    x[4:8, 8:12, :] = np.random.default_rng(12).uniform(1, 2, (4, 4, 32))
    B = source(varemu, extent, F32, mode, a=x)
    assert B[1].size == 128 and (B[1] == 1).sum() == 120
    check_raw(cuda, vc.model_insert(B[0], B[1], S[0], S[1], shape, origin, extent), S[0], S[1], shape, F32, origin,
              extent, box=B)
    # ... and an all-zero brick over the dense block's rows
    Z = source(varemu, (4, 16, 64), F32, mode, a=np.zeros((4, 16, 64), F32))
    assert (Z[1] == 1).all() and not Z[0].any()
    check_raw(cuda, vc.model_insert(Z[0], Z[1], S[0], S[1], shape, (0, 0, 0), (4, 16, 64)), S[0], S[1], shape, F32,
              (0, 0, 0), (4, 16, 64), box=Z)


def test_long_blocks(cuda, varemu):  # noqa: F811
    """float64 3D at precision 64: blocks of thousands of bits, cropped and
    pasted at odd bit offsets (a one-bit zero block first)."""
    shape, mode = (8, 8, 12), ("p", 64)
    rng = np.random.default_rng(21)
    a = tv._random_bits(rng, int(np.prod(shape)), F64).reshape(shape)
    a[:4, :4, :4] = 0
    S = source(varemu, shape, F64, mode, a=a)
    assert S[1][0] == 1 and S[1].max() > 3500
    for origin, extent in (((0, 0, 4), (8, 8, 8)), ((0, 0, 0), shape), ((4, 0, 0), (4, 8, 12))):
        check_raw(cuda, vc.model_extract(S[0], S[1], shape, origin, extent), S[0], S[1], shape, F64, origin, extent)
        x = tv._random_bits(rng, int(np.prod(extent)), F64).reshape(extent)
        x[-4:, -4:, -4:] = 0
        B = source(varemu, extent, F64, mode, a=x)
        check_raw(cuda, vc.model_insert(B[0], B[1], S[0], S[1], shape, origin, extent), S[0], S[1], shape, F64, origin,
                  extent, box=B)


# ---------------------------------------------------------------------------
# Mixed modes, slab assembly

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_mixed_modes(cuda, varemu, dtype):  # noqa: F811
    """A full-precision brick pasted into a tolerance 1e-2 archive:
    decode_variable of the result is the brick's values inside the box and the
    archive's outside it."""
    import cuzfp_amd
    td = _tdtype(dtype)
    S = source(varemu, BIG, dtype, ("a", 1e-2))
    old = tv.emu_decompress(varemu, S[0], S[1], BIG, dtype)
    for origin, extent in (((4, 8, 12), (8, 8, 16)), ((8, 16, 32), (5, 6, 6))):
        B = source(varemu, extent, dtype, ru.full(dtype), a=ru.other_values(extent, dtype, origin))
        want = vc.model_insert(B[0], B[1], S[0], S[1], BIG, origin, extent)
        got = cuzfp_amd.insert_region_variable(*dev_stream(cuda, B), *dev_stream(cuda, S), BIG, td, origin, extent)
        check_wrapper(got, want)
        dec = cuzfp_amd.decode_variable(got[0], got[1], BIG, td).cpu().numpy()
        ref = old.copy()
        ref[ru.box_slices(origin, extent)] = tv.emu_decompress(varemu, B[0], B[1], extent, dtype)
        assert np.array_equal(dec.view(np.uint8), ref.view(np.uint8))


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_slab_assembly(cuda, varemu, dtype):  # noqa: F811
    """The streams of A[0:8] and A[8:13] pasted into the all-zero archive (one
    0 bit a block): encode_variable(A), byte for byte."""
    import torch
    import cuzfp_amd
    td = _tdtype(dtype)
    a = tv.array(BIG, dtype)
    x = _dev(a, cuda)
    for mode in (("p", 16), ("a", 1e-3)):
        kw = kw_of(mode)
        nblocks = tv.nblocks(BIG)
        arch = (torch.zeros((nblocks + 63) // 64, dtype=torch.int64, device=cuda),
                torch.ones(nblocks, dtype=torch.int16, device=cuda))
        arch += (cuzfp_amd.variable_index(arch[1], BIG, td),)
        for z0, z1 in ((0, 8), (8, 13)):
            ext = (z1 - z0,) + BIG[1:]
            sw, sl, _ = cuzfp_amd.encode_variable(x[z0:z1].contiguous(), **kw)
            si = cuzfp_amd.variable_index(sl, ext, td)
            w, l, n, i = cuzfp_amd.insert_region_variable(sw, sl, si, *arch, BIG, td, (z0, 0, 0), ext, with_index=True)
            arch = (w, l, i)
        check_wrapper((arch[0], arch[1], n, arch[2]), source(varemu, BIG, dtype, mode))
        ww, wl, wn = cuzfp_amd.encode_variable(x, **kw)
        assert n == wn and torch.equal(arch[1], wl) and torch.equal(arch[0], ww)


# ---------------------------------------------------------------------------
# Capacity

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_capacity(cuda, varemu, dtype):  # noqa: F811
    """A capacity one word short: nothing at or past it is written, and the
    lengths, the count and the index are the full call's.  d_dst == NULL with
    capacity 0 is the size query."""
    S = source(varemu, BIG, dtype, ("p", 16))
    origin, extent = (0, 0, 0), (13, 22, 20)
    B = source(varemu, extent, dtype, ru.full(dtype), a=ru.other_values(extent, dtype, origin))
    for box, want in ((None, vc.model_extract(S[0], S[1], BIG, origin, extent)),
                      (B, vc.model_insert(B[0], B[1], S[0], S[1], BIG, origin, extent))):
        nwords = want[0].size
        raw = Raw(cuda, S[0], S[1], BIG, dtype, origin, extent, box=box, cap_words=nwords - 1)
        assert raw.call() == 0
        assert raw.canaries_intact()  # the canary at the capacity among them
        got, newL, total, idx = raw.result()
        assert total == want[2] and np.array_equal(newL, want[1]) and np.array_equal(idx, want_index(want[1]))
        assert np.array_equal(got[: nwords - 2], want[0][: nwords - 2])
        for with_index in (True, False):
            raw = Raw(cuda, S[0], S[1], BIG, dtype, origin, extent, box=box)
            assert raw.call(with_index, query=True) == 0
            assert raw.canaries_intact(with_index, query=True)
            _, newL, total, idx = raw.result()
            assert total == want[2] and np.array_equal(newL, want[1])
            if with_index:
                assert np.array_equal(idx, want_index(want[1]))


# ---------------------------------------------------------------------------
# Lengths and indices that are not the stream's

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_untrusted_metadata(cuda, varemu, dtype):  # noqa: F811
    """Lengths and an index taken from another stream, lengths of 65535
    throughout, lengths no encoder writes, an index of zeros and one of huge
    offsets -- for the source and for the box.  Every copied length is clamped,
    every source dword is loaded behind the byte-count bound and every store is
    behind the capacity, so nothing can fault by construction: the call
    returns, the canaries around every output hold, the new lengths are the raw
    ones given, and the count and the index are their sums.  A valid case run
    afterwards is exact."""
    S = source(varemu, BIG, dtype, ("p", 16))
    O = source(varemu, BIG, dtype, ru.full(dtype))  # another stream of the same block count, much longer
    origin, extent = (0, 0, 0), (13, 22, 20)
    B = vc.model_extract(S[0], S[1], BIG, origin, extent)
    OB = vc.model_extract(O[0], O[1], BIG, origin, extent)
    ids = vc.box_blocks(BIG, origin, extent)
    rng = np.random.default_rng(3)

    def bads(L, other):
        n, T = L.size, (L.size + 63) // 64 + 1
        illegal = np.where(rng.random(n) < 0.5, rng.integers(2, tp.ebits(dtype) + 2, n), L).astype(np.uint16)
        illegal[::7] = 40000
        return [(other, want_index(other)), (other, None), (L, want_index(other)),
                (np.full(n, 0xFFFF, np.uint16), None), (illegal, None), (L, np.zeros(T, np.uint64)),
                (L, np.full(T, (1 << 63) + 12345, np.uint64)),
                (np.full(n, 0xFFFF, np.uint16), np.full(T, 2 ** 64 - 1, np.uint64))]

    for badL, badI in bads(S[1], O[1]):
        idx_in = want_index(S[1]) if badI is None else badI
        # crop with a bad source
        raw = Raw(cuda, S[0], badL, BIG, dtype, origin, extent, index=idx_in, cap_words=S[0].size + 64)
        assert raw.call() == 0
        assert raw.canaries_intact()
        _, newL, total, idx = raw.result()
        assert np.array_equal(newL, badL[ids]) and total == int(newL.astype(np.int64).sum())
        assert np.array_equal(idx, want_index(newL))
        # paste with a bad source, a good box
        raw = Raw(cuda, S[0], badL, BIG, dtype, origin, extent, box=B, index=idx_in, cap_words=S[0].size + 64)
        assert raw.call() == 0
        assert raw.canaries_intact()
        _, newL, total, idx = raw.result()
        want = badL.copy()
        want[ids] = B[1]
        assert np.array_equal(newL, want) and total == int(newL.astype(np.int64).sum())
        assert np.array_equal(idx, want_index(newL))
    for badL, badI in bads(B[1], OB[1]):
        # paste with a good source, a bad box
        raw = Raw(cuda, S[0], S[1], BIG, dtype, origin, extent, box=(B[0], badL),
                  box_index=want_index(B[1]) if badI is None else badI, cap_words=S[0].size + 64)
        assert raw.call() == 0
        assert raw.canaries_intact()
        _, newL, total, idx = raw.result()
        want = S[1].copy()
        want[ids] = badL
        assert np.array_equal(newL, want) and total == int(newL.astype(np.int64).sum())
        assert np.array_equal(idx, want_index(newL))
        assert raw.inputs_unchanged(S[0], S[1], (B[0], badL))
    check_raw(cuda, B, S[0], S[1], BIG, dtype, origin, extent)
    check_raw(cuda, vc.model_insert(OB[0], OB[1], S[0], S[1], BIG, origin, extent), S[0], S[1], BIG, dtype, origin,
              extent, box=OB)
