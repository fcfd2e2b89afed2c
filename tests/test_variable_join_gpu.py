"""join_variable on the GPU against the host model of tests/test_variable_join.py
(`model_join`: numpy on bit arrays, the part streams from the host emulation
`varemu`, which the fixture hashes vouch for) and against the device calls it
replaces.

Every comparison is of bytes.  The raw C-ABI runs on buffers with canaries on
both sides of the stream, the lengths, the index, the count and the workspace
(`Raw`, after test_variable_crop_gpu's); the wrapper's `out` is filled with
all-ones words first, and what lies past the result must still hold the fill.
"""
import ctypes

import numpy as np
import pytest

import test_variable as tv
import test_variable_crop as vc
import test_variable_join as vj
import test_variable_paths as tp
import test_variable_region_update as ru
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_crop_gpu import check_wrapper, same, source
from test_variable_gpu import CANARY, _dev, _lengths, _tdtype, _words
from test_variable_paths import F32, F64, want_index
from test_variable_region_update_gpu import FILL, ICANARY, kw_of

pytestmark = pytest.mark.gpu

BIG = (13, 22, 38)


def emu_parts(varemu, shape, depths, dt, mode):  # noqa: F811
    """The emulation's (words, L, nbits) of every slab of tv.array(shape, dt)."""
    a = tv.array(shape, dt)
    return [source(varemu, (z1 - z0,) + tuple(shape[1:]), dt, mode, a=a[z0:z1]) for z0, z1 in vj.slabs(shape, depths)]


class Raw:
    """cuzfp_hip_join_variable on buffers with canaries on both sides of every
    output.  parts: host (words, L[, nbits]); odd: d_dst at an odd multiple of
    8 bytes, where the 16-byte stores pair the words the other way."""
    PAD = 64

    def __init__(self, cuda, parts, shape, dt, cap_words=None, odd=False):
        import torch
        import cuzfp_amd
        self.lib = cuzfp_amd.library()
        self.t = tv.TC[np.dtype(dt)]
        self.ext = cuzfp_amd._extents(shape)
        self.host = [(np.ascontiguousarray(p[0]), np.ascontiguousarray(p[1])) for p in parts]
        self.w = [_dev(w.view(np.int64), cuda) for w, _ in self.host]
        self.l = [_dev(L.view(np.int16), cuda) for _, L in self.host]
        self.tab = (cuzfp_amd.VariablePart * max(len(parts), 1))()
        for k in range(len(parts)):
            self.tab[k] = cuzfp_amd.VariablePart(self.w[k].data_ptr(), self.w[k].numel() * 8, self.l[k].data_ptr(),
                                                 self.l[k].numel())
        self.K = len(parts)
        self.n = tv.nblocks(shape)
        self.need = self.lib.cuzfp_hip_join_variable_workspace_bytes(self.t, *self.ext)
        bound = self.lib.cuzfp_hip_join_variable_maximum_size(self.tab, self.K)
        assert bound == 8 * ((8 * sum(w.nbytes for w, _ in self.host) + 63) // 64) or self.K > 64
        assert self.need >= 8 * (self.n + 1)
        self.T = (self.n + 63) // 64
        self.cap = bound // 8 if cap_words is None else cap_words
        P = self.PAD
        self.d0 = P + (1 if odd else 0)
        self.dst = torch.full((self.cap + 2 * P + 1,), ICANARY, dtype=torch.int64, device=cuda)
        assert (self.dst[self.d0:].data_ptr() % 16 == 8) == odd
        self.len = torch.full((self.n + 2 * P,), 0x5A5A, dtype=torch.int16, device=cuda)
        self.idx = torch.full((self.T + 1 + 2 * P,), ICANARY, dtype=torch.int64, device=cuda)
        self.total = torch.full((3,), ICANARY, dtype=torch.int64, device=cuda)
        self.ws = torch.full((self.need // 8 + P,), ICANARY, dtype=torch.int64, device=cuda)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(self, with_index=True, query=False, nparts=None):
        P = self.PAD
        dst, cap = (None, 0) if query else (self.dst[self.d0:].data_ptr(), self.cap * 8)
        idx = self.idx[P:].data_ptr() if with_index else None
        return self.lib.cuzfp_hip_join_variable(self.tab, self.K if nparts is None else nparts, self.t, *self.ext,
                                                dst, cap, self.len[P:].data_ptr(), idx, self.total[1:].data_ptr(),
                                                self.ws.data_ptr(), self.need, self.st)

    def canaries_intact(self, with_index=True, query=False):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        ok = (bool((self.dst[:self.d0] == ICANARY).all()) and bool((self.dst[self.d0 + self.cap:] == ICANARY).all()) and
              bool((self.len[:P] == 0x5A5A).all()) and bool((self.len[P + self.n:] == 0x5A5A).all()) and
              int(self.total[0]) == ICANARY and int(self.total[2]) == ICANARY and
              bool((self.ws[self.need // 8:] == ICANARY).all()))
        if query:
            ok = ok and bool((self.dst == ICANARY).all())
        if with_index:
            return ok and bool((self.idx[:P] == ICANARY).all()) and bool((self.idx[P + self.T + 1:] == ICANARY).all())
        return ok and bool((self.idx == ICANARY).all())

    def untouched(self):
        """Nothing was launched: every output still holds its fill."""
        import torch
        torch.cuda.synchronize()
        return (bool((self.dst == ICANARY).all()) and bool((self.len == 0x5A5A).all()) and
                bool((self.idx == ICANARY).all()) and bool((self.total == ICANARY).all()) and
                bool((self.ws == ICANARY).all()))

    def result(self):
        import torch
        torch.cuda.synchronize()
        P = self.PAD
        L = self.len[P: P + self.n].cpu().numpy().view(np.uint16)
        return (self.dst[self.d0: self.d0 + self.cap].cpu().numpy().view(np.uint64), L, int(self.total[1]),
                self.idx[P: P + self.T + 1].cpu().numpy().view(np.uint64))

    def inputs_unchanged(self):
        return all(np.array_equal(_words(w), h[0]) and np.array_equal(_lengths(l), h[1])
                   for w, l, h in zip(self.w, self.l, self.host))


def check_raw(cuda, want, parts, shape, dt, with_index=True, odd=False, cid=None):
    """One call of the C-ABI against the model's (words, L, nbits): the count,
    the lengths, the stream's words and the canary after them, the index."""
    raw = Raw(cuda, parts, shape, dt, odd=odd)
    cid = cid or (shape, np.dtype(dt).name, len(parts), with_index, odd)
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
    assert raw.inputs_unchanged(), cid


def dev_parts(cuda, parts):
    return [(_dev(p[0].view(np.int64), cuda), _dev(p[1].view(np.int16), cuda), p[2]) for p in parts]


# ---------------------------------------------------------------------------
# 1. The cases of the CPU file against the model

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("case", vj.CASES, ids=vj.case_id)
def test_cases(cuda, varemu, case, dtype):  # noqa: F811
    """The raw call equals model_join -- which test_variable_join shows to be
    the emulation's stream of the whole array, asserted here again -- with and
    without d_index and with d_dst at both 16-byte phases."""
    shape, depths = case
    for m, mode in enumerate(vj.MODES(dtype)):
        parts = emu_parts(varemu, shape, depths, dtype, mode)
        want = vj.model_join(parts)
        assert same(want, source(varemu, shape, dtype, mode))
        check_raw(cuda, want, parts, shape, dtype, with_index=m != 1, odd=m == 2)


# ---------------------------------------------------------------------------
# 2. Against the device code

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("case", vj.CASES[1:5:3] + vj.CASES[6:7] + vj.CASES[8:], ids=vj.case_id)
def test_against_existing_device_code(cuda, case, dtype):
    """join_variable of encode_variable of the slabs equals encode_variable of
    the array in words, lengths, count and index, and equals K successive
    insert_region_variable pastes into the all-zero archive."""
    import torch
    import cuzfp_amd
    shape, depths = case
    td = _tdtype(dtype)
    x = _dev(tv.array(shape, dtype), cuda)
    for mode in (("p", 16), ("a", 1e-3)):
        kw = kw_of(mode)
        parts = [cuzfp_amd.encode_variable(x[z0:z1].contiguous(), **kw) for z0, z1 in vj.slabs(shape, depths)]
        jw, jl, jn, ji = cuzfp_amd.join_variable(parts, shape, td, with_index=True)
        ww, wl, wn = cuzfp_amd.encode_variable(x, **kw)
        assert jn == wn and torch.equal(jl, wl) and torch.equal(jw, ww), mode
        assert torch.equal(ji, cuzfp_amd.variable_index(wl, shape, td)), mode
        nblocks = tv.nblocks(shape)
        arch = (torch.zeros((nblocks + 63) // 64, dtype=torch.int64, device=cuda),
                torch.ones(nblocks, dtype=torch.int16, device=cuda))
        arch += (cuzfp_amd.variable_index(arch[1], shape, td),)
        for (z0, z1), (sw, sl, _) in zip(vj.slabs(shape, depths), parts):
            ext = (z1 - z0,) + tuple(shape[1:])
            si = cuzfp_amd.variable_index(sl, ext, td)
            w, l, n, i = cuzfp_amd.insert_region_variable(sw, sl, si, *arch, shape, td, (z0,) + (0,) * (len(shape) - 1),
                                                          ext, with_index=True)
            arch = (w, l, i)
        assert jn == n and torch.equal(jl, arch[1]) and torch.equal(jw, arch[0]) and torch.equal(ji, arch[2]), mode


# ---------------------------------------------------------------------------
# 3. Shared words

def test_one_word_from_64_parts(cuda, varemu):  # noqa: F811
    """A float32 zero array (256,) at tolerance 1e-3 as 64 one-block parts of
    one bit each: the one output word takes a bit from each of 64 parts."""
    shape, mode = (256,), ("a", 1e-3)
    a = np.zeros(shape, F32)
    parts = [source(varemu, (4,), F32, mode, a=a[:4])] * 64
    assert all(p[2] == 1 for p in parts)
    want = vj.model_join(parts)
    assert want[2] == 64 and want[0].tolist() == [0] and same(want, source(varemu, shape, F32, mode, a=a))
    check_raw(cuda, want, parts, shape, F32)
    # ... and with set bits: one-bit blocks are legal only as 0, so these parts are foreign, but
    # the move of bits is the same: part k's bit 0 is bit k of the word
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 64).astype(np.uint64)
    parts = [(np.array([b | np.uint64(0xF0)], np.uint64), np.array([1], np.uint16), 1) for b in bits]
    want = vj.model_join(parts)
    assert want[0][0] == sum(int(b) << k for k, b in enumerate(bits))
    check_raw(cuda, want, parts, shape, F32, odd=True)


def test_dense_block_among_one_bit_parts(cuda, varemu):  # noqa: F811
    """(4096,) float32 with one dense block, as 64 parts of 16 blocks: parts of
    16 bits, four to an output word, and one long part that shifts the rest."""
    shape, mode = (4096,), ("a", 1e-3)
    a = np.zeros(shape, F32)
    a[20 * 4: 21 * 4] = np.random.default_rng(11).uniform(1, 2, 4)
    depths = (64,) * 64
    parts = [source(varemu, (64,), F32, mode, a=a[z0:z1]) for z0, z1 in vj.slabs(shape, depths)]
    assert sum(p[2] == 16 for p in parts) == 63 and parts[1][2] > 16
    want = vj.model_join(parts)
    assert same(want, source(varemu, shape, F32, mode, a=a))
    check_raw(cuda, want, parts, shape, F32)
    check_raw(cuda, want, parts, shape, F32, with_index=False, odd=True)


def test_shift_zero(cuda, varemu):  # noqa: F811
    """A zero (768,) as 3 parts of 64 one-bit blocks: every part offset is a
    multiple of 64, the funnel shift by 0.  Then the same offsets with set
    bits in the parts (foreign streams; the move is the same)."""
    shape, mode = (768,), ("a", 1e-3)
    a = np.zeros(shape, F32)
    parts = [source(varemu, (256,), F32, mode, a=a[:256])] * 3
    assert all(p[2] == 64 for p in parts)
    want = vj.model_join(parts)
    assert same(want, source(varemu, shape, F32, mode, a=a))
    check_raw(cuda, want, parts, shape, F32)
    rng = np.random.default_rng(6)
    parts = [(rng.integers(0, 2 ** 63, 1, dtype=np.uint64) * np.uint64(2) + np.uint64(1), np.ones(64, np.uint16), 64)
             for _ in range(3)]
    want = vj.model_join(parts)
    assert np.array_equal(want[0], np.concatenate([p[0] for p in parts]))
    for odd in (False, True):
        check_raw(cuda, want, parts, shape, F32, odd=odd)


# ---------------------------------------------------------------------------
# 4. Long blocks

def test_long_blocks(cuda, varemu):  # noqa: F811
    """float64 (12, 8, 8) of random bit patterns at precision 64 with its first
    block zero: blocks above 3500 bits, every later part at an odd bit."""
    shape, mode, depths = (12, 8, 8), ("p", 64), (4, 4, 4)
    a = tv._random_bits(np.random.default_rng(21), int(np.prod(shape)), F64).reshape(shape)
    a[:4, :4, :4] = 0
    parts = [source(varemu, (4, 8, 8), F64, mode, a=a[z0:z1]) for z0, z1 in vj.slabs(shape, depths)]
    assert parts[0][1][0] == 1 and max(int(p[1].max()) for p in parts) > 3500
    want = vj.model_join(parts)
    assert same(want, source(varemu, shape, F64, mode, a=a))
    for odd in (False, True):
        check_raw(cuda, want, parts, shape, F64, odd=odd)


# ---------------------------------------------------------------------------
# 5. The part count

def test_part_counts(cuda, varemu):  # noqa: F811
    """K = 1 is a copy, K = 64 succeeds, K = 65 is status 1 with nothing launched."""
    S = source(varemu, BIG, F32, ("p", 16))
    check_raw(cuda, S, [S], BIG, F32)
    shape, mode = (260,), ("p", 16)  # 65 blocks
    a = tv.array(shape, F32)
    one = [source(varemu, (4,), F32, mode, a=a[4 * k: 4 * k + 4]) for k in range(65)]
    parts64 = one[:63] + [source(varemu, (8,), F32, mode, a=a[252:])]
    want = vj.model_join(parts64)
    assert same(want, source(varemu, shape, F32, mode, a=a))
    check_raw(cuda, want, parts64, shape, F32)
    raw = Raw(cuda, one, shape, F32, cap_words=want[0].size)
    assert raw.call() == 1 and raw.untouched()
    assert raw.lib.cuzfp_hip_join_variable_maximum_size(raw.tab, 65) == 0
    import cuzfp_amd
    with pytest.raises(ValueError, match="1 to 64 parts, not 65"):
        cuzfp_amd.join_variable(dev_parts(cuda, one), shape, _tdtype(F32))


# ---------------------------------------------------------------------------
# 6. Capacity

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_capacity(cuda, varemu, dtype):  # noqa: F811
    """A capacity one word short: nothing at or past it is written, and the
    lengths, the count and the index are the full call's.  d_dst == NULL with
    capacity 0 is the size query."""
    parts = emu_parts(varemu, BIG, (4, 4, 5), dtype, ("p", 16))
    want = vj.model_join(parts)
    nwords = want[0].size
    for odd in (False, True):
        raw = Raw(cuda, parts, BIG, dtype, cap_words=nwords - 1, odd=odd)
        assert raw.call() == 0
        assert raw.canaries_intact()  # the canary at the capacity among them
        got, newL, total, idx = raw.result()
        assert total == want[2] and np.array_equal(newL, want[1]) and np.array_equal(idx, want_index(want[1]))
        assert np.array_equal(got[: nwords - 1], want[0][: nwords - 1])
    for with_index in (True, False):
        raw = Raw(cuda, parts, BIG, dtype)
        assert raw.call(with_index, query=True) == 0
        assert raw.canaries_intact(with_index, query=True)
        _, newL, total, idx = raw.result()
        assert total == want[2] and np.array_equal(newL, want[1])
        if with_index:
            assert np.array_equal(idx, want_index(want[1]))


# ---------------------------------------------------------------------------
# 7. Lengths that are not the stream's

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_untrusted_lengths(cuda, varemu, dtype):  # noqa: F811
    """Lengths taken from another stream, lengths of 65535 throughout, lengths
    no encoder writes, and all-zero lengths for one part.  The part offsets are
    the scan of what the call itself wrote, every source dword is loaded behind
    its part's byte count and every store is behind the capacity, so nothing
    can fault by construction: the call returns, the canaries around every
    output hold, the new lengths are the raw concatenation, and the count and
    the index are their sums.  A valid case run afterwards is exact."""
    depths = (4, 4, 5)
    parts = emu_parts(varemu, BIG, depths, dtype, ("p", 16))
    other = emu_parts(varemu, BIG, depths, dtype, ru.full(dtype))  # the same block counts, much longer
    rng = np.random.default_rng(3)

    def illegal(L):
        bad = np.where(rng.random(L.size) < 0.5, rng.integers(2, tp.ebits(dtype) + 2, L.size), L).astype(np.uint16)
        bad[::7] = 40000
        return bad

    nwords = sum(p[0].size for p in parts)
    variants = [[(p[0], o[1]) for p, o in zip(parts, other)],
                [(o[0], p[1]) for p, o in zip(parts, other)],
                [(p[0], np.full(p[1].size, 0xFFFF, np.uint16)) for p in parts],
                [(p[0], illegal(p[1])) for p in parts]]
    for k in range(3):  # one part of no bits: first, middle, last
        variants.append([(p[0], np.zeros(p[1].size, np.uint16) if j == k else p[1]) for j, p in enumerate(parts)])
    variants.append([(p[0], np.zeros(p[1].size, np.uint16)) for p in parts])  # a stream of no bits
    for v, bad in enumerate(variants):
        raw = Raw(cuda, bad, BIG, dtype, cap_words=nwords + 64, odd=v % 2 == 1)
        assert raw.call() == 0, v
        assert raw.canaries_intact(), v
        got, newL, total, idx = raw.result()
        wantL = np.concatenate([b[1] for b in bad])
        assert np.array_equal(newL, wantL) and total == int(wantL.astype(np.int64).sum()), v
        assert np.array_equal(idx, want_index(wantL)), v
        assert raw.inputs_unchanged(), v
        if 4 <= v < 7:
            # a part of no bits is stepped over: the other parts' bits, end to end
            want = vj.model_join([b for j, b in enumerate(bad) if j != v - 4])
            assert total == want[2] and np.array_equal(got[: want[0].size], want[0]), v
            assert (got[want[0].size:] == np.uint64(CANARY)).all(), v
        if v == 7:
            assert (got == np.uint64(CANARY)).all()
    check_raw(cuda, vj.model_join(parts), parts, BIG, dtype)


# ---------------------------------------------------------------------------
# 8. The wrapper

@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
def test_wrapper(cuda, varemu, dtype):  # noqa: F811
    """An `out` of all-ones words: the model's bytes, the fill after them; the
    default allocation; a stream of its own; parts without their bit counts."""
    import torch
    import cuzfp_amd
    td = _tdtype(dtype)
    parts = emu_parts(varemu, BIG, (4, 4, 4, 1), dtype, ("a", 1e-3))
    want = vj.model_join(parts)
    d = dev_parts(cuda, parts)
    buf = torch.full((want[0].size + 9,), FILL, dtype=torch.int64, device=cuda)
    check_wrapper(cuzfp_amd.join_variable(d, BIG, td, out=buf, with_index=True), want, buf)
    check_wrapper(cuzfp_amd.join_variable(d, BIG, td), want)
    check_wrapper(cuzfp_amd.join_variable([p[:2] for p in d], BIG, td, with_index=True), want)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    buf = torch.full((want[0].size + 9,), FILL, dtype=torch.int64, device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    got = cuzfp_amd.join_variable(d, BIG, td, out=buf, stream=s, with_index=True)
    s.synchronize()
    check_wrapper(got, want, buf)
    # the join decodes to the array, and the slabs cropped out of it are the parts again
    dec = cuzfp_amd.decode_variable(got[0], got[1], BIG, td).cpu().numpy()
    assert np.array_equal(dec.view(np.uint8), tv.emu_decompress(varemu, want[0], want[1], BIG, dtype).view(np.uint8))
    for (z0, z1), p in zip(vj.slabs(BIG, (4, 4, 4, 1)), parts):
        check_wrapper(cuzfp_amd.extract_region_variable(got[0], got[1], got[3], BIG, td, (z0, 0, 0),
                                                        (z1 - z0,) + BIG[1:]), p)
    with pytest.raises(ValueError, match="the parts have 180 blocks"):
        cuzfp_amd.join_variable(d[:3], BIG, td)
