"""join_variable without a GPU: the host model of the call, the claim it rests
on, the raw C-ABI's argument errors and size functions, and the Python
wrapper's validation.

The model.  zfp codes every block on its own and writes the blocks back to back
in raster order, so the stream of an array is the streams of its slabs along
the slowest axis laid end to end, bit for bit, where every slab but the last is
a multiple of 4 deep (`model_join`: numpy on bit arrays).  The claim is checked
against the host emulation of test_variable (`varemu`, which the fixture hashes
vouch for), not against the code under test; tests/test_variable_join_gpu.py
compares the device call with the model.
"""
import ctypes

import numpy as np
import pytest

import cuzfp_amd as cz
import test_variable as tv
import test_variable_crop as vc
import test_variable_region_update as ru
from cuzfp_amd.dist import slab_extent
from test_variable import varemu  # noqa: F401  (fixture)
from test_variable_crop import Fake
from test_variable_paths import F32, F64

MODES = ru._modes  # p16, full precision, tolerance 1e-3


def _even(n, k):
    """Depths of `k` slabs of an axis of `n`, as cuzfp_amd.dist shards it."""
    return tuple(b - a for a, b in (slab_extent(n, k, r) for r in range(k)))


# (shape, depths of the parts along the slowest axis)
CASES = [((13, 22, 38), (8, 5)), ((13, 22, 38), (4, 4, 5)), ((13, 22, 38), (4, 4, 4, 1)),
         ((33, 70), (16, 17)), ((33, 70), (4, 8, 12, 9)),
         ((1000,), _even(1000, 2)), ((1000,), _even(1000, 7)), ((1000,), _even(1000, 64)),
         ((6, 5, 9), (4, 2))]
assert {c[0] for c in CASES} == set(vc.SHAPES)


def case_id(c):
    return "x".join(map(str, c[0])) + "-%d" % len(c[1])


def slabs(shape, depths):
    """[(z0, z1)] of the parts."""
    assert sum(depths) == shape[0] and all(d > 0 for d in depths) and all(d % 4 == 0 for d in depths[:-1])
    z = np.concatenate([[0], np.cumsum(depths)])
    return [(int(z[i]), int(z[i + 1])) for i in range(len(depths))]


# ---------------------------------------------------------------------------
# The model

def model_join(parts):
    """(words, L, nbits) of the parts' blocks, back to back.  parts: (words, L) or (words, L, nbits)."""
    bits = [ru._bits(p[0])[: int(p[1].astype(np.int64).sum())] for p in parts]
    return vc._pack(bits, np.concatenate([p[1] for p in parts]))


def test_model_join_by_hand():
    """Two parts of 3 and 70 bits: the second begins at bit 3 of word 0 and the pad is zero."""
    a = (np.array([0b101], np.uint64), np.array([1, 2], np.uint16))
    b = (np.array([2 ** 64 - 1, 0b111111], np.uint64), np.array([64, 6], np.uint16))
    w, L, n = model_join([a, b])
    assert n == 73 and L.tolist() == [1, 2, 64, 6]
    assert w.tolist() == [0b101 | ((2 ** 64 - 1) << 3) & (2 ** 64 - 1), 0b111111111]


@pytest.mark.parametrize("dtype", [F32, F64], ids=lambda d: d.name)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_join_is_the_stream_of_the_array(varemu, case, dtype):  # noqa: F811
    """The claim the feature rests on: model_join of the emulation's streams of
    the slabs is the emulation's stream of the whole array."""
    shape, depths = case
    a = tv.array(shape, dtype)
    for mode in MODES(dtype):
        want = tv.emu_compress(varemu, a, *ru.mode_of(dtype, mode))
        parts = [tv.emu_compress(varemu, a[z0:z1], *ru.mode_of(dtype, mode)) for z0, z1 in slabs(shape, depths)]
        got = model_join(parts)
        assert got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), mode


def test_join_inverts_extract(varemu):  # noqa: F811
    """model_extract of the slabs, joined, is the source."""
    shape, depths = (13, 22, 38), (4, 4, 5)
    S = tv.emu_compress(varemu, tv.array(shape, F32), *ru.mode_of(F32, ("a", 1e-3)))
    parts = [vc.model_extract(S[0], S[1], shape, (z0, 0, 0), (z1 - z0,) + shape[1:]) for z0, z1 in slabs(shape, depths)]
    got = model_join(parts)
    assert got[2] == S[2] and np.array_equal(got[1], S[1]) and np.array_equal(got[0], S[0])


# ---------------------------------------------------------------------------
# Argument checks without a device

@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def _at(p, by):
    return ctypes.c_void_p(p.value + by)


def table(entries):
    """A cuzfp_hip_variable_part array from (words, bytes, lengths, nblocks)."""
    t = (cz.VariablePart * max(len(entries), 1))()
    for k, e in enumerate(entries):
        t[k] = cz.VariablePart(*e)
    return t


def test_argument_errors(libs):
    """Every argument error of cuzfp_hip_join_variable: a status, with pointers
    that are never dereferenced."""
    lib = cz.library()
    assert lib.cuzfp_hip_abi_version() == 1
    P = {k: ctypes.c_void_p(0x100000 * (i + 1)) for i, k in enumerate(("dst", "len", "index", "total", "ws"))}
    W0, L0 = 0x4000000, 0x8000000  # part k's stream at W0 + 0x10000 k (4096 bytes), its lengths at L0 + 0x1000 k
    ws16 = lib.cuzfp_hip_join_variable_workspace_bytes(3, 16, 16, 16)
    assert ws16 == 8 * (64 + 1)

    def parts_of(counts, nbytes=4096):
        return [(W0 + 0x10000 * k, nbytes, L0 + 0x1000 * k, c) for k, c in enumerate(counts)]

    def call(t=3, n=(16, 16, 16), parts=None, nparts=None, cap=8192, ws_bytes=None, **over):
        p = dict(P)
        p.update(over)
        if parts is None:
            parts = parts_of((32, 32))
        if ws_bytes is None:
            ws_bytes = lib.cuzfp_hip_join_variable_workspace_bytes(3, *n) or ws16
        tab = table(parts) if parts != "null" else None
        return lib.cuzfp_hip_join_variable(tab, len(parts) if nparts is None else nparts, t, *n, p["dst"], cap,
                                           p["len"], p["index"], p["total"], p["ws"], ws_bytes, None)

    # the table: none, no part, more than 64 parts
    assert call(parts="null", nparts=2) == 1
    assert call(parts=[], nparts=0) == 1 and call(nparts=0) == 1
    assert call(n=(4, 4, 260), parts=parts_of((1,) * 65)) == 1  # 65 one-slab parts of 65 slabs
    assert call(n=(260, 0, 0), parts=parts_of((1,) * 65)) == 1
    # block counts: none, no whole slab (16 blocks a slab here), too few, too many
    assert call(parts=parts_of((0, 64))) == 1 and call(parts=parts_of((64, 0))) == 1
    assert call(parts=parts_of((24, 40))) == 1 and call(parts=parts_of((63, 1))) == 1
    assert call(parts=parts_of((32, 16))) == 1 and call(parts=parts_of((32, 48))) == 1
    assert call(parts=parts_of((32,))) == 1 and call(parts=parts_of((16,) * 5)) == 1
    assert call(parts=parts_of((2 ** 32 - 16, 80))) == 1  # a sum that would wrap 32 bits
    assert call(n=(16, 16, 0), parts=parts_of((6, 10))) == 1  # 2D: 4 blocks a slab
    assert call(n=(18, 16, 0), parts=parts_of((8, 12))) == 1  # ... 5 with a ragged x
    # null and misaligned pointers of a part: the stream 4 bytes, the lengths 2
    good = parts_of((32, 32))
    for k in (0, 1):
        for field, by in ((0, 2), (0, 1), (2, 1)):
            bad = [list(e) for e in good]
            bad[k][field] += by
            assert call(parts=[tuple(e) for e in bad]) == 1, (k, field, by)
            bad[k][field] = None
            assert call(parts=[tuple(e) for e in bad]) == 1, (k, field)
    # null and misaligned outputs (d_index may be null; that call would launch and is not made here)
    for name in ("len", "total", "ws"):
        assert call(**{name: None}) == 1, name
    assert call(dst=None) == 1  # no destination, yet a capacity
    for name, by in (("len", 1), ("index", 4), ("dst", 4), ("total", 4), ("ws", 4)):
        assert call(**{name: _at(P[name], by)}) == 1, name
    # a short workspace
    assert call(ws_bytes=ws16 - 1) == 1 and call(ws_bytes=0) == 1
    # an output over a part's stream (4096 bytes) or lengths (64 bytes), either part, either end
    for k in (0, 1):
        w, l = ctypes.c_void_p(good[k][0]), ctypes.c_void_p(good[k][2])
        for name, size in (("dst", 8192), ("len", 128), ("index", 16), ("total", 8), ("ws", ws16)):
            assert call(**{name: w}) == 1 and call(**{name: _at(w, 4096 - 8)}) == 1, (k, name)
            assert call(**{name: ctypes.c_void_p(w.value - size + 8)}) == 1, (k, name)
            assert call(**{name: l}) == 1 and call(**{name: _at(l, 64 - 8)}) == 1, (k, name)
            assert call(**{name: ctypes.c_void_p(l.value - size + 8)}) == 1, (k, name)
    # byte counts whose bits would wrap
    assert call(parts=parts_of((32, 32), nbytes=2 ** 60)) == 1
    # integer and unknown types (before anything else is looked at), bad dimensions
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2 and call(t=0) == 2
    assert call(t=1, parts="null", nparts=99) == 2
    assert call(n=(16, 0, 16)) == 1 and call(n=(0, 0, 0)) == 1


def test_size_functions(libs):
    lib = cz.library()
    ws = lib.cuzfp_hip_join_variable_workspace_bytes
    for t in (3, 4):
        assert ws(t, 38, 22, 13) == 8 * (240 + 1) == lib.cuzfp_hip_variable_workspace_bytes(t, 38, 22, 13)
        assert ws(t, 1000, 0, 0) == 8 * (250 + 1)
        assert ws(t, 259, 131, 0) == 8 * (65 * 33 + 3)
    assert ws(1, 16, 16, 16) == 0 and ws(2, 16, 16, 16) == 0 and ws(9, 16, 16, 16) == 0
    assert ws(3, 0, 0, 0) == 0 and ws(3, 16, 0, 16) == 0

    mx = lib.cuzfp_hip_join_variable_maximum_size

    def size(*nbytes):
        return mx(table([(0x1000, b, 0x2000, 1) for b in nbytes]), len(nbytes))

    assert size(8) == 8 and size(4, 4) == 8 and size(4, 5) == 16 and size(0) == 0
    assert size(1000, 24) == 1024 and size(1001, 24) == 1032 and size(*([8] * 64)) == 512
    assert size(1, 2, 3) == 8 and size(12, 12, 12, 4) == 40
    # invalid: no table, no part, more than 64 parts, bits that would wrap
    assert mx(None, 2) == 0 and mx(table([(0x1000, 8, 0x2000, 1)]), 0) == 0
    assert mx(table([(0x1000, 8, 0x2000, 1)] * 65), 65) == 0
    assert size(2 ** 60) == 0 and size(8, 2 ** 61) == 0


# ---------------------------------------------------------------------------
# The wrapper's validation

def test_python_validation(libs):
    """The dtype, the shape, the part count, then the tensors and the block
    counts, before anything touches a device."""
    assert "join_variable" in cz.__all__
    shape = (16, 16, 16)  # 16 blocks a slab, 64 blocks
    w = Fake(100)

    def join(parts=None, shape=shape, dtype=np.float32, **kw):
        if parts is None:
            parts = [(w, Fake(32, 2)), (w, Fake(32, 2), 1000)]
        return cz.join_variable(parts, shape, dtype, **kw)

    for dtype in (np.int32, np.int64):
        with pytest.raises(cz.CodecError) as e:
            join(dtype=dtype)
        assert e.value.status == 2
    with pytest.raises(ValueError):
        join(shape=(16,) * 4)
    with pytest.raises(ValueError, match="invalid shape"):
        join(shape=(16, 0, 16))
    with pytest.raises(ValueError, match="1 to 64 parts, not 0"):
        join(parts=[])
    with pytest.raises(ValueError, match="1 to 64 parts, not 65"):
        join(parts=[(w, Fake(1, 2))] * 65, shape=(260,))
    with pytest.raises(ValueError, match="part 1 must be"):
        join(parts=[(w, Fake(32, 2)), (w,)])
    # host tensors, wrong widths, non-contiguous ones
    with pytest.raises(ValueError, match="part 0: expects a device"):
        join(parts=[(Fake(100, cuda=False), Fake(32, 2)), (w, Fake(32, 2))])
    with pytest.raises(ValueError, match="part 1: expects a device"):
        join(parts=[(w, Fake(32, 2)), (w, Fake(32, 2, cuda=False))])
    with pytest.raises(ValueError, match="16-bit"):
        join(parts=[(w, Fake(32, 4)), (w, Fake(32, 2))])
    with pytest.raises(ValueError, match="contiguous"):
        join(parts=[(w, Fake(32, 2, contiguous=False)), (w, Fake(32, 2))])
    with pytest.raises(ValueError, match="contiguous"):
        join(parts=[(Fake(100, contiguous=False), Fake(32, 2)), (w, Fake(32, 2))])
    with pytest.raises(ValueError, match="32- or 64-bit"):
        join(parts=[(Fake(100, 2), Fake(32, 2)), (w, Fake(32, 2))])
    with pytest.raises(ValueError, match="fewer than its 6401 bits"):
        join(parts=[(w, Fake(32, 2), 6401), (w, Fake(32, 2))])
    # block counts that are no whole slabs, or do not add up
    with pytest.raises(ValueError, match="part 0 has 24 blocks, no whole number of slabs of 16"):
        join(parts=[(w, Fake(24, 2)), (w, Fake(40, 2))])
    with pytest.raises(ValueError, match="part 1 has 0 blocks"):
        join(parts=[(w, Fake(64, 2)), (w, Fake(0, 2))])
    with pytest.raises(ValueError, match="the parts have 48 blocks, the array .* has 64"):
        join(parts=[(w, Fake(32, 2)), (w, Fake(16, 2))])
    with pytest.raises(ValueError, match="the parts have 80 blocks"):
        join(parts=[(w, Fake(32, 2)), (w, Fake(48, 2))])
    with pytest.raises(ValueError, match="slabs of 10 blocks"):  # 2D: a slab is a row of ceil(38 / 4) blocks
        join(parts=[(w, Fake(15, 2)), (w, Fake(45, 2))], shape=(22, 38))
    with pytest.raises(ValueError, match="out must be"):
        join(out=Fake(100, cuda=False))
    with pytest.raises(ValueError, match="out must be"):
        join(out=Fake(100, 4))
