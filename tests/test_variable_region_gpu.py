"""Random access into a variable-rate stream on the GPU: variable_index,
decode_region_variable and decode_variable(index=) against the fixture of
tests/test_variable.py.

Blocks decode independently, so the expected value of every box is that box
cut out of the reference's decode of the whole array (test_variable_gpu.ref_of:
the host emulation's bytes, accepted only on the fixture's SHA-256), compared
bit for bit.  The expected index is numpy's uint64 running sum of the
fixture's lengths.
"""
import ctypes

import numpy as np
import pytest

import test_variable as tv
from test_variable import golden, varemu  # noqa: F401  (fixtures)
from test_variable_gpu import CANARY, CASES, VARIANTS, _dev, _kw, _tdtype, ref_of

pytestmark = pytest.mark.gpu


def want_index(L):
    """index[t] = sum of lengths[0 .. 64 t), index[T] = the total, in uint64."""
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(L.astype(np.uint64), dtype=np.uint64)])
    return np.concatenate([c[:-1][::64], c[-1:]])


def boxes(shape):
    """(origin, extent) per shape: the whole array, one element, an interior box
    unaligned on every axis, a block-aligned box, the far corner with the
    partial blocks; (13, 22, 38): a box 3 blocks wide (a wave holds 21 runs of 3
    blocks from all four tiles, one of them straddling the tile edge at block 64)."""
    n = len(shape)
    out = [((0,) * n, shape),
           (tuple(s // 2 for s in shape), (1,) * n),
           (tuple(min(1 + k, s - 2) for k, s in enumerate(shape)), tuple(max(1, s - 3 - k) for k, s in enumerate(shape))),
           (tuple(4 * ((s // 4) // 3) for s in shape), tuple(4 * max(1, (s // 4) // 2) for s in shape)),
           (tuple(max(0, s - 6) for s in shape), tuple(min(6, s) for s in shape))]
    if shape == (13, 22, 38):
        out.append(((0, 0, 9), (13, 22, 10)))  # x blocks 2 .. 4 of 10: blocks 62, 63 | 64 are one run
    for o, e in out:
        assert all(0 <= a and b >= 1 and a + b <= s for a, b, s in zip(o, e, shape)), (shape, o, e)
    return out


def _box(origin, extent):
    return tuple(slice(o, o + e) for o, e in zip(origin, extent))


def _same(t, want):
    return np.array_equal(np.ascontiguousarray(t.cpu().numpy()).view(np.uint8),
                          np.ascontiguousarray(want).view(np.uint8))


def _stream(words, L, cuda):
    """The device tensors of a reference stream: words, lengths, and the index
    from numpy (independent of variable_index)."""
    return (_dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda),
            _dev(want_index(L).view(np.int64), cuda))


@pytest.mark.parametrize("case", CASES, ids=tv.case_id)
def test_index(cuda, varemu, golden, case):  # noqa: F811
    import cuzfp_amd
    _, L, nbits, _ = ref_of(varemu, golden, case)
    want = want_index(L)
    assert want.size == (L.size + 63) // 64 + 1 and int(want[-1]) == nbits == golden.get(case)["nbits"]
    got = cuzfp_amd.variable_index(_dev(L.view(np.int16), cuda), case[0], _tdtype(case[1]))
    assert got.element_size() == 8 and np.array_equal(got.cpu().numpy().view(np.uint64), want)


def test_index_past_32_bits(cuda):
    """70 000 blocks of 65535 bits: the sums pass 2^32 at block 65537."""
    import torch
    import cuzfp_amd
    n = 70000
    L = np.full(n, 65535, np.uint16)
    want = want_index(L)
    assert int(want[-1]) == n * 65535 > 2 ** 32
    got = cuzfp_amd.variable_index(torch.full((n,), -1, dtype=torch.int16, device=cuda), (4 * n,), torch.float32)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)


def test_index_of_odd_view(cuda, varemu, golden):  # noqa: F811
    """`lengths` starting at an odd element of a larger tensor (2-byte aligned
    only), into a given `out` on a non-default stream."""
    import torch
    import cuzfp_amd
    case = ((13, 22, 38), np.dtype(np.float32), "a", 1e-3)
    _, L, _, _ = ref_of(varemu, golden, case)
    wide = torch.full((L.size + 8,), 0x7777, dtype=torch.int16, device=cuda)
    view = wide[3: 3 + L.size]
    view.copy_(_dev(L.view(np.int16), cuda))
    assert view.data_ptr() % 4 == 2
    out = torch.full(((L.size + 63) // 64 + 3,), -1, dtype=torch.int64, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    got = cuzfp_amd.variable_index(view, case[0], torch.float32, out=out, stream=s)
    s.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want_index(L))
    assert (out[got.numel():] == -1).all()


@pytest.mark.parametrize("case", CASES, ids=tv.case_id)
def test_boxes(cuda, varemu, golden, case):  # noqa: F811
    """Every box from the reference's stream and from our own encoder's, with
    the index from numpy and from variable_index."""
    import cuzfp_amd
    words, L, _, want = ref_of(varemu, golden, case)
    td = _tdtype(case[1])
    w, l, idx = _stream(words, L, cuda)
    w2, l2, _ = cuzfp_amd.encode_variable(_dev(tv.array(case[0], case[1]), cuda), **_kw(case))
    idx2 = cuzfp_amd.variable_index(l2, case[0], td)
    for origin, extent in boxes(case[0]):
        got = cuzfp_amd.decode_region_variable(w, l, idx, case[0], td, origin, extent)
        assert tuple(got.shape) == tuple(extent)
        assert _same(got, want[_box(origin, extent)]), (origin, extent)
        got = cuzfp_amd.decode_region_variable(w2, l2, idx2, case[0], td, origin, extent)
        assert _same(got, want[_box(origin, extent)]), (origin, extent, "own stream")


@pytest.mark.parametrize("case", CASES, ids=tv.case_id)
def test_decode_variable_with_index(cuda, varemu, golden, case):  # noqa: F811
    import cuzfp_amd
    words, L, _, want = ref_of(varemu, golden, case)
    td = _tdtype(case[1])
    w, l, idx = _stream(words, L, cuda)
    plain = cuzfp_amd.decode_variable(w, l, case[0], td)
    got = cuzfp_amd.decode_variable(w, l, case[0], td, index=idx)
    assert tuple(got.shape) == tuple(case[0])
    assert _same(got, plain.cpu().numpy()) and _same(got, want)


@pytest.mark.parametrize("case", VARIANTS, ids=tv.case_id)
def test_strided_out_and_stream(cuda, varemu, golden, case):  # noqa: F811
    """Into a strided view of a canary-filled parent on a non-default stream:
    the box changes and nothing else."""
    import torch
    import cuzfp_amd
    words, L, _, want = ref_of(varemu, golden, case)
    td = _tdtype(case[1])
    w, l, idx = _stream(words, L, cuda)
    origin, extent = boxes(case[0])[2]
    big = torch.full(tuple(2 * e + 3 for e in extent), -7.0, dtype=td, device=cuda)
    sl = tuple(slice(2, 2 + 2 * e, 2) for e in extent)
    view = big[sl]
    assert tuple(view.shape) == tuple(extent) and (len(extent) == 1 or not view.is_contiguous())
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    cuzfp_amd.decode_region_variable(w, l, idx, case[0], td, origin, extent, out=view, stream=s)
    s.synchronize()
    got = big.cpu().numpy()
    assert np.array_equal(np.ascontiguousarray(got[sl]).view(np.uint8),
                          np.ascontiguousarray(want[_box(origin, extent)]).view(np.uint8))
    mask = np.ones(got.shape, bool)
    mask[sl] = False
    assert np.all(got[mask] == -7.0)
    with pytest.raises(ValueError):
        cuzfp_amd.decode_region_variable(w, l, idx, case[0], td, origin, extent,
                                         out=torch.zeros((1,) * len(extent), dtype=td, device=cuda).expand(
                                             *[e + 1 for e in extent]))


def test_graph_capture(cuda, varemu, golden):  # noqa: F811
    """One region decode captured into a graph and replayed twice gives the
    eager call's bytes (no allocation or synchronisation inside the call)."""
    import torch
    import cuzfp_amd
    case = ((13, 22, 38), np.dtype(np.float32), "a", 1e-3)
    words, L, _, want = ref_of(varemu, golden, case)
    w, l, idx = _stream(words, L, cuda)
    origin, extent = (1, 2, 3), (11, 9, 30)
    eager = cuzfp_amd.decode_region_variable(w, l, idx, case[0], torch.float32, origin, extent)
    out = torch.zeros(extent, dtype=torch.float32, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cuzfp_amd.decode_region_variable(w, l, idx, case[0], torch.float32, origin, extent, out=out)
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, eager.cpu().numpy())
    assert _same(eager, want[_box(origin, extent)])


def test_offsets_past_32_bits(cuda, varemu, golden):  # noqa: F811
    """2^26 zero words (2^32 bits) in front of a case's stream and 2^32 added to
    every index entry: the index is not trusted, so this is legal input, and a
    32-bit offset would read the zeros."""
    import torch
    import cuzfp_amd
    case = ((9, 20, 36), np.dtype(np.float32), "p", 16)
    words, L, _, want = ref_of(varemu, golden, case)
    lead = 1 << 26
    buf = torch.zeros(lead + words.size, dtype=torch.int64, device=cuda)  # just over 512 MiB
    buf[lead:] = _dev(words.view(np.int64), cuda)
    idx = _dev((want_index(L) + np.uint64(1 << 32)).view(np.int64), cuda)
    l = _dev(L.view(np.int16), cuda)
    origin, extent = boxes(case[0])[2]
    got = cuzfp_amd.decode_region_variable(buf, l, idx, case[0], torch.float32, origin, extent)
    whole = cuzfp_amd.decode_variable(buf, l, case[0], torch.float32, index=idx)
    torch.cuda.synchronize()
    assert _same(got, want[_box(origin, extent)])
    assert _same(whole, want)


def test_bad_index(cuda, varemu, golden):  # noqa: F811
    """test_variable_gpu.test_bad_index for the indexed entry: lengths of 65535
    and index entries that point past the stream (and near 2^64).  Success, the
    canaries after the stream and around the box intact, and the good index
    decodes correctly afterwards.  The decoder clamps every length to the
    type's longest block and loads every stream dword behind a bound test
    (tests/native/variable_index_map.cpp checks that rule on the host), so this
    cannot fault by construction."""
    import torch
    import cuzfp_amd
    case = ((9, 20, 36), np.dtype(np.float64), "p", 64)
    words, L, _, want = ref_of(varemu, golden, case)
    canary = int(np.uint64(CANARY).astype(np.int64))
    buf = torch.full((words.size + 64,), canary, dtype=torch.int64, device=cuda)
    buf[: words.size] = _dev(words.view(np.int64), cuda)
    bad_l = torch.full((L.size,), -1, dtype=torch.int16, device=cuda)  # 0xffff
    T = (L.size + 63) // 64
    bad = np.array([64 * words.size - 100, 64 * words.size + 7, 2 ** 64 - 5000, 2 ** 64 - 1][: T + 1], np.uint64)
    assert bad.size == T + 1
    origin, extent = (1, 3, 5), (7, 13, 22)
    big = torch.full(tuple(e + 2 for e in extent), -7.0, dtype=torch.float64, device=cuda)
    inner = tuple(slice(1, 1 + e) for e in extent)
    cuzfp_amd.decode_region_variable(buf[: words.size], bad_l, _dev(bad.view(np.int64), cuda), case[0],
                                     torch.float64, origin, extent, out=big[inner])
    torch.cuda.synchronize()
    assert (buf[words.size:] == canary).all()
    assert np.array_equal(buf[: words.size].cpu().numpy().view(np.uint64), words)
    outer = big.clone()
    outer[inner] = -7.0
    assert (outer == -7.0).all()
    _, l, idx = _stream(words, L, cuda)
    good = cuzfp_amd.decode_region_variable(buf[: words.size], l, idx, case[0], torch.float64, origin, extent,
                                            out=big[inner])
    assert _same(good, want[_box(origin, extent)])
    outer = big.clone()
    outer[inner] = -7.0
    assert (outer == -7.0).all()


def test_argument_errors(cuda):
    """The C-ABI's size checks with real buffers, and the Python shape checks
    that need a device tensor."""
    import torch
    import cuzfp_amd
    lib = cuzfp_amd.library()
    n = (16, 16, 20)  # 80 blocks: T = 2
    ib = lib.cuzfp_hip_variable_index_bytes(3, *n)
    wb = lib.cuzfp_hip_variable_workspace_bytes(3, *n)
    assert ib == 24
    lengths = torch.full((80,), 1, dtype=torch.int16, device=cuda)
    index = torch.full((4,), -1, dtype=torch.int64, device=cuda)
    ws = torch.zeros(wb // 8 + 1, dtype=torch.int64, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def build(index_bytes, ws_bytes, t=3):
        return lib.cuzfp_hip_variable_index(lengths.data_ptr(), t, n[0], n[1], n[2], index.data_ptr(), index_bytes,
                                            ws.data_ptr(), ws_bytes, st)

    assert build(ib, wb - 1) == 1 and build(ib - 1, wb) == 1 and build(ib, wb, t=1) == 2
    torch.cuda.synchronize()
    assert (index == -1).all()  # nothing was launched
    assert build(ib, wb) == 0
    torch.cuda.synchronize()
    assert index.tolist() == [0, 64, 80, -1]
    words = torch.zeros(2, dtype=torch.int64, device=cuda)
    out = torch.full((4, 4, 4), -7.0, dtype=torch.float32, device=cuda)

    def dec(index_bytes, t=3):
        return lib.cuzfp_hip_decode_region_variable(words.data_ptr(), 16, lengths.data_ptr(), index.data_ptr(),
                                                    index_bytes, t, n[0], n[1], n[2], 4, 4, 4, 4, 4, 4, 0, 0, 0,
                                                    out.data_ptr(), st)

    assert dec(ib - 1) == 1 and dec(ib, t=2) == 2
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert dec(ib) == 0  # 80 one-bit blocks: zeros
    torch.cuda.synchronize()
    assert (out == 0).all()
    shape = (20, 16, 16)
    with pytest.raises(ValueError, match="shape"):
        cuzfp_amd.decode_region_variable(words, lengths, index[:3], shape, torch.float32, (0, 0, 0), (4, 4, 4),
                                         out=torch.zeros((4, 4, 5), device=cuda))
    with pytest.raises(ValueError, match="entries"):
        cuzfp_amd.decode_region_variable(words, lengths[:79], index[:3], shape, torch.float32, (0, 0, 0), (4, 4, 4))
    with pytest.raises(ValueError, match="entries"):
        cuzfp_amd.variable_index(lengths[:79], shape, torch.float32)
    with pytest.raises(cuzfp_amd.CodecError) as e:
        cuzfp_amd.decode_region_variable(words, lengths, index[:2], shape, torch.float32, (0, 0, 0), (4, 4, 4))
    assert e.value.status == 1
    with pytest.raises(cuzfp_amd.CodecError) as e:
        cuzfp_amd.variable_index(lengths, shape, torch.int32)
    assert e.value.status == 2
