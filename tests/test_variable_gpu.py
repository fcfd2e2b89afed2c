"""Variable-rate modes on the GPU: encode_variable / decode_variable against
the fixture of tests/test_variable.py (CPU zfp 0.5.0's streams, lengths and
decoded arrays).

The fixture stores hashes; the stream and the decoded array themselves come
from the host emulation (tests/native/variable_emulate.cpp), accepted only
when their SHA-256 equal the fixture's -- so they are the reference's bytes,
on a machine that has no reference library.
"""
import ctypes

import numpy as np
import pytest

import test_variable as tv
from test_variable import golden, varemu  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A5A5A5A5A
CASES = tv.cases()
# one case a shape, type and mode for the variants (strided, stream, capacity, tail)
VARIANTS = [c for c in CASES if c[2:] in (("p", 16), ("a", 1e-3))]
_REF = {}


def ref_of(varemu, golden, case):  # noqa: F811
    """(words, lengths, nbits, decoded) of the reference for a case: the host
    emulation's, checked against the fixture's hashes; computed once, read only."""
    key = tv.case_id(case)
    if key not in _REF:
        g = golden.get(case)
        words, L, total = tv.emu_compress(varemu, tv.array(case[0], case[1]), *tv.mode_params(case))
        assert total == g["nbits"] and np.array_equal(L, g["lengths"])
        assert np.array_equal(tv.sha(words), g["stream_sha"])
        d = tv.emu_decompress(varemu, words, L, case[0], case[1])
        assert np.array_equal(tv.sha(d), g["decoded_sha"])
        for a in (words, L, d):
            a.setflags(write=False)
        _REF[key] = (words, L, total, d)
    return _REF[key]


def _kw(case):
    return {"precision": case[3]} if case[2] == "p" else {"tolerance": case[3]}


def _tdtype(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _lengths(t):
    return t.cpu().numpy().view(np.uint16)


def _check_encoded(got, ref):
    words, lengths, nbits = got
    assert nbits == ref[2]
    assert np.array_equal(_lengths(lengths), ref[1])
    assert np.array_equal(_words(words), ref[0])


@pytest.mark.parametrize("case", CASES, ids=tv.case_id)
def test_encode(cuda, varemu, golden, case):  # noqa: F811
    import cuzfp_amd
    ref = ref_of(varemu, golden, case)
    x = _dev(tv.array(case[0], case[1]), cuda)
    _check_encoded(cuzfp_amd.encode_variable(x, **_kw(case)), ref)


@pytest.mark.parametrize("case", VARIANTS, ids=tv.case_id)
def test_encode_strided_and_stream(cuda, varemu, golden, case):  # noqa: F811
    """A transposed view of a transposed copy (the same values through
    non-unit strides), and a non-default stream."""
    import torch
    import cuzfp_amd
    ref = ref_of(varemu, golden, case)
    a = tv.array(case[0], case[1])
    perm = tuple(reversed(range(a.ndim)))
    xt = _dev(np.ascontiguousarray(a.transpose(perm)), cuda).permute(perm)  # 1D: a sliced view instead
    if a.ndim == 1:
        wide = torch.zeros(2 * a.size, dtype=_tdtype(a.dtype), device=cuda)
        wide[::2] = _dev(a, cuda)
        xt = wide[::2]
    assert not xt.is_contiguous() and tuple(xt.shape) == a.shape
    _check_encoded(cuzfp_amd.encode_variable(xt, **_kw(case)), ref)
    s = torch.cuda.Stream(device=cuda)
    x = _dev(a, cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    got = cuzfp_amd.encode_variable(x, stream=s, **_kw(case))
    s.synchronize()
    _check_encoded(got, ref)


@pytest.mark.parametrize("case", VARIANTS, ids=tv.case_id)
def test_capacity_and_tail(cuda, varemu, golden, case):  # noqa: F811
    """`out` one word too short: nothing at or past the capacity changes, the
    lengths and the bit count are still right.  The default-size `out`: the
    words after the stream keep their canary."""
    import torch
    import cuzfp_amd
    ref = ref_of(varemu, golden, case)
    x = _dev(tv.array(case[0], case[1]), cuda)
    nwords = ref[0].size
    canary = np.uint64(CANARY).astype(np.int64)
    buf = torch.full((nwords + 8,), int(canary), dtype=torch.int64, device=cuda)
    words, lengths, nbits = cuzfp_amd.encode_variable(x, out=buf[: nwords - 1], **_kw(case))
    assert nbits == ref[2] and np.array_equal(_lengths(lengths), ref[1])
    assert words.numel() == nwords - 1
    assert (buf[nwords - 1:] == int(canary)).all()
    maxprec = tv.mode_params(case)[0]
    full = cuzfp_amd.variable_maximum_size(case[0], case[1], maxprec) // 8
    assert full >= nwords
    buf = torch.full((full,), int(canary), dtype=torch.int64, device=cuda)
    got = cuzfp_amd.encode_variable(x, out=buf, **_kw(case))
    _check_encoded(got, ref)
    assert (buf[nwords:] == int(canary)).all()


@pytest.mark.parametrize("case", CASES, ids=tv.case_id)
def test_decode(cuda, varemu, golden, case):  # noqa: F811
    """The fixture's stream and lengths decode to the fixture's array, bit for
    bit; so does our own encoder's output."""
    import cuzfp_amd
    words, L, _, want = ref_of(varemu, golden, case)
    td = _tdtype(case[1])
    got = cuzfp_amd.decode_variable(_dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda), case[0], td)
    assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))
    x = _dev(tv.array(case[0], case[1]), cuda)
    w2, l2, _ = cuzfp_amd.encode_variable(x, **_kw(case))
    got = cuzfp_amd.decode_variable(w2, l2, case[0], td)
    assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("case", VARIANTS, ids=tv.case_id)
def test_decode_strided_out(cuda, varemu, golden, case):  # noqa: F811
    import torch
    import cuzfp_amd
    words, L, _, want = ref_of(varemu, golden, case)
    td = _tdtype(case[1])
    big = torch.full(tuple(2 * s + 1 for s in case[0]), -7.0, dtype=td, device=cuda)
    view = big[tuple(slice(1, 2 * s + 1, 2) for s in case[0])]
    assert tuple(view.shape) == tuple(case[0]) and not view.is_contiguous()
    s = torch.cuda.Stream(device=cuda)
    w, l = _dev(words.view(np.int64), cuda), _dev(L.view(np.int16), cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    cuzfp_amd.decode_variable(w, l, case[0], td, out=view, stream=s)
    s.synchronize()
    assert np.array_equal(view.cpu().numpy().view(np.uint8), want.view(np.uint8))
    untouched = big.clone()
    untouched[tuple(slice(1, 2 * s_ + 1, 2) for s_ in case[0])] = -7.0
    assert (untouched == -7.0).all()


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "a" and c[3] > 0], ids=tv.case_id)
def test_error_bound(cuda, varemu, golden, case):  # noqa: F811
    """Fixed accuracy keeps every value within the tolerance: first the
    reference's own decode, then ours."""
    import cuzfp_amd
    a = tv.array(case[0], case[1])
    words, L, _, want = ref_of(varemu, golden, case)
    err_ref = np.abs(want.astype(np.float64) - a.astype(np.float64)).max()
    assert err_ref <= case[3], err_ref
    w, l, _ = cuzfp_amd.encode_variable(_dev(a, cuda), tolerance=case[3])
    got = cuzfp_amd.decode_variable(w, l, case[0], _tdtype(case[1])).cpu().numpy()
    err = np.abs(got.astype(np.float64) - a.astype(np.float64)).max()
    assert err <= case[3], err


def test_bad_index(cuda, varemu, golden):  # noqa: F811
    """An index of 65535s: success, the buffer after the stream untouched, and
    a valid case decodes correctly afterwards.  The decoder clamps every
    length to the type's longest block (its LDS columns are sized for that)
    and loads every stream dword behind a bound check, so this cannot fault
    by construction."""
    import torch
    import cuzfp_amd
    case = ((9, 20, 36), np.dtype(np.float64), "p", 64)
    words, L, _, want = ref_of(varemu, golden, case)
    canary = int(np.uint64(CANARY).astype(np.int64))
    buf = torch.full((words.size + 64,), canary, dtype=torch.int64, device=cuda)
    buf[: words.size] = _dev(words.view(np.int64), cuda)
    bad = torch.full((L.size,), -1, dtype=torch.int16, device=cuda)  # 0xffff
    out = cuzfp_amd.decode_variable(buf[: words.size], bad, case[0], torch.float64)
    torch.cuda.synchronize()
    assert tuple(out.shape) == case[0]
    assert (buf[words.size:] == canary).all()
    assert np.array_equal(_words(buf[: words.size]), words)
    good = cuzfp_amd.decode_variable(buf[: words.size], _dev(L.view(np.int16), cuda), case[0], torch.float64)
    assert np.array_equal(good.cpu().numpy().view(np.uint8), want.view(np.uint8))


def test_argument_errors(cuda):
    import torch
    import cuzfp_amd
    x = torch.zeros((8, 8), dtype=torch.float32, device=cuda)
    with pytest.raises(ValueError):
        cuzfp_amd.encode_variable(x)
    with pytest.raises(ValueError):
        cuzfp_amd.encode_variable(x, precision=8, tolerance=1e-3)
    with pytest.raises(cuzfp_amd.CodecError) as e:
        cuzfp_amd.encode_variable(x.to(torch.int32), precision=8)
    assert e.value.status == 2
    for p in (0, 33):
        with pytest.raises(cuzfp_amd.CodecError) as e:
            cuzfp_amd.encode_variable(x, precision=p)
        assert e.value.status == 1
    with pytest.raises(cuzfp_amd.CodecError):
        cuzfp_amd.encode_variable(x.double(), precision=65)
    # the C-ABI itself: maxprec, integer types, a workspace one byte short
    lib = cuzfp_amd.library()
    need = lib.cuzfp_hip_variable_workspace_bytes(3, 8, 8, 0)
    assert need >= 8 * 4
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=cuda)
    out = torch.zeros(cuzfp_amd.variable_maximum_size((8, 8), np.float32, 32) // 8, dtype=torch.int64, device=cuda)
    lengths = torch.zeros(4, dtype=torch.int16, device=cuda)
    total = torch.zeros(1, dtype=torch.int64, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def enc(t, maxprec, ws_bytes):
        return lib.cuzfp_hip_encode_variable(x.data_ptr(), t, 8, 8, 0, 0, 0, 0, maxprec, -1074, out.data_ptr(),
                                             out.numel() * 8, lengths.data_ptr(), total.data_ptr(), ws.data_ptr(),
                                             ws_bytes, st)

    assert enc(3, 16, need) == 0
    assert enc(3, 0, need) == 1 and enc(3, 33, need) == 1
    assert enc(1, 16, need) == 2 and enc(2, 16, need) == 2
    assert enc(3, 16, need - 1) == 1
    dec = lib.cuzfp_hip_decode_variable(out.data_ptr(), out.numel() * 8, lengths.data_ptr(), 3, 8, 8, 0, 0, 0, 0,
                                        x.data_ptr(), ws.data_ptr(), need - 1, st)
    assert dec == 1
    assert lib.cuzfp_hip_variable_maximum_size(1, 8, 8, 0, 16) == 0
    torch.cuda.synchronize()
    assert cuzfp_amd.accuracy_to_minexp(1e-3) == -10 and cuzfp_amd.accuracy_to_minexp(0.0) == -1074
    assert cuzfp_amd.accuracy_to_minexp(1.0) == 0 and cuzfp_amd.accuracy_to_minexp(64.0) == 6
