"""Every maxbits, whole-array encode and decode, on the block zoo
(tests/block_zoo.py), against exact bytes of the CPU oracle.

What this file is for.  zfp_block.hpp takes about thirty decisions a whole
wave at a time (`any_lane(...)`): the wave-uniform exits of decode_half_fixed
and encode_half_fixed, each with its own compile-time zero_fixed<H, C> in 3D;
the 2D 32-bit high-tile-only transposes (encoder load_hi plus the deferred
load, decoder store_hi / permute_inv_copy when `unset >= 15`); the 3D 64-bit
load_split parts; the 1D/2D whole-wave choice in quantize_f32; the zero-wave
returns of encode_block and decode_block; the `maxprec != prec` cut of a
double block's lowest planes (cut_planes); the decoder's any_lane(slow) /
any_lane(open) fallbacks.  None of them exists
in the host emulation, which runs one lane a "wave".  Which side a wave takes
depends on its deepest lane and on maxbits, so the zoo mixes lanes of every
kind in a wave and this file walks maxbits.

Why EVERY maxbits, floor .. top + 1, and not a sample -- read this before
thinning the sweep:

  * at the floor (9 f32, 12 f64, 1 integers) every wave stops before its
    first plane;
  * at top = ebits + 1 + 4^d * prec + 4^d - 1 every lane has coded plane 0
    (test_block_zoo.py::test_zoo_top_is_the_last_bit: the oracle's stream at
    top + 64 is the stream at top plus zero bits);
  * one more bit of budget moves a lane forward by at most one plane.

So a step-1 sweep walks each wave's exit point through every pair of planes
in turn: it cannot step over the 17/16/15 boundary of the 2D split paths, any
zero_fixed<H, C>, or either load_split part.  A sampled sweep can: where top
planes cost one bit each (zero and small blocks), 13 bits are 13 planes.

The ragged shapes (a partial last wave, partial blocks on every far edge, so
the general gather / scatter and not the row paths) run every 5th maxbits:
the plane paths are the same code there.

The CPU oracle is what costs time here, so the sweep of a (dims, type) pair is
cut into consecutive maxbits ranges of about equal oracle work, one test id
each.
"""
import zlib

import numpy as np
import pytest

import block_zoo as bz
import cuzfp_amd as cz

gpu = pytest.mark.gpu

DENSITIES = (0.5, 0.05, 0.95)  # of the random-bit stream, by maxbits % 3


# Test ids a 3D pair's sweep is cut into, from the oracle's measured time for
# the whole sweep (8, 11, 31 and 47 s), so that no id spends more than about
# 3 s in it; 1D and 2D sweeps take under 3 s whole.
PARTS = {"float32": 3, "int32": 4, "float64": 10, "int64": 16}
RAGGED_PARTS = {"float32": 1, "int32": 1, "float64": 2, "int64": 3}


def _ranges(dims, dtype, parts=PARTS):
    """Consecutive ranges covering floor .. top + 1 once.  The oracle's work
    per maxbits grows with maxbits (measured: the sum to m goes as m^1.7), so
    the cuts are at equal sums."""
    lo, hi = bz.floor(dtype), bz.top(dims, dtype) + 1
    n = parts[np.dtype(dtype).name] if dims == 3 else 1
    cuts = [lo + int(round((hi + 1 - lo) * (k / n) ** (1 / 1.7))) for k in range(n + 1)]
    cuts[0], cuts[-1] = lo, hi + 1
    return [range(cuts[k], cuts[k + 1]) for k in range(n)]


def _sweep_cases():
    for dims in (1, 2, 3):
        for dtype in bz.DTYPES:
            for r in _ranges(dims, dtype):
                yield pytest.param(dims, dtype, r, id=f"{dims}d-{np.dtype(dtype).name}-{r.start}..{r.stop - 1}")


def test_sweep_covers_every_maxbits():
    """(CPU) Step 1 from the type's floor to top + 1 for all 12 pairs, each maxbits
    in exactly one id."""
    tops = {(1, "float32"): 140, (1, "float64"): 271, (1, "int32"): 131, (1, "int64"): 259,
            (2, "float32"): 536, (2, "float64"): 1051, (2, "int32"): 527, (2, "int64"): 1039,
            (3, "float32"): 2120, (3, "float64"): 4171, (3, "int32"): 2111, (3, "int64"): 4159}
    for (dims, name), t in tops.items():
        assert bz.top(dims, name) == t
        swept = [mb for r in _ranges(dims, name) for mb in r]
        assert swept == list(range(bz.floor(name), t + 2)), (dims, name)
    ragged = {}
    for case in _ragged_cases():
        dims, dtype, mbs = case.values
        ragged.setdefault((dims, np.dtype(dtype).name), []).extend(mbs)
    for (dims, name), got in ragged.items():
        t = tops[dims, name]
        assert got == sorted(set(range(bz.floor(name), t + 2, 5)) | {t + 1}), (dims, name)


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[np.dtype(dtype)]


def _same_bytes(got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _check(cuda, restatement, a, x, mb, rng, where):
    """At one maxbits: encode == oracle, decode of it == oracle, decode of one
    random-bit stream == oracle."""
    import torch
    td = _torch_dtype(a.dtype)
    ref = restatement.compress(a, mb)
    want = restatement.decompress(ref, a.shape, a.dtype, mb)
    rnd = bz.random_stream(rng, bz.nblocks(a.shape), mb, DENSITIES[mb % 3])
    rwant = restatement.decompress(rnd, a.shape, a.dtype, mb)
    words = cz.encode(x, mb)
    y = cz.decode(words, a.shape, td, mb)
    z = cz.decode(torch.from_numpy(rnd.view(np.int64)).to(cuda), a.shape, td, mb)
    assert _same_bytes(words.cpu().numpy().view(np.uint64), ref), where + (mb, "encode")
    assert _same_bytes(y.cpu().numpy(), want), where + (mb, "decode")
    assert _same_bytes(z.cpu().numpy(), rwant), where + (mb, "decode of random bits")


@gpu
@pytest.mark.parametrize("dims,dtype,mbs", list(_sweep_cases()))
def test_every_maxbits(cuda, restatement, dims, dtype, mbs):
    import torch
    a, _ = bz.zoo(dims, dtype)
    x = torch.from_numpy(np.array(a)).to(cuda)
    rng = np.random.default_rng(zlib.crc32(f"sweep/{dims}/{np.dtype(dtype).str}/{mbs.start}".encode()))
    for mb in mbs:
        _check(cuda, restatement, a, x, mb, rng, (dims, np.dtype(dtype).name))


def _ragged_cases():
    for dims in (1, 2, 3):
        for dtype in bz.DTYPES:
            hi = bz.top(dims, dtype) + 1
            for r in _ranges(dims, dtype, RAGGED_PARTS):
                first = r.start + (bz.floor(dtype) - r.start) % 5  # floor, floor + 5, ... across the cuts
                mbs = sorted(set(range(first, r.stop, 5)) | ({hi} if r.stop == hi + 1 else set()))
                yield pytest.param(dims, dtype, mbs, id=f"{dims}d-{np.dtype(dtype).name}-{mbs[0]}..{mbs[-1]}")


@gpu
@pytest.mark.parametrize("dims,dtype,mbs", list(_ragged_cases()))
def test_ragged_every_fifth_maxbits(cuda, restatement, dims, dtype, mbs):
    """A partial last wave and partial blocks on every far edge: the general
    gather and scatter (fast_ok false), floor .. top + 1 in steps of 5, and
    top + 1 itself."""
    import torch
    a, _ = bz.zoo(dims, dtype, shape=bz.RAGGED[dims])
    x = torch.from_numpy(np.array(a)).to(cuda)
    rng = np.random.default_rng(zlib.crc32(f"ragged/{dims}/{np.dtype(dtype).str}/{mbs[0]}".encode()))
    for mb in mbs:
        _check(cuda, restatement, a, x, mb, rng, (dims, np.dtype(dtype).name, "ragged"))


# ---------------------------------------------------------------------------
# Two anchors of the 2D 32-bit split (planes 31..16 | 15..0), int32.  An
# all-zero integer block costs one bit a plane: 16 bits end exactly after
# plane 16 (`unset` = 15, the high tile alone), 17 bits enter the low tile.

_ANCHORS = {}


def _anchor(which):
    if which not in _ANCHORS:
        if which == "zero wave beside a dense wave":
            names = ["zero"] * 64 + ["full"] * 64
        else:  # the same blocks inside one wave: the zoo's wave 3
            names = bz.block_classes(np.int32)[192:]
            assert names.count("zero") == 1 and names.count("const") == 1 and names.count("full") == 62
        a = bz.build(names, (len(names) // 64, 64), np.int32, "anchor/" + which)
        a.setflags(write=False)
        _ANCHORS[which] = a
    return _ANCHORS[which]


@gpu
@pytest.mark.parametrize("mb", [15, 16, 17, 18])
@pytest.mark.parametrize("which", ["zero wave beside a dense wave", "zero block inside a dense wave"])
def test_2d_int32_split_anchor(cuda, restatement, which, mb):
    import torch
    a = _anchor(which)
    ref = restatement.compress(a, mb)
    # the premise: a zero block's code is mb zero bits, one a plane
    bits = np.unpackbits(ref.view(np.uint8), bitorder="little")
    zero = 0 if a.shape[0] == 8 else bz.ZERO_LANE
    assert not bz.block_of(a, zero).any() and not bits[zero * mb:(zero + 1) * mb].any()
    assert bits[64 * mb if a.shape[0] == 8 else 0:].any()
    rng = np.random.default_rng(zlib.crc32(f"anchor/{which}/{mb}".encode()))
    _check(cuda, restatement, a, torch.from_numpy(np.array(a)).to(cuda), mb, rng, (2, "int32", which))
