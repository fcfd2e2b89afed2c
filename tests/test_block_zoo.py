"""The block zoo itself (tests/block_zoo.py), CPU only: it holds what it
claims, wave by wave, and on it the oracle agrees with the host emulation of
the lane algorithm -- so the GPU tests built on it (test_wave_paths.py and the
zoo cases of the region files) compare the kernels with a recipe that two
independent CPU coders read alike, NaN, inf and denormal blocks included.
"""
import numpy as np
import pytest

import block_zoo as bz
from test_emulation import emu, emu_compress, emu_decompress  # noqa: F401 (emu is a fixture)

CASES = [pytest.param(d, t, id=f"{d}d-{np.dtype(t).name}") for d in (1, 2, 3) for t in bz.DTYPES]


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _is_class(blk, cls):
    """Whether a block is what its class name says (noise: dense enough)."""
    n = blk.size
    if blk.dtype.kind == "f":
        nan, inf = np.isnan(blk), np.isinf(blk)
        mag = np.abs(blk[~nan & ~inf]) if (~nan & ~inf).any() else np.zeros(1)
        tiny = {4: (1e-38, 1e-44, 1e-41), 8: (1e-300, 1e-320, 2.0 ** -1021)}[blk.dtype.itemsize]
        huge = {4: 1e37, 8: 1e306}[blk.dtype.itemsize]
        return {
            "zero": lambda: not blk.any() and not np.signbit(blk).any(),
            "negzero": lambda: not blk.any() and np.signbit(blk).all(),
            "const": lambda: (blk == blk.flat[0]).all() and blk.flat[0] != 0,
            "smooth": lambda: np.ptp(blk) > 0 and np.abs(np.diff(blk, axis=-1)).max() < 0.25 * np.abs(blk).max(),
            "noise": lambda: not nan.any() and not inf.any() and (blk != 0).all() and mag.max() < 8,
            "tiny_a": lambda: not nan.any() and 0 < mag.max() < 8 * tiny[0],
            "tiny_b": lambda: not nan.any() and 0 < mag.max() < 8 * tiny[1],
            "tiny_c": lambda: not nan.any() and 0 < mag.max() < 64 * tiny[2],
            "huge": lambda: not nan.any() and not inf.any() and mag.max() > 0.1 * huge,
            "single": lambda: np.count_nonzero(blk) == 1 and not nan.any(),
            "nan_block": lambda: nan.all(),
            "nan_zeros": lambda: nan.sum() == 1 and not blk[~nan].any(),
            "noise_inf": lambda: (blk == np.inf).sum() == 1 and not nan.any() and (blk != 0).all() and mag.max() < 8,
            "noise_nan_ninf": lambda: nan.sum() == 1 and (blk == -np.inf).sum() == 1 and inf.sum() == 1,
        }[cls]()
    full = 30 if blk.dtype.itemsize == 4 else 60
    v = blk.astype(np.int64)
    assert np.abs(v).max() < 2 ** full
    if cls == "zero":
        return not v.any()
    if cls == "const":
        return (v == 7).all()
    if cls == "smooth":
        return np.ptp(v) > 0 and np.abs(np.diff(v, axis=-1)).max() <= 3
    if cls.startswith("noise"):
        s = int(cls[5:])
        return np.abs(v).max() <= 2 ** s and (n < 16 or np.abs(v).max() >= 2 ** (s - 2))
    if cls.startswith("single"):
        return np.count_nonzero(v) == 1 and v.min() == -2 ** int(cls[6:])
    if cls == "full":
        return np.abs(v).max() >= 2 ** (full - 3)
    raise ValueError(cls)


@pytest.mark.parametrize("dims,dtype", CASES)
def test_zoo_holds_its_classes(dims, dtype):
    a, names = bz.zoo(dims, dtype)
    assert a.shape == bz.SHAPES[dims] and a.dtype == np.dtype(dtype) and len(names) == 256
    # 64 blocks along x: block b = wave * 64 + lane is x-block `lane` of block row `wave`
    for b in (0, 63, 64, 200, 255):
        x, y = slice(4 * (b % 64), 4 * (b % 64) + 4), slice(4 * (b // 64), 4 * (b // 64) + 4)
        want = a[4 * b:4 * b + 4] if dims == 1 else a[y, x] if dims == 2 else a[:, y, x]
        assert _same_bytes(bz.block_of(a, b), want), b
    for b, cls in enumerate(names):
        assert _is_class(bz.block_of(a, b), cls), (b, cls)
    noise = "noise" if np.dtype(dtype).kind == "f" else f"noise{bz.WAVE_NOISE_GRADE}"
    dense = "noise" if np.dtype(dtype).kind == "f" else "full"
    assert set(names[:64]) == {"zero"}
    assert set(names[64:128]) == {noise}
    assert set(names[128:192]) == set(bz.classes(dtype)) and len(bz.classes(dtype)) <= 64
    w3 = list(names[192:])
    assert w3[bz.ZERO_LANE] == "zero" and w3[bz.CONST_LANE] == "const"
    assert all(c == dense for i, c in enumerate(w3) if i not in (bz.ZERO_LANE, bz.CONST_LANE))
    # the rotations move the recipes r waves up
    for r in (1, 2):
        b, rn = bz.zoo(dims, dtype, rotate=r)
        assert all(_is_class(bz.block_of(b, i), c) for i, c in enumerate(rn))
        assert set(rn[64 * ((4 - r) % 4):64 * ((4 - r) % 4) + 64]) == {"zero"}
        assert set(rn[64 * (2 - r):64 * (2 - r) + 64]) == set(bz.classes(dtype))
    # the ragged shape: the same recipe by block index, cropped
    c, cn = bz.zoo(dims, dtype, shape=bz.RAGGED[dims])
    assert c.shape == bz.RAGGED[dims] and len(cn) == bz.nblocks(bz.RAGGED[dims])
    assert cn == names[:len(cn)] and len(cn) % 64 != 0 and len(cn) > 192
    assert all(n % 4 == 3 for n in c.shape)
    # made once, read only
    assert bz.zoo(dims, dtype)[0] is a and not a.flags.writeable


@pytest.mark.parametrize("dims,dtype", CASES)
def test_zoo_oracle_equals_emulation(emu, restatement, dims, dtype):
    """Stream and decode of the zoo, oracle against emulation, over a stride-7
    sweep of maxbits from the type's floor to top + 1 (and at both ends)."""
    a, _ = bz.zoo(dims, dtype)
    lo, hi = bz.floor(dtype), bz.top(dims, dtype) + 1
    for mb in sorted(set(range(lo, hi + 1, 7)) | {hi - 1, hi}):
        s = restatement.compress(a, mb)
        assert np.array_equal(emu_compress(emu, a, mb), s), mb
        assert _same_bytes(emu_decompress(emu, s, a.shape, dtype, mb), restatement.decompress(s, a.shape, dtype, mb)), mb
    b, _ = bz.zoo(dims, dtype, shape=bz.RAGGED[dims])
    for mb in (lo, 64, 100, hi):
        s = restatement.compress(b, mb)
        assert np.array_equal(emu_compress(emu, b, mb), s), mb
        assert _same_bytes(emu_decompress(emu, s, b.shape, dtype, mb), restatement.decompress(s, b.shape, dtype, mb)), mb


@pytest.mark.parametrize("dims,dtype", CASES)
def test_zoo_top_is_the_last_bit(restatement, dims, dtype):
    """At top every lane has coded plane 0: the stream at top + 64 is the
    stream at top plus zero bits (the every-maxbits sweep may end at top + 1)."""
    a, _ = bz.zoo(dims, dtype)
    t = bz.top(dims, dtype)
    nb = bz.nblocks(a.shape)
    lo = np.unpackbits(restatement.compress(a, t).view(np.uint8), bitorder="little")[:nb * t].reshape(nb, t)
    hi = np.unpackbits(restatement.compress(a, t + 64).view(np.uint8), bitorder="little")[:nb * (t + 64)]
    hi = hi.reshape(nb, t + 64)
    assert np.array_equal(hi[:, :t], lo) and not hi[:, t:].any()
