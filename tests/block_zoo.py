"""A zoo of 4^d blocks, assembled block by block so that a test decides which
blocks share a wave (a plain module: the tests import it, pytest does not).

A wave is 64 consecutive blocks in raster order, x fastest (b = wave * 64 +
lane in csrc/kernels.hpp; region blocks follow the same order).  The aligned
shapes have 64 blocks along x, so every x-row of blocks is one wave: 256
blocks, 4 waves.

    wave 0   zero blocks only
    wave 1   64 noise blocks of one magnitude
    wave 2   every class in turn
    wave 3   dense noise, with one zero block (lane ZERO_LANE) and one constant
             block (lane CONST_LANE): the lanes that go deeper than the rest

The ragged shapes hold the same recipe by block index, cropped: a partial
last wave and partial blocks on every far edge.

`rotate` = r moves the recipes r waves up and the classes r lanes along
(block (w, l) gets what block (w + r, l + r) had): pasted over the plain zoo,
r = 1 puts noise over the zero wave and every class, zeros and NaN among them,
over the noise wave; r = 2 puts every class over the zero wave and zeros over
the every-class wave.

Integer magnitudes stay below 2^30 (int32) and 2^60 (int64), which keeps the
oracle's transform away from overflow.
"""
import zlib

import numpy as np

DTYPES = (np.float32, np.float64, np.int32, np.int64)
SHAPES = {1: (1024,), 2: (16, 256), 3: (4, 16, 256)}
# 1D: 3 waves + 21 blocks, the last one partial; 2D: 7 x 31 = 217 blocks; 3D:
# 3 x 5 x 15 = 225 blocks; partial blocks on every far edge
RAGGED = {1: (4 * (3 * 64 + 20) + 3,), 2: (4 * 6 + 3, 4 * 30 + 3), 3: (4 * 2 + 3, 4 * 4 + 3, 4 * 14 + 3)}
ZERO_LANE, CONST_LANE = 17, 40

FLOAT_CLASSES = ("zero", "negzero", "const", "smooth", "noise", "tiny_a", "tiny_b", "tiny_c", "huge", "single",
                 "nan_block", "nan_zeros", "noise_inf", "noise_nan_ninf")
# graded magnitudes 2^s of the integer noise and single-element blocks
INT_GRADES = {4: (2, 8, 13, 15, 16, 17, 24, 29), 8: (2, 15, 31, 32, 33, 47, 59)}
# the exact quantisation path; for doubles the last two have maxprec < prec (the planes below 64 - maxprec are
# not coded), tiny_b with one exponent (-1022, denormals) and tiny_c with exponents that vary from block to
# block, so that the lanes of a wave stop at different planes, odd and even
_TINY = {4: (1e-38, 1e-44, 1e-41), 8: (1e-300, 1e-320, 2.0 ** -1021)}
_HUGE = {4: 1e37, 8: 1e306}
WAVE_NOISE_GRADE = 13  # wave 1 of an integer zoo: top planes around 15


def int_classes(dtype):
    size = np.dtype(dtype).itemsize
    return (("zero", "const", "smooth") + tuple(f"noise{s}" for s in INT_GRADES[size]) +
            tuple(f"single{s}" for s in INT_GRADES[size]) + ("full",))


def classes(dtype):
    return FLOAT_CLASSES if np.dtype(dtype).kind == "f" else int_classes(dtype)


def floor(dtype):
    """The least maxbits of a type: 1 + the exponent bits of a float."""
    return {np.dtype(np.float32): 9, np.dtype(np.float64): 12}.get(np.dtype(dtype), 1)


def top(dims, dtype):
    """ebits + 1 + 4^d * prec + 4^d - 1: with this budget every lane has coded
    plane 0 whatever its block."""
    size = np.dtype(dtype).itemsize
    ebits = {4: 8, 8: 11}[size] + 1 if np.dtype(dtype).kind == "f" else 0
    return ebits + 4 ** dims * 8 * size + 4 ** dims - 1


def _block(rng, cls, dims, dtype):
    """One block of a class, as a (4,) * dims array of dtype."""
    dtype = np.dtype(dtype)
    shape = (4,) * dims
    n = 4 ** dims
    ramp = np.indices(shape).sum(axis=0)
    if dtype.kind == "f":
        noise = rng.standard_normal(shape)
        if cls == "zero":
            v = np.zeros(shape)
        elif cls == "negzero":
            v = np.full(shape, -0.0)
        elif cls == "const":
            v = np.full(shape, 1.5)
        elif cls == "smooth":
            v = 1.0 + ramp / 8.0 - (ramp / 16.0) ** 2
        elif cls == "noise":
            v = noise
        elif cls == "tiny_a":
            v = noise * _TINY[dtype.itemsize][0]
        elif cls == "tiny_b":
            v = noise * _TINY[dtype.itemsize][1]
        elif cls == "tiny_c":
            v = noise * _TINY[dtype.itemsize][2] * 2.0 ** int(rng.integers(0, 4))
        elif cls == "huge":
            v = noise * _HUGE[dtype.itemsize]
        elif cls == "single":
            v = np.zeros(shape)
            v.flat[rng.integers(n)] = noise.flat[0] + 3.0
        elif cls == "nan_block":
            v = np.full(shape, np.nan)
        elif cls == "nan_zeros":
            v = np.zeros(shape)
            v.flat[rng.integers(n)] = np.nan
        elif cls == "noise_inf":
            v = noise
            v.flat[rng.integers(n)] = np.inf
        elif cls == "noise_nan_ninf":
            v = noise
            i, j = rng.choice(n, 2, replace=False)
            v.flat[i] = np.nan
            v.flat[j] = -np.inf
        else:
            raise ValueError(cls)
        return v.astype(dtype)
    full = 30 if dtype.itemsize == 4 else 60
    if cls == "zero":
        v = np.zeros(shape, np.int64)
    elif cls == "const":
        v = np.full(shape, 7, np.int64)
    elif cls == "smooth":
        v = 100 + 3 * ramp.astype(np.int64)
    elif cls.startswith("noise"):
        s = int(cls[5:])
        v = rng.integers(-2 ** s, 2 ** s, size=shape)
    elif cls.startswith("single"):
        v = np.zeros(shape, np.int64)
        v.flat[rng.integers(n)] = -2 ** int(cls[6:])
    elif cls == "full":
        v = rng.integers(-2 ** full + 1, 2 ** full, size=shape)
    else:
        raise ValueError(cls)
    assert np.abs(v).max() < 2 ** full
    return v.astype(dtype)


def block_classes(dtype, nblocks=256, rotate=0):
    """The class name of every block, by block index."""
    cl = classes(dtype)
    is_float = np.dtype(dtype).kind == "f"
    out = []
    for b in range(nblocks):
        wave, lane = (b // 64 + rotate) % 4, (b % 64 + rotate) % 64
        if wave == 0:
            out.append("zero")
        elif wave == 1:
            out.append("noise" if is_float else f"noise{WAVE_NOISE_GRADE}")
        elif wave == 2:
            out.append(cl[lane % len(cl)])
        else:
            out.append("zero" if lane == ZERO_LANE else "const" if lane == CONST_LANE else
                       "noise" if is_float else "full")
    return out


def assemble(blocks, nb):
    """blocks[b] (each (4,) * dims), b in raster order over nb = blocks per
    axis (numpy order, slowest first) -> the array of 4 * nb elements an axis."""
    dims = len(nb)
    a = np.stack(blocks).reshape(tuple(nb) + (4,) * dims)
    order = [k for i in range(dims) for k in (i, dims + i)]
    return np.ascontiguousarray(a.transpose(order).reshape(tuple(4 * n for n in nb)))


def block_of(a, b):
    """Block b (raster order) of an array whose extents are multiples of 4."""
    idx = np.unravel_index(b, tuple(n // 4 for n in a.shape))
    return a[tuple(slice(4 * i, 4 * i + 4) for i in idx)]


def build(names, nb, dtype, seed):
    """The array of the blocks named by `names` (raster order over nb = blocks
    per axis, numpy order), drawn from a generator seeded with crc32(seed)."""
    rng = np.random.default_rng(zlib.crc32(seed.encode()))
    assert len(names) == int(np.prod(nb))
    with np.errstate(over="ignore", invalid="ignore"):
        return assemble([_block(rng, c, len(nb), dtype) for c in names], nb)


_ZOO = {}


def zoo(dims, dtype, shape=None, rotate=0):
    """(array, class of every block): made once per argument set, read only.
    `shape` is SHAPES[dims] unless given; its blocks take the recipe by block
    index and the array is cropped to it."""
    shape = tuple(shape or SHAPES[dims])
    key = (dims, np.dtype(dtype).str, shape, rotate)
    if key not in _ZOO:
        nb = tuple((n + 3) // 4 for n in shape)
        names = block_classes(dtype, int(np.prod(nb)), rotate)
        a = build(names, nb, dtype, repr(("zoo",) + key))
        a = np.ascontiguousarray(a[tuple(slice(0, n) for n in shape)])
        a.setflags(write=False)
        _ZOO[key] = (a, tuple(names))
    return _ZOO[key]


def random_stream(rng, nblocks, maxbits, density):
    """A stream of nblocks * maxbits arbitrary bits (whole 64-bit words), each
    set with probability `density`: not encoder output."""
    words = (nblocks * maxbits + 63) // 64
    bits = rng.random(words * 64) < density
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def nblocks(shape):
    return int(np.prod([(n + 3) // 4 for n in shape]))
