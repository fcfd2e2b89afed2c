"""Random access into a variable-rate stream, the part that needs no GPU: the
size of the offset index, the argument checks of cuzfp_hip_variable_index and
cuzfp_hip_decode_region_variable (every error is a status before any launch),
the Python validation, and the host program over csrc/variable_index.hpp --
the offset rule and the copy-in bounds the kernel itself calls.  The kernels
are checked in tests/test_variable_region_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cuzfp_amd as cz
import test_variable as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    from cuzfp_amd.build import build
    return build()


def _ext(shape):
    return tuple(shape[::-1]) + (0,) * (3 - len(shape))


def test_variable_index_bytes(libs):
    lib = cz.library()
    for shape in tv.SHAPES:
        T = (tv.nblocks(shape) + 63) // 64
        for t in (cz.TYPE_FLOAT, cz.TYPE_DOUBLE):
            assert lib.cuzfp_hip_variable_index_bytes(t, *_ext(shape)) == 8 * (T + 1), shape
    assert [(tv.nblocks(s) + 63) // 64 for s in tv.SHAPES] == [4, 3, 3, 1, 4]
    assert lib.cuzfp_hip_variable_index_bytes(3, 256, 0, 0) == 8 * 2  # a whole tile: T = 1
    assert lib.cuzfp_hip_variable_index_bytes(3, 257, 0, 0) == 8 * 3
    # invalid dimensions, integer and unknown types
    assert lib.cuzfp_hip_variable_index_bytes(3, 0, 0, 0) == 0
    assert lib.cuzfp_hip_variable_index_bytes(3, 16, 0, 16) == 0
    assert lib.cuzfp_hip_variable_index_bytes(4, 0, 16, 16) == 0
    assert lib.cuzfp_hip_variable_index_bytes(1, 16, 16, 16) == 0
    assert lib.cuzfp_hip_variable_index_bytes(2, 16, 16, 16) == 0
    assert lib.cuzfp_hip_variable_index_bytes(9, 16, 16, 16) == 0


def test_variable_index_argument_errors(libs):
    lib = cz.library()
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: rejected before any launch
    n = (16, 16, 16)  # 64 blocks: T = 1
    ib = lib.cuzfp_hip_variable_index_bytes(3, *n)
    wb = lib.cuzfp_hip_variable_workspace_bytes(3, *n)
    assert ib == 16 and wb > 0

    def call(lengths=buf, t=3, n=n, index=buf, index_bytes=ib, ws=buf, ws_bytes=wb):
        return lib.cuzfp_hip_variable_index(lengths, t, n[0], n[1], n[2], index, index_bytes, ws, ws_bytes, None)

    # null pointers
    assert call(lengths=None) == 1
    assert call(index=None) == 1
    assert call(ws=None) == 1
    # misaligned pointers: the index and the workspace 8 bytes, the lengths 2
    assert call(index=ctypes.c_void_p(0x1004)) == 1
    assert call(ws=ctypes.c_void_p(0x1004)) == 1
    assert call(lengths=ctypes.c_void_p(0x1001)) == 1
    # short index_bytes, short workspace
    assert call(index_bytes=ib - 1) == 1
    assert call(index_bytes=0) == 1
    assert call(ws_bytes=wb - 1) == 1
    assert call(n=(16, 16, 20), index_bytes=ib) == 1  # 80 blocks: T = 2
    # integer and unknown types, bad dimensions
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2
    assert call(n=(0, 0, 0)) == 1
    assert call(n=(16, 0, 16)) == 1


def test_decode_region_variable_argument_errors(libs):
    lib = cz.library()
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: rejected before any launch
    big = 1 << 30
    ib16 = lib.cuzfp_hip_variable_index_bytes(3, 16, 16, 16)

    def call(stream=buf, nbytes=big, lengths=buf, index=buf, index_bytes=None, t=3, n=(16, 16, 16), o=(0, 0, 0),
             e=(4, 4, 4), out=buf):
        if index_bytes is None:
            index_bytes = lib.cuzfp_hip_variable_index_bytes(3, *n) or ib16
        return lib.cuzfp_hip_decode_region_variable(stream, nbytes, lengths, index, index_bytes, t, n[0], n[1], n[2],
                                                    o[0], o[1], o[2], e[0], e[1], e[2], 0, 0, 0, out, None)

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
    assert call(lengths=None) == 1
    assert call(index=None) == 1
    assert call(out=None) == 1
    # misaligned index, stream and lengths
    assert call(index=ctypes.c_void_p(0x1004)) == 1
    assert call(stream=ctypes.c_void_p(0x1002)) == 1
    assert call(lengths=ctypes.c_void_p(0x1001)) == 1
    # short index_bytes
    assert call(index_bytes=ib16 - 1) == 1
    assert call(index_bytes=8) == 1
    assert call(n=(16, 16, 20), index_bytes=ib16) == 1
    # integer and unknown types, bad dimensions
    assert call(t=1) == 2 and call(t=2) == 2 and call(t=9) == 2
    assert call(n=(16, 0, 16)) == 1
    assert call(n=(0, 0, 0)) == 1


def test_python_validation(libs):
    class NoStream:  # the rank and box checks come before the stream is looked at
        is_cuda = False

    ns = NoStream()
    for origin, extent in (((0, 0), (4, 4, 4)), ((0, 0, 0), (4, 4)), ((0,), (4,)), ((0, 0, 0, 0), (4, 4, 4, 4))):
        with pytest.raises(ValueError, match="rank"):
            cz.decode_region_variable(ns, ns, ns, (16, 16, 16), np.float32, origin, extent)
    with pytest.raises(ValueError):
        cz.decode_region_variable(ns, ns, ns, (16, 16, 16, 16), np.float32, (0,) * 4, (4,) * 4)
    with pytest.raises(ValueError, match="non-negative"):
        cz.decode_region_variable(ns, ns, ns, (16, 16, 16), np.float32, (0, -1, 0), (4, 4, 4))
    with pytest.raises(ValueError, match="positive"):
        cz.decode_region_variable(ns, ns, ns, (16, 16, 16), np.float32, (0, 0, 0), (4, 0, 4))
    with pytest.raises(ValueError, match="device"):
        cz.decode_region_variable(ns, ns, ns, (16, 16, 16), np.float32, (0, 0, 0), (4, 4, 4))
    # decode_variable(index=) takes the same road: the whole array as the box
    with pytest.raises(ValueError, match="decode_region_variable.*device"):
        cz.decode_variable(ns, ns, (16, 16, 16), np.float32, index=ns)
    with pytest.raises(ValueError, match="device"):
        cz.variable_index(ns, (16, 16, 16), np.float32)
    for name in ("variable_index", "decode_region_variable"):
        assert name in cz.__all__ and callable(getattr(cz, name))


def test_variable_index_map(tmp_path):
    """tests/native/variable_index_map.cpp over csrc/variable_index.hpp and
    region.hpp: every block's offset is the 64-bit running sum, its loads stay
    inside lengths[0 .. nblocks) and index[0 .. T), every box of every shape up
    to 9 x 9 x 9 visits each of its blocks once, and with hostile index and
    length contents every stream dword the copy-in loads lies in the stream."""
    exe = str(tmp_path / "variable_index_map")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "variable_index_map.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
