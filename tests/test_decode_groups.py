"""The 3D decoder's workgroups: which wave each slot decodes.

In one resident round of waves the 3D 32-bit decoder runs 16-wave workgroups
that take the waves of the four encoder workgroups of their own XCD
(cuzfp_amd/csrc/wave_index.hpp, kernels.hpp kDecWavesRound) when the launch's
wave count is a multiple of 8 x 16; every other launch keeps 4-wave workgroups
and consecutive waves.  The index function is checked on the host; on the GPU
the decoded array must equal the CPU oracle's bit for bit at wave counts on
both sides of every condition.
"""
import os
import subprocess

import numpy as np
import pytest

import cuzfp_amd as cz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WPG = 16  # kDecWavesRound


def test_wave_index_function(tmp_path):
    """decode_wave_of over every launch size 1..700 and the GPU cases' sizes,
    workgroups of 4, 8, 12 and 16 waves: a bijection of the launch's slots onto
    its waves, padding slots past the end, and under the remap every wave from
    an encoder workgroup of the decoder workgroup's own index mod 8."""
    exe = str(tmp_path / "wave_index")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "wave_index.cpp")])
    for args in ([], [str(n) for n in (8 * WPG, 16 * WPG, 8 * WPG + 1, 8 * WPG - 1, 1, 130, 4096, 4097, 262144)]):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr


def _field(shape, dtype, seed):
    """Smooth values, noise and zero blocks mixed within every wave."""
    from cuzfp_amd.datagen import polynomial_field, splitmix_uniform
    if np.dtype(dtype).kind == "i":
        rng = np.random.default_rng(seed)
        return rng.integers(-2 ** 28, 2 ** 28, size=shape).astype(dtype)
    a = polynomial_field(shape, dtype) + (splitmix_uniform(shape, dtype, seed=seed) - 0.5) * 1e-3
    a = a.astype(dtype)
    a[:, :, 32:48] = 0  # four zero blocks in every row of blocks
    a[::3, 1::2, 100:140] *= 1e10
    return a


# (nz, ny, nx) with nx = 256: a wave is one x-row of 64 blocks, so the launch
# has (nz / 4) (ny / 4) waves
_SHAPES = {
    "8xWPG": (128, 16, 256),        # 128 waves: one round of 8 workgroups
    "16xWPG": (256, 16, 256),       # 256 waves: two
    "8xWPG+1": (172, 12, 256),      # 129 waves: consecutive, 4-wave workgroups
    "8xWPG-1": (508, 4, 256),       # 127 waves, a partial last workgroup
    "one wave": (4, 4, 256),
    "partial group": (260, 8, 256),  # 130 waves
    "partial wave": (12, 8, 68),    # 102 blocks
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_SHAPES))
def test_decode_wave_counts(cuda, restatement, case):
    """3D f32 at rate 8 (and one maxbits that is no multiple of 64): stream and
    decoded array against the oracle."""
    import torch
    shape = _SHAPES[case]
    a = _field(shape, np.float32, 3)
    x = torch.from_numpy(a).to(cuda)
    for mb in (cz.rate_to_maxbits(8, np.float32, 3), 200):
        ref = restatement.compress(a, mb)
        w = cz.encode(x, mb)
        y = cz.decode(w, shape, x.dtype, mb)
        torch.cuda.synchronize()
        assert np.array_equal(w.cpu().numpy().view(np.uint64), ref), (case, mb)
        want = restatement.decompress(ref, shape, np.float32, mb)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32)), (case, mb)


@pytest.mark.gpu
def test_decode_groups_general_gather(cuda, restatement):
    """The 16-wave workgroups of the kernels that gather by strides: int32
    (128 waves) and a float32 destination with an element stride of 2."""
    import torch
    shape = _SHAPES["8xWPG"]
    a = _field(shape, np.int32, 5)
    mb = 512
    ref = restatement.compress(a, mb)
    y = cz.decode(torch.from_numpy(ref.view(np.int64)).to(cuda), shape, torch.int32, mb)
    assert np.array_equal(y.cpu().numpy(), restatement.decompress(ref, shape, np.int32, mb))
    f = _field(shape, np.float32, 6)
    ref = restatement.compress(f, mb)
    want = restatement.decompress(ref, shape, np.float32, mb)
    dst = torch.full(shape[:2] + (2 * shape[2],), -7.0, dtype=torch.float32, device=cuda)
    cz.decode(torch.from_numpy(ref.view(np.int64)).to(cuda), shape, torch.float32, mb, out=dst[:, :, ::2])
    got = dst.cpu().numpy()
    assert np.array_equal(got[:, :, ::2].view(np.uint32), want.view(np.uint32))
    assert np.all(got[:, :, 1::2] == -7.0)


@pytest.mark.gpu
def test_decode_groups_sub_range(cuda, restatement, monkeypatch):
    """The host pipeline's range launches: 65 slabs of 4 waves in chunks of 33
    and 32 slabs (the unordered schedule), so the second decode launch is 8 x
    16 waves starting at wave 132, which is no multiple of the workgroup's 16;
    then chunks of a few slabs each (4-wave workgroups)."""
    shape = (260, 16, 256)
    a = _field(shape, np.float32, 7)
    mb = cz.rate_to_maxbits(8, np.float32, 3)
    ref = restatement.compress(a, mb)
    want = restatement.decompress(ref, shape, np.float32, mb)
    slab = 4 * shape[1] * shape[2] * 4
    monkeypatch.setenv("CUZFP_HOST_ORDERED", "0")
    for chunk in (33 * slab, 5 * slab):
        monkeypatch.setenv("CUZFP_HOST_CHUNK_BYTES", str(chunk))
        s = cz.compress_host(a, mb, nstreams=2)
        assert np.array_equal(s, ref), chunk
        y = cz.decompress_host(ref, shape, np.float32, mb, nstreams=2)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), chunk
