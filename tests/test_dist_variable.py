"""cuzfp_amd.dist.allgather_variable: every rank holds the variable-rate stream
of its z-slab, one exchange of sizes, two all-gathers and one join_variable give
every rank the stream of the whole array -- byte for byte encode_variable of it,
with its index.

As in tests/test_dist.py the ranks are spawned processes that share cuda:0 and
meet through gloo (RCCL needs one GPU a rank); a world-size-1 RCCL group runs
the device path of the gathers.  A multi-rank RCCL run needs more than one GPU
and is not made here.
"""
import os

import numpy as np
import pytest

from test_dist import _free_port

SHAPE = (16, 12, 20)


def _np(t):
    return t.cpu().numpy().copy()


def _worker(rank, world, port, backend, shape, kw, q):
    import torch
    import torch.distributed as dist
    import cuzfp_amd as cz
    from cuzfp_amd import dist as zd
    from cuzfp_amd.datagen import polynomial_field
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = torch.from_numpy(polynomial_field(shape, np.float32)).to(dev)
        z0, z1 = zd.slab_extent(shape[0], world, rank)
        if z1 > z0:
            words, lengths, nbits = cz.encode_variable(x[z0:z1].contiguous(), **kw)
        else:  # more ranks than 4-deep slabs: this one holds nothing
            words = torch.empty(0, dtype=torch.int64, device=dev)
            lengths = torch.empty(0, dtype=torch.int16, device=dev)
            nbits = 0
        gw, gl, gn, gi = zd.allgather_variable(words, lengths, nbits, shape, torch.float32, with_index=True)
        plain = zd.allgather_variable(words, lengths, nbits, shape, torch.float32)
        ww, wl, wn = cz.encode_variable(x, **kw)
        wi = cz.variable_index(wl, shape, torch.float32)
        torch.cuda.synchronize()
        assert len(plain) == 3 and plain[2] == gn and torch.equal(plain[0], gw) and torch.equal(plain[1], gl)
        q.put((rank, dist.get_backend(), gw.is_cuda and gl.is_cuda and gi.is_cuda, z1 - z0,
               (_np(gw), _np(gl), gn, _np(gi)), (_np(ww), _np(wl), wn, _np(wi))))
    finally:
        dist.destroy_process_group()


def _run(world, backend, shape, kw):
    import multiprocessing as mp
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, shape, kw, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        r = q.get(timeout=200)
        results[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(results) == list(range(world))
    for r in range(world):
        got_backend, on_gpu, depth, got, want = results[r]
        assert got_backend == backend and on_gpu
        assert got[2] == want[2] and want[2] > 0, r
        for g, w in zip(got[:2] + got[3:], want[:2] + want[3:]):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), r
    return results


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kw", [{"tolerance": 1e-3}, {"precision": 16}], ids=["a1e-3", "p16"])
def test_two_gloo_ranks(kw):
    """Two ranks, two slabs of 8 planes: both get encode_variable of the whole
    array, byte for byte, and its index."""
    results = _run(2, "gloo", SHAPE, kw)
    assert [results[r][2] for r in range(2)] == [8, 8]


@pytest.mark.gpu
@pytest.mark.timeout(240)
def test_rccl_one_rank():
    """A world-size-1 RCCL group: the gathers run on the device."""
    _run(1, "nccl", SHAPE, {"tolerance": 1e-3})


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_empty_rank():
    """Three ranks on an array of two 4-deep slabs: the third holds nothing
    and contributes no part, and still gets the whole stream."""
    results = _run(3, "gloo", (8, 12, 20), {"tolerance": 1e-3})
    assert [results[r][2] for r in range(3)] == [4, 4, 0]
