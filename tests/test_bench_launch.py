"""bench.py's multi-rank launcher on CPU: `python bench.py --gpus 2` with no
torchrun around it starts its two ranks itself (torch.distributed.run, gloo in
the dry-run mode, the CPU oracle standing in for the codec) and the line it
prints reports both ranks -- the scaling run cannot under-report its ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True,
                          text=True, timeout=300, env=env, cwd=ROOT)


def test_gpus2_launches_two_ranks():
    r = _run(["--gpus", "2", "--dry-run-cpu", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 prints one line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["world_size_seen"] == 2
    assert d["backend"] == "gloo"
    assert len(d["rank_devices"]) == 2
    assert d["value"] > 0


def test_world_size_mismatch_is_an_error():
    # a launcher that started fewer ranks than --gpus asks for: refused, no line
    r = _run(["--gpus", "2", "--dry-run-cpu", "--steps", "1", "--warmup", "0"],
             {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert "WORLD_SIZE" in r.stderr


def test_single_rank_dry_run():
    r = _run(["--dry-run-cpu", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["world_size_seen"] == 1


@pytest.mark.gpu
@pytest.mark.timeout(290)
def test_gpus2_gloo_same_device_bench():
    """bench.main()'s N > 1 path on a one-GPU box (verdict r03): two ranks on
    cuda:0, gloo with host-copy collectives in place of RCCL.  Exercises the
    multi-rank bookkeeping the driver's scaling run depends on -- the rank
    gather, max-over-ranks timing, configs[4] strong-scaled over 2 z-slabs with
    its all-gather and the per-slab reference hashes -- before such a run does.
    Not a measurement (two ranks share one GPU)."""
    r = _run(["--gpus", "2", "--full", "--backend", "gloo", "--same-device", "--steps", "10", "--warmup", "2",
              "--no-cpu-baseline", "--no-host-path", "--no-copy-probe", "--config5-steps", "2",
              "--kernel-ms", "5"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_seen"] == 2
    assert d["rank_devices"] == [0, 0]
    assert d["backend"].startswith("gloo")
    c5 = d["config5"]
    assert c5["n_ranks"] == 2 and len(c5["encode_ms_per_rank"]) == 2
    assert c5["parity"]["slabs_match_reference_word_ranges"] is True
    assert c5["parity"]["stream_matches_reference"] is True
    assert c5["allgather"]["backend"].startswith("gloo")
    assert d["allgather"] is not None and d["value"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(290)
def test_rccl_one_rank_bench():
    """bench.main() through its RCCL branch on a one-GPU box (--dist-init):
    init_process_group("nccl", world_size=1, device_id=cuda:0), the headline's
    and configs[4]'s stream all-gathers on RCCL, the gathered segment equal to
    the local stream.  Not a scaling measurement (one rank)."""
    r = _run(["--gpus", "1", "--full", "--dist-init", "--steps", "10", "--warmup", "2", "--no-cpu-baseline",
              "--no-host-path", "--no-copy-probe", "--config5-steps", "2", "--kernel-ms", "5"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["world_size_seen"] == 1
    assert d["backend"].startswith("nccl")
    ag = d["allgather"]
    assert ag is not None and ag["backend"].startswith("nccl") and ag["own_segment_matches"] is True
    c5 = d["config5"]
    assert c5["allgather"]["backend"].startswith("nccl")
    assert c5["parity"]["stream_matches_reference"] is True
    assert d["parity"].startswith("stream and decoded sha256 == reference")


def _words_of(pieces):
    # stream.npy's 16-bit pieces (float32, least significant first) back to 64-bit words
    assert pieces.dtype == np.float32
    return np.ascontiguousarray(pieces.astype("<u2")).view(np.uint64)


def test_dump_outputs_dry_run(tmp_path, restatement):
    """--dump-outputs writes the last step's stream and decoded array as float
    .npy files, the same from run to run (dry run: the CPU oracle's step)."""
    from cuzfp_amd.datagen import polynomial_field
    outs = []
    for d in ("a", "b"):
        r = _run(["--dry-run-cpu", "--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert line["ms_per_step"] > 0 and sorted(line["dumped"]) == ["decoded.npy", "stream.npy"]
        outs.append((np.load(tmp_path / d / "stream.npy"), np.load(tmp_path / d / "decoded.npy")))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    a = polynomial_field((16, 16, 16), np.float32)
    want = restatement.compress(a, 512)
    assert np.array_equal(_words_of(outs[0][0]), want)
    assert outs[0][1].dtype == np.float32
    assert np.array_equal(outs[0][1], restatement.decompress(want, a.shape, np.float32, 512))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """An output beyond its share of the budget is written as the same seeded,
    sorted sample of its elements every time; a smaller one whole."""
    import bench
    assert bench.DUMP_BUDGET_BYTES < 64_000_000
    assert bench.sample_indices(100, 100) is None
    idx = bench.sample_indices(1000, 64)
    assert idx.shape == (64,) and np.all(np.diff(idx) >= 0) and 0 <= idx[0] and idx[-1] < 1000
    assert np.array_equal(idx, bench.sample_indices(1000, 64))
    rng = np.random.default_rng(1)
    words = rng.integers(-2 ** 63, 2 ** 63 - 1, size=4096, dtype=np.int64)
    y = rng.standard_normal((8, 16, 64))
    assert np.array_equal(_words_of(bench.stream_pieces(words)), words.view(np.uint64))
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 16384)  # the stream 60 % of it, the array the rest
    files = bench.dump_outputs(str(tmp_path), words, y)
    s, d = np.load(tmp_path / "stream.npy"), np.load(tmp_path / "decoded.npy")
    assert files["stream.npy"]["sampled"] and files["decoded.npy"]["sampled"]
    assert s.dtype == np.float32 and d.dtype == np.float64 and s.nbytes + d.nbytes <= 16384
    assert np.array_equal(_words_of(s), words.view(np.uint64)[bench.sample_indices(4096, 9830 // 16)])
    assert np.array_equal(d, y.reshape(-1)[bench.sample_indices(y.size, (16384 - 9830) // 8)])
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 120000)  # the stream whole (65536 B), the array sampled
    files = bench.dump_outputs(str(tmp_path), words, y)
    assert not files["stream.npy"]["sampled"] and files["decoded.npy"]["sampled"]
    assert np.array_equal(_words_of(np.load(tmp_path / "stream.npy")), words.view(np.uint64))
    assert np.load(tmp_path / "decoded.npy").nbytes == (120000 - 65536) // 8 * 8


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_run_is_lean_and_dumps_the_step(tmp_path, restatement):
    """A plain run times its steps and nothing else (no --full record in its
    line), and --dump-outputs holds what the GPU step returned: the oracle's
    stream and decoded array for the same input, bit for bit."""
    from cuzfp_amd.datagen import polynomial_field
    r = _run(["--gpus", "1", "--size", "64", "--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 6 and d["value"] > 0 and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["full"] is False
    assert abs(d["ms_per_step"] * 1e-3 * d["value"] * 1e9 / (64 ** 3 * 4) - 1) < 1e-2  # value = bytes / step time
    for k in ("config5", "configs", "cpu_baseline", "host_path", "hbm_copy", "encode_ms", "roofline", "parity"):
        assert k not in d
    a = polynomial_field((64, 64, 64), np.float32)
    want = restatement.compress(a, 512)
    assert np.array_equal(_words_of(np.load(tmp_path / "stream.npy")), want)
    back = np.load(tmp_path / "decoded.npy")
    assert back.dtype == np.float32 and back.shape == a.shape
    assert np.array_equal(back, restatement.decompress(want, a.shape, np.float32, 512))


def test_same_device_needs_gloo():
    # two RCCL ranks on one GPU are refused at argument parsing
    r = _run(["--gpus", "2", "--same-device", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "--same-device needs --backend gloo" in r.stderr
