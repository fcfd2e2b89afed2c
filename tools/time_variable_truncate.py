"""Time truncate_variable against what it replaces and against a plain copy
(design tool, not a test).

  python tools/time_variable_truncate.py [--n 256] [--out FILE]

One configuration -- a 3D f32 n^3 polynomial field (cuzfp_amd.datagen) coded
at full precision (p32) and cut to tolerance 1e-3 -- and three legs through the
C-ABI on buffers made beforehand:

  truncate       cuzfp_hip_truncate_variable: two scans, the lengths pass, the
                 zero fill, the copy pass
  decode+encode  cuzfp_hip_decode_variable of the p32 stream into an array, then
                 cuzfp_hip_encode_variable of that array at tolerance 1e-3.
                 NOTE: this gives a different stream (the second encode sees
                 decoded values) and needs the uncompressed array in memory.
  copy           cuzfp_hip_copy of the source stream's bytes

Each leg is a hipGraph of `reps` calls (eager launches can be host-bound),
timed with device events after a warm-up replay; the legs are replayed in turn,
round after round, in one process; the median round is reported with the
fastest and slowest.  The truncated stream is first checked against
encode_variable of the original array at the tolerance, byte for byte.  Prints
one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--tolerance", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuzfp_amd as cz
    from cuzfp_amd.datagen import polynomial_field

    lib = cz.library()
    shape = (a.n,) * 3
    dev = torch.device("cuda:0")
    x = torch.from_numpy(polynomial_field(shape, np.float32)).to(dev)
    src, src_len, src_bits = cz.encode_variable(x, precision=32)
    want, want_len, want_bits = cz.encode_variable(x, tolerance=a.tolerance)
    got, got_len, got_bits = cz.truncate_variable(src, src_len, shape, torch.float32, from_precision=32,
                                                  tolerance=a.tolerance)
    torch.cuda.synchronize()
    assert got_bits == want_bits and torch.equal(got_len, want_len) and torch.equal(got, want)
    minexp = cz.accuracy_to_minexp(a.tolerance)
    nx, ny, nz = cz._extents(shape)
    nblocks = src_len.numel()
    ws_t = torch.empty(lib.cuzfp_hip_truncate_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=torch.int64, device=dev)
    ws_v = torch.empty(lib.cuzfp_hip_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=torch.int64, device=dev)
    dst = torch.empty(src.numel(), dtype=torch.int64, device=dev)  # no new block is longer than its source
    new_len = torch.empty(nblocks, dtype=torch.int16, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    y = torch.empty_like(x)
    nbytes = src.numel() * 8 // 16 * 16
    ca = src[: nbytes // 8].clone()
    cb = torch.empty_like(ca)

    def truncate():
        rc = lib.cuzfp_hip_truncate_variable(src.data_ptr(), src.numel() * 8, src_len.data_ptr(), 3, nx, ny, nz, 32,
                                             -1074, 32, minexp, dst.data_ptr(), dst.numel() * 8, new_len.data_ptr(),
                                             total.data_ptr(), ws_t.data_ptr(), ws_t.numel() * 8, cz._stream_handle(None))
        assert rc == 0

    def recode():
        st = cz._stream_handle(None)
        rc = lib.cuzfp_hip_decode_variable(src.data_ptr(), src.numel() * 8, src_len.data_ptr(), 3, nx, ny, nz, 0, 0, 0,
                                           y.data_ptr(), ws_v.data_ptr(), ws_v.numel() * 8, st)
        assert rc == 0
        rc = lib.cuzfp_hip_encode_variable(y.data_ptr(), 3, nx, ny, nz, 0, 0, 0, 32, minexp, dst.data_ptr(),
                                           dst.numel() * 8, new_len.data_ptr(), total.data_ptr(), ws_v.data_ptr(),
                                           ws_v.numel() * 8, st)
        assert rc == 0

    legs = {"truncate": truncate, "decode+encode": recode, "copy": lambda: cz.copy(ca, cb)}
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    graphs = {}
    for leg, fn in legs.items():
        fn()  # the kernels' code objects, outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.reps):
                fn()
        g.replay()  # warm-up
        torch.cuda.synchronize()
        graphs[leg] = g
    t = {leg: [] for leg in graphs}
    for _ in range(a.rounds):
        for leg, g in graphs.items():
            torch.cuda.synchronize()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            t[leg].append(e0.elapsed_time(e1) / a.reps * 1000)
    truncate()
    torch.cuda.synchronize()
    assert int(total.item()) == want_bits and torch.equal(dst[: want.numel()], want)
    rec = {"config": "3D f32 %d^3, p32 -> tolerance %g" % (a.n, a.tolerance), "blocks": nblocks,
           "array_bytes": x.numel() * 4, "source_bytes": src.numel() * 8, "source_bits": src_bits,
           "stream_bytes": want.numel() * 8, "stream_bits": want_bits, "index_bytes": 2 * nblocks,
           "source": "tools/time_variable_truncate.py: event times, hipGraph of %d calls, median of %d "
                     "interleaved rounds" % (a.reps, a.rounds)}
    for leg, v in t.items():
        v = sorted(v)
        rec[leg + "_us"] = round(v[len(v) // 2], 2)
        rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    rec["decode+encode_over_truncate"] = round(rec["decode+encode_us"] / rec["truncate_us"], 2)
    rec["truncate_over_copy"] = round(rec["truncate_us"] / rec["copy_us"], 2)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
