"""Time encode_region_variable against the route it replaces and against a
plain copy of the stream (design tool, not a test).

  python tools/time_variable_region_update.py [--n 256] [--out FILE]

One archive -- a 3D f32 n^3 polynomial field (cuzfp_amd.datagen) coded at full
precision (p32) -- and three boxes of new values, written at p32:

  brick    64^3 at (64, 64, 64): block-aligned, every touched block covered
  brick+1  64^3 at (65, 65, 65): 17^3 touched blocks, all through the merge
           variant (its surface blocks need their old values)
  slab     4 x n x n at the origin: a one-block-thick halo, covered

and three legs through the C-ABI on buffers made beforehand:

  update         cuzfp_hip_encode_region_variable, the new index included
  decode+encode  the route without it: cuzfp_hip_decode_variable of the whole
                 stream into an array, a device copy of the box into the array,
                 cuzfp_hip_encode_variable of the whole array.  NOTE: this
                 re-codes every untouched block from decoded values and needs
                 the uncompressed array in memory.
  copy           cuzfp_hip_copy of the source stream's bytes: the floor of any
                 out-of-place update

Each leg is a hipGraph of `reps` calls (eager launches can be host-bound),
timed with device events after a warm-up replay; the legs are replayed in turn,
round after round, in one process; the median round is reported with the
fastest and slowest.  The covered results are first checked against
encode_variable of the updated array, byte for byte.  --once runs every leg
once, eagerly, and times nothing (for a kernel trace).  Prints one JSON line and
writes it to --out.
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuzfp_amd as cz
    from cuzfp_amd.datagen import polynomial_field

    lib = cz.library()
    n = a.n
    shape = (n,) * 3
    dev = torch.device("cuda:0")
    x = torch.from_numpy(polynomial_field(shape, np.float32)).to(dev)
    src, src_len, src_bits = cz.encode_variable(x, precision=32)
    src_idx = cz.variable_index(src_len, shape, torch.float32)
    nx, ny, nz = cz._extents(shape)
    nblocks = src_len.numel()
    boxes = {"brick": ((64, 64, 64), (64, 64, 64)), "brick+1": ((65, 65, 65), (64, 64, 64)),
             "slab": ((0, 0, 0), (4, n, n))}
    new = {}
    for name, (o, e) in boxes.items():
        sl = tuple(slice(p, p + q) for p, q in zip(o, e))
        new[name] = (x[sl] * 1.5 + 0.25).contiguous()
        # the covered boxes: byte for byte encode_variable of the updated array
        got = cz.encode_region_variable(new[name], src, src_len, src_idx, shape, o, precision=32, with_index=True)
        if name != "brick+1":
            y = x.clone()
            y[sl] = new[name]
            want = cz.encode_variable(y, precision=32)
            assert got[2] == want[2] and torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), name
            assert torch.equal(got[3], cz.variable_index(want[1], shape, torch.float32)), name
        torch.cuda.synchronize()

    ws = torch.empty(lib.cuzfp_hip_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=torch.int64, device=dev)
    cap = cz.variable_maximum_size(shape, np.float32, 32)
    dst = torch.empty(cap // 8, dtype=torch.int64, device=dev)
    new_len = torch.empty(nblocks, dtype=torch.int16, device=dev)
    new_idx = torch.empty_like(src_idx)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    y = torch.empty_like(x)
    nbytes = src.numel() * 8 // 16 * 16
    ca = src[: nbytes // 8].clone()
    cb = torch.empty_like(ca)

    def update(name):
        o, e = boxes[name]
        b = new[name]

        def run():
            rc = lib.cuzfp_hip_encode_region_variable(
                b.data_ptr(), 0, 0, 0, 3, nx, ny, nz, 32, -1074, *cz._extents(o), *cz._extents(e), src.data_ptr(),
                src.numel() * 8, src_len.data_ptr(), src_idx.data_ptr(), src_idx.numel() * 8, dst.data_ptr(),
                dst.numel() * 8, new_len.data_ptr(), new_idx.data_ptr(), total.data_ptr(), ws.data_ptr(),
                ws.numel() * 8, cz._stream_handle(None))
            assert rc == 0
        return run

    def recode(name):
        o, e = boxes[name]
        sl = tuple(slice(p, p + q) for p, q in zip(o, e))
        b = new[name]

        def run():
            st = cz._stream_handle(None)
            rc = lib.cuzfp_hip_decode_variable(src.data_ptr(), src.numel() * 8, src_len.data_ptr(), 3, nx, ny, nz,
                                               0, 0, 0, y.data_ptr(), ws.data_ptr(), ws.numel() * 8, st)
            assert rc == 0
            y[sl].copy_(b)
            rc = lib.cuzfp_hip_encode_variable(y.data_ptr(), 3, nx, ny, nz, 0, 0, 0, 32, -1074, dst.data_ptr(),
                                               dst.numel() * 8, new_len.data_ptr(), total.data_ptr(), ws.data_ptr(),
                                               ws.numel() * 8, st)
            assert rc == 0
        return run

    legs = {"copy": lambda: cz.copy(ca, cb)}
    for name in boxes:
        legs["update:" + name] = update(name)
        legs["decode+encode:" + name] = recode(name)
    if a.once:
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        return
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
    rec = {"config": "3D f32 %d^3 archived at p32, boxes written at p32" % n, "blocks": nblocks,
           "array_bytes": x.numel() * 4, "source_bytes": src.numel() * 8, "source_bits": src_bits,
           "boxes": {k: {"origin": v[0], "extent": v[1]} for k, v in boxes.items()},
           "source": "tools/time_variable_region_update.py: event times, hipGraph of %d calls, median of %d "
                     "interleaved rounds" % (a.reps, a.rounds)}
    for leg, v in t.items():
        v = sorted(v)
        rec[leg + "_us"] = round(v[len(v) // 2], 2)
        rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    for name in boxes:
        rec["decode+encode_over_update:" + name] = round(rec["decode+encode:" + name + "_us"] /
                                                         rec["update:" + name + "_us"], 2)
        rec["update_over_copy:" + name] = round(rec["update:" + name + "_us"] / rec["copy_us"], 2)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
