"""Time extract_region_variable and insert_region_variable against the routes
they replace and against plain copies (design tool, not a test).

  python tools/time_variable_crop.py [--n 256] [--out FILE]

One archive -- a 3D f32 n^3 polynomial field (cuzfp_amd.datagen) coded at full
precision (p32) -- and two block-aligned boxes:

  brick  64^3 at (64, 64, 64)
  slab   4 x n x n at the origin: one block thick

Legs for the crop, through the C-ABI on buffers made beforehand:

  crop           cuzfp_hip_extract_region_variable, the box's index included
  decode+encode  the route without it: cuzfp_hip_decode_region_variable of the
                 box plus cuzfp_hip_encode_variable of the decoded box at p32
  copy:box       cuzfp_hip_copy of as many bytes as the box's stream has: the
                 floor of any crop

Legs for the paste (the box's own stream, cropped beforehand, pasted back):

  paste          cuzfp_hip_insert_region_variable, the new index included
  update         cuzfp_hip_encode_region_variable of the same box from its
                 decoded values at p32
  copy           cuzfp_hip_copy of the whole stream's bytes: the floor of any
                 out-of-place paste

Each leg is a hipGraph of `reps` calls (eager launches can be host-bound),
timed with device events after a warm-up replay; the legs are replayed in turn,
round after round, in one process; the median round is reported with the
fastest and slowest.  The results are first checked byte for byte: the crop
against encode_variable of the box, the paste against the source stream.
--once runs every leg once, eagerly, and times nothing (for a kernel trace).
Prints one JSON line and writes it to --out.
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
    f32 = torch.float32
    x = torch.from_numpy(polynomial_field(shape, np.float32)).to(dev)
    src, src_len, src_bits = cz.encode_variable(x, precision=32)
    src_idx = cz.variable_index(src_len, shape, f32)
    nx, ny, nz = cz._extents(shape)
    nblocks = src_len.numel()
    boxes = {"brick": ((64, 64, 64), (64, 64, 64)), "slab": ((0, 0, 0), (4, n, n))}
    box = {}
    for name, (o, e) in boxes.items():
        sl = tuple(slice(p, p + q) for p, q in zip(o, e))
        got = cz.extract_region_variable(src, src_len, src_idx, shape, f32, o, e, with_index=True)
        want = cz.encode_variable(x[sl].contiguous(), precision=32)
        assert got[2] == want[2] and torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), name
        assert torch.equal(got[3], cz.variable_index(want[1], e, f32)), name
        back = cz.insert_region_variable(got[0], got[1], got[3], src, src_len, src_idx, shape, f32, o, e,
                                         with_index=True)
        assert back[2] == src_bits and torch.equal(back[1], src_len) and torch.equal(back[0], src), name
        assert torch.equal(back[3], src_idx), name
        # the decoded box, for the legs that code from values
        vals = cz.decode_region_variable(src, src_len, src_idx, shape, f32, o, e)
        box[name] = (got[0].clone(), got[1], got[3], vals)
        torch.cuda.synchronize()

    ws = torch.empty(lib.cuzfp_hip_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=torch.int64, device=dev)
    dst = torch.empty(cz.variable_maximum_size(shape, np.float32, 32) // 8 + src.numel(), dtype=torch.int64, device=dev)
    new_len = torch.empty(nblocks, dtype=torch.int16, device=dev)
    new_idx = torch.empty_like(src_idx)
    total = torch.empty(1, dtype=torch.int64, device=dev)

    def whole16(t):  # a copy pair of the tensor's bytes, rounded down to 16
        ca = t[: t.numel() * 8 // 16 * 2].clone()
        return ca, torch.empty_like(ca)

    def crop(name):
        o, e = boxes[name]

        def run():
            st = cz._stream_handle(None)  # inside a capture: the capturing stream
            rc = lib.cuzfp_hip_extract_region_variable(
                src.data_ptr(), src.numel() * 8, src_len.data_ptr(), src_idx.data_ptr(), src_idx.numel() * 8, 3,
                nx, ny, nz, *cz._extents(o), *cz._extents(e), dst.data_ptr(), dst.numel() * 8, new_len.data_ptr(),
                new_idx.data_ptr(), new_idx.numel() * 8, total.data_ptr(), ws.data_ptr(), ws.numel() * 8, st)
            assert rc == 0
        return run

    def decode_encode(name):
        o, e = boxes[name]
        y = torch.empty(e, dtype=f32, device=dev)
        ex, ey, ez = cz._extents(e)

        def run():
            st = cz._stream_handle(None)  # inside a capture: the capturing stream
            rc = lib.cuzfp_hip_decode_region_variable(
                src.data_ptr(), src.numel() * 8, src_len.data_ptr(), src_idx.data_ptr(), src_idx.numel() * 8, 3,
                nx, ny, nz, *cz._extents(o), ex, ey, ez, 0, 0, 0, y.data_ptr(), st)
            assert rc == 0
            rc = lib.cuzfp_hip_encode_variable(y.data_ptr(), 3, ex, ey, ez, 0, 0, 0, 32, -1074, dst.data_ptr(),
                                               dst.numel() * 8, new_len.data_ptr(), total.data_ptr(), ws.data_ptr(),
                                               ws.numel() * 8, st)
            assert rc == 0
        return run

    def paste(name):
        o, e = boxes[name]
        bw, bl, bi, _ = box[name]

        def run():
            st = cz._stream_handle(None)  # inside a capture: the capturing stream
            rc = lib.cuzfp_hip_insert_region_variable(
                bw.data_ptr(), bw.numel() * 8, bl.data_ptr(), bi.data_ptr(), bi.numel() * 8, src.data_ptr(),
                src.numel() * 8, src_len.data_ptr(), src_idx.data_ptr(), src_idx.numel() * 8, 3, nx, ny, nz,
                *cz._extents(o), *cz._extents(e), dst.data_ptr(), dst.numel() * 8, new_len.data_ptr(),
                new_idx.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel() * 8, st)
            assert rc == 0
        return run

    def update(name):
        o, e = boxes[name]
        b = box[name][3]

        def run():
            st = cz._stream_handle(None)  # inside a capture: the capturing stream
            rc = lib.cuzfp_hip_encode_region_variable(
                b.data_ptr(), 0, 0, 0, 3, nx, ny, nz, 32, -1074, *cz._extents(o), *cz._extents(e), src.data_ptr(),
                src.numel() * 8, src_len.data_ptr(), src_idx.data_ptr(), src_idx.numel() * 8, dst.data_ptr(),
                dst.numel() * 8, new_len.data_ptr(), new_idx.data_ptr(), total.data_ptr(), ws.data_ptr(),
                ws.numel() * 8, st)
            assert rc == 0
        return run

    pair = whole16(src)
    legs = {"copy": lambda: cz.copy(*pair)}
    for name in boxes:
        bp = whole16(box[name][0])
        legs["crop:" + name] = crop(name)
        legs["decode+encode:" + name] = decode_encode(name)
        legs["copy:" + name] = (lambda p: lambda: cz.copy(*p))(bp)
        legs["paste:" + name] = paste(name)
        legs["update:" + name] = update(name)
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
    rec = {"config": "3D f32 %d^3 archived at p32" % n, "blocks": nblocks, "array_bytes": x.numel() * 4,
           "source_bytes": src.numel() * 8, "source_bits": src_bits,
           "boxes": {k: {"origin": v[0], "extent": v[1], "stream_bytes": box[k][0].numel() * 8}
                     for k, v in boxes.items()},
           "source": "tools/time_variable_crop.py: event times, hipGraph of %d calls, median of %d interleaved rounds"
                     % (a.reps, a.rounds)}
    for leg, v in t.items():
        v = sorted(v)
        rec[leg + "_us"] = round(v[len(v) // 2], 2)
        rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    for name in boxes:
        rec["decode+encode_over_crop:" + name] = round(rec["decode+encode:" + name + "_us"] /
                                                       rec["crop:" + name + "_us"], 2)
        rec["crop_over_copy:" + name] = round(rec["crop:" + name + "_us"] / rec["copy:" + name + "_us"], 2)
        rec["update_over_paste:" + name] = round(rec["update:" + name + "_us"] / rec["paste:" + name + "_us"], 2)
        rec["paste_over_copy:" + name] = round(rec["paste:" + name + "_us"] / rec["copy_us"], 2)
        # done: the slowest round of the new call below the fastest round of the old route
        rec["crop_faster:" + name] = rec["crop:" + name + "_us_min_max"][1] < rec["decode+encode:" + name +
                                                                                   "_us_min_max"][0]
        rec["paste_faster:" + name] = rec["paste:" + name + "_us_min_max"][1] < rec["update:" + name +
                                                                                     "_us_min_max"][0]
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
