"""Time the coarse decode of a variable-rate stream against what it replaces
(design tool, not a test).

  python tools/time_variable_coarse.py [--n 256] [--out FILE]

One source -- a 3D f32 n^3 polynomial field (cuzfp_amd.datagen) coded at full
precision (p32) -- three targets (tolerance 1e-2, tolerance 1e-4, precision 16)
and three boxes (the whole array, a 64^3 brick at (64, 64, 64), the same brick
at (65, 66, 67)).  Four legs a target and box, through the C-ABI on buffers
made beforehand:

  coarse     (a) cuzfp_hip_decode_region_variable_coarse of the p32 stream at
                 the target
  full       (b) cuzfp_hip_decode_region_variable of the p32 stream: the one
                 launch there was before, at full precision (other values)
  route      (c) the same values without the new call: cuzfp_hip_truncate_variable
                 of the whole stream, cuzfp_hip_variable_index of the new
                 lengths, cuzfp_hip_decode_region_variable of the box
  floor      (d) cuzfp_hip_decode_region_variable on a stream already cut to
                 the target: (a) - (d) is the walk

Each leg is a hipGraph of `reps` calls (eager launches can be host-bound),
timed with device events after a warm-up replay; the legs are replayed in turn,
round after round, in one process; the median round is reported with the
fastest and slowest.  (a)'s bytes are first checked against (c)'s.  Prints one
JSON line a target and writes them to --out.
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
    ap.add_argument("--rounds", type=int, default=11)
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
    ws_t = torch.empty(lib.cuzfp_hip_truncate_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=torch.int64,
                       device=dev)
    ws_v = torch.empty(lib.cuzfp_hip_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=torch.int64, device=dev)
    dst = torch.empty(src.numel(), dtype=torch.int64, device=dev)  # no new block is longer than its source
    new_len = torch.empty(nblocks, dtype=torch.int16, device=dev)
    new_idx = torch.empty(src_idx.numel(), dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    b = min(64, n)
    o = min(64, n - b)
    o2 = tuple(min(o + k, n - b) for k in (1, 2, 3))
    boxes = {"whole": ((0, 0, 0), shape), "brick": ((o,) * 3, (b,) * 3), "brick_unaligned": (o2, (b,) * 3)}
    targets = {"a1e-2": (32, cz.accuracy_to_minexp(1e-2)), "a1e-4": (32, cz.accuracy_to_minexp(1e-4)),
               "p16": (16, -1074)}
    kws = {"a1e-2": {"tolerance": 1e-2}, "a1e-4": {"tolerance": 1e-4}, "p16": {"precision": 16}}
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    lines = []
    for tname, (maxprec, minexp) in targets.items():
        cut, cut_len, cut_bits = cz.truncate_variable(src, src_len, shape, torch.float32, from_precision=32,
                                                      **kws[tname])
        cut_idx = cz.variable_index(cut_len, shape, torch.float32)
        rec = {"config": "3D f32 %d^3, p32 at %s" % (n, tname), "blocks": nblocks, "source_bits": src_bits,
               "target_bits": cut_bits,
               "source": "tools/time_variable_coarse.py: event times, hipGraph of %d calls, median of %d interleaved "
                         "rounds" % (a.reps, a.rounds)}
        for bname, (origin, extent) in boxes.items():
            out = torch.empty(extent, dtype=torch.float32, device=dev)
            oz, oy, ox = origin
            ez, ey, ex = extent

            def region(words, lengths, index):
                rc = lib.cuzfp_hip_decode_region_variable(words.data_ptr(), words.numel() * 8, lengths.data_ptr(),
                                                          index.data_ptr(), index.numel() * 8, 3, nx, ny, nz, ox, oy,
                                                          oz, ex, ey, ez, 0, 0, 0, out.data_ptr(),
                                                          cz._stream_handle(None))
                assert rc == 0

            def coarse():
                rc = lib.cuzfp_hip_decode_region_variable_coarse(src.data_ptr(), src.numel() * 8, src_len.data_ptr(),
                                                                 src_idx.data_ptr(), src_idx.numel() * 8, 3, nx, ny,
                                                                 nz, maxprec, minexp, ox, oy, oz, ex, ey, ez, 0, 0, 0,
                                                                 out.data_ptr(), cz._stream_handle(None))
                assert rc == 0

            def route():
                st = cz._stream_handle(None)  # (the capture's stream while a graph is recorded)
                rc = lib.cuzfp_hip_truncate_variable(src.data_ptr(), src.numel() * 8, src_len.data_ptr(), 3, nx, ny,
                                                     nz, 32, -1074, maxprec, minexp, dst.data_ptr(), dst.numel() * 8,
                                                     new_len.data_ptr(), total.data_ptr(), ws_t.data_ptr(),
                                                     ws_t.numel() * 8, st)
                assert rc == 0
                rc = lib.cuzfp_hip_variable_index(new_len.data_ptr(), 3, nx, ny, nz, new_idx.data_ptr(),
                                                  new_idx.numel() * 8, ws_v.data_ptr(), ws_v.numel() * 8, st)
                assert rc == 0
                region(dst, new_len, new_idx)

            legs = {"coarse": coarse, "full": lambda: region(src, src_len, src_idx), "route": route,
                    "floor": lambda: region(cut, cut_len, cut_idx)}
            # (a)'s bytes against (c)'s, before any timing
            out.fill_(-1.0)
            route()
            want = out.clone()
            out.fill_(-2.0)
            coarse()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (tname, bname)
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
            r = {}
            for leg, v in t.items():
                v = sorted(v)
                r[leg + "_us"] = round(v[len(v) // 2], 2)
                r[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
            r["coarse_over_route"] = round(r["coarse_us"] / r["route_us"], 3)
            r["coarse_over_floor"] = round(r["coarse_us"] / r["floor_us"], 3)
            r["coarse_over_full"] = round(r["coarse_us"] / r["full_us"], 3)
            rec[bname] = r
            del graphs
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
