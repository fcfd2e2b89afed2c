"""Time decode_region against the whole-array decoder (design tool, not a test).

  python tools/region_time.py [--size 256] [--out FILE]

For 3D f32 at rate 8 and 3D f64 at rate 16 and three boxes -- a 64^3 brick at
an unaligned origin, a block-aligned 64 x N x N slab, the whole array -- three
legs:

  region       decode_region of the box
  full         decode of the whole array (what every leg below has to beat)
  full+slice   decode of the whole array, then a device copy of the box out of
               it: the only way to get the box without decode_region

Each leg is a hipGraph of `reps` launches (eager launches can be host-bound),
timed with events after a warm-up replay; the legs of one box are replayed in
turn, round after round, in one process, and the median round is reported.
Prints one JSON line per case and writes all of them to --out.
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
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuzfp_amd as cz
    from cuzfp_amd.datagen import polynomial_field

    n = a.size
    shape = (n, n, n)
    boxes = {"brick 64^3 at (5,6,7)": ((5, 6, 7), (64, 64, 64)),
             f"slab 64x{n}x{n} at z=64": ((64, 0, 0), (64, n, n)),
             "whole array": ((0, 0, 0), shape)}
    results = []
    for dtype, rate in ((np.float32, 8), (np.float64, 16)):
        arr = polynomial_field(shape, dtype)
        x = torch.from_numpy(arr).cuda()
        mb = cz.rate_to_maxbits(rate, arr.dtype, 3)
        w = cz.encode(x, mb)
        y = cz.decode(w, shape, x.dtype, mb)
        torch.cuda.synchronize()
        for name, (origin, extent) in boxes.items():
            sl = tuple(slice(o, o + e) for o, e in zip(origin, extent))
            out = torch.empty(extent, dtype=x.dtype, device=x.device)
            cz.decode_region(w, shape, x.dtype, mb, origin, extent, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out, y[sl]), name  # the same bytes as the slice

            def full_slice():
                cz.decode(w, shape, x.dtype, mb, out=y)
                out.copy_(y[sl])

            legs = {"region": lambda: cz.decode_region(w, shape, x.dtype, mb, origin, extent, out=out),
                    "full": lambda: cz.decode(w, shape, x.dtype, mb, out=y),
                    "full+slice": full_slice}
            graphs = {}
            for leg, fn in legs.items():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(a.reps):
                        fn()
                g.replay()  # warm-up
                torch.cuda.synchronize()
                graphs[leg] = g
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            t = {leg: [] for leg in graphs}
            for _ in range(a.rounds):
                for leg, g in graphs.items():
                    torch.cuda.synchronize()
                    e0.record()
                    g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    t[leg].append(e0.elapsed_time(e1) / a.reps * 1000)
            rec = {"dtype": np.dtype(dtype).name, "shape": list(shape), "rate": rate, "maxbits": mb, "box": name,
                   "source": "tools/region_time.py: hipGraph of %d launches, median of %d interleaved rounds" % (a.reps, a.rounds)}
            for leg, v in t.items():
                v = sorted(v)
                rec[leg + "_us"] = round(v[len(v) // 2], 2)
                rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
            rec["region_over_full"] = round(rec["region_us"] / rec["full_us"], 3)
            results.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in results:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
