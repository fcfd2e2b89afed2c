"""Time encode_region against the whole-array coders (design tool, not a test).

  python tools/region_update_time.py [--size 256] [--out FILE]

For 3D f32 at 512 bits a block and 3D f64 at 1024 and five boxes -- a
block-aligned 64^3 brick and 64 x N x N slab (the covered variant), the same
two shifted by (1, 1, 1) (the merge variant; the slab loses one element in y
and x to stay inside the array), the whole array -- three legs:

  update       encode_region of the box into the stream
  encode       encode of the whole array
  decode+encode  decode of the whole array, then encode of it: the only way to
               change part of a stream without encode_region (pasting the box
               into the decoded array is not even counted)

Each leg is a hipGraph of `reps` launches (eager launches can be host-bound),
timed with events after a warm-up replay; the legs of one box are replayed in
turn, round after round, in one process, and the median round is reported
with the fastest and slowest round.  Prints one JSON line per case and writes
all of them to --out.
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
    boxes = {"brick 64^3 at (64,64,64)": ((64, 64, 64), (64, 64, 64)),
             f"slab 64x{n}x{n} at z=64": ((64, 0, 0), (64, n, n)),
             "brick 64^3 at (65,65,65)": ((65, 65, 65), (64, 64, 64)),
             f"slab 64x{n - 1}x{n - 1} at (65,1,1)": ((65, 1, 1), (64, n - 1, n - 1)),
             "whole array": ((0, 0, 0), shape)}
    results = []
    for dtype, mb in ((np.float32, 512), (np.float64, 1024)):
        arr = polynomial_field(shape, dtype)
        x = torch.from_numpy(arr).cuda()
        ref = cz.encode(x, mb)
        w = ref.clone()      # the stream the updates write
        w2 = ref.clone()     # the whole-array legs' stream
        y = cz.decode(ref, shape, x.dtype, mb)
        torch.cuda.synchronize()
        for name, (origin, extent) in boxes.items():
            sl = tuple(slice(o, o + e) for o, e in zip(origin, extent))
            box = x[sl].contiguous()
            covered = all(o % 4 == 0 and ((o + e) % 4 == 0 or o + e == n) for o, e in zip(origin, extent))
            if covered:
                # the array's own values into a scrambled copy of its stream:
                # the box's blocks come back, every other word keeps the scramble
                w.copy_(ref ^ 0x5555)
                cz.encode_region(box, w, shape, mb, origin)
                torch.cuda.synchronize()
                nb = n // 4
                blk = torch.zeros((nb, nb, nb), dtype=torch.bool, device=x.device)
                blk[tuple(slice(o // 4, (o + e + 3) // 4) for o, e in zip(origin, extent))] = True
                words = mb // 64
                inside = blk.reshape(-1, 1).expand(-1, words).reshape(-1)
                assert torch.equal(w[inside], ref[inside]), name
                assert torch.equal(w[~inside], (ref ^ 0x5555)[~inside]), name
            w.copy_(ref)

            def both():
                cz.decode(w2, shape, x.dtype, mb, out=y)
                cz.encode(y, mb, out=w2)

            legs = {"update": lambda: cz.encode_region(box, w, shape, mb, origin),
                    "encode": lambda: cz.encode(x, mb, out=w2),
                    "decode+encode": both}
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
            rec = {"dtype": np.dtype(dtype).name, "shape": list(shape), "maxbits": mb, "box": name,
                   "variant": "covered" if covered else "merge",
                   "source": "tools/region_update_time.py: hipGraph of %d launches, median of %d interleaved rounds"
                             % (a.reps, a.rounds)}
            for leg, v in t.items():
                v = sorted(v)
                rec[leg + "_us"] = round(v[len(v) // 2], 2)
                rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
            rec["update_over_encode"] = round(rec["update_us"] / rec["encode_us"], 3)
            rec["update_over_decode+encode"] = round(rec["update_us"] / rec["decode+encode_us"], 3)
            results.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in results:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
