"""Time truncate against a plain copy and against decode + encode (design tool,
not a test).

  python tools/time_truncate.py [--recode-lib PATH] [--out FILE]

Three configurations -- 3D f32 256^3 at 512 -> 256 bits a block (the headline
workload's stream), 3D f32 512^3 at 1024 -> 512 (384 MiB of source plus
destination, more than the Infinity Cache holds) and, for the general path,
2D f32 8192^2 at 128 -> 33 -- and three legs:

  truncate       cz.truncate of the stream at M into a buffer at m
  copy           cz.copy of stream_bytes(m) bytes: the floor, the same bytes
                 written and the same useful bytes read
  decode+encode  what truncate replaces: decode at M, then encode at m.  NOTE:
                 this gives a different stream, quantised twice, not the rate-m
                 stream of the original values.  --recode-lib names the
                 library whose decode and encode run this leg (default: the
                 one in use), e.g. a build of the commit before truncate.

Each leg is a hipGraph of `reps` launches (eager launches can be host-bound),
timed with device events after a warm-up replay; the legs of a configuration
are replayed in turn, round after round, in one process, for as many rounds
as make every leg run for at least --seconds in all; the median round is
reported with the fastest and slowest.  The truncated stream is first checked
against encode at m, byte for byte.  Prints one JSON line per configuration
and writes all of them to --out.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--max-rounds", type=int, default=400)
    ap.add_argument("--recode-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuzfp_amd as cz
    from cuzfp_amd.datagen import polynomial_field

    lib = cz.library()
    recode = lib
    if a.recode_lib:
        recode = ctypes.CDLL(os.path.abspath(a.recode_lib))
        for fn in (recode.cuzfp_hip_encode, recode.cuzfp_hip_decode):
            fn.restype = ctypes.c_int
        recode.cuzfp_hip_encode.argtypes = lib.cuzfp_hip_encode.argtypes
        recode.cuzfp_hip_decode.argtypes = lib.cuzfp_hip_decode.argtypes

    # (name, shape, tile the field is repeated from, M, m)
    configs = [("3D f32 256^3", (256, 256, 256), (256, 256, 256), 512, 256),
               ("3D f32 512^3", (512, 512, 512), (256, 256, 256), 1024, 512),
               ("2D f32 8192^2", (8192, 8192), (1024, 1024), 128, 33)]
    results = []
    for name, shape, tile, M, m in configs:
        x = torch.from_numpy(polynomial_field(tile, np.float32)).cuda()
        x = x.repeat(*[n // t for n, t in zip(shape, tile)]).contiguous()
        src = cz.encode(x, M)
        want = cz.encode(x, m)
        dst = torch.zeros_like(want)
        cz.truncate(src, shape, np.float32, M, m, out=dst)
        torch.cuda.synchronize()
        assert torch.equal(dst, want), name
        nbytes = want.numel() * 8 // 16 * 16
        ca = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device).copy_(want[:nbytes // 8])
        cb = torch.empty_like(ca)
        y = torch.empty_like(x)
        w2 = torch.empty_like(want)
        nx, ny, nz = cz._extents(shape)

        def both():
            st = cz._stream_handle(None)
            rc = recode.cuzfp_hip_decode(src.data_ptr(), src.numel() * 8, 3, nx, ny, nz, 0, 0, 0, M,
                                         y.data_ptr(), st)
            assert rc == 0
            rc = recode.cuzfp_hip_encode(y.data_ptr(), 3, nx, ny, nz, 0, 0, 0, m, w2.data_ptr(),
                                         w2.numel() * 8, None, st)
            assert rc == 0

        legs = {"truncate": lambda: cz.truncate(src, shape, np.float32, M, m, out=dst),
                "copy": lambda: cz.copy(ca, cb),
                "decode+encode": both}
        graphs = {}
        once = {}
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        for leg, fn in legs.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(a.reps):
                    fn()
            g.replay()  # warm-up
            torch.cuda.synchronize()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            once[leg] = e0.elapsed_time(e1) / 1000
            graphs[leg] = g
        rounds = max(5, min(a.max_rounds, int(a.seconds / min(once.values())) + 1))
        t = {leg: [] for leg in graphs}
        for _ in range(rounds):
            for leg, g in graphs.items():
                torch.cuda.synchronize()
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                t[leg].append(e0.elapsed_time(e1) / a.reps * 1000)
        rec = {"config": name, "shape": list(shape), "maxbits": M, "new_maxbits": m,
               "source_bytes": src.numel() * 8, "stream_bytes": want.numel() * 8,
               "path": "word" if M % 64 == 0 and m % 64 == 0 else "general",
               "recode_lib": a.recode_lib or "the library in use",
               "source": "tools/time_truncate.py: event times, hipGraph of %d launches, median of %d "
                         "interleaved rounds" % (a.reps, rounds)}
        for leg, v in t.items():
            v = sorted(v)
            rec[leg + "_us"] = round(v[len(v) // 2], 2)
            rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
        rec["truncate_over_copy"] = round(rec["truncate_us"] / rec["copy_us"], 3)
        rec["decode+encode_over_truncate"] = round(rec["decode+encode_us"] / rec["truncate_us"], 2)
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del x, y, src, want, dst, ca, cb, w2, graphs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in results:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
