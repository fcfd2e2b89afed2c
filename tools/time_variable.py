"""Time the variable-rate modes against fixed rate and a plain copy (design
tool, not a test).

  python tools/time_variable.py [--out FILE]

The 256^3 f32 polynomial field at tolerances 1e-2 and 1e-4, eleven legs:

  encode_variable  cuzfp_hip_encode_variable (lengths, scan, zero, coder) into
                   preallocated buffers -- no read-back of the bit count
  decode_variable  cuzfp_hip_decode_variable (scan, decoder) of that stream
  encode, decode   the fixed-rate calls at the maxbits whose stream is nearest
                   in size to the variable one (the mean block length, rounded)
  copy             cz.copy of the uncompressed array: the bandwidth floor
  variable_index   cuzfp_hip_variable_index (scan, pick) of the stream's lengths
  region_variable_brick, _brick_off
                   cuzfp_hip_decode_region_variable of a 64^3 brick at (64, 64, 64)
                   (block aligned) and at (65, 66, 67), one launch each
  region_variable_whole
                   the same call with the whole array as the box: what
                   decode_variable(index=) runs, beside decode_variable
  region_fixed_brick, _brick_off
                   cz.decode_region of the same bricks of the fixed-rate stream

Each leg is a hipGraph of `reps` calls, timed with device events after a
warm-up replay; the legs are replayed in turn, round after round, in one
process, for as many rounds as make every leg run for at least --seconds in
all; the median round is reported with the fastest and slowest.  GB/s are
the uncompressed bytes the call produces (the brick's for the brick legs)
over the call's time.  The variable stream's round-trip
error is reported beside the tolerance.  Prints one JSON line per tolerance
and writes them to --out.
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuzfp_amd as cz
    from cuzfp_amd.datagen import polynomial_field

    lib = cz.library()
    shape = (a.size,) * 3
    x = torch.from_numpy(polynomial_field(shape, np.float32)).cuda()
    nx, ny, nz = cz._extents(shape)
    nblocks = ((a.size + 3) // 4) ** 3
    raw = x.numel() * 4
    results = []
    for tol in (1e-2, 1e-4):
        words, lengths, nbits = cz.encode_variable(x, tolerance=tol)
        back = cz.decode_variable(words, lengths, shape, torch.float32)
        err = float((back - x).abs().max())
        minexp = cz.accuracy_to_minexp(tol)
        mb = max(9, int(round(nbits / nblocks)))
        ws_bytes = lib.cuzfp_hip_variable_workspace_bytes(3, nx, ny, nz)
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=x.device)
        vout = torch.empty(cz.variable_maximum_size(shape, np.float32, 32) // 8, dtype=torch.int64, device=x.device)
        vlen = torch.empty(nblocks, dtype=torch.int16, device=x.device)
        vtot = torch.empty(1, dtype=torch.int64, device=x.device)
        y = torch.empty_like(x)
        fixed = cz.encode(x, mb)
        cb = torch.empty_like(x)

        def enc_var():
            rc = lib.cuzfp_hip_encode_variable(x.data_ptr(), 3, nx, ny, nz, 0, 0, 0, 32, minexp, vout.data_ptr(),
                                               vout.numel() * 8, vlen.data_ptr(), vtot.data_ptr(), ws.data_ptr(),
                                               ws_bytes, cz._stream_handle(None))
            assert rc == 0

        def dec_var():
            rc = lib.cuzfp_hip_decode_variable(words.data_ptr(), words.numel() * 8, lengths.data_ptr(), 3, nx, ny, nz,
                                               0, 0, 0, y.data_ptr(), ws.data_ptr(), ws_bytes,
                                               cz._stream_handle(None))
            assert rc == 0

        index = cz.variable_index(lengths, shape, torch.float32)
        vidx = torch.empty_like(index)
        brick = min(64, a.size // 2)
        bout = torch.empty((brick,) * 3, dtype=torch.float32, device=x.device)
        aligned, off = (brick,) * 3, (brick + 1, brick + 2, brick + 3)
        assert torch.equal(cz.decode_region_variable(words, lengths, index, shape, torch.float32, off, (brick,) * 3),
                           back[tuple(slice(o, o + brick) for o in off)])
        assert torch.equal(cz.decode_variable(words, lengths, shape, torch.float32, index=index), back)

        def build_index():
            rc = lib.cuzfp_hip_variable_index(lengths.data_ptr(), 3, nx, ny, nz, vidx.data_ptr(), vidx.numel() * 8,
                                              ws.data_ptr(), ws_bytes, cz._stream_handle(None))
            assert rc == 0

        def region_var(origin, extent, out):
            return lambda: cz.decode_region_variable(words, lengths, index, shape, torch.float32, origin, extent,
                                                     out=out)

        def region_fixed(origin):
            return lambda: cz.decode_region(fixed, shape, torch.float32, mb, origin, (brick,) * 3, out=bout)

        produced = {leg: bout.numel() * 4 for leg in ("region_variable_brick", "region_variable_brick_off",
                                                      "region_fixed_brick", "region_fixed_brick_off")}
        legs = {"variable_index": build_index,
                "region_variable_brick": region_var(aligned, (brick,) * 3, bout),
                "region_variable_brick_off": region_var(off, (brick,) * 3, bout),
                "region_variable_whole": region_var((0, 0, 0), shape, y),
                "region_fixed_brick": region_fixed(aligned), "region_fixed_brick_off": region_fixed(off),
                "encode_variable": enc_var, "decode_variable": dec_var,
                "encode": lambda: cz.encode(x, mb, out=fixed),
                "decode": lambda: cz.decode(fixed, shape, torch.float32, mb, out=y),
                "copy": lambda: cz.copy(x, cb)}
        graphs, once = {}, {}
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        for leg, fn in legs.items():
            fn()
            torch.cuda.synchronize()
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
        assert torch.equal(vlen, lengths) and int(vtot.item()) == nbits
        assert torch.equal(vout[: words.numel()], words) and torch.equal(vidx, index)
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
        rec = {"config": "3D f32 %d^3 polynomial" % a.size, "tolerance": tol, "max_abs_error": err,
               "variable_stream_bytes": words.numel() * 8, "index_bytes": lengths.numel() * 2,
               "offset_index_bytes": index.numel() * 8, "brick": brick,
               "variable_ratio": round(raw / (words.numel() * 8), 2),
               "variable_ratio_with_index": round(raw / (words.numel() * 8 + lengths.numel() * 2), 2),
               "fixed_maxbits": mb, "fixed_stream_bytes": fixed.numel() * 8,
               "fixed_ratio": round(raw / (fixed.numel() * 8), 2),
               "source": "tools/time_variable.py: event times, hipGraph of %d calls, median of %d interleaved "
                         "rounds" % (a.reps, rounds)}
        for leg, v in t.items():
            v = sorted(v)
            med = v[len(v) // 2]
            rec[leg + "_us"] = round(med, 2)
            rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
            rec[leg + "_GBps"] = round(produced.get(leg, raw) / med / 1e3, 1)
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del graphs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in results:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
