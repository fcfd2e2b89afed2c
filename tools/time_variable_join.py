"""Time join_variable against the route it replaces and against a plain copy
(design tool, not a test).

  python tools/time_variable_join.py [--n 256] [--out FILE]

One array -- a 3D f32 n^3 polynomial field (cuzfp_amd.datagen) -- at two modes,
full precision (p32) and tolerance 1e-3, cut into K = 2, 8 and 64 z-slabs, each
slab coded on its own beforehand.  Legs, through the C-ABI on buffers made
beforehand:

  join    cuzfp_hip_join_variable of the K slab streams, the index included
  paste   the route without it: for every slab cuzfp_hip_variable_index of its
          lengths and cuzfp_hip_insert_region_variable of its stream into the
          archive so far, beginning with the all-zero archive (one 0 bit a
          block); the archive ping-pongs between two sets of buffers
  copy    cuzfp_hip_copy of as many bytes as the result has: the floor

Each leg is a hipGraph of `reps` calls (eager launches can be host-bound),
timed with device events after a warm-up replay; the legs are replayed in turn,
round after round, in one process; the median round is reported with the
fastest and slowest.  Every leg's result is first checked byte for byte against
encode_variable of the whole array.  --once runs the join legs once, eagerly,
and times nothing (for a kernel trace).  Prints one JSON line and writes it to
--out.
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--parts", type=int, nargs="+", default=[2, 8, 64])
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuzfp_amd as cz
    from cuzfp_amd.dist import slab_extent
    from cuzfp_amd.datagen import polynomial_field

    lib = cz.library()
    n = a.n
    shape = (n,) * 3
    dev = torch.device("cuda:0")
    f32 = torch.float32
    i64, i16 = torch.int64, torch.int16
    x = torch.from_numpy(polynomial_field(shape, np.float32)).to(dev)
    nx, ny, nz = cz._extents(shape)
    nblocks = cz._block_count(shape)
    T1 = (nblocks + 63) // 64 + 1
    ws = torch.empty(lib.cuzfp_hip_variable_workspace_bytes(3, nx, ny, nz) // 8, dtype=i64, device=dev)
    modes = {"p32": {"precision": 32}, "a1e-3": {"tolerance": 1e-3}}
    legs, rec_modes = {}, {}
    keep = []  # every buffer a graph touches
    for mname, kw in modes.items():
        whole = cz.encode_variable(x, **kw)
        whole_idx = cz.variable_index(whole[1], shape, f32)
        nwords = whole[0].numel()
        rec_modes[mname] = {"stream_bytes": nwords * 8, "bits": whole[2]}
        # the outputs: two sets, for the paste route's ping-pong; the join writes set 0
        sets = [(torch.empty(nwords + 64, dtype=i64, device=dev), torch.empty(nblocks, dtype=i16, device=dev),
                 torch.empty(T1, dtype=i64, device=dev), torch.empty(1, dtype=i64, device=dev)) for _ in range(2)]
        zero = (torch.zeros((nblocks + 63) // 64, dtype=i64, device=dev), torch.ones(nblocks, dtype=i16, device=dev))
        zero += (cz.variable_index(zero[1], shape, f32),)
        keep += [whole, whole_idx, sets, zero]

        def same(s):
            torch.cuda.synchronize()
            return (int(s[3]) == whole[2] and torch.equal(s[1], whole[1]) and torch.equal(s[0][:nwords], whole[0]) and
                    torch.equal(s[2], whole_idx))

        for K in a.parts:
            spans = [slab_extent(n, K, r) for r in range(K)]
            parts = [cz.encode_variable(x[z0:z1].contiguous(), **kw) for z0, z1 in spans]
            pidx = [torch.empty((p[1].numel() + 63) // 64 + 1, dtype=i64, device=dev) for p in parts]
            table = (cz.VariablePart * K)()
            for k, p in enumerate(parts):
                table[k] = cz.VariablePart(p[0].data_ptr(), p[0].numel() * 8, p[1].data_ptr(), p[1].numel())
            keep += [parts, pidx, table]

            def join(table=table, K=K, out=sets[0]):
                st = cz._stream_handle(None)  # inside a capture: the capturing stream
                rc = lib.cuzfp_hip_join_variable(table, K, 3, nx, ny, nz, out[0].data_ptr(), out[0].numel() * 8,
                                                 out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                                 ws.data_ptr(), ws.numel() * 8, st)
                assert rc == 0

            def paste(parts=parts, pidx=pidx, spans=spans, sets=sets, zero=zero):
                st = cz._stream_handle(None)
                src = zero
                for k, (p, pi, (z0, z1)) in enumerate(zip(parts, pidx, spans)):
                    ex, ey, ez = cz._extents((z1 - z0, n, n))
                    rc = lib.cuzfp_hip_variable_index(p[1].data_ptr(), 3, ex, ey, ez, pi.data_ptr(), pi.numel() * 8,
                                                      ws.data_ptr(), ws.numel() * 8, st)
                    assert rc == 0
                    out = sets[k % 2]
                    rc = lib.cuzfp_hip_insert_region_variable(
                        p[0].data_ptr(), p[0].numel() * 8, p[1].data_ptr(), pi.data_ptr(), pi.numel() * 8,
                        src[0].data_ptr(), src[0].numel() * 8, src[1].data_ptr(), src[2].data_ptr(),
                        src[2].numel() * 8, 3, nx, ny, nz, 0, 0, z0, ex, ey, ez, out[0].data_ptr(),
                        out[0].numel() * 8, out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(),
                        ws.numel() * 8, st)
                    assert rc == 0
                    src = out

            # each leg checked byte for byte first
            join()
            assert same(sets[0]), ("join", mname, K)
            legs["join:%s:K%d" % (mname, K)] = join
            if not a.once:  # (a trace of the join alone: the scan's kernels are the paste's too)
                for s in sets:
                    for t in s:
                        t.fill_(-1)
                paste()
                assert same(sets[(K - 1) % 2]), ("paste", mname, K)
                legs["paste:%s:K%d" % (mname, K)] = paste
        pair = (whole[0][: nwords // 2 * 2].clone(), torch.empty(nwords // 2 * 2, dtype=i64, device=dev))
        keep.append(pair)
        legs["copy:%s" % mname] = (lambda p: lambda: cz.copy(*p))(pair)
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
    rec = {"config": "3D f32 %d^3, K z-slabs coded on their own" % n, "blocks": nblocks, "array_bytes": x.numel() * 4,
           "modes": rec_modes,
           "source": "tools/time_variable_join.py: event times, hipGraph of %d calls, median of %d interleaved rounds"
                     % (a.reps, a.rounds)}
    for leg, v in t.items():
        v = sorted(v)
        rec[leg + "_us"] = round(v[len(v) // 2], 2)
        rec[leg + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    for mname in modes:
        for K in a.parts:
            j, p = "join:%s:K%d" % (mname, K), "paste:%s:K%d" % (mname, K)
            rec["paste_over_join:%s:K%d" % (mname, K)] = round(rec[p + "_us"] / rec[j + "_us"], 2)
            rec["join_over_copy:%s:K%d" % (mname, K)] = round(rec[j + "_us"] / rec["copy:%s_us" % mname], 2)
            # done: the slowest round of the join below the fastest round of the route it replaces
            rec["join_faster:%s:K%d" % (mname, K)] = rec[j + "_us_min_max"][1] < rec[p + "_us_min_max"][0]
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
