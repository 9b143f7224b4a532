#!/usr/bin/env python3
"""Inversion on the device against the route without it, in one process.

Per shape (bench.py's input maker) the deltas A = delta(R -> V) are encoded on
the device with the shape's own encoder.  Then, alternating run by run:

  invert    dg_invert_plan_run(R, A): HIP-event stages "map", "scan", "emit",
            "total"
  baseline  what a caller does today for delta(V -> R): an encode plan run on
            (V, R), between two events

  c2  4096 x 64 KiB pairs, 1 % edits, onepass deltas: the COPYs are in key
      order, the map kernel does not sort
  c4  4096 x 256 KiB transposition pairs, correcting deltas: the COPYs jump
      back and forth in R, the map kernel sorts

20 warm-up and 100 timed runs of each (--warmup / --runs); medians, minima and
maxima, and the sum of |invert(A)| against the sum of |encode(V, R)|, go to
--out as JSON (profiles/invert_rate.json is a recorded run).  No threshold is
attached.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(name, bench, dg, ctx, torch, stream, pairs, warmup, runs):
    npg, L, rate, q, seed_base, desc, algo = bench.CONFIGS[name]
    n = pairs or npg
    ref, ver, layout = bench.make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    s = stream.cuda_stream
    ts = torch.cuda.ExternalStream(s)

    def encode(r, v, lay):
        plan = dg.EncodePlan(ctx, algo, lay, q=q)
        out = torch.empty(max(plan.output_bound, 1), dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        plan.run(r.data_ptr(), v.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        if int(st.abs().sum()) != 0:
            raise SystemExit(f"{name}: encode failed: status {st.unique().tolist()}")
        return plan, out, off, st

    enc_a, d_a, off_a, st_a = encode(ref, ver, layout)
    back = [(vo, vl, ro, rl) for ro, rl, vo, vl in layout]
    enc_b, d_b, off_b, st_b = encode(ver, ref, back)

    inv = dg.InvertPlan(ctx, for_plan=enc_a)
    d_i = torch.empty(max(inv.output_bound, 1), dtype=torch.uint8, device="cuda")
    off_i = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st_i = torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def invert():
        inv.run(ref.data_ptr(), d_a.data_ptr(), d_i.data_ptr(), d_i.numel(), off_i.data_ptr(), st_i.data_ptr(),
                d_delta_offsets=off_a.data_ptr(), d_delta_status=st_a.data_ptr(), stream=s)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def baseline():
        e0.record(ts)
        enc_b.run(ver.data_ptr(), ref.data_ptr(), d_b.data_ptr(), d_b.numel(), off_b.data_ptr(), st_b.data_ptr(), s)
        e1.record(ts)

    # one checked run: the inverses decode against V to R
    torch.cuda.synchronize()   # (the buffers above were filled on torch's stream)
    invert()
    torch.cuda.synchronize()
    if int(st_i.abs().sum()) != 0:
        raise SystemExit(f"{name}: invert failed: status {st_i.unique().tolist()}")
    oi = off_i.cpu().tolist()
    dec = dg.DecodePlan(ctx, [(vo, vl, oi[i], oi[i + 1] - oi[i], ro, rl) for i, (ro, rl, vo, vl) in enumerate(layout)])
    chk = torch.zeros_like(ref)
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    st_d = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.run(ver.data_ptr(), d_i.data_ptr(), chk.data_ptr(), lens.data_ptr(), st_d.data_ptr(), s)
    torch.cuda.synchronize()
    spans_equal = all(torch.equal(chk[ro:ro + rl], ref[ro:ro + rl]) for ro, rl, _, _ in layout[:64])
    if int(st_d.abs().sum()) != 0 or not spans_equal:
        raise SystemExit(f"{name}: the inverted deltas do not decode to R: status {st_d.unique().tolist()}")

    inv.set_timing(1)
    t = {"baseline": [], "map": [], "scan": [], "emit": [], "total": []}
    for it in range(warmup + runs):   # alternating, so that both see the same machine
        invert()
        torch.cuda.synchronize()
        tc = inv.stage_times()
        baseline()
        torch.cuda.synchronize()
        if it >= warmup:
            for k in ("map", "scan", "emit", "total"):
                t[k].append(tc[k])
            t["baseline"].append(e0.elapsed_time(e1))

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}

    res = {"name": name, "workload": desc, "algorithm": algo, "pairs": n, "a_bytes": int(off_a[-1]),
           "inverted_bytes": oi[-1], "encode_v_r_bytes": int(off_b[-1]),
           "invert": {k: summary(t[k]) for k in ("map", "scan", "emit", "total")},
           "encode_v_r": summary(t["baseline"])}
    res["inverted_over_encoded_bytes"] = res["inverted_bytes"] / res["encode_v_r_bytes"]
    res["baseline_over_invert_median"] = res["encode_v_r"]["median_ms"] / res["invert"]["total"]["median_ms"]
    for p in (inv, dec, enc_a, enc_b):
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2,c4")
    ap.add_argument("--pairs", type=int, default=0, help="pairs per shape (0: the shape's own count)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "invert_rate.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("invert_rate.py needs a GPU: there is nothing to time without one")
    import bench
    import __graft_entry__ as entry
    dg = entry._load_product()
    ctx = dg.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    results = [measure(nm, bench, dg, ctx, torch, stream, args.pairs, args.warmup, args.runs)
               for nm in args.shapes.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "runs": args.runs, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
