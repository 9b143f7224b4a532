#!/usr/bin/env python3
"""Composition on the device against the route without it, in one process.

At the C2 shape (4096 x 64 KiB pairs, 1 % edits, from bench.py's input maker; V2
= V1 with 1 % further substitutions, made with torch) the deltas A = delta(R ->
V1) and B = delta(V1 -> V2) are encoded on the device.  Then, alternating run by
run:

  compose   dg_compose_plan_run(A, B): HIP-event stages "map", "scan", "emit",
            "total"
  baseline  what a caller does today for one delta R -> V2:
            dg_decode_plan_run(A), dg_decode_plan_run(B), dg_encode_plan_run(R,
            V2), on the same stream, between two events

20 warm-up and 100 timed runs of each (--warmup / --runs); medians, minima and
maxima, and the sum of |C| against the sum of |encode(R, V2)|, go to --out as JSON
(profiles/compose_rate.json is a recorded run).  No threshold is attached.
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
    npg, L, rate, q, seed_base, desc, _ = bench.CONFIGS[name]
    n = pairs or npg
    ref, v1, layout = bench.make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    # V2: rate x L further substitutions per pair
    g = torch.Generator(device="cuda")
    g.manual_seed(0xC0DE)
    v2 = v1.clone()
    for_pair = int(rate * L + 0.5)
    idx = (torch.arange(n, device="cuda").repeat_interleave(for_pair) * L +
           torch.randint(0, L, (n * for_pair,), device="cuda", generator=g))
    v2[idx] = v2[idx] ^ 0x5A
    s = stream.cuda_stream
    ts = torch.cuda.ExternalStream(s)

    def encode(r, v):
        plan = dg.EncodePlan(ctx, "onepass", layout, q=q)
        out = torch.empty(max(plan.output_bound, 1), dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        plan.run(r.data_ptr(), v.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        if int(st.abs().sum()) != 0:
            raise SystemExit(f"{name}: encode failed: status {st.unique().tolist()}")
        return plan, out, off, st

    enc_a, d_a, off_a, st_a = encode(ref, v1)
    enc_b, d_b, off_b, st_b = encode(v1, v2)
    enc_c, d_rv2, off_rv2, st_rv2 = encode(ref, v2)
    oa, ob = off_a.cpu().tolist(), off_b.cpu().tolist()

    comp = dg.ComposePlan(ctx, for_plans=(enc_a, enc_b))
    off_c = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st_c = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    kw = dict(d_a_offsets=off_a.data_ptr(), d_a_status=st_a.data_ptr(), d_b_offsets=off_b.data_ptr(),
              d_b_status=st_b.data_ptr(), stream=s)
    comp.run(d_a.data_ptr(), d_b.data_ptr(), 0, 0, off_c.data_ptr(), st_c.data_ptr(), **kw)   # the sizing run
    torch.cuda.synchronize()
    total_c = int(off_c[-1])
    d_c = torch.empty(max(total_c, 1), dtype=torch.uint8, device="cuda")

    def compose():
        comp.run(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), d_c.numel(), off_c.data_ptr(), st_c.data_ptr(), **kw)

    # the route without composition: decode A, decode B, encode (R, V2)
    dec_a = dg.DecodePlan(ctx, [(ro, rl, oa[i], oa[i + 1] - oa[i], vo, vl) for i, (ro, rl, vo, vl) in enumerate(layout)])
    dec_b = dg.DecodePlan(ctx, [(vo, vl, ob[i], ob[i + 1] - ob[i], vo, vl) for i, (ro, rl, vo, vl) in enumerate(layout)])
    t1, t2 = torch.zeros_like(v1), torch.zeros_like(v2)
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    st_d = torch.empty(n, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def baseline():
        e0.record(ts)
        dec_a.run(ref.data_ptr(), d_a.data_ptr(), t1.data_ptr(), lens.data_ptr(), st_d.data_ptr(), s)
        dec_b.run(t1.data_ptr(), d_b.data_ptr(), t2.data_ptr(), lens.data_ptr(), st_d.data_ptr(), s)
        enc_c.run(ref.data_ptr(), t2.data_ptr(), d_rv2.data_ptr(), d_rv2.numel(), off_rv2.data_ptr(), st_rv2.data_ptr(), s)
        e1.record(ts)

    # one checked run of each: C decodes against R to V2; the baseline reproduces V2
    compose()
    torch.cuda.synchronize()
    if int(st_c.abs().sum()) != 0:
        raise SystemExit(f"{name}: compose failed: status {st_c.unique().tolist()}")
    oc = off_c.cpu().tolist()
    dec_c = dg.DecodePlan(ctx, [(ro, rl, oc[i], oc[i + 1] - oc[i], vo, vl) for i, (ro, rl, vo, vl) in enumerate(layout)])
    chk = torch.zeros_like(v2)
    dec_c.run(ref.data_ptr(), d_c.data_ptr(), chk.data_ptr(), lens.data_ptr(), st_d.data_ptr(), s)
    torch.cuda.synchronize()
    if int(st_d.abs().sum()) != 0 or not torch.equal(chk, v2):
        raise SystemExit(f"{name}: the composed deltas do not decode to V2: status {st_d.unique().tolist()}")
    baseline()
    torch.cuda.synchronize()
    if int(st_d.abs().sum()) != 0 or int(st_rv2.abs().sum()) != 0 or not torch.equal(t2, v2):
        raise SystemExit(f"{name}: the baseline route failed")

    comp.set_timing(1)
    t = {"baseline": [], "map": [], "scan": [], "emit": [], "total": []}
    for it in range(warmup + runs):   # alternating, so that both see the same machine
        compose()
        torch.cuda.synchronize()
        tc = comp.stage_times()
        baseline()
        torch.cuda.synchronize()
        if it >= warmup:
            for k in ("map", "scan", "emit", "total"):
                t[k].append(tc[k])
            t["baseline"].append(e0.elapsed_time(e1))

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}

    res = {"name": name, "workload": desc + "; V2 = V1 with 1 % further substitutions", "pairs": n,
           "a_bytes": oa[-1], "b_bytes": ob[-1], "composed_bytes": total_c, "encode_r_v2_bytes": int(off_rv2[-1]),
           "compose": {k: summary(t[k]) for k in ("map", "scan", "emit", "total")},
           "decode_decode_encode": summary(t["baseline"])}
    res["composed_over_encoded_bytes"] = res["composed_bytes"] / res["encode_r_v2_bytes"]
    res["baseline_over_compose_median"] = res["decode_decode_encode"]["median_ms"] / res["compose"]["total"]["median_ms"]
    for p in (comp, dec_a, dec_b, dec_c, enc_a, enc_b, enc_c):
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2")
    ap.add_argument("--pairs", type=int, default=0, help="pairs per shape (0: the shape's own 4096)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_rate.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("compose_rate.py needs a GPU: there is nothing to time without one")
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
