#!/usr/bin/env python3
"""Reference selection on the device next to the other passes over the same
bytes, in one process.

Per shape (bench.py's input maker) R and V of every pair are put in one arena,
2 n spans.  Then, alternating run by run:

  sketch   dg_sketch_plan_run over the 2 n spans (p = 16, K = 256): HIP-event
           stage "total" (the fill of the output and the kernel)
  crc      dg_crc64_xz_batch_device over the same spans, the library's other
           read-everything pass, between two events
  encode   the onepass encode plan of the n pairs, stage "total"

  c2  4096 x 64 KiB pairs, 1 % edits: 8192 spans of 64 KiB
  c6  1024 x 1 MiB pairs, 1 % edits: 2048 spans of 1 MiB

and once per process

  match    dg_sketch_match_device of 4096 target sketches against 4096
           candidate sketches at K = 256 (the c2 sketches: V against R), between
           two events; the picks are checked: V_i picks R_i

20 warm-up and 100 timed runs of each (--warmup / --runs); medians, minima and
maxima and the rates in GB/s of arena bytes go to --out as JSON
(profiles/sketch_rate.json is a recorded run).  No threshold is attached.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, K = 16, 256


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}


def measure(name, bench, dg, ctx, torch, stream, pairs, warmup, runs):
    npg, L, rate, q, seed_base, desc, algo = bench.CONFIGS[name]
    n = pairs or npg
    ref, ver, layout = bench.make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    s = stream.cuda_stream
    ts = torch.cuda.ExternalStream(s)
    arena = torch.cat([ref, ver])
    base = ref.numel()
    assert base % 16 == 0
    spans = [(ro, rl) for ro, rl, _, _ in layout] + [(base + vo, vl) for _, _, vo, vl in layout]
    total = sum(ln for _, ln in spans)

    plan = dg.SketchPlan(ctx, spans, p=P, k=K)
    d_sk = torch.empty(len(spans) * K, dtype=torch.int64, device="cuda")
    span_arr = (dg._lib.Span * len(spans))(*[dg._lib.Span(*x) for x in spans])
    d_crc = torch.empty(len(spans), dtype=torch.int64, device="cuda")
    enc = dg.EncodePlan(ctx, "onepass", layout, q=q)
    d_out = torch.empty(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def sketch():
        plan.run(arena.data_ptr(), d_sk.data_ptr(), stream=s)

    def crc():
        e0.record(ts)
        ctx.check(dg.lib.dg_crc64_xz_batch_device(ctx.handle, arena.data_ptr(), span_arr, len(spans), d_crc.data_ptr(), s), "crc")
        e1.record(ts)

    def encode():
        enc.run(ref.data_ptr(), ver.data_ptr(), d_out.data_ptr(), d_out.numel(), off.data_ptr(), st.data_ptr(), s)

    # one checked run: a few spans against the host function
    sketch()
    torch.cuda.synchronize()
    for i in (0, len(spans) // 2, len(spans) - 1):
        o, ln = spans[i]
        got = d_sk[i * K:(i + 1) * K].cpu().numpy().view("uint64").tolist()
        if got != dg.sketch(bytes(arena[o:o + ln].cpu().numpy()), P, K):
            raise SystemExit(f"{name}: span {i}: the device sketch differs from dg_sketch")

    plan.set_timing(1)
    enc.set_timing(1)
    t = {"sketch": [], "crc": [], "encode": []}
    for it in range(warmup + runs):   # alternating, so that all three see the same machine
        sketch()
        torch.cuda.synchronize()
        ts_ = plan.stage_times()["total"]
        crc()
        torch.cuda.synchronize()
        tc = e0.elapsed_time(e1)
        encode()
        torch.cuda.synchronize()
        te = enc.stage_times()["total"]
        if it >= warmup:
            t["sketch"].append(ts_)
            t["crc"].append(tc)
            t["encode"].append(te)
    if int(st.abs().sum()) != 0:
        raise SystemExit(f"{name}: encode failed: status {st.unique().tolist()}")

    res = {"name": name, "workload": desc, "pairs": n, "spans": len(spans), "arena_bytes": total, "p": P, "bins": K,
           "chunk_bytes": plan.chunk_bytes}
    for key in t:
        res[key] = summary(t[key])
        res[key]["gb_per_s"] = total / res[key]["median_ms"] / 1e6
    res["sketch_over_crc_median"] = res["sketch"]["median_ms"] / res["crc"]["median_ms"]
    res["sketch_over_encode_median"] = res["sketch"]["median_ms"] / res["encode"]["median_ms"]
    keep = (d_sk, n) if name == "c2" else None
    plan.close()
    enc.close()
    return res, keep


def measure_match(dg, ctx, torch, stream, d_sk, n, warmup, runs):
    """V's sketches (the second half) against R's (the first half)."""
    s = stream.cuda_stream
    ts = torch.cuda.ExternalStream(s)
    d_m = torch.zeros(n * 4, dtype=torch.int32, device="cuda")
    cands, targets = d_sk.data_ptr(), d_sk.data_ptr() + 8 * K * n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for it in range(warmup + runs):
        e0.record(ts)
        dg.match_sketches_device(ctx, targets, n, cands, n, d_m.data_ptr(), k=K, stream=s)
        e1.record(ts)
        torch.cuda.synchronize()
        if it >= warmup:
            t.append(e0.elapsed_time(e1))
    m = d_m.cpu().view(n, 4)
    if m[:, 0].tolist() != list(range(n)):
        raise SystemExit("match: a version did not pick its own reference")
    res = {"targets": n, "candidates": n, "bins": K, "match": summary(t), "min_equal_seen": int(m[:, 1].min())}
    res["pairs_per_s"] = n * n / res["match"]["median_ms"] * 1e3
    res["word_compares_per_s"] = res["pairs_per_s"] * K
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2,c6")
    ap.add_argument("--pairs", type=int, default=0, help="pairs per shape (0: the shape's own count)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_rate.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sketch_rate.py needs a GPU: there is nothing to time without one")
    import bench
    import __graft_entry__ as entry
    dg = entry._load_product()
    ctx = dg.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    results, match = [], None
    for nm in args.shapes.split(","):
        res, keep = measure(nm, bench, dg, ctx, torch, stream, args.pairs, args.warmup, args.runs)
        results.append(res)
        if keep is not None:
            match = measure_match(dg, ctx, torch, stream, *keep, args.warmup, args.runs)
    doc = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(dg.LIB_PATH), "warmup": args.warmup,
           "runs": args.runs, "results": results, "match": match}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results + ([match] if match else []):
        print(json.dumps(r))


if __name__ == "__main__":
    main()
