#!/usr/bin/env python3
"""Range reads on the device against a full decode, in one process.

Per shape (bench.py's input maker) the deltas are encoded on the device.  Then,
alternating run by run:

  index      dg_read_plan_index over the batch, between two events
  read_4k    dg_read_plan_run, one 4 KiB request per stream at seeded random
             offsets (HIP-event stage "read")
  read_64k   one 64 KiB request per stream
  read_16x4k 16 requests of 4 KiB per stream
  fallback   read_4k's requests on the same deltas with their first two
             commands exchanged in stream order: still valid, the same V, but
             no longer in sequence, so every request parses its whole stream
  decode     dg_decode_plan_run on the same deltas, with both CRC checks and
             with ignore_hash

  c2  4096 x 64 KiB pairs, 1 % edits, onepass deltas
  c6  1024 x 1 MiB pairs, 1 % edits, onepass deltas

--alt 64 (or 256) also times the read kernel's other block shape, request set
by request set next to the shipped one ("alt_" keys): it is lib/dg_read_alt.hsaco
of `make read_alt`, loaded by the A/B library build (DG_LIB_VARIANT=ab) into a
context of its own.  --append FILE adds the process's results to a list in FILE:
profiles/read_rate_c6_processes.json holds three processes' runs of
`--shapes c6 --only read_4k,fallback --append ...`, the spread the index is
judged against.

20 warm-up and 100 timed runs of each (--warmup / --runs); medians, minima and
maxima, the range bytes per request and the stream bytes a request parses (the
whole stream on the fallback path; on the indexed path the model's count: from
the index entry before the range to the end of the 4 KiB window in which the
first command at or after the range's end lies) go to --out as JSON
(profiles/read_rate.json is a recorded run).  No threshold is attached.
"""
from __future__ import annotations

import argparse
import bisect
import json
import os
import random
import re
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRIDE, WINDOW = 1024, 4096


def commands(d, limit=None):
    """[(stream offset, dst, len)] of a well-formed standard stream (the first `limit` of them)."""
    out, pos = [], 25
    while pos < len(d) and d[pos] and (limit is None or len(out) < limit):
        if d[pos] == 1:
            dst, n = struct.unpack_from(">II", d, pos + 5)
            out.append((pos, dst, n))
            pos += 13
        else:
            dst, n = struct.unpack_from(">II", d, pos + 1)
            out.append((pos, dst, n))
            pos += 9 + n
    return out


def exchanged(d):
    """The stream with its first two commands exchanged in stream order."""
    c = commands(d, 3)
    if len(c) < 2:
        return d
    a, b = c[0][0], c[1][0]
    e = c[2][0] if len(c) > 2 else (len(d) - 1 if d[-1] == 0 else len(d))
    return d[:a] + d[b:e] + d[a:b] + d[e:]


def parsed_bytes(d, off, n):
    """Stream bytes the indexed path parses for (off, n): the model of dg_read_kernel's window loop."""
    c = commands(d)
    starts = [s for s, _, _ in c]
    ents = []   # entry k: the first command at or after STRIDE * k
    for k in range(len(d) // STRIDE + 1):
        j = bisect.bisect_left(starts, STRIDE * k)
        if j < len(c):
            ents.append(c[j])
    start = max((s for s, dst, _ in ents if dst <= off), default=25)
    stop = next((s for s, dst, _ in c if dst >= off + n), len(d))
    return ((stop - start) // WINDOW + 1) * WINDOW


def shipped_block():
    """Threads per request of the product's read kernel (csrc/dg_read_dev.h)."""
    src = open(os.path.join(ROOT, "delta-compression_amd", "csrc", "dg_read_dev.h")).read()
    return int(re.search(r"kRdReadBlock = (\d+);", src).group(1))


def measure(name, bench, dg, ctx, torch, stream, pairs, warmup, runs, only, alt):
    npg, L, rate, q, seed_base, desc, algo = bench.CONFIGS[name]
    n = pairs or npg
    ref, ver, layout = bench.make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    s = stream.cuda_stream
    ts = torch.cuda.ExternalStream(s)
    enc = dg.EncodePlan(ctx, algo, layout, q=q)
    d_a = torch.empty(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    off_a = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st_a = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    enc.run(ref.data_ptr(), ver.data_ptr(), d_a.data_ptr(), d_a.numel(), off_a.data_ptr(), st_a.data_ptr(), s)
    torch.cuda.synchronize()
    if int(st_a.abs().sum()) != 0:
        raise SystemExit(f"{name}: encode failed: status {st_a.unique().tolist()}")
    enc.close()
    offs = off_a.cpu().tolist()
    total = offs[-1]
    d_a = d_a[:total + 16].clone()
    h_a = bytes(d_a[:total].cpu().numpy())
    h_x = b"".join(exchanged(h_a[offs[i]:offs[i + 1]]) for i in range(n))
    assert len(h_x) == total
    d_x = torch.frombuffer(bytearray(h_x + bytes(16)), dtype=torch.uint8).cuda()
    streams = [(ro, rl, offs[i], offs[i + 1] - offs[i]) for i, (ro, rl, _, _) in enumerate(layout)]

    rng = random.Random(0x5EED + len(name))

    def requests(per, size):
        out, at = [], 0
        for i, (_, _, _, vl) in enumerate(layout):
            for _ in range(per):
                ln = min(size, vl)
                out.append((i, rng.randrange(vl - ln + 1), ln, at))
                at += (ln + 15) & ~15
        arr = (dg.ReadReq * len(out))(*[dg.ReadReq(i, o, ln, 0, a) for i, o, ln, a in out])
        return out, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), at

    sets = {"read_4k": requests(1, 4096), "read_64k": requests(1, 65536), "read_16x4k": requests(16, 4096)}
    m_max = max(len(v[0]) for v in sets.values())
    d_out = torch.empty(max(v[2] for v in sets.values()) + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(m_max, dtype=torch.int32, device="cuda")
    d_st = torch.empty(m_max, dtype=torch.int32, device="cuda")
    d_sst = torch.empty(n, dtype=torch.int32, device="cuda")
    plan = dg.ReadPlan(ctx, streams, m_max)
    fb = dg.ReadPlan(ctx, streams, m_max)
    plans = {"": (plan, fb)}
    if alt:   # the other block shape: its code object in a context of its own, run on the same stream
        os.environ["DG_READ_HSACO"], os.environ["DG_READ_BLOCK"] = "dg_read_alt.hsaco", str(alt)
        ctx_alt = dg.Context(0)
        plans["alt_"] = (dg.ReadPlan(ctx_alt, streams, m_max), dg.ReadPlan(ctx_alt, streams, m_max))
        del os.environ["DG_READ_HSACO"], os.environ["DG_READ_BLOCK"]

    def index(p, delta):
        p.index(delta.data_ptr(), d_sst.data_ptr(), stream=s)

    def read(p, delta, key):
        reqs, d_req, _ = sets[key]
        p.run(ref.data_ptr(), delta.data_ptr(), d_req.data_ptr(), len(reqs), d_out.data_ptr(), d_len.data_ptr(),
              d_st.data_ptr(), stream=s)

    # checked runs: both plans serve V's bytes
    fbs = [v[1] for v in plans.values()]
    for p, delta in [(v[0], d_a) for v in plans.values()] + [(f, d_x) for f in fbs]:
        index(p, delta)
        torch.cuda.synchronize()
        if int(d_sst.abs().sum()) != 0:
            raise SystemExit(f"{name}: index failed: status {d_sst.unique().tolist()}")
        for key in (("read_4k",) if p in fbs else sets):
            d_out.zero_()
            torch.cuda.synchronize()
            read(p, delta, key)
            torch.cuda.synchronize()
            reqs = sets[key][0]
            if int(d_st[:len(reqs)].abs().sum()) != 0:
                raise SystemExit(f"{name}: {key} failed: status {d_st.unique().tolist()}")
            for i, o, ln, a in reqs[:48] + reqs[-16:]:
                vo = layout[i][2]
                if not torch.equal(d_out[a:a + ln], ver[vo + o:vo + o + ln]):
                    raise SystemExit(f"{name}: {key}: request ({i}, {o}, {ln}) is not V's bytes")

    descs = [(ro, rl, offs[i], offs[i + 1] - offs[i], vo, vl) for i, (ro, rl, vo, vl) in enumerate(layout)]
    dec = {False: dg.DecodePlan(ctx, descs, ignore_hash=False), True: dg.DecodePlan(ctx, descs, ignore_hash=True)}
    d_dec = torch.empty_like(ver)
    d_dlen = torch.empty(n, dtype=torch.int64, device="cuda")
    d_dst = torch.empty(n, dtype=torch.int32, device="cuda")
    for p in dec.values():
        p.set_timing(1)
    for v in plans.values():
        v[0].set_timing(1)
        v[1].set_timing(1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    keys = ["index", "read_4k", "read_64k", "read_16x4k", "fallback", "decode", "decode_ignore_hash"]
    if only:
        keys = [k for k in keys if k in only]
    if alt:   # the same reads by the other block shape, next to the shipped one's
        keys = [x for k in keys for x in ([k, "alt_" + k] if k.startswith("read") or k == "fallback" else [k])]
    t = {k: [] for k in keys}
    for it in range(warmup + runs):   # alternating, so that all see the same machine
        got = {}
        for k in keys:
            if k == "index":
                e0.record(ts)
                index(plan, d_a)
                e1.record(ts)
                torch.cuda.synchronize()
                got[k] = e0.elapsed_time(e1)
            elif k.endswith("fallback"):
                p = plans[k[:-len("fallback")]][1]
                read(p, d_x, "read_4k")
                torch.cuda.synchronize()
                got[k] = p.stage_times()["read"]
            elif "read" in k:
                p = plans["alt_" if k.startswith("alt_") else ""][0]
                read(p, d_a, k[4:] if k.startswith("alt_") else k)
                torch.cuda.synchronize()
                got[k] = p.stage_times()["read"]
            else:
                p = dec[k != "decode"]
                p.run(ref.data_ptr(), d_a.data_ptr(), d_dec.data_ptr(), d_dlen.data_ptr(), d_dst.data_ptr(), s)
                torch.cuda.synchronize()
                got[k] = p.stage_times()["decode"]
        if it >= warmup:
            for k in keys:
                t[k].append(got[k])
    if any(k.startswith("decode") for k in keys) and (int(d_dst.abs().sum()) != 0 or not torch.equal(d_dec, ver)):
        raise SystemExit(f"{name}: decode did not reproduce V")

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}

    res = {"name": name, "workload": desc, "streams": n, "delta_bytes": total, "version_bytes": int(ver.numel()),
           "read_kernel_block": shipped_block(), "alt_read_kernel_block": alt or None,
           "times": {k: summary(v) for k, v in t.items()}, "requests": {}}
    for key, (reqs, _, _) in sets.items():
        sample = reqs[:: max(len(reqs) // 64, 1)][:64]
        res["requests"][key] = {
            "count": len(reqs), "range_bytes": sum(r[2] for r in reqs) / len(reqs),
            "stream_bytes_parsed_indexed": statistics.mean(parsed_bytes(h_a[offs[i]:offs[i + 1]], o, ln)
                                                           for i, o, ln, _ in sample),
            "stream_bytes_parsed_fallback": total / n}
    for p in (*[q for v in plans.values() for q in v], *dec.values()):
        p.close()
    if alt:
        ctx_alt.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2,c6")
    ap.add_argument("--pairs", type=int, default=0, help="streams per shape (0: the shape's own count)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--only", default="", help="comma-separated measurements (default: all)")
    ap.add_argument("--alt", type=int, default=0,
                    help="also time the read kernel's other block shape (64 or 256 threads): lib/dg_read_alt.hsaco of "
                         "`make read_alt`, with DG_LIB_VARIANT=ab in the environment")
    ap.add_argument("--append", default="", help="append this process's results to the list in this file and write "
                                                 "no --out (several processes' runs side by side)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_rate.json"))
    args = ap.parse_args()

    if args.alt and os.environ.get("DG_LIB_VARIANT") != "ab":
        raise SystemExit("--alt needs the A/B library build: make read_alt, then DG_LIB_VARIANT=ab")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("read_rate.py needs a GPU: there is nothing to time without one")
    import bench
    import __graft_entry__ as entry
    dg = entry._load_product()
    ctx = dg.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    only = [k for k in args.only.split(",") if k]
    results = [measure(nm, bench, dg, ctx, torch, stream, args.pairs, args.warmup, args.runs, only, args.alt)
               for nm in args.shapes.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "runs": args.runs, "results": results}
    out = args.append or args.out
    if args.append:
        doc = (json.load(open(out)) if os.path.exists(out) else []) + [doc]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
