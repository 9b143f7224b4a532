#!/usr/bin/env python3
"""One large delta consumed: the chunked index against the one-block index, and
the decode by tiles against the one-block decode.

Per size (MiB; default 64, 256 and 1024) one pair is made on the device: R is
random, V is R with 1 % of its bytes substituted (bench.py's C2 generator, laid
out back to back).  It is encoded as segments (256 KiB, window 0, onepass) and
spliced, so the input is the delta this project itself emits for a large pair.
Then, on the context's stream, timed with HIP events, medians:

  index      dg_read_plan_index against dg_read_plan_index_chunked (the default
             chunk size) on the same one-stream plan, alternating run by run;
             the chunked pass's stage times at chunks of 64 KiB, 256 KiB and
             1 MiB (a plan each); both passes' indexes compared once
             (dg_read_plan_index_get)
  read_4k    one 4 KiB read in the middle of V after each pass
  decode     the device part of dg_decode_large: the chunked index, V as tiles
             of 16, 64 and 256 KiB (dg_tile_requests), both CRCs
             (dg_crc64_xz_batch_device), against dg_decode_plan_run of the same
             stream as a one-stream plan (CRC checks on); the tiled output is
             compared with V once

The one-block paths take seconds on the larger sizes.  Their runs get a time
limit derived from the first size's row before a larger size is started
(milliseconds per stream megabyte, scaled) and are skipped where that estimate
is beyond --serial-limit seconds.

A last row (--batch) is bench.py's c6 batch, 1024 streams of about 216 KB,
under both index passes: many streams already fill the GPU with one block
each, so the one-block pass is expected to win there; the row says where the
crossover lies.

Every row runs in a child process of its own under a time limit; the first
failure stops the script.  Results go to --out as JSON
(profiles/index_rate.json is a recorded run).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIB = 1 << 20
BLOCK = 64 << 10   # the generator's pair length
CHUNKS = (64 << 10, 256 << 10, 1 << 20)
DEFAULT_CHUNK = int(re.search(r"#define DG_CHUNK_BYTES_DEFAULT (\d+)u", open(os.path.join(ROOT, "include", "delta_gpu.h")).read()).group(1))
TILES = (16 << 10, 64 << 10, 256 << 10)


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}


def load():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("index_rate.py needs a GPU: there is nothing to time without one")
    import __graft_entry__ as entry
    dg = entry._load_product()
    return torch, dg, dg.Context(0)


def timed(torch, ts, fn, warmup, runs):
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    out = []
    for it in range(warmup + runs):
        e0.record(ts)
        fn()
        e1.record(ts)
        ts.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def req_array(torch, dg, reqs):
    arr = (dg.ReadReq * max(len(reqs), 1))(*[dg.ReadReq(0, off, ln, 0, at) for off, ln, at in reqs])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def measure(mib, args):
    torch, dg, ctx = load()
    s = ctx.stream
    ts = torch.cuda.ExternalStream(s)
    L = mib * MIB
    ref = torch.empty(L, dtype=torch.uint8, device="cuda")
    ver = torch.empty(L, dtype=torch.uint8, device="cuda")
    ctx.check(dg.lib.dg_synth_edit_pairs_device(ctx.handle, ref.data_ptr(), ver.data_ptr(), L // BLOCK, BLOCK, 0x5E6000,
                                                BLOCK // 100, s), "synth")
    ts.synchronize()
    whole = (0, L, 0, L)
    segs, first = dg.segment_pairs(whole, args.segment, 0)
    enc = dg.EncodePlan(ctx, "onepass", segs)
    sp = dg.SplicePlan(ctx, [whole], first, for_plan=enc)
    n = len(segs)
    d_seg = torch.empty(enc.output_bound, dtype=torch.uint8, device="cuda")
    d_big = torch.zeros(sp.output_bound, dtype=torch.uint8, device="cuda")
    so = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ss = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    go, crc = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
    gs = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    span = (dg._lib.Span * 1)(dg._lib.Span(0, L))
    ctx.check(dg.lib.dg_crc64_xz_batch_device(ctx.handle, ref.data_ptr(), span, 1, crc.data_ptr(), s), "crc")
    enc.run(ref.data_ptr(), ver.data_ptr(), d_seg.data_ptr(), d_seg.numel(), so.data_ptr(), ss.data_ptr(), s)
    sp.run(d_seg.data_ptr(), so.data_ptr(), crc.data_ptr(), d_big.data_ptr(), d_big.numel(), go.data_ptr(), gs.data_ptr(),
           d_seg_status=ss.data_ptr(), stream=s)
    ts.synchronize()
    if int(ss.abs().sum()) != 0 or int(gs[0]) != 0:
        raise SystemExit(f"{mib} MiB: the chain failed: segments {ss.unique().tolist()}, splice {gs.tolist()}")
    size = int(go[1])
    delta = d_big[:size + 16].clone()
    enc.close()
    sp.close()
    del d_seg, d_big
    torch.cuda.synchronize()

    res = {"device": torch.cuda.get_device_name(0), "mib": mib, "segment_bytes": args.segment, "delta_bytes": size,
           "edits": "1 % substitutions", "chunk_bytes_default": DEFAULT_CHUNK}
    est = args.serial_ms_per_mb * size / 1e6 / 1e3 if args.serial_ms_per_mb else 0.0   # seconds per one-block run
    serial_ok = est <= args.serial_limit
    res["one_block_estimate_s"] = est
    tiles = {t: dg.tile_requests(L, t) for t in TILES}
    max_req = max(len(v) for v in tiles.values())
    stream_desc = [(0, L, 0, size)]
    sst = torch.full((1,), -1, dtype=torch.int32, device="cuda")

    # ── index ──
    plan = dg.ReadPlan(ctx, stream_desc, max_req)
    plan.chunk_index(0)
    plan.set_index_timing(1)
    t = {"serial": [], "chunked": []}
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    serial_runs = min(args.runs, args.serial_runs) if serial_ok else 0
    idx = {}
    for it in range(args.warmup + args.runs):   # alternating, so that both see the same machine
        if it >= args.warmup - 1 and it - args.warmup < serial_runs and serial_ok:   # one warm-up run of its own
            e0.record(ts)
            plan.index(delta.data_ptr(), sst.data_ptr(), stream=s)
            e1.record(ts)
            ts.synchronize()
            if it >= args.warmup:
                t["serial"].append(e0.elapsed_time(e1))
            if "serial" not in idx:
                idx["serial"] = (plan.index_get(0), int(sst[0]))
        e0.record(ts)
        plan.index_chunked(delta.data_ptr(), sst.data_ptr(), stream=s)
        e1.record(ts)
        ts.synchronize()
        if it >= args.warmup:
            t["chunked"].append(e0.elapsed_time(e1))
    idx["chunked"] = (plan.index_get(0), int(sst[0]))
    if idx["chunked"][1] != 0:
        raise SystemExit(f"{mib} MiB: the chunked index refused the stream: status {idx['chunked'][1]}")
    if "serial" in idx and idx["serial"] != idx["chunked"]:
        raise SystemExit(f"{mib} MiB: the two passes left different indexes")
    res["index"] = {"chunked": summary(t["chunked"]), "indexes_equal": "serial" in idx}
    if t["serial"]:
        res["index"]["one_block"] = summary(t["serial"])
        res["index"]["one_block_over_chunked_median"] = res["index"]["one_block"]["median_ms"] / res["index"]["chunked"]["median_ms"]
        res["one_block_index_ms_per_mb"] = res["index"]["one_block"]["median_ms"] / (size / 1e6)
    res["index"]["stages"] = {}
    for cb in CHUNKS:
        p = plan if cb == DEFAULT_CHUNK else dg.ReadPlan(ctx, stream_desc, 1)
        if p is not plan:
            p.chunk_index(cb)
        st = {k: [] for k in ("map", "resolve", "fill", "total")}
        p.set_index_timing(1)
        for it in range(args.warmup + args.runs):
            p.index_chunked(delta.data_ptr(), sst.data_ptr(), stream=s)
            ts.synchronize()
            if it >= args.warmup:
                for k, v in p.index_stage_times().items():
                    st[k].append(v)
        res["index"]["stages"][str(cb)] = {k: summary(v) for k, v in st.items()}
        if p is not plan:
            p.close()

    # ── one 4 KiB read after each pass ──
    out = torch.zeros(L + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(max_req, dtype=torch.int32, device="cuda")
    d_st = torch.full((max_req,), -1, dtype=torch.int32, device="cuda")
    one = req_array(torch, dg, [(L // 2 + 1000, 4096, 0)])
    res["read_4k"] = {}
    for name in (["one_block"] if serial_ok else []) + ["chunked"]:
        (plan.index if name == "one_block" else plan.index_chunked)(delta.data_ptr(), sst.data_ptr(), stream=s)
        v = timed(torch, ts, lambda: plan.run(ref.data_ptr(), delta.data_ptr(), one.data_ptr(), 1, out.data_ptr(),
                                              d_len.data_ptr(), d_st.data_ptr(), s), args.warmup, args.runs)
        if int(d_st[0]) != 0 or not torch.equal(out[:4096], ver[L // 2 + 1000:L // 2 + 1000 + 4096]):
            raise SystemExit(f"{mib} MiB: the 4 KiB read after the {name} pass is wrong")
        res["read_4k"][name] = summary(v)

    # ── decode ──
    crc2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    span_v = (dg._lib.Span * 1)(dg._lib.Span(0, L))
    res["decode"] = {"tiles": {}}
    for tb in TILES:
        rq = req_array(torch, dg, tiles[tb])
        m = len(tiles[tb])

        def tiled():
            plan.index_chunked(delta.data_ptr(), sst.data_ptr(), stream=s)
            plan.run(ref.data_ptr(), delta.data_ptr(), rq.data_ptr(), m, out.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), s)
            ctx.check(dg.lib.dg_crc64_xz_batch_device(ctx.handle, ref.data_ptr(), span, 1, crc2.data_ptr(), s), "crc")
            ctx.check(dg.lib.dg_crc64_xz_batch_device(ctx.handle, out.data_ptr(), span_v, 1, crc2.data_ptr() + 8, s), "crc")

        out.zero_()
        torch.cuda.synchronize()
        v = timed(torch, ts, tiled, args.warmup, args.runs)
        if int(d_st[:m].abs().sum()) != 0 or not torch.equal(out[:L], ver):
            raise SystemExit(f"{mib} MiB: tiles of {tb} bytes do not give V")
        hdr = bytes(delta[:25].cpu().numpy())
        want = [int.from_bytes(hdr[9:17], "big"), int.from_bytes(hdr[17:25], "big")]
        if [x & (2 ** 64 - 1) for x in crc2.cpu().tolist()] != want:
            raise SystemExit(f"{mib} MiB: the CRCs of R and of the tiled output are not the header's")
        res["decode"]["tiles"][str(tb)] = summary(v)
    if serial_ok:
        dec = dg.DecodePlan(ctx, [(0, L, 0, size, 0, L)])
        vlen = torch.zeros(1, dtype=torch.int64, device="cuda")
        ds = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        out.zero_()
        torch.cuda.synchronize()
        v = timed(torch, ts, lambda: dec.run(ref.data_ptr(), delta.data_ptr(), out.data_ptr(), vlen.data_ptr(), ds.data_ptr(), s),
                  1, min(args.runs, args.serial_runs))
        if int(ds[0]) != 0 or not torch.equal(out[:L], ver):
            raise SystemExit(f"{mib} MiB: the one-block decode failed: status {ds.tolist()}")
        res["decode"]["one_block"] = summary(v)
        best = min(x["median_ms"] for x in res["decode"]["tiles"].values())
        res["decode"]["one_block_over_best_tiles_median"] = res["decode"]["one_block"]["median_ms"] / best
    return res


def measure_batch(args):
    """bench.py's c6 batch under both index passes."""
    torch, dg, ctx = load()
    import bench
    stream = torch.cuda.ExternalStream(ctx.stream)
    s = ctx.stream
    npg, L, rate, q, seed_base, desc, algo = bench.CONFIGS["c6"]
    n = args.batch_pairs or npg
    ref, ver, layout = bench.make_inputs(dg, ctx, torch, "c6", 0, n, stream)
    torch.cuda.synchronize()
    enc = dg.EncodePlan(ctx, algo, layout, q=q)
    d_a = torch.empty(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    enc.run(ref.data_ptr(), ver.data_ptr(), d_a.data_ptr(), d_a.numel(), off.data_ptr(), st.data_ptr(), s)
    torch.cuda.synchronize()
    if int(st.abs().sum()) != 0:
        raise SystemExit(f"c6: encode failed: status {st.unique().tolist()}")
    offs = off.cpu().tolist()
    streams = [(ro, rl, offs[i], offs[i + 1] - offs[i]) for i, (ro, rl, _, _) in enumerate(layout)]
    sst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    plan = dg.ReadPlan(ctx, streams, 1)
    plan.chunk_index(0)
    res = {"device": torch.cuda.get_device_name(0), "shape": "c6", "streams": n, "delta_bytes": offs[-1], "index": {}}
    got = {}
    for name, fn in (("one_block", plan.index), ("chunked", plan.index_chunked)):
        v = timed(torch, stream, lambda: fn(d_a.data_ptr(), sst.data_ptr(), stream=s), args.warmup, args.runs)
        if int(sst.abs().sum()) != 0:
            raise SystemExit(f"c6: the {name} pass refused a stream")
        got[name] = [plan.index_get(i) for i in range(0, n, 37)]
        res["index"][name] = summary(v)
    if got["one_block"] != got["chunked"]:
        raise SystemExit("c6: the two passes left different indexes")
    res["index"]["one_block_over_chunked_median"] = res["index"]["one_block"]["median_ms"] / res["index"]["chunked"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="64,256,1024", help="pair sizes in MiB")
    ap.add_argument("--segment", type=int, default=256 << 10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--serial-runs", type=int, default=3, help="timed runs of the one-block paths")
    ap.add_argument("--serial-limit", type=float, default=60.0,
                    help="skip a size's one-block runs when one is estimated to take longer than this many seconds")
    ap.add_argument("--serial-ms-per-mb", type=float, default=0.0, help=argparse.SUPPRESS)   # the child's: from the first size
    ap.add_argument("--batch", type=int, default=1, help="1: also the c6 batch row")
    ap.add_argument("--batch-pairs", type=int, default=0)
    ap.add_argument("--limit", type=int, default=280, help="seconds each row's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_rate.json"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)   # the child: one size, its JSON on stdout
    ap.add_argument("--one-batch", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        print("RESULT " + json.dumps(measure(args.one, args)))
        return
    if args.one_batch:
        print("RESULT " + json.dumps(measure_batch(args)))
        return
    results = []
    per_mb = 0.0
    jobs = [["--one", x] for x in args.sizes.split(",") if x] + ([["--one-batch", "1"]] if args.batch else [])
    for job in jobs:
        cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + job + ["--serial-ms-per-mb", repr(per_mb)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"{' '.join(job)} failed (exit {p.returncode}): stopping here")
        results.append(json.loads(line[0][7:]))
        print(json.dumps(results[-1]), flush=True)
        if not per_mb:   # the first size's one-block rate bounds the larger sizes' runs
            per_mb = max(results[-1].get("one_block_index_ms_per_mb", 0.0),
                         results[-1].get("decode", {}).get("one_block", {}).get("median_ms", 0.0) / (results[-1]["delta_bytes"] / 1e6))
        if len(results) > 1:
            results[-1].pop("device")
    doc = {"device": results[0].pop("device"), "warmup": args.warmup, "runs": args.runs, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
