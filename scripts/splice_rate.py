#!/usr/bin/env python3
"""One large pair as segments: encode + splice against the one-pair encode.

Per size (MiB; default 64, 256 and 1024) one pair is made on the device: R is
random, V is R with 1 % of its bytes substituted (bench.py's C2 generator, laid
out back to back, so every 64 KiB of the pair has its share of edits).  Then,
alternating run by run on the context's stream, timed with HIP events:

  segmented  dg_encode_plan_run over dg_segment_pairs' segments (1 MiB segments,
             1 MiB windows, onepass) followed by dg_splice_plan_run: one event
             pair around both, the encode plan's and the splice plan's own
             stage times beside it
  one_pair   the same pair as ONE pair of an ordinary encode plan, the only way
             without the splice (sizes up to --one-pair-max MiB; in its automatic
             mode a large onepass pair on its diagonal runs through verified
             members on many waves, any other pair on one wave)

After the sizes come further sets (--extras): every size again with a window
of 0 bytes, where segment j is encoded against R's own segment j and the pairs
lie on their diagonals; the same with 256 KiB segments; a 16 MiB pair with
4 KiB inserted into V, where the one-pair encode leaves its diagonal; and the
first size with the correcting encoder, which gives one wave to a pair.

The spliced delta is decoded once on the device with both CRC checks on.  For
the sizes in --ref-sizes the reference's own whole-pair onepass delta
(oracle/_ref, same table size) is made on the CPU and the spliced size is
given over its size: the price of matching only inside a segment's window.

Every size runs in a child process of its own under a time limit; the first
failure stops the script.  Medians of the timed runs go to --out as JSON
(profiles/splice_rate.json is a recorded run).  No threshold is attached.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MIB = 1 << 20
BLOCK = 64 << 10   # the generator's pair length


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}


def measure(mib, args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("splice_rate.py needs a GPU: there is nothing to time without one")
    import __graft_entry__ as entry
    dg = entry._load_product()
    ctx = dg.Context(0)
    s = ctx.stream
    ts = torch.cuda.ExternalStream(s)
    L = mib * MIB
    ref = torch.empty(L, dtype=torch.uint8, device="cuda")
    ver = torch.empty(L, dtype=torch.uint8, device="cuda")
    ctx.check(dg.lib.dg_synth_edit_pairs_device(ctx.handle, ref.data_ptr(), ver.data_ptr(), L // BLOCK, BLOCK, 0x5E6000,
                                                BLOCK // 100, s), "synth")
    ts.synchronize()
    Lv = L
    if args.drift:   # an insertion at an eighth of V: everything after it leaves the diagonal
        ins = torch.randint(0, 256, (args.drift,), dtype=torch.uint8, device="cuda")
        ver = torch.cat([ver[:L // 8], ins, ver[L // 8:]])
        Lv = L + args.drift
        torch.cuda.synchronize()
    whole = (0, L, 0, Lv)
    segs, first = dg.segment_pairs(whole, args.segment, args.window)
    enc = dg.EncodePlan(ctx, args.algorithm, segs)
    sp = dg.SplicePlan(ctx, [whole], first, for_plan=enc)
    n = len(segs)
    d_seg = torch.empty(enc.output_bound, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(sp.output_bound, dtype=torch.uint8, device="cuda")
    so = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ss = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    go, crc, vlen = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(3))
    gs, ds = (torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    span = (dg._lib.Span * 1)(dg._lib.Span(0, L))
    ctx.check(dg.lib.dg_crc64_xz_batch_device(ctx.handle, ref.data_ptr(), span, 1, crc.data_ptr(), s), "crc")
    e0, e1, b0, b1 = (torch.cuda.Event(enable_timing=True) for _ in range(4))

    def segmented():
        e0.record(ts)
        enc.run(ref.data_ptr(), ver.data_ptr(), d_seg.data_ptr(), d_seg.numel(), so.data_ptr(), ss.data_ptr(), s)
        sp.run(d_seg.data_ptr(), so.data_ptr(), crc.data_ptr(), d_out.data_ptr(), d_out.numel(), go.data_ptr(), gs.data_ptr(),
               d_seg_status=ss.data_ptr(), stream=s)
        e1.record(ts)

    # one checked run: the spliced delta decodes to V with both CRC checks on
    segmented()
    ts.synchronize()
    if int(ss.abs().sum()) != 0 or int(gs[0]) != 0:
        raise SystemExit(f"{mib} MiB: the chain failed: segments {ss.unique().tolist()}, splice {gs.tolist()}")
    size = int(go[1])
    dec = dg.DecodePlan(ctx, [(0, L, 0, size, 0, Lv)])
    chk = torch.zeros(Lv, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dec.run(ref.data_ptr(), d_out.data_ptr(), chk.data_ptr(), vlen.data_ptr(), ds.data_ptr(), s)
    ts.synchronize()
    if int(ds[0]) != 0 or not torch.equal(chk, ver):
        raise SystemExit(f"{mib} MiB: the spliced delta does not decode to V: status {ds.tolist()}")
    dec.close()
    del chk

    one = None
    if mib <= args.one_pair_max:
        one = dg.EncodePlan(ctx, args.algorithm, [whole])
        d_one = torch.empty(one.output_bound, dtype=torch.uint8, device="cuda")
        oo = torch.zeros(2, dtype=torch.int64, device="cuda")
        os_ = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def one_pair():
            b0.record(ts)
            one.run(ref.data_ptr(), ver.data_ptr(), d_one.data_ptr(), d_one.numel(), oo.data_ptr(), os_.data_ptr(), s)
            b1.record(ts)

    enc.set_timing(1)
    sp.set_timing(1)
    t = {"chain": [], "encode": [], "map": [], "resolve": [], "scan": [], "emit": [], "total": [], "one_pair": []}
    for it in range(args.warmup + args.runs):   # alternating, so that both see the same machine
        segmented()
        ts.synchronize()
        tc, te = sp.stage_times(), enc.stage_times()
        if one is not None and args.warmup - 1 <= it < args.warmup + args.one_pair_runs:   # one warm-up run of its own
            one_pair()
            ts.synchronize()
            if int(os_[0]) != 0:
                raise SystemExit(f"{mib} MiB: the one-pair encode failed: status {os_.tolist()}")
            if it >= args.warmup:
                t["one_pair"].append(b0.elapsed_time(b1))
        if it >= args.warmup:
            t["chain"].append(e0.elapsed_time(e1))
            t["encode"].append(te["total"])
            for k in ("map", "resolve", "scan", "emit", "total"):
                t[k].append(tc[k])
    res = {"device": torch.cuda.get_device_name(0), "mib": mib, "segments": n, "segment_bytes": args.segment, "window_bytes": args.window,
           "drift_bytes": args.drift, "algorithm": args.algorithm, "edits": "1 % substitutions", "spliced_bytes": size, "segment_delta_bytes": int(so[-1]),
           "segmented_chain": summary(t["chain"]), "encode_plan_total": summary(t["encode"]),
           "splice": {k: summary(t[k]) for k in ("map", "resolve", "scan", "emit", "total")}}
    res["chain_gib_per_s"] = (Lv / (1 << 30)) / (res["segmented_chain"]["median_ms"] / 1e3)
    if t["one_pair"]:
        res["one_pair"] = summary(t["one_pair"])
        res["one_pair_bytes"] = int(oo[1])
        res["one_pair_members_mode"] = bool(one.members)
        res["one_pair_over_chain_median"] = res["one_pair"]["median_ms"] / res["segmented_chain"]["median_ms"]
    if mib in args.ref_sizes and args.algorithm == "onepass" and not args.drift:
        import oracle as O
        if O.reference_available():
            R, V = bytes(ref.cpu().numpy()), bytes(ver.cpu().numpy())
            res["reference_whole_pair_bytes"] = len(O.Reference().encode(O.ONEPASS, R, V))
            res["spliced_over_reference_bytes"] = size / res["reference_whole_pair_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="64,256,1024", help="pair sizes in MiB")
    ap.add_argument("--segment", type=int, default=MIB)
    ap.add_argument("--window", type=int, default=MIB)
    ap.add_argument("--algorithm", default="onepass")
    ap.add_argument("--extras", default="window0,small,drift,correcting",
                    help="further sets after the sizes: window0 = every size again with a window of 0 bytes (segment j "
                         "against R's own segment j: the pairs lie on their diagonals), small = the same with segments of a quarter the size, drift = a "
                         "pair of --drift-mib with --drift-bytes random bytes inserted into V (the one-pair encode leaves "
                         "its diagonal), correcting = the first size with the correcting encoder")
    ap.add_argument("--drift-bytes", type=int, default=4096)
    ap.add_argument("--drift-mib", type=int, default=16)
    ap.add_argument("--drift", type=int, default=0, help=argparse.SUPPRESS)   # the child's
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--one-pair-max", type=int, default=1024, help="largest size (MiB) also encoded as one pair")
    ap.add_argument("--one-pair-runs", type=int, default=3, help="timed runs of the one-pair encode")
    ap.add_argument("--ref-sizes", default="64", help="sizes (MiB) whose reference whole-pair delta is made on the CPU")
    ap.add_argument("--limit", type=int, default=280, help="seconds each size's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_rate.json"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)   # the child: one size, its JSON on stdout
    args = ap.parse_args()
    args.ref_sizes = [int(x) for x in args.ref_sizes.split(",") if x]
    if args.one:
        print("RESULT " + json.dumps(measure(args.one, args)))
        return
    results = []
    sizes = [int(x) for x in args.sizes.split(",")]
    jobs = [(mib, args.segment, args.window, 0, args.algorithm) for mib in sizes]
    extras = [x for x in args.extras.split(",") if x]
    if "window0" in extras:
        jobs += [(mib, args.segment, 0, 0, args.algorithm) for mib in sizes]
    if "small" in extras:
        jobs += [(mib, args.segment // 4, 0, 0, args.algorithm) for mib in sizes]
    if "drift" in extras:
        jobs.append((args.drift_mib, args.segment, args.window, args.drift_bytes, args.algorithm))
    if "correcting" in extras:
        jobs.append((sizes[0], args.segment, args.window, 0, "correcting"))
    for mib, segment, window, drift, algo in jobs:
        cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + [
            "--one", str(mib), "--segment", str(segment), "--window", str(window), "--drift", str(drift), "--algorithm", algo]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"{mib} MiB (window {window}, drift {drift}) failed (exit {p.returncode}): stopping here")
        results.append(json.loads(line[0][7:]))
        print(json.dumps(results[-1]), flush=True)
        if len(results) > 1:
            results[-1].pop("device")
    doc = {"device": results[0].pop("device"), "warmup": args.warmup, "runs": args.runs, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
