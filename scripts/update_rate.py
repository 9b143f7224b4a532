#!/usr/bin/env python3
"""In-place update against decode on the same in-place deltas, in one process.

At the C5 shape (1024 x 64 KiB pairs, 1 % edits) and the C5o shape (1024
transposition pairs of ~256 KiB), both from bench.py's input makers, the
in-place deltas (localmin) are made on the device (EncodePlan -> InplacePlan).
Then, alternating run by run:

  decode  dg_decode_plan_run: reference arena + output arena, HIP-event stage "decode"
  update  dg_update_plan_run: one arena that holds R and then V, HIP-event stage
          "update"; the buffers are restored by an untimed device copy before
          every run

20 warm-up and 100 timed runs of each (--warmup / --runs); median, minimum and
maximum of both, and the device memory each path needs for the batch, go to
--out as JSON (profiles/update_rate.json is a recorded run).  "Slower" counts
only beyond decode's own spread in the same session.

--phases: instead of timing, the per-phase cycles of both kernels from the
profiling builds (`make -C delta-compression_amd update_prof`; run with
DG_LIB_VARIANT=prof DG_UPDATE_HSACO=dg_update_prof.hsaco): s_memtime ticks per
stream, averaged over 20 runs, to --out (profiles/update_phases.json).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


DEC_PHASES = ["fill", "load", "n1", "dbl", "walk", "exp", "hdr", "copy", "wait", "windows", "batches", "total",
              "ordered", "c_cmd", "c_flat", "c_bar", "crc_sync", "crc_seg", "crc_tail"]
UPD_PHASES = ["a_parse", "a_crc", "b_zero", "b_parse", "b_apply", "c_crc", "total", "blocks"]


def phase_cycles(dg, torch, n, decode, update, uplan, reps=20):
    """Ticks per stream of each phase (thread 0's clock reads, summed over blocks by the profiling kernels)."""
    import ctypes as C
    lib = dg.lib
    lib.dg_update_plan_prof.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    lib.dg_decode_prof_read.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    if lib.dg_update_plan_prof(uplan.handle, None, 0) != 0 or lib.dg_decode_prof_reset() != 0:
        raise SystemExit("the phase counters need the profiling builds (see --help)")
    for _ in range(reps):
        decode()
    torch.cuda.synchronize()
    dv = (C.c_ulonglong * len(DEC_PHASES))()
    assert lib.dg_decode_prof_read(dv, len(DEC_PHASES)) == len(DEC_PHASES)
    for _ in range(reps):
        update()
    torch.cuda.synchronize()
    uv = (C.c_ulonglong * len(UPD_PHASES))()
    assert lib.dg_update_plan_prof(uplan.handle, uv, len(UPD_PHASES)) == len(UPD_PHASES)
    if uv[UPD_PHASES.index("blocks")] != reps * n:
        raise SystemExit("the update kernel wrote no phase cycles: DG_UPDATE_HSACO=dg_update_prof.hsaco?")
    per = reps * n
    dec = {k: dv[i] / per for i, k in enumerate(DEC_PHASES)}
    dec["parse"] = sum(dec[k] for k in ("load", "n1", "dbl", "walk", "exp", "hdr"))
    dec["crc"] = dec["crc_sync"] + dec["crc_seg"] + dec["crc_tail"]
    return {"decode": dec, "update": {k: uv[i] / per for i, k in enumerate(UPD_PHASES) if k != "blocks"}}


def measure(name, bench, dg, ctx, torch, stream, pairs, warmup, runs, phases=False):
    npg, L, rate, q, seed_base, desc, _ = bench.CONFIGS[name]
    n = pairs or npg
    ref, ver, layout = bench.make_inputs(dg, ctx, torch, name, 0, n, stream)
    enc = dg.EncodePlan(ctx, "onepass" if rate >= 0 else "correcting", layout, q=q)
    ip = dg.InplacePlan(ctx, policy="localmin", for_plan=enc)
    d_std = torch.empty(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    d_ipd = torch.empty(max(ip.output_bound, 1), dtype=torch.uint8, device="cuda")
    off1, off2 = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    st1, st2 = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    s = stream.cuda_stream
    enc.run(ref.data_ptr(), ver.data_ptr(), d_std.data_ptr(), d_std.numel(), off1.data_ptr(), st1.data_ptr(), s)
    ip.run(ref.data_ptr(), d_std.data_ptr(), d_ipd.data_ptr(), d_ipd.numel(), off2.data_ptr(), st2.data_ptr(),
           d_delta_offsets=off1.data_ptr(), d_delta_status=st1.data_ptr(), stream=s)
    torch.cuda.synchronize()
    if int(st2.abs().sum()) != 0:
        raise SystemExit(f"{name}: making the in-place deltas failed: status {st2.unique().tolist()}")
    o = off2.cpu().tolist()
    delta = d_ipd[:o[-1]].clone()
    enc.close()
    ip.close()
    del d_std, d_ipd

    # decode: R arena + output arena (output i at V's arena offset, room for max(|R|, |V|))
    ddesc = [(ro, rl, o[i], o[i + 1] - o[i], vo, max(rl, vl)) for i, (ro, rl, vo, vl) in enumerate(layout)]
    dplan = dg.DecodePlan(ctx, ddesc)
    out = torch.zeros(max(max(d[4] + d[5] for d in ddesc), ver.numel()), dtype=torch.uint8, device="cuda")
    # update: one arena, buffer i of max(|R|, |V|) bytes at a 16-byte aligned offset, holding R_i
    udesc, pos = [], 0
    for i, (ro, rl, vo, vl) in enumerate(layout):
        cap = max(rl, vl)
        udesc.append((pos, cap, rl, o[i], o[i + 1] - o[i]))
        pos = (pos + cap + 15) // 16 * 16
    uplan = dg.UpdatePlan(ctx, udesc)
    master = torch.zeros(max(pos, 1), dtype=torch.uint8, device="cuda")
    for (bo, _, rl, _, _), (ro, _, _, _) in zip(udesc, layout):
        master[bo:bo + rl] = ref[ro:ro + rl]
    buf = torch.empty_like(master)
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    ts = torch.cuda.ExternalStream(s)

    def decode():
        dplan.run(ref.data_ptr(), delta.data_ptr(), out.data_ptr(), lens.data_ptr(), status.data_ptr(), s)

    def update():
        with torch.cuda.stream(ts):
            buf.copy_(master)   # untimed: the events are around the kernel
        uplan.run(buf.data_ptr(), delta.data_ptr(), lens.data_ptr(), status.data_ptr(), stream=s)

    # one checked run of each
    torch.cuda.synchronize()
    decode()
    torch.cuda.synchronize()
    ok = int(status.abs().sum()) == 0 and all(
        torch.equal(out[vo:vo + vl], ver[vo:vo + vl]) for _, _, vo, vl in layout[:: max(n // 64, 1)])
    if not ok:
        raise SystemExit(f"{name}: decode failed: status {status.unique().tolist()}")
    update()
    torch.cuda.synchronize()
    ok = int(status.abs().sum()) == 0 and all(
        torch.equal(buf[bo:bo + vl], ver[vo:vo + vl]) for (bo, _, _, _, _), (_, _, vo, vl) in zip(udesc, layout))
    if not ok:
        raise SystemExit(f"{name}: update failed: status {status.unique().tolist()}")

    if phases:
        res = {"name": name, "streams": n, "unit": "s_memtime ticks per stream", **phase_cycles(dg, torch, n, decode, update, uplan)}
        dplan.close()
        uplan.close()
        return res
    dplan.set_timing(1)
    uplan.set_timing(1)
    t = {"decode": [], "update": []}
    for it in range(warmup + runs):   # alternating, so that both see the same machine
        decode()
        torch.cuda.synchronize()
        td = dplan.stage_times()["decode"]
        update()
        torch.cuda.synchronize()
        tu = uplan.stage_times()["update"]
        if it >= warmup:
            t["decode"].append(td)
            t["update"].append(tu)

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}

    res = {"name": name, "workload": desc, "streams": n, "delta_bytes": o[-1],
           "r_bytes": sum(x[1] for x in layout), "v_bytes": sum(x[3] for x in layout),
           "decode": summary(t["decode"]), "update": summary(t["update"]),
           # the arenas a caller must hold for the batch, the deltas aside
           "device_bytes": {"decode_ref_plus_out": ref.numel() + out.numel(), "update_buf": buf.numel()}}
    d, u = res["decode"], res["update"]
    res["update_over_decode_median"] = u["median_ms"] / d["median_ms"]
    res["update_slower_beyond_decode_spread"] = u["median_ms"] > d["max_ms"]
    dplan.close()
    uplan.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c5,c5o")
    ap.add_argument("--pairs", type=int, default=0, help="streams per shape (0: the shape's own 1024)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--out", default=None, help="default: profiles/update_rate.json (--phases: update_phases.json)")
    ap.add_argument("--phases", action="store_true", help="phase cycles from the profiling builds instead of times")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "update_phases.json" if args.phases else "update_rate.json")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("update_rate.py needs a GPU: there is nothing to time without one")
    import bench
    import __graft_entry__ as entry
    dg = entry._load_product()
    ctx = dg.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    results = [measure(nm, bench, dg, ctx, torch, stream, args.pairs, args.warmup, args.runs, args.phases)
               for nm in args.shapes.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "runs": args.runs, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        if args.phases:
            print(json.dumps(r))
            continue
        print(json.dumps({k: r[k] for k in ("name", "decode", "update", "update_over_decode_median",
                                            "update_slower_beyond_decode_spread", "device_bytes")}))


if __name__ == "__main__":
    main()
