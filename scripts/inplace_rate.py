#!/usr/bin/env python3
"""One recorded run of the device in-place conversion (not a gate).

Two batches from the device generators bench.py uses: the C2 shape (4096 x
64 KiB pairs, 1 % edits, onepass at --table-size 4099) and 256 C4 transposition
pairs (~256 KiB, correcting, --table-size 1), p = 16.  Each batch is encoded
once by an encode plan; an in-place plan made from it (dg_inplace_plan_create_for)
then converts the packed standard deltas, for both cycle policies, warmed up
and timed over --steps runs between two device synchronisations, with the
plan's stage timing averaged over the same runs.  Written to
profiles/inplace_rate.json, per shape and policy:

  ms_per_run, stages_ms    ("order", "scan", "emit", "total")
  deltas_per_s
  copies, victims          COPY commands of the batch, and those converted to ADDs
  host_single_thread_us_per_delta   dg_make_inplace (the host converter, one
                           thread) over the first 64 of the same deltas
  host_16_threads_us_per_delta      that divided by 16: a run on these machines
                           may use 16 CPUs, so this is the figure to beat
  device_us_per_delta, speedup_vs_host_16

usage: python scripts/inplace_rate.py [--steps 10] [--warmup 3] [--c2-pairs 4096] [--c4-pairs 256]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

P = 16
HOST_DELTAS = 64


def measure(dg, torch, ctx, name, algo, q, n, steps, warmup):
    from bench import make_inputs
    stream = torch.cuda.current_stream()
    ref, ver, layout = make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    enc = dg.EncodePlan(ctx, algo, layout, p=P, q=q)
    std = torch.empty(enc.output_bound, dtype=torch.uint8, device="cuda")
    off1 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st1 = torch.empty(n, dtype=torch.int32, device="cuda")
    enc.run(ref.data_ptr(), ver.data_ptr(), std.data_ptr(), std.numel(), off1.data_ptr(), st1.data_ptr(), ctx.stream)
    torch.cuda.synchronize()
    if int(st1.abs().sum()) != 0:
        raise RuntimeError("an encode failed")
    o1 = off1.cpu().tolist()
    m = min(n, HOST_DELTAS)
    refc, stdc = ref.cpu().numpy(), std[:o1[m]].cpu().numpy()
    host_items = [(bytes(refc[layout[i][0]:layout[i][0] + layout[i][1]]), bytes(stdc[o1[i]:o1[i + 1]])) for i in range(m)]
    res = {"pairs": n, "algorithm": algo, "q": q, "p": P, "standard_delta_bytes": o1[n], "policies": {}}
    for policy in ("localmin", "constant"):
        ip = dg.InplacePlan(ctx, policy=policy, for_plan=enc)
        out = torch.empty(ip.output_bound, dtype=torch.uint8, device="cuda")
        off2 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        st2 = torch.empty(n, dtype=torch.int32, device="cuda")

        def step():
            ip.run(ref.data_ptr(), std.data_ptr(), out.data_ptr(), out.numel(), off2.data_ptr(), st2.data_ptr(),
                   d_delta_offsets=off1.data_ptr(), d_delta_status=st1.data_ptr(), stream=ctx.stream)

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        ip.set_timing(steps)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        if int(st2.abs().sum()) != 0:
            raise RuntimeError("a conversion failed: status " + str(st2[st2 != 0][:8].tolist()))
        stages = ip.stage_times()
        o2 = off2.cpu().tolist()
        outc = out[:o2[m]].cpu().numpy()
        # the host converter on the first deltas: the comparator and the clock to beat
        t0 = time.perf_counter()
        host = [dg.make_inplace(R, d, policy, stats=True) for R, d in host_items]
        host_us = (time.perf_counter() - t0) * 1e6 / m
        for i, (h, _) in enumerate(host):
            if bytes(outc[o2[i]:o2[i + 1]]) != h:
                raise RuntimeError(f"{name} {policy}: delta {i} differs from dg_make_inplace")
        dev_us = ms * 1e3 / n
        res["policies"][policy] = {
            "ms_per_run": round(ms, 4), "stages_ms": {k: round(v, 4) for k, v in stages.items()},
            "deltas_per_s": round(n / (ms * 1e-3)), "inplace_delta_bytes": o2[n],
            "first_deltas": {"n": m, "copies_kept": sum(s["num_copies"] for _, s in host),
                             "adds": sum(s["num_adds"] for _, s in host)},
            "host_single_thread_us_per_delta": round(host_us, 2),
            "host_16_threads_us_per_delta": round(host_us / 16, 2),
            "device_us_per_delta": round(dev_us, 3),
            "speedup_vs_host_16": round(host_us / 16 / dev_us, 2)}
        ip.close()
    enc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c2-pairs", type=int, default=4096)
    ap.add_argument("--c4-pairs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inplace_rate.json"))
    args = ap.parse_args()
    import torch
    from bench import load_product
    if not torch.cuda.is_available():
        sys.exit("inplace_rate.py: no GPU")
    dg = load_product()
    ctx = dg.Context(0)
    out = {"note": "one run on one MI355X; host clock around `steps` plan runs between device synchronisations; "
                   "the host figures are dg_make_inplace on one thread over the first 64 deltas of the batch",
           "steps": args.steps, "warmup": args.warmup,
           "c2": measure(dg, torch, ctx, "c2", "onepass", 4099, args.c2_pairs, args.steps, args.warmup),
           "c4_256": measure(dg, torch, ctx, "c4", "correcting", 1, args.c4_pairs, args.steps, args.warmup)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
