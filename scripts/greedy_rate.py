#!/usr/bin/env python3
"""One recorded run of the greedy encoder on the benchmark's inputs (not a gate).

Two batches from the device generators bench.py uses: the C2 batch (4096 x
64 KiB pairs, 1 % edits) and a 256-pair C4-shaped batch (~256 KiB pairs, 8-64
block transpositions), p = 16.  A greedy plan is warmed up, then timed over
--steps runs between two device synchronisations, with the plan's stage timing
(greedy_build, greedy_scan) averaged over the same runs.  Written to
profiles/greedy_rate.json:

  gib_s              sum(|R| + |V|) of the batch per step time
  ms_per_step, stages_ms
  index_bytes_per_pair   4 (B + 1) + 8 S for S = |R| - p + 1 seeds, B = S rounded
                         up to a power of two (include/delta_gpu.h), mean over the batch
  delta_bytes        total delta bytes of the batch: greedy, greedy --splay,
                     onepass and correcting (the benchmark's --table-size) on the same pairs
  ref_single_thread_gib_s   the reference's own greedy (oracle/_ref, where it is
                     built) on the first 64 pairs, one thread, for scale

usage: python scripts/greedy_rate.py [--steps 10] [--warmup 3] [--c2-pairs 4096] [--c4-pairs 256]
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


def index_bytes(r_len):
    seeds = r_len - P + 1 if r_len >= P else 0
    nb = 1
    while nb < seeds:
        nb <<= 1
    return 4 * (nb + 1) + 8 * seeds


def run_plan(torch, ctx, plan, ref, ver, steps, warmup, timing):
    n = plan.n
    out = torch.empty(plan.output_bound, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")

    def step():
        plan.run(ref.data_ptr(), ver.data_ptr(), out.data_ptr(), out.numel(), offs.data_ptr(), st.data_ptr(),
                 ctx.stream)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if timing:
        plan.set_timing(steps)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    if int(st.abs().sum()) != 0:
        raise RuntimeError("a pair failed: status " + str(st[st != 0][:8].tolist()))
    return ms, int(offs[-1]), (plan.stage_times() if timing else {})


def measure(dg, torch, ctx, name, n, steps, warmup):
    from bench import CONFIGS, make_inputs
    stream = torch.cuda.current_stream()
    ref, ver, layout = make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    in_bytes = sum(rl + vl for _, rl, _, vl in layout)
    res = {"pairs": n, "input_bytes": in_bytes, "p": P,
           "index_bytes_per_pair": round(sum(index_bytes(rl) for _, rl, _, _ in layout) / n)}
    plan = dg.EncodePlan(ctx, "greedy", layout, p=P)
    ms, total, stages = run_plan(torch, ctx, plan, ref, ver, steps, warmup, True)
    plan.close()
    res["ms_per_step"] = round(ms, 4)
    res["gib_s"] = round(in_bytes / (ms * 1e-3) / 2**30, 3)
    res["stages_ms"] = {k: round(v, 4) for k, v in stages.items()}
    res["delta_bytes"] = {"greedy": total}
    q = CONFIGS[name][3]
    for key, algo, kw in (("greedy_splay", "greedy", {"splay": True}), ("onepass", "onepass", {"q": q}),
                          ("correcting", "correcting", {"q": q})):
        plan = dg.EncodePlan(ctx, algo, layout, p=P, **kw)
        res["delta_bytes"][key] = run_plan(torch, ctx, plan, ref, ver, 1, 0, False)[1]
        plan.close()
    import oracle as O
    if O.reference_available():
        r = O.Reference()
        m = min(n, 64)
        refc, verc = ref.cpu().numpy(), ver.cpu().numpy()
        pairs = [(bytes(refc[ro:ro + rl]), bytes(verc[vo:vo + vl])) for ro, rl, vo, vl in layout[:m]]
        t0 = time.perf_counter()
        for R, V in pairs:
            r.encode(0, R, V, p=P)
        dt = time.perf_counter() - t0
        res["ref_single_thread_gib_s"] = round(sum(len(R) + len(V) for R, V in pairs) / dt / 2**30, 4)
        res["ref_pairs"] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c2-pairs", type=int, default=4096)
    ap.add_argument("--c4-pairs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_rate.json"))
    args = ap.parse_args()
    import torch
    from bench import load_product
    if not torch.cuda.is_available():
        sys.exit("greedy_rate.py: no GPU")
    dg = load_product()
    ctx = dg.Context(0)
    out = {"note": "one run on one MI355X; host clock around `steps` plan runs between device synchronisations",
           "steps": args.steps, "warmup": args.warmup,
           "c2": measure(dg, torch, ctx, "c2", args.c2_pairs, args.steps, args.warmup),
           "c4_256": measure(dg, torch, ctx, "c4", args.c4_pairs, args.steps, args.warmup)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
