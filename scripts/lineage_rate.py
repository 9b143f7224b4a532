#!/usr/bin/env python3
"""Lineage reads on the device against what a caller had before them, in one
process.

Per shape, n lineages of depth 16 are made on the device: V0 and V1 from
bench.py's input maker, every further version the one before it with 1 %
further substitutions (torch); every level's deltas are encoded on the device
(onepass) and all of them sit in one delta arena as the streams of one read
plan, level j's streams on level j - 1's.  Then, per depth k in --depths and
alternating run by run:

  lineage_4k   dg_lineage_plan_run, one 4 KiB request per lineage at seeded
               random offsets of V_k (HIP-event stage "read")
  lineage_64k  one 64 KiB request per lineage
  read_4k,     (k = 1 only) dg_read_plan_run with the same requests on the same
  read_64k     streams: the new kernel's overhead where both apply
  decode_k     what the library offered before: k dg_decode_plan_runs with
               ignore_hash, each level materialised whole, between two events
  compose_4k,  k - 1 dg_compose_plan_runs (d_1 .. d_k into one delta), then
  compose_64k  dg_read_plan_index and dg_read_plan_run on it, between two events
               (k >= 2, up to --compose-max-depth)

and once: index, dg_read_plan_index over all 16 n streams.

  c2  4096 lineages of 64 KiB versions
  c6  1024 lineages of 1 MiB versions

5 warm-up and 30 timed runs of each (--warmup / --runs); medians, minima and
maxima go to --out as JSON (profiles/lineage_rate.json is a recorded run), with
the bar of the feature's issue: at c2 and depth 8, lineage_4k takes at most
half of decode_k's time.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = 0xFFFFFFFF


def measure(name, bench, dg, ctx, torch, stream, pairs, depths, warmup, runs, compose_max):
    npg, L, rate, q, seed_base, desc, _ = bench.CONFIGS[name]
    n = pairs or npg
    K = max(depths)
    ref, v1, layout = bench.make_inputs(dg, ctx, torch, name, 0, n, stream)
    torch.cuda.synchronize()
    s = stream.cuda_stream
    ts = torch.cuda.ExternalStream(s)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x11EA)
    for_pair = int(rate * L + 0.5)
    V = [ref, v1]
    for j in range(2, K + 1):   # rate x L further substitutions per lineage and level
        v = V[-1].clone()
        idx = (torch.tensor([vo for _, _, vo, _ in layout], device="cuda").repeat_interleave(for_pair) +
               torch.randint(0, L, (n * for_pair,), device="cuda", generator=g))
        v[idx] = v[idx] ^ (0x11 * (1 + j % 14))
        V.append(v)
    upper = [(vo, vl, vo, vl) for _, _, vo, vl in layout]   # level j >= 2: V_{j-1} and V_j share the version arena's layout

    # every level's deltas, encoded on the device
    plans = {1: dg.EncodePlan(ctx, "onepass", layout, q=q), 2: dg.EncodePlan(ctx, "onepass", upper, q=q)}
    deltas, offs = [], []
    for j in range(1, K + 1):
        p = plans[min(j, 2)]
        out = torch.empty(max(p.output_bound, 1), dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # torch's fills are on its own stream
        p.run(V[j - 1].data_ptr(), V[j].data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        if int(st.abs().sum()) != 0:
            raise SystemExit(f"{name}: encode of level {j} failed: status {st.unique().tolist()}")
        o = off.cpu().tolist()
        deltas.append(out[:(o[-1] + 15) & ~15].clone())
        offs.append(o)
    for p in plans.values():
        p.close()
    base, at = [], 0
    for d in deltas:
        base.append(at)
        at += d.numel()
    D = torch.cat(deltas + [torch.zeros(16, dtype=torch.uint8, device="cuda")])

    # one read plan over all levels, the lineage plan over it
    streams, parents = [], []
    for j in range(1, K + 1):
        for i, (ro, rl, vo, vl) in enumerate(layout):
            o = offs[j - 1]
            streams.append((ro if j == 1 else 0, rl if j == 1 else vl, base[j - 1] + o[i], o[i + 1] - o[i]))
            parents.append(BASE if j == 1 else (j - 2) * n + i)
    reads = dg.ReadPlan(ctx, streams, n)
    lin = dg.LineagePlan(reads, parents, n)
    d_sst = torch.empty(len(streams), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_index = []
    for _ in range(3 + 10):
        e0.record(ts)
        reads.index(D.data_ptr(), d_sst.data_ptr(), stream=s)
        e1.record(ts)
        torch.cuda.synchronize()
        t_index.append(e0.elapsed_time(e1))
    if int(d_sst.abs().sum()) != 0:
        raise SystemExit(f"{name}: index failed: status {d_sst.unique().tolist()}")

    rng = random.Random(0x5EED + len(name))
    sizes = {"4k": 4096, "64k": 65536}
    picks = {}
    for key, size in sizes.items():
        out, pos = [], 0
        for i, (_, _, _, vl) in enumerate(layout):
            ln = min(size, vl)
            out.append((i, rng.randrange(vl - ln + 1), ln, pos))
            pos += (ln + 15) & ~15
        picks[key] = (out, pos)
    d_out = torch.empty(max(v[1] for v in picks.values()) + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")

    def req_array(key, level):
        arr = (dg.ReadReq * n)(*[dg.ReadReq((level - 1) * n + i, o, ln, 0, a) for i, o, ln, a in picks[key][0]])
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()

    def check(what, k, key):
        torch.cuda.synchronize()
        if int(d_st.abs().sum()) != 0:
            raise SystemExit(f"{name}: {what} at depth {k} failed: status {d_st.unique().tolist()}")
        rq = picks[key][0]
        for i, o, ln, a in rq[:32] + rq[-16:]:
            vo = layout[i][2]
            if not torch.equal(d_out[a:a + ln], V[k][vo + o:vo + o + ln]):
                raise SystemExit(f"{name}: {what} at depth {k}: request ({i}, {o}, {ln}) is not V_{k}'s bytes")

    # the routes before lineage reads: materialise every level; or compose, index, read
    dec = []
    for j in range(1, K + 1):
        o = offs[j - 1]
        dec.append(dg.DecodePlan(ctx, [((ro, rl) if j == 1 else (vo, vl)) + (base[j - 1] + o[i], o[i + 1] - o[i], vo, vl)
                                       for i, (ro, rl, vo, vl) in enumerate(layout)], ignore_hash=True))
    buf = [torch.zeros_like(v1), torch.zeros_like(v1)]
    d_dlen = torch.empty(n, dtype=torch.int64, device="cuda")
    d_dst = torch.empty(n, dtype=torch.int32, device="cuda")

    def decode_k(k):
        e0.record(ts)
        src = ref
        for j in range(1, k + 1):
            dst = buf[j & 1]
            dec[j - 1].run(src.data_ptr(), D.data_ptr(), dst.data_ptr(), d_dlen.data_ptr(), d_dst.data_ptr(), s)
            src = dst
        e1.record(ts)
        return src

    comp, c_arena, c_off, c_st = {}, {1: (D, None)}, {1: [base[0] + x for x in offs[0]]}, {}
    comp_reads = {}

    def build_compose(k):
        """Plans for c_j = compose(c_{j-1}, d_j), j = 2 .. k, and a read plan over c_k."""
        for j in range(2, k + 1):
            if j in comp:
                continue
            a, ob = c_off[j - 1], offs[j - 1]
            p = dg.ComposePlan(ctx, [(a[i], a[i + 1] - a[i], base[j - 1] + ob[i], ob[i + 1] - ob[i]) for i in range(n)],
                               ignore_hash=True)
            off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()   # torch's fills are on its own stream
            p.run(c_arena[j - 1][0].data_ptr(), D.data_ptr(), 0, 0, off.data_ptr(), st.data_ptr(), stream=s)   # the sizing run
            torch.cuda.synchronize()
            out = torch.empty(int(off[-1]) + 16, dtype=torch.uint8, device="cuda")
            p.run(c_arena[j - 1][0].data_ptr(), D.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), st.data_ptr(), stream=s)
            torch.cuda.synchronize()
            if int(st.abs().sum()) != 0:
                raise SystemExit(f"{name}: compose of level {j} failed: status {st.unique().tolist()}")
            comp[j], c_arena[j], c_off[j], c_st[j] = p, (out, off), off.cpu().tolist(), st
        o = c_off[k]
        comp_reads[k] = dg.ReadPlan(ctx, [(ro, rl, o[i], o[i + 1] - o[i]) for i, (ro, rl, _, _) in enumerate(layout)], n)

    def compose_k(k, d_req):
        e0.record(ts)
        for j in range(2, k + 1):
            out, off = c_arena[j]
            comp[j].run(c_arena[j - 1][0].data_ptr(), D.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(),
                        c_st[j].data_ptr(), stream=s)
        rp = comp_reads[k]
        rp.index(c_arena[k][0].data_ptr(), stream=s)
        rp.run(ref.data_ptr(), c_arena[k][0].data_ptr(), d_req.data_ptr(), n, d_out.data_ptr(), d_len.data_ptr(),
               d_st.data_ptr(), stream=s)
        e1.record(ts)

    lin.set_timing(1)
    reads.set_timing(1)
    res = {"name": name, "workload": f"{n} lineages of {L}-byte versions, {rate:.0%} substitutions per level, onepass deltas",
           "lineages": n, "version_bytes_per_level": int(v1.numel()), "delta_bytes_per_level": [o[-1] for o in offs],
           "work_items": dg.lineage_work_items(), "index_all_levels": None, "depths": {}}

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}

    res["index_all_levels"] = dict(summary(t_index[3:]), streams=len(streams))
    for k in depths:
        rq_lin = {key: req_array(key, k) for key in sizes}
        rq_one = {key: req_array(key, 1) for key in sizes}   # stream i of a one-level plan
        with_compose = 2 <= k <= compose_max
        torch.cuda.synchronize()   # the request arrays were copied on torch's stream
        if with_compose:
            build_compose(k)
        # checked runs
        for key in sizes:
            lin.run(ref.data_ptr(), D.data_ptr(), rq_lin[key].data_ptr(), n, d_out.data_ptr(), d_len.data_ptr(), d_st.data_ptr(),
                    stream=s)
            check("the lineage read", k, key)
            if with_compose:
                compose_k(k, rq_one[key])
                check("the composed read", k, key)
        got = decode_k(k)
        torch.cuda.synchronize()
        if int(d_dst.abs().sum()) != 0 or not torch.equal(got, V[k]):
            raise SystemExit(f"{name}: {k} decodes did not reproduce V_{k}")
        keys = ["lineage_4k", "lineage_64k", "decode_k"] + (["read_4k", "read_64k"] if k == 1 else []) + \
               (["compose_4k", "compose_64k"] if with_compose else [])
        t = {x: [] for x in keys}
        for it in range(warmup + runs):   # alternating, so that all see the same machine
            now = {}
            for x in keys:
                what, _, key = x.partition("_")
                if what == "lineage":
                    lin.run(ref.data_ptr(), D.data_ptr(), rq_lin[key].data_ptr(), n, d_out.data_ptr(), d_len.data_ptr(),
                            d_st.data_ptr(), stream=s)
                    torch.cuda.synchronize()
                    now[x] = lin.stage_times()["read"]
                elif what == "read":
                    reads.run(ref.data_ptr(), D.data_ptr(), rq_lin[key].data_ptr(), n, d_out.data_ptr(), d_len.data_ptr(),
                              d_st.data_ptr(), stream=s)
                    torch.cuda.synchronize()
                    now[x] = reads.stage_times()["read"]
                elif what == "decode":
                    decode_k(k)
                    torch.cuda.synchronize()
                    now[x] = e0.elapsed_time(e1)
                else:
                    compose_k(k, rq_one[key])
                    torch.cuda.synchronize()
                    now[x] = e0.elapsed_time(e1)
            if it >= warmup:
                for x in keys:
                    t[x].append(now[x])
        row = {x: summary(v) for x, v in t.items()}
        if with_compose:
            row["composed_bytes"] = c_off[k][-1]
        res["depths"][str(k)] = row
    for p in [lin, reads] + dec + list(comp.values()) + list(comp_reads.values()):
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2,c6")
    ap.add_argument("--pairs", type=int, default=0, help="lineages per shape (0: the shape's own count)")
    ap.add_argument("--depths", default="1,2,4,8,16")
    ap.add_argument("--compose-max-depth", type=int, default=16, help="the deepest depth at which the compose route is built")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lineage_rate.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lineage_rate.py needs a GPU: there is nothing to time without one")
    import bench
    import __graft_entry__ as entry
    dg = entry._load_product()
    ctx = dg.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    depths = [int(x) for x in args.depths.split(",")]
    results = [measure(nm, bench, dg, ctx, torch, stream, args.pairs, depths, args.warmup, args.runs, args.compose_max_depth)
               for nm in args.shapes.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "runs": args.runs, "results": results}
    for r in results:   # the bar: at c2 and depth 8, a 4 KiB lineage read per lineage takes at most half of 8 decodes
        if r["name"] == "c2" and "8" in r["depths"]:
            a, b = r["depths"]["8"]["lineage_4k"]["median_ms"], r["depths"]["8"]["decode_k"]["median_ms"]
            doc["bar"] = {"shape": "c2", "depth": 8, "lineage_4k_ms": a, "decode_k_ms": b, "ratio": b / a, "met": 2 * a <= b}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        print(json.dumps(r))
    if "bar" in doc:
        print(json.dumps(doc["bar"]))


if __name__ == "__main__":
    main()
