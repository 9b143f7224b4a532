"""GPU: in-place conversion of batches on the device (dg_inplace_plan_*,
dg_make_inplace_batch, dg_encode_pipelined with DG_OPT_INPLACE).

The comparator is dg.make_inplace, the host converter that
tests/test_inplace_cpu.py pins byte for byte to the reference; the named
graphs are additionally held to tests/golden/golden_inplace_graphs.json,
minted from the reference's `delta inplace` itself.
"""
from __future__ import annotations

import hashlib
import json
import os
import random

import pytest

import window_cases as wc

from inplace_graphs import POLICIES, build, named_graphs, seam_graphs
from stage_timing import check_ring_phases
from test_oracle import inplace_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = {(c["name"], c["policy"]): c
        for c in json.load(open(os.path.join(HERE, "golden", "golden_inplace_graphs.json")))["cases"]}
SEAM_GOLD = {(c["name"], c["policy"]): c
             for c in json.load(open(os.path.join(HERE, "golden", "golden_inplace_seams.json")))["cases"]}
OLD = json.load(open(os.path.join(HERE, "golden", "golden_inplace.json")))["cases"]
OK, UNSUPPORTED, CAPACITY, MALFORMED = 0, 2, 7, 8
ALGO = {1: "onepass", 2: "correcting"}


def _arena(torch, chunks, size):
    buf = bytearray(max(size, 1))
    for o, b in chunks:
        buf[o:o + len(b)] = b
    return torch.frombuffer(buf, dtype=torch.uint8).cuda()


def _run(torch, dg, ctx, items, policy, *, caps=None, out_cap=None, odd=False, timing=False, after=None):
    """items: (R, stream) per delta -> (status list, outputs, offsets, plan).  odd:
    streams and references at odd offsets, the last of each ending its arena.
    after(plan, go): called after the first run; go() runs the plan once more."""
    n = len(items)
    descs, rch, dch = [], [], []
    rt = dt = 1 if odd else 0
    for k, (R, d) in enumerate(items):
        cap = len(d) if caps is None or caps[k] is None else caps[k]
        descs.append((rt, len(R), dt, cap))
        rch.append((rt, R))
        dch.append((dt, d))
        rt, dt = rt + len(R), dt + max(len(d), cap)
        if odd and k + 1 < n:
            rt, dt = (rt + 2) | 1, (dt + 2) | 1
    ref_t, del_t = _arena(torch, rch, rt), _arena(torch, dch, dt)
    assert ref_t.numel() == max(rt, 1) and del_t.numel() == max(dt, 1)
    plan = dg.InplacePlan(ctx, descs, policy)
    if timing:
        plan.set_timing(2)
    # an in-place delta is at most the stream plus its version bytes
    cap_total = out_cap if out_cap is not None else sum(len(d) + 4096 * 5 for _, d in items) + 64
    out = torch.zeros(max(cap_total, 1), dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def go():
        plan.run(ref_t.data_ptr(), del_t.data_ptr(), out.data_ptr(), cap_total, off.data_ptr(), st.data_ptr(),
                 stream=ctx.stream)
        torch.cuda.synchronize()
    go()
    if after:
        after(plan, go)
    offs = off.cpu().tolist()
    outc = bytes(out.cpu().numpy())
    return st.cpu().tolist(), [outc[offs[i]:offs[i + 1]] for i in range(n)], offs, plan


@pytest.fixture(scope="module")
def graphs(dg, orc):
    return [(name, R, *build(dg, orc, R, cmds)) for name, _, R, cmds in named_graphs()]


@pytest.fixture(scope="module")
def host_ref(dg, graphs):
    """dg.make_inplace of every named graph, computed once."""
    return {(name, pol): dg.make_inplace(R, std, pol) for name, R, std, _ in graphs for pol in POLICIES}


# 1. every named graph, one plan run per policy
@pytest.mark.parametrize("policy", POLICIES)
def test_named_graphs(dg, ctx, torch_cuda, graphs, host_ref, policy):
    cap = sum(len(host_ref[(name, policy)]) for name, *_ in graphs)
    st, outs, _, _ = _run(torch_cuda, dg, ctx, [(R, std) for _, R, std, _ in graphs], policy, out_cap=cap)
    assert st == [OK] * len(graphs), dict(zip([g[0] for g in graphs], st))
    for (name, R, std, V), got in zip(graphs, outs):
        c = GOLD[(name, policy)]
        assert len(got) == c["len"] and hashlib.sha256(got).hexdigest() == c["sha256"], name
        assert got == host_ref[(name, policy)], name
        if len(V) <= 4096:   # (the large permutations decode in test 2's shapes)
            assert dg.decode(R, got, ctx=ctx) == V, name
    # and through the host-buffer entry point
    assert dg.make_inplace_batch([(R, std) for _, R, std, _ in graphs], policy, ctx=ctx) == \
        [host_ref[(name, policy)] for name, *_ in graphs]


# 2. the 44 cases of golden_inplace.json: dg.encode -> device conversion
def test_existing_goldens(dg, ctx, orc, torch_cuda):
    by_policy = {0: [], 1: []}
    groups = {}
    for c in OLD:
        groups.setdefault((c["algo"], c["q"]), []).append((c, *inplace_inputs(orc, c)))
    for (algo, q), cs in groups.items():
        stds = dg.encode_batch([(R, V) for _, R, V in cs], ALGO[algo], p=16, q=q, ctx=ctx)
        for (c, R, _), d in zip(cs, stds):
            by_policy[c["policy"]].append((c, R, d))
    assert sum(map(len, by_policy.values())) == 44
    for pol, cases in by_policy.items():
        got = dg.make_inplace_batch([(R, d) for _, R, d in cases], POLICIES[pol], ctx=ctx)
        for (c, _, _), g in zip(cases, got):
            assert g == bytes.fromhex(c["delta_hex"]), c["name"]


def _random_items(dg, orc, seed, n):
    rng = random.Random(seed)
    items = []
    for _ in range(n):
        R = rng.randbytes(rng.randrange(2048, 4097))
        cmds = []
        for _ in range(rng.randrange(1, 81)):
            if rng.random() < 0.8:
                ln = rng.randrange(1, 201)
                cmds.append(("copy", rng.randrange(0, len(R) - ln + 1), ln))
            else:
                cmds.append(("add", rng.randbytes(rng.randrange(1, 17))))
        items.append((R, build(dg, orc, R, cmds)[0]))
    return items


# 3. 256 random deltas per policy in one batch, at odd offsets, the last stream
#    and the last R ending at the last byte of their arenas
@pytest.mark.parametrize("policy", POLICIES)
def test_random_batch(dg, ctx, orc, torch_cuda, policy):
    items = _random_items(dg, orc, 0x1B9 + len(policy), 256)
    exp = [dg.make_inplace(R, d, policy) for R, d in items]
    st, outs, _, _ = _run(torch_cuda, dg, ctx, items, policy, odd=True, out_cap=sum(map(len, exp)))
    assert st == [OK] * len(items)
    bad = [i for i, (g, e) in enumerate(zip(outs, exp)) if g != e]
    assert not bad, bad[:10]
    assert sum(dg.info(e)["num_adds"] > dg.info(d)["num_adds"] for e, (_, d) in zip(exp, items)) > 64   # cycles


# 4. one batch with every per-stream status; the neighbours stay correct
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_status_batch(dg, ctx, orc, torch_cuda, policy):
    good = _random_items(dg, orc, 77, 8)
    R = random.Random(5).randbytes(4096)
    std = build(dg, orc, R, [("copy", 100, 300), ("add", b"abcdef"), ("copy", 0, 100)])[0]
    crc = std[9:25]
    truncated = std[:-5]                                    # the last COPY is cut short
    past_r = build(dg, orc, R + b"xx", [("copy", 4000, 98)])[0]   # reads R[4000:4098) of a 4096-byte R
    already = dg.make_inplace(R, std, policy)
    # the same commands listed in another order: dst no longer sequential
    nonseq = dg.encode_delta([dg.PlacedCopy(0, 306, 100), dg.PlacedCopy(100, 0, 300), dg.PlacedAdd(300, b"abcdef")],
                             inplace=False, version_size=406, src_crc=crc[:8], dst_crc=crc[8:])
    items = [good[0], (R, truncated), good[1], (R, past_r), good[2], (R, already), good[3], (R, nonseq), good[4],
             (R, std), good[5]]
    caps = [None] * len(items)
    caps[9] = len(std) - 1                                  # a stream longer than its delta_cap ...
    exp = [dg.make_inplace(r, d, policy) if k not in (1, 3, 7, 9) else b"" for k, (r, d) in enumerate(items)]
    want = [OK, MALFORMED, OK, MALFORMED, OK, OK, OK, UNSUPPORTED, OK, CAPACITY, OK]

    # ... which only d_delta_offsets can express: with NULL the stream is exactly
    # delta_cap bytes, so item 9 is then the stream cut one byte short (its END
    # byte is missing, which the format allows: encoding.c:111-178)
    st, outs, _, _ = _run(torch_cuda, dg, ctx, items, policy, caps=caps)
    assert st[:9] + st[10:] == want[:9] + want[10:]
    assert st[9] == OK and outs[9] == dg.make_inplace(R, std[:-1], policy)
    for k in (0, 2, 4, 5, 6, 8, 10):
        assert outs[k] == exp[k], k
    for k in (1, 3, 7):
        assert outs[k] == b""
    assert outs[5] == already
    _capacity_through_offsets(torch_cuda, dg, ctx, items, caps, policy, want, exp)

    # make_inplace_batch converts the non-sequential stream on the host
    ok_items = [it for k, it in enumerate(items) if k not in (1, 3)]
    assert dg.make_inplace_batch(ok_items, policy, ctx=ctx) == [dg.make_inplace(r, d, policy) for r, d in ok_items]
    with pytest.raises(dg.DeltaError) as e:
        dg.make_inplace_batch(items, policy, ctx=ctx)
    assert e.value.code == MALFORMED

    # out_cap one byte short of stream 5's end: it and the one after it get CAPACITY
    fit = [it for k, it in enumerate(items) if k not in (1, 3, 7, 9)]
    fexp = [dg.make_inplace(r, d, policy) for r, d in fit]
    short = sum(map(len, fexp[:6])) - 1
    st2, outs2, offs2, _ = _run(torch_cuda, dg, ctx, fit, policy, out_cap=short)
    assert st2 == [OK] * 5 + [CAPACITY] * 2
    assert outs2[:5] == fexp[:5]
    assert offs2[-1] == sum(map(len, fexp))   # the offsets still count every size, as the encode plan's do


def _capacity_through_offsets(torch, dg, ctx, items, caps, policy, want, exp):
    """The same batch packed, located by an offsets array (as dg_encode_plan_run
    writes) and with an incoming status: item 9 is longer than its delta_cap."""
    n = len(items)
    offs, rch, dch, descs = [0], [], [], []
    rt = 0
    for k, (R, d) in enumerate(items):
        descs.append((rt, len(R), 0, len(d) if caps[k] is None else caps[k]))
        rch.append((rt, R))
        dch.append((offs[-1], d))
        rt += len(R)
        offs.append(offs[-1] + len(d))
    ref_t, del_t = _arena(torch, rch, rt), _arena(torch, dch, offs[-1])
    d_offs = torch.tensor(offs, dtype=torch.int64, device="cuda")
    in_st = [0] * n
    in_st[2] = 11                                           # an incoming status is passed on
    d_in = torch.tensor(in_st, dtype=torch.int32, device="cuda")
    plan = dg.InplacePlan(ctx, descs, policy)
    cap_total = sum(map(len, exp)) + 16
    out = torch.zeros(cap_total, dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan.run(ref_t.data_ptr(), del_t.data_ptr(), out.data_ptr(), cap_total, off.data_ptr(), st.data_ptr(),
             d_delta_offsets=d_offs.data_ptr(), d_delta_status=d_in.data_ptr(), stream=ctx.stream)
    torch.cuda.synchronize()
    o = off.cpu().tolist()
    outc = bytes(out.cpu().numpy())
    got = [outc[o[i]:o[i + 1]] for i in range(n)]
    assert st.cpu().tolist() == want[:2] + [11] + want[3:]
    assert got == exp[:2] + [b""] + exp[3:]


def _chain(torch, dg, ctx, pairs, algo, policy, q, bad=None):
    """EncodePlan.run -> InplacePlan(for_plan).run on one stream, no host step."""
    n = len(pairs)
    lay, rch, vch, rt, vt = [], [], [], 0, 0
    for R, V in pairs:
        lay.append((rt, len(R), vt, len(V)))
        rch.append((rt, R))
        vch.append((vt, V))
        rt, vt = (rt + len(R) + 15) & ~15, (vt + len(V) + 15) & ~15
    ref_t, ver_t = _arena(torch, rch, rt), _arena(torch, vch, vt)
    enc = dg.EncodePlan(ctx, algo, lay, p=16, q=q)
    ip = dg.InplacePlan(ctx, policy=policy, for_plan=enc)
    d_std = torch.zeros(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(max(ip.output_bound, 1), dtype=torch.uint8, device="cuda")
    off1, off2 = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    st1, st2 = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    enc.run(ref_t.data_ptr(), ver_t.data_ptr(), d_std.data_ptr(), d_std.numel(), off1.data_ptr(), st1.data_ptr(),
            ctx.stream)
    if bad is not None:   # (a device-side write, ordered after the encode: still no host step)
        with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream)):
            st1[bad] = 11
    ip.run(ref_t.data_ptr(), d_std.data_ptr(), d_out.data_ptr(), d_out.numel(), off2.data_ptr(), st2.data_ptr(),
           d_delta_offsets=off1.data_ptr(), d_delta_status=st1.data_ptr(), stream=ctx.stream)
    torch.cuda.synchronize()
    o1, o2 = off1.cpu().tolist(), off2.cpu().tolist()
    s, c = bytes(d_std.cpu().numpy()), bytes(d_out.cpu().numpy())
    return ([s[o1[i]:o1[i + 1]] for i in range(n)], [c[o2[i]:o2[i + 1]] for i in range(n)], st2.cpu().tolist())


# 5. encode plan -> in-place plan, chained on one stream
@pytest.mark.parametrize("policy", POLICIES)
def test_chained_after_encode_plan(dg, ctx, orc, torch_cuda, policy):
    transp = [orc.synth_transpose(0xC4000000 + i, 8 + i % 5, 8192 // (8 + i % 5), 50)[:2] for i in range(32)]
    std, got, st = _chain(torch_cuda, dg, ctx, transp, "correcting", policy, 1)
    assert st == [OK] * 32
    assert got == [dg.make_inplace(R, d, policy) for (R, _), d in zip(transp, std)]
    assert any(dg.info(g)["num_adds"] > dg.info(d)["num_adds"] for g, d in zip(got, std))   # cycles were broken
    edits = [orc.synth_pair(0xC2000000 + i, 8192, 80) for i in range(32)]
    std, got, st = _chain(torch_cuda, dg, ctx, edits, "onepass", policy, 4099, bad=7)
    assert st == [OK] * 7 + [11] + [OK] * 24
    exp = [dg.make_inplace(R, d, policy) for (R, _), d in zip(edits, std)]
    exp[7] = b""
    assert got == exp


# 6. the pipelined host-to-host path with DG_OPT_INPLACE
@pytest.mark.parametrize("policy", POLICIES)
def test_pipelined_inplace(dg, ctx, orc, policy):
    rng = random.Random(31)
    pairs = []
    for i in range(40):
        nb, blk = rng.randrange(2, 12), rng.randrange(40, 200)
        R = rng.randbytes(nb * blk)
        blocks = [R[k * blk:(k + 1) * blk] for k in range(nb)]
        rng.shuffle(blocks)
        pairs.append((R, b"".join(blocks) + rng.randbytes(i % 7)))
    exp = [dg.make_inplace(R, d, policy) for (R, _), d in zip(pairs, dg.encode_batch(pairs, "correcting", q=1, ctx=ctx))]
    for _ in range(2):   # the second call reuses the slots' plans
        assert dg.encode_pipelined(pairs, "correcting", q=1, chunk_bytes=4096, inplace=True, policy=policy,
                                   ctx=ctx) == exp
    ctxs = [dg.Context(0), dg.Context(0)]
    assert dg.encode_pipelined(pairs, "correcting", q=1, chunk_bytes=4096, inplace=True, policy=policy,
                               ctxs=ctxs) == exp
    # without the flag the path is what it was
    assert dg.encode_pipelined(pairs, "correcting", q=1, chunk_bytes=4096, ctx=ctx) == \
        dg.encode_batch(pairs, "correcting", q=1, ctx=ctx)


# 7. streams longer than a parse window: cuts and payloads across window borders
def test_streams_across_parse_windows(dg, ctx, orc, torch_cuda):
    rng = random.Random(41)
    R = rng.randbytes(4096)
    perm = [("copy", 4 * b, 4) for b in rng.sample(range(1024), 300)]          # 3.9 KiB of COPYs
    long_std = build(dg, orc, R, perm)[0]
    big_add = build(dg, orc, R, perm[:70] + [("add", rng.randbytes(3000))] + perm[70:90] +
                    [("add", b"\x01\x02\x00" * 400)] + perm[90:140])[0]       # payloads that look like commands
    lying = bytearray(big_add)
    at = 25 + 13 * 70 + 5
    assert lying[at - 5] == 2
    lying[at:at + 4] = (len(big_add)).to_bytes(4, "big")                       # an ADD running past the stream's end
    items = [(R, long_std), (R, long_std[:-1]), (R, long_std[:-5]), (R, long_std[:1030]), (R, big_add),
             (R, bytes(lying)), (R, long_std[:25 + 13 * 78 + 1])]
    want, exp = [], []
    for r, d in items:
        try:
            exp.append(dg.make_inplace(r, d, "localmin"))
            want.append(OK)
        except dg.DeltaError as e:
            exp.append(b"")
            want.append(e.code)
    assert want == [OK, OK, MALFORMED, MALFORMED, OK, MALFORMED, MALFORMED]
    st, outs, _, _ = _run(torch_cuda, dg, ctx, items, "localmin", odd=True)
    assert st == want
    assert outs == exp


# 8. stage timing
def test_stage_times(dg, ctx, orc, torch_cuda):
    items = _random_items(dg, orc, 3, 16)
    def first_then_phases(plan, go):
        t = plan.stage_times()
        assert set(t) == {"order", "scan", "emit", "total"}
        assert t["order"] > 0 and t["emit"] > 0 and t["total"] >= t["order"]
        check_ring_phases(plan, go, ["order", "scan", "emit", "total"])
    st, outs, _, _ = _run(torch_cuda, dg, ctx, items, "localmin", timing=True, after=first_then_phases)
    assert st == [OK] * len(items)
    assert outs == [dg.make_inplace(R, d, "localmin") for R, d in items]


# 9. commands cut by, ending at and starting at the end of a parse window (tests/window_cases.py)
def test_parse_window_edges(dg, ctx, orc, torch_cuda):
    items = [(R, d) for _, R, _, d, _ in wc.standard_cases(dg, orc)]
    st, outs, _, _ = _run(torch_cuda, dg, ctx, items, "localmin", odd=True)
    assert st == [OK] * len(items)
    for (name, *_), (R, d), got in zip(wc.standard_cases(dg, orc), items, outs):
        assert got == dg.make_inplace(R, d, "localmin"), name


# 10. the storage seams of the order kernel (tests/inplace_graphs.py seam_graphs): the dst column in LDS up to 2048
#     copies, the ready bitmap in LDS up to 65536 copies and in work memory above; three radix passes on the Kahn
#     path.  One batch per policy, a small graph before and after, against the reference's goldens
@pytest.fixture(scope="module")
def seams(dg, orc):
    return [(name, R, *build(dg, orc, R, cmds)) for name, _, R, cmds in seam_graphs()]


def _first_difference(dg, name, R, std, policy, got):
    exp = dg.make_inplace(R, std, policy)   # computed only to describe a difference
    at = next((k for k, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
    return f"{name} ({policy}): {len(got)} bytes for {len(exp)}, the first difference at byte {at}: {got[at:at + 26].hex()} for {exp[at:at + 26].hex()}"


@pytest.mark.parametrize("policy", POLICIES)
def test_seam_graphs(dg, ctx, torch_cuda, graphs, seams, policy):
    small = {g[0]: g for g in graphs}
    batch = [small["figure_eight"]] + seams + [small["reverse_8"]]
    gold = [(GOLD if name in small else SEAM_GOLD)[(name, policy)] for name, *_ in batch]
    times = {}
    st, outs, offs, _ = _run(torch_cuda, dg, ctx, [(R, std) for _, R, std, _ in batch], policy, out_cap=sum(g["len"] for g in gold),
                             timing=True, after=lambda plan, go: times.update(plan.stage_times()))
    print(f"seam graphs ({policy}): stage times in ms {times}")
    assert st == [OK] * len(batch), dict(zip([g[0] for g in batch], st))
    assert offs[-1] == sum(g["len"] for g in gold)
    for (name, R, std, V), got, g in zip(batch, outs, gold):
        assert len(got) == g["len"] and hashlib.sha256(got).hexdigest() == g["sha256"], _first_difference(dg, name, R, std, policy, got)
    k = [name for name, *_ in batch].index("perm_65537")
    assert dg.decode(batch[k][1], outs[k], ctx=ctx) == batch[k][3]
    # and through the host-buffer entry point
    for (name, R, std, V), got, g in zip(batch, dg.make_inplace_batch([(R, std) for _, R, std, _ in batch], policy, ctx=ctx), gold):
        assert len(got) == g["len"] and hashlib.sha256(got).hexdigest() == g["sha256"], _first_difference(dg, name, R, std, policy, got)


# 11. the order stage of the 65 537-copy graph alone (one lane runs Tarjan over its vertices in work memory)
def test_seam_order_stage_time(dg, ctx, torch_cuda, seams):
    name, R, std, V = next(s for s in seams if s[0] == "perm_65537")
    g = SEAM_GOLD[(name, "localmin")]
    times = {}
    st, outs, _, _ = _run(torch_cuda, dg, ctx, [(R, std)], "localmin", out_cap=g["len"], timing=True,
                          after=lambda plan, go: times.update(plan.stage_times()))
    print(f"perm_65537 alone (localmin): stage times in ms {times}")
    assert st == [OK] and hashlib.sha256(outs[0]).hexdigest() == g["sha256"]
    assert times["order"] > 0 and times["total"] >= times["order"]
