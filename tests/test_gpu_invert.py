"""GPU: dg_invert_plan_* and dg_invert_batch (csrc/dg_invert_dev.hip) produce byte
for byte what the host function dg_invert produces, which
tests/test_invert_cpu.py pins to the Python model.

One batch of every CPU case; a plan over torch buffers at odd arena offsets, with
and without the offsets array; literal spans up to R's last byte, which is the
allocation's last; an out_cap that fits only the first deltas; damaged streams
between good neighbours; the capacities; a re-run on other bytes, sorted after
unsorted; stage times; and the device chain encode -> invert -> decode on one
stream.
"""
from __future__ import annotations

import os
import random
import subprocess

import pytest

import compose_cases as cc
import invert_cases as ic
import window_cases as wc
from stage_timing import check_ring_phases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")

OK, UNSUPPORTED, TOO_LARGE, CAPACITY, MALFORMED = 0, 2, 3, 7, 8
GUARD = 0xA5


def host(dg, r, a):
    """(status, bytes) of the host function."""
    try:
        return OK, dg.invert(r, a)
    except dg.DeltaError as e:
        return e.code, b""


class Run:
    """One plan over items (R, A): the references in one arena and the streams in
    another, at odd offsets with guard bytes between them; the last one of each
    arena ends at the arena's last byte.  offsets=True packs the streams and
    passes n + 1 offsets, the descriptors then holding capacities only."""

    def __init__(self, torch, dg, ctx, items, *, offsets=False, slack=0, timing=False, caps=None):
        self.torch, self.dg, self.ctx, self.n = torch, dg, ctx, len(items)
        self.offsets = offsets
        n = self.n
        descs, self.pos = [], [[], []]
        at = [1, 3]
        for k, it in enumerate(items):
            d = []
            for w in (0, 1):
                ln = len(it[w])
                self.pos[w].append(at[w])
                if w == 0:
                    d += [at[w], ln]
                else:
                    d += [0 if offsets else at[w], (caps[k] if caps else ln + slack) if offsets else ln]
                at[w] += ln + (0 if (w and offsets) or k + 1 == n else 5 + 2 * w)
            descs.append(tuple(d))
        self.size = at
        self.plan = dg.InvertPlan(ctx, descs)
        if timing:
            self.plan.set_timing(2)
        self.off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        self.st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.load(items)

    def load(self, items):
        torch = self.torch
        self.arena = []
        for w in (0, 1):
            buf = bytearray([GUARD]) * self.size[w]
            for k, it in enumerate(items):
                buf[self.pos[w][k]:self.pos[w][k] + len(it[w])] = it[w]
            assert self.pos[w][-1] + len(items[-1][w]) == len(buf)
            self.arena.append(torch.frombuffer(buf, dtype=torch.uint8).cuda())
        self.in_off = torch.tensor(self.pos[1] + [self.size[1]], dtype=torch.int64, device="cuda")

    def run(self, out_cap=None, delta_status=None):
        torch = self.torch
        kw = {}
        if self.offsets:
            kw = dict(d_delta_offsets=self.in_off.data_ptr())
        if delta_status is not None:
            keep = torch.tensor(delta_status, dtype=torch.int32, device="cuda")
            kw["d_delta_status"] = keep.data_ptr()
        if out_cap is None:
            out_cap = self.plan.output_bound
        self.out_cap = out_cap
        pad = 32
        self.out = torch.full((out_cap + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.plan.run(self.arena[0].data_ptr(), self.arena[1].data_ptr(), self.out.data_ptr() + pad, out_cap,
                      self.off.data_ptr(), self.st.data_ptr(), stream=self.ctx.stream, **kw)
        torch.cuda.synchronize()
        raw = bytes(self.out.cpu().numpy())
        assert raw[:pad] == bytes([GUARD]) * pad and raw[pad + out_cap:] == bytes([GUARD]) * pad, "a byte outside the output arena"
        self.bytes = raw[pad:pad + out_cap]
        self.offs = self.off.cpu().tolist()
        self.status = self.st.cpu().tolist()
        return self

    def result(self, k):
        return self.bytes[self.offs[k]:min(self.offs[k + 1], self.out_cap)]

    def check(self, items):
        """Every delta as the host function has it; the outputs packed without gaps."""
        at = 0
        for k, (r, a) in enumerate(items):
            st, exp = host(self.dg, r, a)
            assert self.status[k] == st, (k, self.status[k], st)
            assert self.offs[k] == at, k
            assert self.result(k) == exp, k
            at += len(exp)
        assert self.offs[self.n] == at
        assert self.bytes[at:] == bytes([GUARD]) * (self.out_cap - at)


# 1. every CPU case in one batch
def test_all_cpu_cases_in_one_batch(dg, ctx, orc):
    cases = ic.all_cases(dg, orc)
    got = dg.invert_batch([(c[1], c[3]) for c in cases], ctx=ctx)
    for c, g in zip(cases, got):
        assert g == dg.invert(c[1], c[3]), c[0]
    for c, g in zip(cases[-6:], got[-6:]):   # the realistic ones, decoded on the device too
        assert dg.decode(c[2], g, ctx=ctx) == c[1], c[0]
    assert dg.invert_batch([], ctx=ctx) == []


# 2. a plan over torch buffers: odd offsets, the arenas' last bytes, with and without the offsets array
@pytest.mark.parametrize("offsets", [False, True])
def test_plan_over_torch_buffers(dg, ctx, orc, torch_cuda, offsets):
    cases = ic.random_cases(dg, orc)[:12] + ic.shaped_cases(dg, orc) + ic.count_cases(dg, orc) + ic.realistic_cases(dg, orc)[2:]
    items = [(c[1], c[3]) for c in cases]
    r = Run(torch_cuda, dg, ctx, items, offsets=offsets, slack=7).run()
    r.check(items)
    assert r.offs[-1] <= r.plan.output_bound


# 3. literal spans up to the last byte of R, which is the last byte of its allocation
def test_literal_spans_at_the_end_of_the_allocation(dg, ctx, orc, torch_cuda):
    by = {c[0]: c for c in ic.shaped_cases(dg, orc)}
    for name in ("literal_spans", "literal_spans_shifted"):
        c = by[name]
        assert {len(x.data) for x in dg.decode_delta(dg.invert(c[1], c[3]))[0] if isinstance(x, dg.PlacedAdd)} >= set(ic.SPANS)
        # R last in its arena; then a 5000-byte literal tail that ends there
        R2 = c[1] + bytes(range(256)) * 20
        items = [(by["nested"][1], by["nested"][3]), (c[1], c[3])]
        r = Run(torch_cuda, dg, ctx, items).run()
        assert r.pos[0][1] + len(c[1]) == r.arena[0].numel()
        r.check(items)
        items = [(R2, cc.make_delta(dg, orc, [("C", x.src, x.length) for x in dg.decode_delta(c[3])[0]], R2))]
        r = Run(torch_cuda, dg, ctx, items).run()
        r.check(items)
        assert dg.decode_delta(r.result(0))[0][-1].dst == len(c[1]) - 1   # one ADD: R's last byte and the tail


# 4. an out_cap that fits only the first k deltas
def test_out_cap_fits_first_deltas(dg, ctx, orc, torch_cuda):
    cases = ic.shaped_cases(dg, orc)[:8]
    items = [(c[1], c[3]) for c in cases]
    exp = [dg.invert(r, a) for r, a in items]
    k = 5
    cap = sum(len(e) for e in exp[:k]) + len(exp[k]) - 1   # one byte short for delta k
    r = Run(torch_cuda, dg, ctx, items).run(out_cap=cap)
    assert r.status == [OK] * k + [CAPACITY] * (len(items) - k)
    at = 0
    for i, e in enumerate(exp):   # the offsets still count every delta's size
        assert r.offs[i] == at
        at += len(e)
        if i < k:
            assert r.result(i) == e
    assert r.offs[-1] == at
    assert r.bytes[sum(len(e) for e in exp[:k]):] == bytes([GUARD]) * (len(exp[k]) - 1)   # a failed output is empty


# 5. each kind of damage between good neighbours; incoming statuses are passed on
@pytest.mark.parametrize("offsets", [False, True])
def test_damage_between_good_neighbours(dg, ctx, orc, torch_cuda, offsets):
    (R, V, A), bad = ic.damaged(dg, orc)
    good = ic.realistic_cases(dg, orc)[2]
    items = [(good[1], good[3])]
    for _, a, _ in bad:
        items += [(R, a), (R, A)]
    r = Run(torch_cuda, dg, ctx, items, offsets=offsets).run()
    r.check(items)
    assert [r.status[1 + 2 * k] for k in range(len(bad))] == [x[2] for x in bad]
    assert all(r.offs[2 + 2 * k] == r.offs[1 + 2 * k] for k in range(len(bad)))
    assert all(r.result(2 + 2 * k) == dg.invert(R, A) for k in range(len(bad)))
    # an incoming status beats the delta's own defect; a failed input's bytes are not looked at
    st = [0] * len(items)
    st[0], st[1], st[2] = 11, 4, 6
    r2 = Run(torch_cuda, dg, ctx, items, offsets=offsets).run(delta_status=st)
    assert r2.status[:3] == [11, 4, 6] and r2.status[3:] == r.status[3:]
    assert r2.result(0) == b"" and r2.result(2) == b"" and r2.result(4) == r.result(4)


# 6. the capacities: a stream longer than its capacity, more COPYs than the work memory holds
def test_stream_longer_than_capacity(dg, ctx, orc, torch_cuda):
    (R, V, A), _ = ic.damaged(dg, orc)
    items = [(R, A), (R, A), (R, A)]
    r = Run(torch_cuda, dg, ctx, items, offsets=True, caps=[len(A), len(A) - 1, len(A) + 1]).run()
    assert r.status == [OK, CAPACITY, OK]
    assert r.result(0) == dg.invert(R, A) == r.result(2) and r.result(1) == b""


def test_more_copies_than_work_memory(dg, ctx, orc, torch_cuda):
    """A stream without its END byte holds one COPY more than (len - 26) // 13."""
    rng = random.Random(91)
    R = rng.randbytes(500)
    cmds = [("C", rng.randrange(0, 480), rng.randint(1, 20)) for _ in range(70)]
    A = cc.make_delta(dg, orc, cmds, R)
    assert A[-1] == 0 and len(A) == 25 + 13 * 70 + 1
    items = [(R, A), (R, A[:-1]), (R, A)]
    for offsets in (False, True):
        r = Run(torch_cuda, dg, ctx, items, offsets=offsets).run()
        assert r.status == [OK, CAPACITY, OK]
        assert r.result(0) == dg.invert(R, A) == r.result(2) and r.result(1) == b""
    # the host-buffer wrapper hands such a stream to the host function
    assert dg.invert_batch(items, ctx=ctx) == [dg.invert(R, A)] * 3


# 7. the same plan on other bytes of the same layout: no stale records, sorted after unsorted
def test_rerun_on_other_bytes(dg, ctx, orc, torch_cuda):
    rng = random.Random(92)
    R = rng.randbytes(900)

    def variant(seed, order):
        g = random.Random(seed)
        out = []
        for n in (0, 5, 70, 140):
            # fixed stream sizes: n COPYs of 3 bytes and one 8-byte ADD
            cs = [("C", g.randrange(0, 890), 3) for _ in range(n)]
            if order == "key":
                cs.sort(key=lambda c: c[1])
            out.append(ic.case(dg, orc, f"v{n}", R, cs + [("A", g.randbytes(8))]))
        return out

    first, second, third = variant(1, "any"), variant(2, "key"), variant(3, "any")
    assert [len(c[3]) for c in first] == [len(c[3]) for c in second] == [len(c[3]) for c in third]
    assert not ic.in_key_order(dg, first[3][3]) and ic.in_key_order(dg, second[3][3])
    i1, i2, i3 = ([(c[1], c[3]) for c in v] for v in (first, second, third))
    r = Run(torch_cuda, dg, ctx, i1).run()
    r.check(i1)
    r.load(i2)
    r.run()
    r.check(i2)
    r.load(i3)
    r.run()
    r.check(i3)
    assert [r.result(k) for k in range(4)] != [dg.invert(x, a) for x, a in i1]


# 8. stage times
def test_stage_times(dg, ctx, orc, torch_cuda):
    cases = ic.shaped_cases(dg, orc)[:4]
    items = [(c[1], c[3]) for c in cases]
    r = Run(torch_cuda, dg, ctx, items, timing=True).run()
    t = r.plan.stage_times()
    assert list(t) == ["map", "scan", "emit", "total"]
    assert all(v > 0 for v in t.values()) and t["total"] >= max(t["map"], t["scan"], t["emit"])
    first = r.bytes
    check_ring_phases(r.plan, lambda: r.run(out_cap=r.out_cap), ["map", "scan", "emit", "total"])
    assert r.bytes == first


# 9. the empty plan and the limits
def test_empty_plan_and_limits(dg, ctx, torch_cuda):
    torch = torch_cuda
    p = dg.InvertPlan(ctx, [])
    assert p.output_bound == 0
    off = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    p.run(0, 0, 0, 0, off.data_ptr(), 0, stream=ctx.stream)
    torch.cuda.synchronize()
    assert off.cpu().tolist() == [0]
    for d in [(0, 100, 0, 1 << 32), (0, 1 << 32, 0, 100)]:
        with pytest.raises(dg.DeltaError) as e:
            dg.InvertPlan(ctx, [d])
        assert e.value.code == TOO_LARGE
    assert dg.InvertPlan(ctx, [(0, 1000, 0, 52)]).output_bound == 25 + 13 * 2 + 9 * 3 + 1000 + 1


# 10. encode -> invert -> decode against V: one stream, no host step
def test_device_chain_back_to_r(dg, ctx, orc, torch_cuda):
    import oracle as O
    torch = torch_cuda
    pairs = [orc.synth_pair(0xD00 + k, 16384, 164) for k in range(8)]
    pairs += [orc.synth_transpose(0xE00 + k, 16, 1024) for k in range(8)]
    n = len(pairs)

    def arena(bufs):   # 16-byte aligned spans
        lay, buf = [], bytearray()
        for b in bufs:
            lay.append((len(buf), len(b)))
            buf += b + bytes(-len(b) % 16)
        return torch.frombuffer(buf, dtype=torch.uint8).cuda(), lay, bytes(buf)

    d_r, lr, h_r = arena([p[0] for p in pairs])
    d_v, lv, _ = arena([p[1] for p in pairs])
    enc = dg.EncodePlan(ctx, "correcting", [(a[0], a[1], b[0], b[1]) for a, b in zip(lr, lv)], p=16, q=1)
    inv = dg.InvertPlan(ctx, for_plan=enc)
    # where the inverses will be: the encoder is bit-exact with the oracle, the device inverter with the host's
    deltas = [orc.encode(O.CORRECTING, R, V, p=16, q=1) for R, V in pairs]
    assert sum(not ic.in_key_order(dg, d) for d in deltas) >= 4 and sum(ic.in_key_order(dg, d) for d in deltas) >= 4
    exp = [dg.invert(R, d) for (R, _), d in zip(pairs, deltas)]
    descs, at = [], 0
    for (vo, vl), (ro, rl), e in zip(lv, lr, exp):
        descs.append((vo, vl, at, len(e), ro, rl))
        at += len(e)
    dec = dg.DecodePlan(ctx, descs)
    d_a = torch.zeros(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    d_i = torch.zeros(inv.output_bound, dtype=torch.uint8, device="cuda")
    d_out = torch.full((d_r.numel(),), 0, dtype=torch.uint8, device="cuda")
    oa, oi, olen = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    sa, si, sd = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    s = ctx.stream
    enc.run(d_r.data_ptr(), d_v.data_ptr(), d_a.data_ptr(), d_a.numel(), oa.data_ptr(), sa.data_ptr(), s)
    inv.run(d_r.data_ptr(), d_a.data_ptr(), d_i.data_ptr(), d_i.numel(), oi.data_ptr(), si.data_ptr(),
            d_delta_offsets=oa.data_ptr(), d_delta_status=sa.data_ptr(), stream=s)
    dec.run(d_v.data_ptr(), d_i.data_ptr(), d_out.data_ptr(), olen.data_ptr(), sd.data_ptr(), s)
    torch.cuda.synchronize()
    assert sa.cpu().tolist() == [OK] * n and si.cpu().tolist() == [OK] * n and sd.cpu().tolist() == [OK] * n
    assert bytes(d_out.cpu().numpy()) == h_r
    assert olen.cpu().tolist()[:n] == [ln for _, ln in lr]
    hi, fi = bytes(d_i.cpu().numpy()), oi.cpu().tolist()
    assert [hi[fi[k]:fi[k + 1]] for k in range(n)] == exp


# 11. the CLI checks R's CRC on the GPU
def test_cli_checks_the_reference(dg, orc, tmp_path):
    (R, V, A), _ = ic.damaged(dg, orc)
    pr, pa, po = tmp_path / "r.bin", tmp_path / "a.delta", tmp_path / "inv.delta"
    pa.write_bytes(A)
    pr.write_bytes(bytes([R[0] ^ 1]) + R[1:])
    r = subprocess.run([CLI, "invert", str(pr), str(pa), str(po)], capture_output=True, text=True)
    assert r.returncode == 1 and "source file does not match delta" in r.stderr and not po.exists()
    assert orc.crc64_xz(R).hex() in r.stderr
    pr.write_bytes(R)
    r = subprocess.run([CLI, "invert", str(pr), str(pa), str(po)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert po.read_bytes() == dg.invert(R, A)


# 12. commands cut by, ending at and starting at the end of a parse window (tests/window_cases.py)
def test_parse_window_edges(dg, ctx, orc, torch_cuda):
    items = [(R, d) for _, R, _, d, _ in wc.standard_cases(dg, orc)]
    r = Run(torch_cuda, dg, ctx, items).run()
    assert r.status == [OK] * len(items)
    r.check(items)
