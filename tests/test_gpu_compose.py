"""GPU: dg_compose_plan_* and dg_compose_batch (csrc/dg_compose_dev.hip) produce
byte for byte what the host function dg_compose produces, which
tests/test_compose_cpu.py pins to the Python model.

One batch of every CPU case; a plan over torch buffers at odd arena offsets, with
and without the offsets arrays; payload spans; runs crossing 64-command tiles
and 1 KiB parse windows; the sizing protocol; damaged pairs between good
neighbours; a re-run on other bytes; stage times; and the device chain encode,
encode -> compose -> in-place conversion -> update on one stream.
"""
from __future__ import annotations

import random

import pytest

import compose_cases as cc
import window_cases as wc
from stage_timing import check_ring_phases

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, CAPACITY, MALFORMED, SRC_CRC = 0, 2, 7, 8, 9
GUARD = 0xA5


def host(dg, a, b, ignore_hash=False):
    """(status, bytes) of the host function."""
    try:
        return OK, dg.compose(a, b, ignore_hash=ignore_hash)
    except dg.DeltaError as e:
        return e.code, b""


class Run:
    """One plan over pairs (A, B): the streams in two arenas at odd offsets with
    guard bytes between them; the last stream of each arena ends at the arena's
    last byte.  offsets=True packs the streams and passes n + 1 offsets, the
    descriptors then holding capacities only."""

    def __init__(self, torch, dg, ctx, pairs, *, offsets=False, ignore_hash=False, slack=0, timing=False):
        self.torch, self.dg, self.ctx, self.n = torch, dg, ctx, len(pairs)
        self.offsets = offsets
        n = self.n
        descs, self.pos = [], [[], []]
        at = [1, 3]
        for k, pair in enumerate(pairs):
            d = []
            for w in (0, 1):
                ln = len(pair[w])
                self.pos[w].append(at[w])
                d += [0 if offsets else at[w], ln + slack if offsets else ln]
                at[w] += ln + (0 if offsets or k + 1 == n else 5 + 2 * w)
            descs.append(tuple(d))
        self.size = at
        self.plan = dg.ComposePlan(ctx, descs, ignore_hash=ignore_hash)
        if timing:
            self.plan.set_timing(2)
        self.off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        self.st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.load(pairs)

    def load(self, pairs):
        torch = self.torch
        self.arena, self.in_off = [], []
        for w in (0, 1):
            buf = bytearray([GUARD]) * self.size[w]
            for k, pair in enumerate(pairs):
                buf[self.pos[w][k]:self.pos[w][k] + len(pair[w])] = pair[w]
            assert self.pos[w][-1] + len(pairs[-1][w]) == len(buf)
            self.arena.append(torch.frombuffer(buf, dtype=torch.uint8).cuda())
            self.in_off.append(torch.tensor(self.pos[w] + [len(buf)], dtype=torch.int64, device="cuda"))

    def run(self, out_cap=None, a_status=None, b_status=None):
        """out_cap None: the sizing run first, then the real run into exactly that many bytes."""
        torch = self.torch
        kw = {}
        if self.offsets:
            kw = dict(d_a_offsets=self.in_off[0].data_ptr(), d_b_offsets=self.in_off[1].data_ptr())
        keep = []
        for name, s in (("d_a_status", a_status), ("d_b_status", b_status)):
            if s is not None:
                keep.append(torch.tensor(s, dtype=torch.int32, device="cuda"))
                kw[name] = keep[-1].data_ptr()
        torch.cuda.synchronize()
        if out_cap is None:
            self.plan.run(self.arena[0].data_ptr(), self.arena[1].data_ptr(), 0, 0, self.off.data_ptr(), self.st.data_ptr(),
                          stream=self.ctx.stream, **kw)
            torch.cuda.synchronize()
            self.sizing_off = self.off.cpu().tolist()
            self.sizing_st = self.st.cpu().tolist()
            out_cap = self.sizing_off[-1]
        self.out_cap = out_cap
        pad = 32
        self.out = torch.full((out_cap + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
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

    def check(self, pairs, ignore_hash=False):
        """Every pair as the host function has it; the outputs packed without gaps."""
        at = 0
        for k, (a, b) in enumerate(pairs):
            st, exp = host(self.dg, a, b, ignore_hash)
            assert self.status[k] == st, (k, self.status[k], st)
            assert self.offs[k] == at, k
            assert self.result(k) == exp, k
            at += len(exp)
        assert self.offs[self.n] == at
        assert self.bytes[at:] == bytes([GUARD]) * (self.out_cap - at)


# 1. every CPU case in one batch
def test_all_cpu_cases_in_one_batch(dg, ctx, orc):
    cases = cc.all_cases(dg, orc)
    got = dg.compose_batch([(c[4], c[5]) for c in cases], ctx=ctx)
    for c, g in zip(cases, got):
        assert g == dg.compose(c[4], c[5]), c[0]
        assert dg.decode(c[1], g, ctx=ctx) == c[3], c[0]
    assert dg.compose_batch([], ctx=ctx) == []


# 2. a plan over torch buffers: odd offsets, the arenas' last bytes, with and without offsets arrays
@pytest.mark.parametrize("offsets", [False, True])
def test_plan_over_torch_buffers(dg, ctx, orc, torch_cuda, offsets):
    cases = cc.random_cases(dg, orc)[:12] + cc.shaped_cases(dg, orc) + cc.realistic_cases(dg, orc)[2:]
    pairs = [(c[4], c[5]) for c in cases]
    r = Run(torch_cuda, dg, ctx, pairs, offsets=offsets, slack=7).run()
    assert r.sizing_st == [CAPACITY] * len(pairs)   # the sizing run: every OK pair reports out_cap
    assert r.sizing_off == r.offs
    r.check(pairs)


# 3. payload spans at odd source and destination offsets
def test_payload_spans(dg, ctx, orc, torch_cuda):
    c = next(c for c in cc.shaped_cases(dg, orc) if c[0] == "payload_spans")
    assert {len(x.data) for x in dg.decode_delta(c[5])[0] if isinstance(x, dg.PlacedAdd)} >= set(cc.SPANS)
    # shifted by one more literal byte in front, so that every span moves to the other parity
    R, V1 = c[1], c[2]
    b2 = [("A", b"\x02\x03")] + [("C", x.src, x.length) if isinstance(x, dg.PlacedCopy) else ("A", bytes(x.data))
                                 for x in dg.decode_delta(c[5])[0]]
    pairs = [(c[4], c[5]), (c[4], cc.make_delta(dg, orc, b2, V1))]
    r = Run(torch_cuda, dg, ctx, pairs).run()
    r.check(pairs)
    assert dg.decode(R, r.result(1), ctx=ctx) == cc.apply(b2, V1)


# 4. runs crossing 64-command tiles of B, streams crossing 1 KiB parse windows
def test_long_runs_and_windows(dg, ctx, orc, torch_cuda):
    rng = random.Random(31)
    R = rng.randbytes(4000)
    lit = rng.randbytes
    cases = [
        # one COPY run swallowing 200 whole commands of B, across three tiles and two windows
        cc.case(dg, orc, "copy_run", R, [("C", 100, 3000)], [("A", lit(3))] + [("C", 7 * k, 7) for k in range(200)] + [("A", lit(1))]),
        # one ADD run of 150 commands of B mixed from B's literals and A's
        cc.case(dg, orc, "add_run", R, [("C", 0, 10), ("A", lit(500)), ("C", 10, 10)],
                [("C", 0, 10)] + [("A", lit(2)) if k % 3 else ("C", 10 + 3 * k, 3) for k in range(150)] + [("C", 510, 10)]),
        # a run that ends exactly at a tile's last command, and one that begins at a tile's first
        cc.case(dg, orc, "tile_edges", R, [("C", 0, 2000)],
                [("C", 5 * k, 5) for k in range(64)] + [("C", 1000 + 5 * k, 5) for k in range(64)] + [("A", lit(4))]),
        # many commands of A under one COPY of B, and B copying A's commands piecewise
        cc.case(dg, orc, "wide_copy", R, cc.random_cmds(rng, len(R), 400, bytes(range(256)), max_len=9), [("C", 1, 900), ("C", 0, 901)]),
        next(c for c in cc.shaped_cases(dg, orc) if c[0] == "window_cut"),
    ]
    assert all(len(c[5]) > 1024 + 25 for c in cases[:3]) and len(cases[3][4]) > 3 * 1024
    pairs = [(c[4], c[5]) for c in cases]
    r = Run(torch_cuda, dg, ctx, pairs, offsets=True).run()
    r.check(pairs)
    for k, c in enumerate(cases):
        assert dg.decode(c[1], r.result(k), ctx=ctx) == c[3], c[0]
    assert [type(x).__name__ for x in dg.decode_delta(r.result(0))[0]] == ["PlacedAdd", "PlacedCopy", "PlacedAdd"]


# 5. sizing: an out_cap that fits only the first k pairs
def test_out_cap_fits_first_pairs(dg, ctx, orc, torch_cuda):
    cases = cc.shaped_cases(dg, orc)[:8]
    pairs = [(c[4], c[5]) for c in cases]
    exp = [dg.compose(a, b) for a, b in pairs]
    k = 5
    cap = sum(len(e) for e in exp[:k]) + len(exp[k]) - 1   # one byte short for pair k
    r = Run(torch_cuda, dg, ctx, pairs).run(out_cap=cap)
    assert r.status == [OK] * k + [CAPACITY] * (len(pairs) - k)
    at = 0
    for i, e in enumerate(exp):   # the offsets still count every pair's size
        assert r.offs[i] == at
        at += len(e)
        if i < k:
            assert r.result(i) == e
    assert r.offs[-1] == at
    assert r.bytes[sum(len(e) for e in exp[:k]):] == bytes([GUARD]) * (len(exp[k]) - 1)   # a failed output is empty


# 6. each kind of damage between good neighbours; incoming statuses are passed on
@pytest.mark.parametrize("offsets", [False, True])
def test_damage_between_good_neighbours(dg, ctx, orc, torch_cuda, offsets):
    (R, V1, V2, A, B), bad = cc.damaged(dg, orc)
    good = cc.realistic_cases(dg, orc)[2]
    pairs = [(good[4], good[5])]
    for _, a, b, _ in bad:
        pairs += [(a, b), (A, B)]
    r = Run(torch_cuda, dg, ctx, pairs, offsets=offsets).run()
    r.check(pairs)
    assert [r.status[1 + 2 * k] for k in range(len(bad))] == [x[3] for x in bad]
    assert all(r.offs[2 + 2 * k] == r.offs[1 + 2 * k] for k in range(len(bad)))
    # incoming statuses: A's first, then B's; a failed input's bytes are not looked at
    n = len(pairs)
    sa, sb = [0] * n, [0] * n
    sa[0], sb[0] = 11, 5
    sb[2] = 6
    sa[1] = 4   # beats the pair's own defect
    r2 = Run(torch_cuda, dg, ctx, pairs, offsets=offsets).run(out_cap=r.offs[-1], a_status=sa, b_status=sb)
    assert r2.status[:3] == [11, 4, 6] and r2.status[3:] == r.status[3:]
    assert r2.result(0) == b"" and r2.result(2) == b"" and r2.result(4) == r.result(4)
    # ignore_hash skips the CRC comparison alone
    r3 = Run(torch_cuda, dg, ctx, pairs, offsets=offsets, ignore_hash=True).run()
    r3.check(pairs, ignore_hash=True)
    assert r3.status != r.status


def test_stream_longer_than_capacity(dg, ctx, orc, torch_cuda):
    """With offsets a capacity bounds the stream; one byte more is DG_ERR_CAPACITY."""
    (R, V1, V2, A, B), _ = cc.damaged(dg, orc)
    pairs = [(A, B), (A, B), (A, B)]
    r = Run(torch_cuda, dg, ctx, pairs, offsets=True)
    r.plan.close()
    r.plan = dg.ComposePlan(ctx, [(0, len(A), 0, len(B)), (0, len(A) - 1, 0, len(B)), (0, len(A), 0, len(B) - 1)])
    r.run()
    assert r.status == [OK, CAPACITY, CAPACITY]
    assert r.result(0) == dg.compose(A, B) and r.offs[1:] == [len(r.result(0))] * 3


# 7. the same plan on other bytes of the same layout: no stale tables
def test_rerun_on_other_bytes(dg, ctx, orc, torch_cuda):
    rng = random.Random(41)
    R = rng.randbytes(600)

    def variant(seed):
        g = random.Random(seed)
        out = []
        for n in (0, 5, 70, 140):
            # fixed stream sizes: n COPYs in A, n COPYs and one 4-byte ADD in B
            a = [("C", g.randrange(0, 500), 3) for _ in range(n)] + [("A", g.randbytes(8))]
            b = [("C", g.randrange(0, 3 * n + 5), 2) for _ in range(n)] + [("A", g.randbytes(4))]
            out.append(cc.case(dg, orc, f"v{n}", R, a, b))
        return out

    first, second = variant(1), variant(2)
    assert [len(c[4]) for c in first] == [len(c[4]) for c in second] and [len(c[5]) for c in first] == [len(c[5]) for c in second]
    p1, p2 = [(c[4], c[5]) for c in first], [(c[4], c[5]) for c in second]
    r = Run(torch_cuda, dg, ctx, p1).run()
    r.check(p1)
    r.load(p2)
    r.run()
    r.check(p2)
    assert [r.result(k) for k in range(4)] != [dg.compose(a, b) for a, b in p1]


# 8. stage times
def test_stage_times(dg, ctx, orc, torch_cuda):
    cases = cc.shaped_cases(dg, orc)[:4]
    pairs = [(c[4], c[5]) for c in cases]
    r = Run(torch_cuda, dg, ctx, pairs, timing=True).run()
    t = r.plan.stage_times()
    assert list(t) == ["map", "scan", "emit", "total"]
    assert all(v > 0 for v in t.values()) and t["total"] >= max(t["map"], t["scan"], t["emit"])
    first = r.bytes
    check_ring_phases(r.plan, lambda: r.run(out_cap=r.out_cap), ["map", "scan", "emit", "total"])
    assert r.bytes == first


def test_empty_plan_and_limits(dg, ctx, torch_cuda):
    torch = torch_cuda
    p = dg.ComposePlan(ctx, [])
    off = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    p.run(0, 0, 0, 0, off.data_ptr(), 0, stream=ctx.stream)
    torch.cuda.synchronize()
    assert off.cpu().tolist() == [0]
    with pytest.raises(dg.DeltaError) as e:
        dg.ComposePlan(ctx, [(0, 1 << 32, 0, 100)])
    assert e.value.code == 3


# 9. encode, encode -> compose -> in-place conversion -> update: one stream, no host step
def test_device_chain_r_to_v2(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    rng = random.Random(61)
    n = 16
    Rs, V1s, V2s = [], [], []
    for _ in range(n):
        R = rng.randbytes(rng.randint(150, 200))
        V1 = bytearray(R)
        V1[40:44] = rng.randbytes(9)
        V2 = bytearray(V1)
        V2[100:103] = b""
        V2[10] ^= 0xFF
        Rs.append(R), V1s.append(bytes(V1)), V2s.append(bytes(V2))

    def arena(bufs):
        lay, at = [], 0
        for b in bufs:
            lay.append((at, len(b)))
            at += len(b)
        return torch.frombuffer(bytearray(b"".join(bufs)), dtype=torch.uint8).cuda(), lay

    d_r, lr = arena(Rs)
    d_v1, l1 = arena(V1s)
    d_v2, l2 = arena(V2s)
    enc_a = dg.EncodePlan(ctx, "onepass", [(a[0], a[1], b[0], b[1]) for a, b in zip(lr, l1)], p=16, q=1)
    enc_b = dg.EncodePlan(ctx, "onepass", [(a[0], a[1], b[0], b[1]) for a, b in zip(l1, l2)], p=16, q=1)
    comp = dg.ComposePlan(ctx, for_plans=(enc_a, enc_b))
    cap = 1024   # a composed delta of these pairs is a few hundred bytes
    ip = dg.InplacePlan(ctx, [(o, ln, 0, cap) for o, ln in lr])
    # the buffers that hold R: max(|R|, |V2|) bytes each
    descs, buf, pos = [], bytearray(), 0
    for R, V2 in zip(Rs, V2s):
        room = max(len(R), len(V2))
        descs.append((pos, room, len(R), 0, 2 * cap))
        buf += R + bytes([GUARD]) * (room - len(R))
        pos += room
    up = dg.UpdatePlan(ctx, descs)
    d_buf = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    d_a = torch.zeros(max(enc_a.output_bound, 1), dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(max(enc_b.output_bound, 1), dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    d_i = torch.zeros(2 * n * cap, dtype=torch.uint8, device="cuda")
    oa, ob, oc, oi, ulen = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(5))
    sa, sb, sc, si, su = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(5))
    torch.cuda.synchronize()
    s = ctx.stream
    enc_a.run(d_r.data_ptr(), d_v1.data_ptr(), d_a.data_ptr(), d_a.numel(), oa.data_ptr(), sa.data_ptr(), s)
    enc_b.run(d_v1.data_ptr(), d_v2.data_ptr(), d_b.data_ptr(), d_b.numel(), ob.data_ptr(), sb.data_ptr(), s)
    comp.run(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), d_c.numel(), oc.data_ptr(), sc.data_ptr(),
             d_a_offsets=oa.data_ptr(), d_a_status=sa.data_ptr(), d_b_offsets=ob.data_ptr(), d_b_status=sb.data_ptr(), stream=s)
    ip.run(d_r.data_ptr(), d_c.data_ptr(), d_i.data_ptr(), d_i.numel(), oi.data_ptr(), si.data_ptr(),
           d_delta_offsets=oc.data_ptr(), d_delta_status=sc.data_ptr(), stream=s)
    up.run(d_buf.data_ptr(), d_i.data_ptr(), ulen.data_ptr(), su.data_ptr(), d_delta_offsets=oi.data_ptr(),
           d_delta_status=si.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert sc.cpu().tolist() == [OK] * n and su.cpu().tolist() == [OK] * n
    got, lens = bytes(d_buf.cpu().numpy()), ulen.cpu().tolist()
    for k, (o, *_rest) in enumerate(descs):
        assert lens[k] == len(V2s[k]) and got[o:o + len(V2s[k])] == V2s[k], k
    # and the composed deltas are the host function's, of the encoders' outputs
    ha, hb, hc = bytes(d_a.cpu().numpy()), bytes(d_b.cpu().numpy()), bytes(d_c.cpu().numpy())
    fa, fb, fc = oa.cpu().tolist(), ob.cpu().tolist(), oc.cpu().tolist()
    for k in range(n):
        assert hc[fc[k]:fc[k + 1]] == dg.compose(ha[fa[k]:fa[k + 1]], hb[fb[k]:fb[k + 1]]), k


# 12. commands cut by, ending at and starting at the end of a parse window
#     (tests/window_cases.py): each stream as A before an identity B, and as B after an identity A
def test_parse_window_edges(dg, ctx, orc, torch_cuda):
    cases = wc.standard_cases(dg, orc)
    ident_r = cc.identity_delta(dg, orc, cases[0][1])
    pairs = [(d, cc.identity_delta(dg, orc, V)) for _, _, V, d, _ in cases] + [(ident_r, d) for _, _, _, d, _ in cases]
    r = Run(torch_cuda, dg, ctx, pairs).run()
    assert r.status == [OK] * len(pairs)
    r.check(pairs)
