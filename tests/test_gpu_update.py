"""GPU: in-place deltas applied in place (dg_update_plan_*, dg_update_batch).

Each stream's buffer holds R and must hold V afterwards; the expected bytes are
the oracle's sequential replay (apply.c:271-284).  A stream that does not pass
validation must keep every byte.  Buffers sit in one arena between 0xA5 guard
bytes, which no run may change.

Sizes: |R| about 20 000 gives a command stream of three or more 4 KiB parse
windows, |R| about 3000 one partial window.  The 4096-byte block rotation has no
one-window form (its ADD payload alone fills a window); it runs at the large
size only.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import random

import pytest

import window_cases as wc

from stage_timing import check_ring_phases
from test_oracle import inplace_inputs
from update_cases import (DAMAGES, DECODE_AGREES, MOVE_KINDS, ORDER_KINDS, WINDOW, damage, make_delta, moves_case,
                          order_case, pad_noops, three_window_stream, version_size)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden_inplace.json")))["cases"]
OK, INVALID_ARG, UNSUPPORTED, CAPACITY, MALFORMED, SRC_CRC, DST_CRC = 0, 1, 2, 7, 8, 9, 10
GUARD = 0xA5


class Run:
    """One plan over `items` = (R, delta) laid out in one arena: `start` guard
    bytes, then every region (buf_cap bytes, default max(|R|, version_size)),
    `gap` guard bytes between regions and `tail` after the last.  Bytes of a
    region past |R| start as `fill`."""

    def __init__(self, torch, dg, ctx, items, *, caps=None, start=16, gap=16, tail=16, fill=GUARD, ignore_hash=False,
                 timing=False):
        self.torch, self.ctx, self.items = torch, ctx, items
        n = self.n = len(items)
        self.regions, descs, pos, dpos = [], [], start, 0
        for k, (R, d) in enumerate(items):
            cap = caps[k] if caps and caps[k] is not None else max(len(R), version_size(d))
            room = max(cap, len(R))   # (a buf_cap below |R| is a test of the capacity check)
            self.regions.append((pos, room))
            descs.append((pos, cap, len(R), dpos, len(d)))
            pos += room + (gap if k + 1 < n else tail)
            dpos += len(d)
        self.size = max(pos if n else start + tail, 1)
        self.fill = fill
        self.descs = descs
        self.plan = dg.UpdatePlan(ctx, descs, ignore_hash=ignore_hash)
        if timing:
            self.plan.set_timing(2)
        self.d_delta = torch.frombuffer(bytearray(b"".join(d for _, d in items) or b"\0"), dtype=torch.uint8).cuda()
        self.d_len = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
        self.d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
        self.load(items)

    def load(self, items):
        """The arena as before a run: guards, every R at its region's start."""
        buf = bytearray([GUARD]) * self.size
        for (o, room), (R, _) in zip(self.regions, items):
            buf[o:o + room] = bytes([self.fill]) * room
            buf[o:o + len(R)] = R
        self.before = bytes(buf)
        self.d_buf = self.torch.frombuffer(buf, dtype=self.torch.uint8).cuda()
        assert self.d_buf.numel() == self.size and self.d_buf.data_ptr() % 16 == 0

    def run(self):
        self.torch.cuda.synchronize()
        self.plan.run(self.d_buf.data_ptr(), self.d_delta.data_ptr(), self.d_len.data_ptr(), self.d_st.data_ptr(),
                      stream=self.ctx.stream)
        self.torch.cuda.synchronize()
        self.after = bytes(self.d_buf.cpu().numpy())
        self.st = self.d_st.cpu().tolist()[:self.n]
        self.out_len = self.d_len.cpu().tolist()[:self.n]
        return self

    def region(self, k, after=True):
        o, room = self.regions[k]
        return (self.after if after else self.before)[o:o + room]

    def outside_unchanged(self):
        """Guards, and every region's bytes at and past bsz, are as they were."""
        keep = bytearray(b"\1") * self.size
        for (o, _), (R, d), s in zip(self.regions, self.items, self.st):
            if s in (OK, DST_CRC):
                bsz = max(len(R), version_size(d))
                keep[o:o + bsz] = bytes(bsz)
        return all(a == b for a, b, k in zip(self.after, self.before, keep) if k)

    def check_ok(self, k, V):
        assert self.st[k] == OK, (k, self.st[k])
        assert self.out_len[k] == len(V), k
        assert self.region(k)[:len(V)] == V, k


def _apply_all(torch, dg, ctx, cases, **kw):
    """cases: (R, delta, V); one run, every buffer must become V."""
    r = Run(torch, dg, ctx, [(R, d) for R, d, _ in cases], **kw).run()
    for k, (_, _, V) in enumerate(cases):
        r.check_ok(k, V)
    assert r.outside_unchanged()
    return r


# 1. order cases and moving families, at three or more windows and at one partial window
@pytest.mark.parametrize("size", ["windows", "one_window"])
@pytest.mark.parametrize("kind", ORDER_KINDS)
def test_order_cases(dg, ctx, orc, torch_cuda, kind, size):
    rng = random.Random(3000 + ORDER_KINDS.index(kind))
    cases = []
    for _ in range(3):
        if size == "windows":
            R, cmds, vs = order_case(dg, rng, kind)
        else:
            R, cmds, vs = order_case(dg, rng, kind, n_r=3000, n_cmds=rng.randint(2, 110))
        d, V = make_delta(dg, orc, R, cmds, vs)
        assert len(d) > 3 * WINDOW if size == "windows" else len(d) < WINDOW
        cases.append((R, d, V))
    _apply_all(torch_cuda, dg, ctx, cases)


@pytest.mark.parametrize("size", ["windows", "one_window"])
@pytest.mark.parametrize("kind", MOVE_KINDS)
def test_moving_families(dg, ctx, orc, torch_cuda, kind, size):
    if kind == "rotate4096" and size == "one_window":
        return   # no such stream: the rotation's ADD carries 4096 payload bytes (see the module docstring)
    rng = random.Random(4000 + MOVE_KINDS.index(kind))
    cases = []
    for _ in range(2):
        R, cmds, vs = moves_case(dg, rng, kind, 20000 if size == "windows" else 3000)
        if size == "windows":   # COPYs onto themselves in front, until the stream spans three windows
            est = sum(13 if isinstance(c, dg.PlacedCopy) else 9 + len(c.data) for c in cmds)
            cmds = pad_noops(dg, rng, cmds, len(R), max(0, (3 * WINDOW + 200 - est) // 13 + 1))
        d, V = make_delta(dg, orc, R, cmds, vs)
        assert len(d) > 3 * WINDOW if size == "windows" else len(d) < WINDOW, len(d)
        cases.append((R, d, V))
    _apply_all(torch_cuda, dg, ctx, cases)


# 2. the reference's own in-place deltas: the buffer becomes V
def test_reference_goldens(dg, ctx, orc, torch_cuda):
    assert len(GOLDEN) == 44
    cases = []
    for c in GOLDEN:
        R, V = inplace_inputs(orc, c)
        cases.append((R, bytes.fromhex(c["delta_hex"]), V))
    _apply_all(torch_cuda, dg, ctx, cases, start=1, gap=0)


# 3. encode -> in-place conversion -> update on one stream, device offsets and status, no host step
def _chain(torch, dg, ctx, ref_t, ver_t, lay, algo, policy, q):
    n = len(lay)
    ref_h, ver_h = bytes(ref_t.cpu().numpy()), bytes(ver_t.cpu().numpy())
    enc = dg.EncodePlan(ctx, algo, lay, p=16, q=q)
    ip = dg.InplacePlan(ctx, policy=policy, for_plan=enc)
    # a copy of the reference arena, stream i in a buffer of max(|R|, |V|) bytes
    descs, pos, buf = [], 0, bytearray()
    bound = min(ip.output_bound, (1 << 32) - 1)
    for ro, rl, vo, vl in lay:
        cap = max(rl, vl)
        descs.append((pos, cap, rl, 0, bound))
        buf += ref_h[ro:ro + rl] + bytes([GUARD]) * (cap - rl)
        pos += cap
    up = dg.UpdatePlan(ctx, descs)
    d_buf = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    d_std = torch.zeros(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
    d_ipd = torch.zeros(max(ip.output_bound, 1), dtype=torch.uint8, device="cuda")
    off1, off2, ulen = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    st1, st2, st3 = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    enc.run(ref_t.data_ptr(), ver_t.data_ptr(), d_std.data_ptr(), d_std.numel(), off1.data_ptr(), st1.data_ptr(),
            ctx.stream)
    ip.run(ref_t.data_ptr(), d_std.data_ptr(), d_ipd.data_ptr(), d_ipd.numel(), off2.data_ptr(), st2.data_ptr(),
           d_delta_offsets=off1.data_ptr(), d_delta_status=st1.data_ptr(), stream=ctx.stream)
    up.run(d_buf.data_ptr(), d_ipd.data_ptr(), ulen.data_ptr(), st3.data_ptr(), d_delta_offsets=off2.data_ptr(),
           d_delta_status=st2.data_ptr(), stream=ctx.stream)
    torch.cuda.synchronize()
    assert st3.cpu().tolist() == [OK] * n
    got, lens = bytes(d_buf.cpu().numpy()), ulen.cpu().tolist()
    for k, ((o, cap, _, _, _), (_, _, vo, vl)) in enumerate(zip(descs, lay)):
        assert lens[k] == vl and got[o:o + vl] == ver_h[vo:vo + vl], k


@pytest.mark.parametrize("policy", ["localmin", "constant"])
def test_device_chain(dg, ctx, orc, torch_cuda, policy):
    torch = torch_cuda
    # 16 onepass pairs of 64 KiB with substitutions
    pairs = [orc.synth_pair(0xC5000000 + i, 65536, 655) for i in range(16)]
    lay = [(65536 * i, 65536, 65536 * i, 65536) for i in range(16)]
    ref_t = torch.frombuffer(bytearray(b"".join(r for r, _ in pairs)), dtype=torch.uint8).cuda()
    ver_t = torch.frombuffer(bytearray(b"".join(v for _, v in pairs)), dtype=torch.uint8).cuda()
    _chain(torch, dg, ctx, ref_t, ver_t, lay, "onepass", policy, 4099)
    # 16 correcting pairs of about 16 KiB of transposed blocks, made on the device
    n, target, seed = 16, 16384, 0xC4100000
    pr = (dg._lib.Pair * n)()
    rb, vb = C.c_uint64(), C.c_uint64()
    ctx.check(dg.lib.dg_synth_transpose_pairs_device(ctx.handle, seed, n, target, 50, pr, C.byref(rb), C.byref(vb),
                                                     None, None, None), "layout")
    ref_t = torch.empty(rb.value, dtype=torch.uint8, device="cuda")
    ver_t = torch.empty(vb.value, dtype=torch.uint8, device="cuda")
    ctx.check(dg.lib.dg_synth_transpose_pairs_device(ctx.handle, seed, n, target, 50, pr, C.byref(rb), C.byref(vb),
                                                     ref_t.data_ptr(), ver_t.data_ptr(), None), "synth")
    torch.cuda.synchronize()
    _chain(torch, dg, ctx, ref_t, ver_t, [(p.r_off, p.r_len, p.v_off, p.v_len) for p in pr], "correcting", policy, 1)


# 4. all or nothing: a damaged stream between two good neighbours keeps every byte
@pytest.fixture(scope="module")
def base3(dg, orc):
    rng = random.Random(51)
    good = []
    for _ in range(2):
        R, cmds, vs = order_case(dg, rng, "c5_shape", n_r=5000, n_cmds=300)
        good.append((R, *make_delta(dg, orc, R, cmds, vs)))
    return three_window_stream(dg, orc, rng), good


@pytest.mark.parametrize("how", DAMAGES)
def test_all_or_nothing(dg, ctx, orc, torch_cuda, base3, how):
    (R, d, V), good = base3
    bad, cap, want = damage(d, R, how)
    items = [good[0][:2], (R, bad), good[1][:2]]
    r = Run(torch_cuda, dg, ctx, items, caps=[None, cap, None]).run()
    assert r.st[1] == want and r.out_len[1] == 0
    assert r.region(1) == r.region(1, after=False)        # the damaged stream's buffer, byte for byte
    r.check_ok(0, good[0][2])
    r.check_ok(2, good[1][2])
    assert r.outside_unchanged()                          # all guards
    if how in DECODE_AGREES:
        with pytest.raises(dg.DeltaError) as e:
            dg.decode(R, bad, ctx=ctx)
        assert e.value.code == r.st[1]


# 5. a wrong dst_crc is reported after the replay; ignore_hash skips both checks
def test_dst_crc_and_ignore_hash(dg, ctx, orc, torch_cuda, base3):
    (R, d, V), _ = base3
    wrong_dst = d[:17] + bytes([d[17] ^ 1]) + d[18:]
    both = d[:9] + bytes([d[9] ^ 1]) + d[10:17] + bytes([d[17] ^ 1]) + d[18:]
    r = Run(torch_cuda, dg, ctx, [(R, wrong_dst), (R, d)]).run()
    assert r.st == [DST_CRC, OK] and r.out_len == [len(V)] * 2
    assert r.region(0)[:len(V)] == V and r.region(1)[:len(V)] == V
    assert r.outside_unchanged()
    r = Run(torch_cuda, dg, ctx, [(R, both)], ignore_hash=True).run()
    r.check_ok(0, V)
    r = Run(torch_cuda, dg, ctx, [(R, both)]).run()
    assert r.st == [SRC_CRC] and r.after == r.before


# 6. layout: odd offsets, touching regions, the arena's last byte, tiny and empty streams, an uncovered tail
def test_layout_edges(dg, ctx, orc, torch_cuda):
    rng = random.Random(61)
    cases = []
    for n_r in (0, 1, 7, 8):
        R = rng.randbytes(n_r)
        cmds = [dg.PlacedCopy(src=0, dst=0, length=n_r)] if n_r else []
        cmds.append(dg.PlacedAdd(dst=n_r, data=rng.randbytes(5 + n_r)))
        cases.append((R, *make_delta(dg, orc, R, cmds, 2 * n_r + 5)))
    R = rng.randbytes(33)
    cases.append((R, *make_delta(dg, orc, R, [], 0)))                       # version_size = 0
    R = rng.randbytes(1001)                                                 # grows by 600; bytes [1101, 1501) uncovered
    cmds = [dg.PlacedCopy(src=0, dst=0, length=1001), dg.PlacedAdd(dst=1001, data=rng.randbytes(100)),
            dg.PlacedAdd(dst=1501, data=rng.randbytes(100))]
    grow = (R, *make_delta(dg, orc, R, cmds, 1601))
    assert grow[2][1101:1501] == bytes(400)
    cases.append(grow)
    for kind in ("moving", "shrink"):
        R, cmds, vs = order_case(dg, rng, kind, n_r=3001, n_cmds=150)
        cases.append((R, *make_delta(dg, orc, R, cmds, vs)))
    # regions touch (gap 0) from an odd start, each buf_cap one byte larger where the next offset would be even;
    # 0xFF where a region is not R; the last region ends the allocation
    caps, pos = [], 1
    for R, d, _ in cases:
        cap = max(len(R), version_size(d))
        cap += (pos + cap) % 2 == 0   # the next region starts at an odd offset too
        caps.append(cap)
        pos += cap
    r = _apply_all(torch_cuda, dg, ctx, cases, caps=caps, start=1, gap=0, tail=0, fill=0xFF)
    assert all(o % 2 == 1 for o, _ in r.regions)
    assert r.regions[-1][0] + r.regions[-1][1] == r.size == r.d_buf.numel()
    assert r.region(5)[1101:1501] == bytes(400)


# 7. one plan, run again on other data in the same layout, then on buffers that already hold V
def test_rerun(dg, ctx, orc, torch_cuda):
    shape = random.Random(71)
    n_r, spots, p = 12000, [], 0
    while p < n_r - 64:
        ln = shape.randint(1, 24)
        spots.append((p, ln))
        p += ln + shape.randint(0, 30)

    def batch(seed):   # the same commands at the same places: equal stream lengths, other bytes
        rng, out = random.Random(seed), []
        for _ in range(4):
            R = rng.randbytes(n_r)
            cmds = [dg.PlacedCopy(src=0, dst=0, length=n_r)] + [dg.PlacedAdd(dst=o, data=rng.randbytes(ln)) for o, ln in spots]
            out.append((R, *make_delta(dg, orc, R, cmds, n_r)))
        return out

    A, B = batch(1), batch(2)
    assert [len(d) for _, d, _ in A] == [len(d) for _, d, _ in B] and len(A[0][1]) > 2 * WINDOW
    r = Run(torch_cuda, dg, ctx, [(R, d) for R, d, _ in A]).run()
    for k, (_, _, V) in enumerate(A):
        r.check_ok(k, V)
    r.items = [(R, d) for R, d, _ in B]
    r.load(r.items)
    r.d_delta.copy_(torch_cuda.frombuffer(bytearray(b"".join(d for _, d, _ in B)), dtype=torch_cuda.uint8))
    r.run()
    for k, (_, _, V) in enumerate(B):
        r.check_ok(k, V)
    assert r.outside_unchanged()
    held = r.after
    r.run()   # the buffers hold V now, not the deltas' R
    assert r.st == [SRC_CRC] * 4 and r.out_len == [0] * 4 and r.after == held


# 7b. a stream with more commands than the plan keeps lists for (64 KiB: 2 bytes per command and 32 per
#     window): phase B parses it again; its neighbour's lists are kept
def test_stream_longer_than_the_kept_lists(dg, ctx, orc, torch_cuda, base3):
    rng = random.Random(81)
    n_r = 300000
    R = rng.randbytes(n_r)
    cmds = [dg.PlacedCopy(src=8 * k, dst=8 * k, length=8) for k in range(34000)]
    cmds += [dg.PlacedCopy(src=280000 + 100 * k, dst=272000 + 100 * k, length=100) for k in range(50)]   # moving
    cmds += [dg.PlacedAdd(dst=rng.randrange(0, n_r - 40), data=rng.randbytes(rng.randint(1, 40))) for _ in range(500)]
    d, V = make_delta(dg, orc, R, cmds, n_r)
    assert 2 * len(cmds) + 32 * (len(d) // WINDOW) > 65536
    (R3, d3, V3), _ = base3
    _apply_all(torch_cuda, dg, ctx, [(R3, d3, V3), (R, d, V), (R3, d3, V3)])
    bad = d[:len(d) - 30]   # cut inside the last ADDs: nothing may change
    r = Run(torch_cuda, dg, ctx, [(R, bad), (R3, d3)]).run()
    assert r.st == [MALFORMED, OK] and r.region(0) == r.region(0, after=False)


# 8. plan errors and the other surfaces
def test_plan_errors_and_surfaces(dg, ctx, orc, torch_cuda, base3):
    (R, d, V), good = base3
    with pytest.raises(dg.DeltaError) as e:
        dg.UpdatePlan(ctx, [(0, 100, 50, 0, 40), (99, 100, 50, 40, 40)])
    assert e.value.code == INVALID_ARG
    dg.UpdatePlan(ctx, [(0, 100, 50, 0, 40), (100, 100, 50, 40, 40)]).close()   # touching is not overlapping
    empty = dg.UpdatePlan(ctx, [])
    empty.run(0, 0, 0, 0, stream=ctx.stream)
    empty.close()
    assert dg.update_batch([], ctx=ctx) == []
    r = Run(torch_cuda, dg, ctx, [(R, d)], timing=True).run()
    t = r.plan.stage_times()
    assert set(t) >= {"update", "total"} and t["update"] > 0 and t["total"] >= t["update"]

    def rerun():   # the buffer holds R again
        r.load([(R, d)])
        r.run().check_ok(0, V)
    check_ring_phases(r.plan, rerun, ["update", "total"])
    # a mixed batch with one failing item: the host entry point equals the plan
    bad, _, want = damage(d, R, "cut_window3")
    items = [good[0][:2], (R, bad), (R, d), good[1][:2]]
    r = Run(torch_cuda, dg, ctx, items).run()
    assert r.st == [OK, want, OK, OK]
    res, st = dg.update_batch(items, ctx=ctx, status=True)
    assert st == r.st
    for k, ((Rk, dk), got) in enumerate(zip(items, res)):
        if st[k] == OK:
            assert got == r.region(k)[:r.out_len[k]], k
        else:
            assert got is None
    assert res[2] == V
    with pytest.raises(dg.DeltaError) as e:
        dg.update_batch(items, ctx=ctx)
    assert e.value.code == want
    assert dg.update_batch([items[0], items[2]], ctx=ctx) == [good[0][2], V]


# commands cut by, ending at and starting at the end of a parse window, in in-place
# streams built directly (tests/window_cases.py); V is the oracle's replay
def test_parse_window_edges(dg, ctx, orc, torch_cuda):
    _apply_all(torch_cuda, dg, ctx, [(R, d, V) for _, R, V, d, _ in wc.inplace_cases(dg, orc)])
