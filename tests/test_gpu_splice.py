"""GPU: dg_splice_plan_*, dg_splice_batch and dg_encode_large
(csrc/dg_splice_dev.hip, csrc/dg_splice_host.cpp) produce byte for byte what the
host function dg_splice produces, which tests/test_splice_cpu.py pins to the
Python model.

The whole CPU corpus in one batch of mixed groups; a plan over torch buffers
with the sizing run; out_cap cut inside each group in turn between guard bytes;
damaged segments between good groups; a stream longer than its capacity; a
re-run on other bytes; the chain encode plan -> splice plan -> decode plan on
one stream for the three algorithms; encode_large and the CLI's --segment-size
against the decoders.
"""
from __future__ import annotations

import os
import random
import subprocess

import pytest

import compose_cases as cc
import splice_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")
OK, CAPACITY = 0, 7
GUARD = 0xA5


def host(dg, grp):
    """(status, bytes) of the host function for (segments, deltas, whole, src_crc[, seg_status])."""
    try:
        return OK, dg.splice(grp[0], grp[1], grp[2], grp[3], grp[4] if len(grp) > 4 else None)
    except dg.DeltaError as e:
        return e.code, b""


def group_of(orc, c):
    return (c[4], c[5], c[3], orc.crc64_xz(c[1]))


class Run:
    """One plan over groups: every segment stream packed into one arena from an
    odd offset, n_seg + 1 offsets, capacities = the lengths + slack."""

    def __init__(self, torch, dg, ctx, groups, *, slack=0, caps=True, timing=False):
        self.torch, self.dg, self.ctx, self.groups = torch, dg, ctx, groups
        self.ng = len(groups)
        segs, first, lens = [], [0], []
        for g in groups:
            segs += list(g[0])
            lens += [len(d) for d in g[1]]
            first.append(len(segs))
        self.ns = len(segs)
        self.plan = dg.SplicePlan(ctx, [g[2] for g in groups], first, segments=segs,
                                  caps=[n + slack for n in lens] if caps else None)
        if timing:
            self.plan.set_timing(2)
        self.off = torch.zeros(self.ng + 1, dtype=torch.int64, device="cuda")
        self.st = torch.full((self.ng,), -1, dtype=torch.int32, device="cuda")
        self.load(groups)

    def load(self, groups):
        torch = self.torch
        blob, offs = bytearray([GUARD]), []
        for g in groups:
            for d in g[1]:
                offs.append(len(blob))
                blob += d
        offs.append(len(blob))
        self.arena = torch.frombuffer(blob, dtype=torch.uint8).cuda()
        self.in_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        crc = [int.from_bytes(g[3], "big") for g in groups]
        self.crc = torch.tensor([x - (1 << 64) if x >> 63 else x for x in crc], dtype=torch.int64, device="cuda")
        sst = [s for g in groups for s in (g[4] if len(g) > 4 and g[4] is not None else [0] * len(g[0]))]
        self.sst = torch.tensor(sst, dtype=torch.int32, device="cuda")

    def _go(self, d_out, out_cap):
        self.plan.run(self.arena.data_ptr(), self.in_off.data_ptr(), self.crc.data_ptr(), d_out, out_cap, self.off.data_ptr(),
                      self.st.data_ptr(), d_seg_status=self.sst.data_ptr(), stream=self.ctx.stream)
        self.torch.cuda.synchronize()

    def run(self, out_cap=None):
        """out_cap None: the sizing run first, then the real run into exactly that many bytes."""
        torch = self.torch
        torch.cuda.synchronize()
        if out_cap is None:
            self._go(0, 0)
            self.sizing_off = self.off.cpu().tolist()
            self.sizing_st = self.st.cpu().tolist()
            out_cap = self.sizing_off[-1]
        self.out_cap = out_cap
        pad = 64
        self.out = torch.full((out_cap + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
        self._go(self.out.data_ptr() + pad, out_cap)
        raw = bytes(self.out.cpu().numpy())
        assert raw[:pad] == bytes([GUARD]) * pad and raw[pad + out_cap:] == bytes([GUARD]) * pad, "a byte outside the output arena"
        self.bytes = raw[pad:pad + out_cap]
        self.offs = self.off.cpu().tolist()
        self.status = self.st.cpu().tolist()
        return self

    def result(self, k):
        return self.bytes[self.offs[k]:min(self.offs[k + 1], self.out_cap)]

    def check(self):
        """Every group as the host function has it; the outputs packed without gaps."""
        at = 0
        for k, g in enumerate(self.groups):
            st, exp = host(self.dg, g)
            assert self.status[k] == st, (k, self.status[k], st)
            assert self.offs[k] == at, k
            assert self.result(k) == exp, k
            at += len(exp)
        assert self.offs[self.ng] == at
        assert self.bytes[at:] == bytes([GUARD]) * (self.out_cap - at)


# 1. the whole corpus in one batch of mixed groups, host buffers in and out
def test_corpus_in_one_batch(dg, ctx, orc):
    cases = sc.all_cases(dg, orc)
    got = dg.splice_batch([group_of(orc, c) for c in cases], ctx=ctx)
    for c, g in zip(cases, got):
        assert g == dg.splice(c[4], c[5], c[3], orc.crc64_xz(c[1])), c[0]
    for c, g in list(zip(cases, got))[::7]:
        assert dg.decode(c[1], g, ctx=ctx) == c[2], c[0]
    assert dg.splice_batch([], ctx=ctx) == []


# 2. a plan over torch buffers: the sizing run reports the sizes that the real run fills
@pytest.mark.parametrize("caps", [True, False])
def test_plan_and_sizing_run(dg, ctx, orc, torch_cuda, caps):
    groups = [group_of(orc, c) for c in sc.all_cases(dg, orc)]
    r = Run(torch_cuda, dg, ctx, groups, slack=3, caps=caps).run()
    assert r.sizing_st == [CAPACITY] * len(groups)   # the sizing run: every OK group reports out_cap
    assert r.sizing_off == r.offs
    r.check()
    total = sum(len(d) + 3 for g in groups for d in g[1])
    assert r.plan.output_bound == (total + len(groups) if caps else 0)
    assert r.offs[-1] <= total + len(groups)


# 3. out_cap cut inside each group in turn: later groups fail, offsets stay true, nothing else is touched
def test_out_cap_cut_inside_each_group(dg, ctx, orc, torch_cuda):
    cases = [c for c in sc.all_cases(dg, orc) if c[0] in ("identical", "unrelated", "alternating", "empty_v", "group65", "zero_lengths",
                                                          "merged_first_then_more", "random3", "long_payloads")]
    groups = [group_of(orc, c) for c in cases]
    exp = [host(dg, g)[1] for g in groups]
    r = Run(torch_cuda, dg, ctx, groups)
    ends = [sum(len(e) for e in exp[:k + 1]) for k in range(len(exp))]
    for k in range(len(groups)):
        cap = ends[k] - 1 - (len(exp[k]) // 2)   # inside group k
        r.run(out_cap=cap)   # (checks the guard bytes around d_out)
        assert r.status == [OK] * k + [CAPACITY] * (len(groups) - k), k
        assert r.offs == [0] + ends, k
        start = ends[k] - len(exp[k])
        assert r.bytes[:start] == b"".join(exp[:k]), k
        assert r.bytes[start:] == bytes([GUARD]) * (cap - start), k   # a failed output is empty, its header included


# 4. each kind of damage in a segment between good groups
def test_damaged_segment_fails_its_group_alone(dg, ctx, orc, torch_cuda):
    (R, V, whole, segs, good), bad = sc.damaged(dg, orc)
    crc = orc.crc64_xz(R)
    ok = (segs, good, whole, crc)
    groups = [ok]
    for name, sg, ds, st, want in bad:
        groups += [(sg, ds, whole, crc, st), ok]
    r = Run(torch_cuda, dg, ctx, groups).run()
    r.check()
    assert [r.status[1 + 2 * k] for k in range(len(bad))] == [x[4] for x in bad]
    assert all(r.offs[2 + 2 * k] == r.offs[1 + 2 * k] for k in range(len(bad)))
    assert all(r.result(2 * k) == r.result(0) and r.status[2 * k] == OK for k in range(len(bad) + 1))
    assert dg.decode(R, r.result(0), ctx=ctx) == V


def test_stream_longer_than_capacity(dg, ctx, orc, torch_cuda):
    (R, V, whole, segs, good), _ = sc.damaged(dg, orc)
    crc = orc.crc64_xz(R)
    groups = [(segs, good, whole, crc)] * 3
    r = Run(torch_cuda, dg, ctx, groups)
    r.plan.close()
    caps = [len(d) for d in good]
    r.plan = dg.SplicePlan(ctx, [whole] * 3, [0, 3, 6, 9], segments=segs * 3, caps=caps + [caps[0], caps[1] - 1, caps[2]] + caps)
    r.run()
    assert r.status == [OK, CAPACITY, OK]
    assert r.result(0) == r.result(2) == dg.splice(segs, good, whole, crc) and r.result(1) == b""


# 5. the same plan on other bytes of the same layout: nothing of the first run is left
def test_rerun_on_other_bytes(dg, ctx, orc, torch_cuda):
    rng = random.Random(71)
    R = rng.randbytes(900)

    def variant(contiguous):
        out = []
        for n in (1, 5, 70):
            segs, lists, at = [], [], 0
            for j in range(n):
                src = 10 * j if contiguous or j % 3 else 10 * j + 1
                lists.append([("C", src, 10)] if j % 2 or not contiguous else [("C", src, 6), ("C", src + 6, 4)])
                if not contiguous and j % 2 == 0:
                    lists[-1] = [("C", src, 6), ("A", rng.randbytes(4))]
                segs.append((0, 900, at, 10))
                at += 10
            V = b"".join(cc.apply(c, R) for c in lists)
            out.append(sc.case(dg, orc, f"v{n}", R, V, segs, sc.hand(dg, orc, R, V, segs, lists)))
        return [group_of(orc, c) for c in out]

    first, second = variant(True), variant(False)
    assert [[len(d) for d in g[1]] for g in first] == [[len(d) for d in g[1]] for g in second]
    r = Run(torch_cuda, dg, ctx, first).run()
    r.check()
    assert [len(r.result(k)) for k in range(3)] == [39, 39, 39]
    r.groups = second
    r.load(second)
    r.run()
    r.check()
    r.groups = first
    r.load(first)
    r.run()
    r.check()


def test_stage_times_and_empty_plan(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    groups = [group_of(orc, c) for c in sc.all_cases(dg, orc)[:6]]
    r = Run(torch, dg, ctx, groups, timing=True).run()
    t = r.plan.stage_times()
    assert list(t) == ["map", "resolve", "scan", "emit", "total"]
    assert all(v > 0 for v in t.values()) and t["total"] >= max(t["map"], t["resolve"], t["scan"], t["emit"])
    p = dg.SplicePlan(ctx, [], [0], segments=[])
    off = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    p.run(0, 0, 0, 0, 0, off.data_ptr(), 0, stream=ctx.stream)
    torch.cuda.synchronize()
    assert off.cpu().tolist() == [0]
    with pytest.raises(dg.DeltaError) as e:   # geometry errors come from plan creation
        dg.SplicePlan(ctx, [(0, 100, 0, 100)], [0, 1], segments=[(0, 100, 0, 99)])
    assert e.value.code == 1


# 6. encode plan -> splice plan (made for it) -> decode plan, CRC checks on, one stream, no host step
@pytest.fixture(scope="module")
def big_pair(orc):
    return orc.synth_pair(0xB16, 4 << 20, (4 << 20) // 100)


@pytest.mark.parametrize("algorithm", ["onepass", "correcting", "greedy"])
def test_chain_encode_splice_decode(dg, ctx, orc, torch_cuda, big_pair, algorithm):
    torch = torch_cuda
    R, V = big_pair
    whole = (0, len(R), 0, len(V))
    segs, first = dg.segment_pairs(whole, 256 << 10, 256 << 10)
    assert len(segs) == 16
    d_r = torch.frombuffer(bytearray(R), dtype=torch.uint8).cuda()
    d_v = torch.frombuffer(bytearray(V), dtype=torch.uint8).cuda()
    enc = dg.EncodePlan(ctx, algorithm, segs, p=16)
    sp = dg.SplicePlan(ctx, [whole], first, for_plan=enc)
    cap = sp.output_bound
    assert 0 < cap <= enc.output_bound + 1
    dec = dg.DecodePlan(ctx, [(0, len(R), 0, cap, 0, len(V))])
    d_seg = torch.zeros(enc.output_bound, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_ver = torch.zeros(len(V), dtype=torch.uint8, device="cuda")
    so = torch.zeros(len(segs) + 1, dtype=torch.int64, device="cuda")
    ss = torch.full((len(segs),), -1, dtype=torch.int32, device="cuda")
    go, crc, vlen = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(3))
    gs, ds = (torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    s = ctx.stream
    span = (dg._lib.Span * 1)(dg._lib.Span(0, len(R)))
    ctx.check(dg.lib.dg_crc64_xz_batch_device(ctx.handle, d_r.data_ptr(), span, 1, crc.data_ptr(), s), "crc")
    enc.run(d_r.data_ptr(), d_v.data_ptr(), d_seg.data_ptr(), d_seg.numel(), so.data_ptr(), ss.data_ptr(), s)
    sp.run(d_seg.data_ptr(), so.data_ptr(), crc.data_ptr(), d_out.data_ptr(), cap, go.data_ptr(), gs.data_ptr(),
           d_seg_status=ss.data_ptr(), stream=s)
    dec.run(d_r.data_ptr(), d_out.data_ptr(), d_ver.data_ptr(), vlen.data_ptr(), ds.data_ptr(), s)
    torch.cuda.synchronize()
    assert ss.cpu().tolist() == [OK] * len(segs) and gs.cpu().tolist() == [OK] and ds.cpu().tolist() == [OK]
    assert vlen.cpu().tolist()[0] == len(V) and bytes(d_ver.cpu().numpy()) == V
    # and the spliced delta is the host function's, of the encoder's segment deltas
    offs, raw = so.cpu().tolist(), bytes(d_seg.cpu().numpy())
    size = go.cpu().tolist()[1]
    got = bytes(d_out.cpu().numpy())[:size]
    assert got == dg.splice(segs, [raw[offs[j]:offs[j + 1]] for j in range(len(segs))], whole, orc.crc64_xz(R))
    # every segment but one gives up its header and END byte, and merging only shortens
    assert size <= offs[-1] - 26 * (len(segs) - 1)


# 7. encode_large and the CLI flag against the decoders
def test_encode_large_and_cli(dg, ctx, orc, big_pair, tmp_path):
    import oracle as O
    R, V = big_pair[0][:3 << 20], big_pair[1][:(3 << 20) - 12345]
    d = dg.encode_large(R, V, "onepass", seg_bytes=256 << 10, window_bytes=128 << 10, ctx=ctx)
    assert dg.decode(R, d, ctx=ctx) == V
    assert orc.decode(R, d) == (0, V)
    one = dg.encode_large(R[:100000], R[:100000], "correcting", seg_bytes=4096, window_bytes=0, ctx=ctx)
    assert len(one) == 39
    ip = dg.encode_large(R, V, "onepass", seg_bytes=512 << 10, window_bytes=512 << 10, inplace=True, ctx=ctx)
    assert dg.info(ip)["inplace"] and dg.decode(R, ip, ctx=ctx) == V
    sk = dg.encode_large(R, V, "onepass", seg_bytes=256 << 10, window_bytes=128 << 10, windows="sketch", ctx=ctx)
    assert dg.decode(R, sk, ctx=ctx) == V
    pr, pv, pd, po = (tmp_path / x for x in ("r", "v", "d", "o"))
    pr.write_bytes(R)
    pv.write_bytes(V)
    p = subprocess.run([CLI, "encode", "onepass", str(pr), str(pv), str(pd), "--segment-size", str(256 << 10),
                        "--segment-window", str(128 << 10)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert pd.read_bytes() == d
    assert f"Delta:        {pd} ({len(d)} bytes)" in p.stdout and "Dst CRC:      " + orc.crc64_xz(V).hex() in p.stdout
    p = subprocess.run([CLI, "decode", str(pr), str(pd), str(po)], capture_output=True, text=True)
    assert p.returncode == 0 and po.read_bytes() == V, p.stderr
    if os.path.exists(O.REF_CLI):   # the reference's own decoder, both CRC checks on
        po.unlink()
        p = subprocess.run([O.REF_CLI, "decode", str(pr), str(pd), str(po)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert po.read_bytes() == V
