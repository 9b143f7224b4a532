"""GPU: byte ranges of versions kept as R plus a delta (dg_read_plan_*,
dg_read_batch), against the Python model of tests/read_cases.py.

The streams of a run sit in one reference arena and one delta arena, at
unaligned offsets for half of them.  Every request has a slot in one output
arena, at out_off = 0, 1, 7, 13 (mod 16) in turn, 64 guard bytes of 0xA5
between slots, the slots pre-filled with 0x5A.  The expected arena is built on
the host (the model's bytes in the first n bytes of every served slot, nothing
else changed) and compared whole, so a byte written past n, into a guard or
into a failing request's slot fails the test.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import read_cases as rc

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED, MALFORMED = 0, 1, 2, 8
GUARD, FILL = 0xA5, 0x5A
MODS = [0, 1, 7, 13]


class Run:
    """A plan over items = (R, delta) and requests = (stream, off, length)."""

    def __init__(self, torch, dg, ctx, items, requests, *, unaligned=True, max_requests=None):
        self.torch, self.dg, self.ctx, self.items = torch, dg, ctx, items
        self.n = len(items)
        ref, dlt, self.streams = bytearray(), bytearray(), []
        for k, (R, d) in enumerate(items):
            if unaligned and k % 2:
                ref += bytes([GUARD]) * (1 + k % 15)
                dlt += bytes([GUARD]) * (1 + (3 * k) % 15)
            else:
                ref += bytes([GUARD]) * (-len(ref) % 16)
                dlt += bytes([GUARD]) * (-len(dlt) % 16)
            self.streams.append((len(ref), len(R), len(dlt), len(d)))
            ref += R
            dlt += d
        self.d_ref = torch.frombuffer(ref + b"\0", dtype=torch.uint8).cuda()
        self.d_delta = torch.frombuffer(dlt + b"\0", dtype=torch.uint8).cuda()
        self.plan = dg.ReadPlan(ctx, self.streams, len(requests) if max_requests is None else max_requests)
        self.d_sst = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device="cuda")
        self.set_requests(requests)

    def set_requests(self, requests, sizes=None):
        """sizes[j]: the version size of request j's stream where known (it bounds the slot's room)."""
        torch = self.torch
        self.requests = requests
        m = self.m = len(requests)
        self.slots, pos = [], 64
        arr = (self.dg.ReadReq * max(m, 1))()
        for j, (s, off, ln) in enumerate(requests):
            pos += (MODS[j % 4] - pos) % 16
            vs = sizes[j] if sizes else (1 << 32)
            n_max = 0 if off >= vs else min(ln, vs - off)
            room = min(ln, n_max + 64, 1 << 20)
            self.slots.append((pos, room))
            arr[j] = self.dg.ReadReq(s, off, ln, 0, pos)
            pos += room + 64
        before = np.full(pos + 64, GUARD, dtype=np.uint8)
        for o, room in self.slots:
            before[o:o + room] = FILL
        self.before = before
        self.d_out = torch.from_numpy(before.copy()).cuda()
        assert self.d_out.data_ptr() % 16 == 0
        self.d_req = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        self.d_len = torch.full((max(m, 1),), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        self.d_st = torch.full((max(m, 1),), -1, dtype=torch.int32, device="cuda")

    def index(self, **kw):
        self.plan.index(self.d_delta.data_ptr(), self.d_sst.data_ptr(), stream=self.ctx.stream, **kw)
        return self

    def run(self):
        self.plan.run(self.d_ref.data_ptr(), self.d_delta.data_ptr(), self.d_req.data_ptr(), self.m, self.d_out.data_ptr(),
                      self.d_len.data_ptr(), self.d_st.data_ptr(), stream=self.ctx.stream)
        self.torch.cuda.synchronize()
        self.after = self.d_out.cpu().numpy()
        self.st = self.d_st.cpu().tolist()[:self.m]
        self.out_len = self.d_len.cpu().tolist()[:self.m]
        self.stream_st = self.d_sst.cpu().tolist()[:self.n]
        return self

    def check(self, versions, statuses):
        """versions[s]: V of stream s (None for a failing one); statuses[s]: its expected status."""
        exp = self.before.copy()
        for j, (s, off, ln) in enumerate(self.requests):
            want_st = INVALID_ARG if s >= self.n else statuses[s]
            assert self.st[j] == want_st, (j, s, off, ln, self.st[j], want_st)
            got = b"" if want_st else rc.model_read(versions[s], off, ln)
            assert self.out_len[j] == len(got), (j, s, off, ln, self.out_len[j], len(got))
            o, room = self.slots[j]
            assert len(got) <= room
            exp[o:o + len(got)] = np.frombuffer(got, dtype=np.uint8)
        bad = np.flatnonzero(self.after != exp)
        if bad.size:
            at = int(bad[0])
            j = max(k for k, (o, _) in enumerate(self.slots) if o - 64 <= at)
            raise AssertionError(f"{bad.size} bytes differ, the first at {at}: request {j} {self.requests[j]}, "
                                 f"slot at {self.slots[j]}, got {int(self.after[at])} want {int(exp[at])}")


def _corpus_run(torch, dg, ctx, orc):
    cases = rc.with_ranges(dg, orc)
    items = [(R, d) for _, R, d, _, _, _ in cases]
    reqs, sizes = [], []
    for s, (_, _, _, st, V, rs) in enumerate(cases):
        for off, ln in rs:
            reqs.append((s, off, ln))
            sizes.append(0 if st else len(V))
    r = Run(torch, dg, ctx, items, [])
    r.set_requests(reqs, sizes)
    r.plan.close()
    r.plan = dg.ReadPlan(ctx, r.streams, len(reqs))
    return cases, r


# 1. the whole corpus in one plan, every range a request
def test_whole_corpus(dg, ctx, orc, torch_cuda):
    cases, r = _corpus_run(torch_cuda, dg, ctx, orc)
    assert len(r.requests) > 10000
    r.index().run()
    assert r.stream_st == [c[3] for c in cases]
    r.check([c[4] for c in cases], [c[3] for c in cases])
    # every damaged stream's neighbours were served: whole reads of both are among the requests
    for s, c in enumerate(cases):
        if c[3]:
            for nb in (s - 1, s + 1):
                assert cases[nb][3] == OK
                j = r.requests.index((nb, 0, len(cases[nb][4])))
                assert r.st[j] == OK and r.out_len[j] == len(cases[nb][4])


# 2. stream statuses are decode's on every standard stream
def test_stream_statuses_are_decodes(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    cases = [c for c in rc.with_ranges(dg, orc) if not (len(c[2]) >= 25 and c[2][4] & 1)]
    assert sum(1 for c in cases if c[3]) >= 8
    r = Run(torch, dg, ctx, [(c[1], c[2]) for c in cases], [(0, 0, 1)], unaligned=False).index().run()
    n = len(cases)
    descs, at = [], 0
    for (ro, rl, do, dl), c in zip(r.streams, cases):
        cap = max(len(c[4]) if c[4] is not None else 1 << 16, 16)
        descs.append(dg._lib.DecodeDesc(ro, rl, do, dl, at, cap))
        at += (cap + 15) & ~15
    out = torch.zeros(at, dtype=torch.uint8, device="cuda")
    dlen = torch.zeros(n, dtype=torch.int64, device="cuda")
    dst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(dg.lib.dg_decode_batch_device(ctx.handle, r.d_ref.data_ptr(), r.d_delta.data_ptr(),
                                            (dg._lib.DecodeDesc * n)(*descs), n, 1, out.data_ptr(), dlen.data_ptr(),
                                            dst.data_ptr(), None), "decode batch")
    torch.cuda.synchronize()
    assert r.stream_st == dst.cpu().tolist()
    assert r.stream_st == [c[3] for c in cases]


# 3. many requests on one stream; a second run of the same plan gives the same bytes
@pytest.mark.parametrize("name", ["onepass_dense24", "many_overlapping"])
def test_shared_stream_and_rerun(dg, ctx, orc, torch_cuda, name):
    c = next(c for c in rc.with_ranges(dg, orc) if c[0] == name)
    V = c[4]
    rng = random.Random(5)
    reqs = [(0, rng.randrange(len(V)), rng.choice([1, 100, 4096, 20000])) for _ in range(64)]
    r = Run(torch_cuda, dg, ctx, [(c[1], c[2])], reqs)
    r.set_requests(reqs, [len(V)] * 64)
    r.index().run()
    r.check([V], [OK])
    first = r.after.copy()
    r.d_out.copy_(torch_cuda.from_numpy(r.before))
    r.run()
    assert np.array_equal(r.after, first)


# 4. empty and invalid shapes
def test_empty_and_invalid(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    name, R, d, _, V, _ = rc.with_ranges(dg, orc)[0]
    r = Run(torch, dg, ctx, [(R, d)], [(0, 3, 10), (1, 0, 10), (0, 5, 7), (7, 0, 1)], max_requests=8)
    with pytest.raises(dg.DeltaError) as e:   # before any index
        r.run()
    assert e.value.code == INVALID_ARG and "index" in str(e.value)
    r.index().run()
    r.check([V], [OK])
    assert r.st == [OK, INVALID_ARG, OK, INVALID_ARG]
    # reserved != 0: that request only
    raw = bytearray(r.d_req.cpu().numpy().tobytes())
    raw[12] = 1
    r.d_req = torch.frombuffer(raw, dtype=torch.uint8).cuda()
    r.d_out.copy_(torch.from_numpy(r.before))
    r.run()
    assert r.st == [INVALID_ARG, INVALID_ARG, OK, INVALID_ARG] and r.out_len[0] == 0
    o, room = r.slots[0]
    assert (r.after[o:o + room] == FILL).all()
    # more requests than the plan was made for
    with pytest.raises(dg.DeltaError) as e:
        r.plan.run(r.d_ref.data_ptr(), r.d_delta.data_ptr(), r.d_req.data_ptr(), 9, r.d_out.data_ptr(),
                   r.d_len.data_ptr(), r.d_st.data_ptr())
    assert e.value.code == INVALID_ARG
    # no requests: nothing runs, nothing is needed
    r.plan.run(0, 0, 0, 0, 0, 0, 0)
    # no streams: every request names a stream that is not there
    z = Run(torch, dg, ctx, [], [(0, 0, 4), (3, 1, 1)])
    z.index().run()
    assert z.st == [INVALID_ARG, INVALID_ARG] and z.out_len == [0, 0]
    assert np.array_equal(z.after, z.before)


# 5. the index follows the delta bytes: another valid batch of the same layout, indexed again
def test_reindex_after_the_deltas_change(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    rng = random.Random(6)
    R = rng.randbytes(3000)

    def batch(seed):
        g = random.Random(seed)
        out = []
        for k in range(6):   # the same stream lengths for every seed: 100 COPYs and 100 ADDs of 7 bytes
            cmds, vs = rc.sequential([("C", g.randrange(0, 2900), g.randint(1, 90)) if j % 2 else ("A", g.randbytes(7))
                                      for j in range(200)])
            if k == 3:
                cmds = cmds[::-1]   # one that is not in sequence
            out.append(rc.stream(orc, R, cmds, version_size=vs))
        return out

    a, b = batch(1), batch(2)
    assert [len(x) for x in a] == [len(x) for x in b] and a != b
    va = [rc.model_version(R, d)[1] for d in a]
    vb = [rc.model_version(R, d)[1] for d in b]
    reqs = [(s, o, 300) for s in range(6) for o in (0, 1000, 2500, 6000)]
    r = Run(torch, dg, ctx, [(R, d) for d in a], reqs)
    r.index().run()
    r.check(va, [OK] * 6)
    dl = bytearray(r.d_delta.cpu().numpy().tobytes())
    for (_, _, do, n), d in zip(r.streams, b):
        dl[do:do + n] = d
    r.d_delta.copy_(torch.frombuffer(dl, dtype=torch.uint8))
    r.d_out.copy_(torch.from_numpy(r.before))
    r.index().run()
    r.check(vb, [OK] * 6)


# 6. encode -> index -> read on one stream, no host step between them
def test_chain_after_the_encoder(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    pairs = [orc.synth_pair(0xAB00 + k, 16384 + 160 * k, 164) for k in range(6)]
    pairs += [orc.synth_transpose(0xAC00 + k, 16, 1024) for k in range(2)]
    n = len(pairs)

    def arena(bufs):
        lay, buf = [], bytearray()
        for x in bufs:
            lay.append((len(buf), len(x)))
            buf += x + bytes(-len(x) % 16)
        return torch.frombuffer(buf, dtype=torch.uint8).cuda(), lay

    d_r, lr = arena([p[0] for p in pairs])
    d_v, lv = arena([p[1] for p in pairs])
    enc = dg.EncodePlan(ctx, "onepass", [(a[0], a[1], b[0], b[1]) for a, b in zip(lr, lv)], p=16, q=1)
    bound = enc.output_bound
    rng = random.Random(7)
    reqs = [(s, rng.randrange(len(pairs[s][1])), rng.choice([1, 17, 4096, 70000])) for s in range(n) for _ in range(8)]
    # delta_len bounds each stream; the encoder's offsets say where it is
    r = Run(torch, dg, ctx, [], [])
    r.plan.close()
    r.n = n
    r.streams = [(ro, rl, 0, bound) for ro, rl in lr]
    r.plan = dg.ReadPlan(ctx, r.streams, len(reqs))
    r.d_sst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r.set_requests(reqs, [len(pairs[s][1]) for s, _, _ in reqs])
    r.d_ref = d_r
    r.d_delta = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = ctx.stream
    enc.run(d_r.data_ptr(), d_v.data_ptr(), r.d_delta.data_ptr(), bound, off.data_ptr(), st.data_ptr(), s)
    r.index(d_delta_offsets=off.data_ptr(), d_delta_status=st.data_ptr())
    r.run()
    assert st.cpu().tolist() == [OK] * n and r.stream_st == [OK] * n
    r.check([p[1] for p in pairs], [OK] * n)


# 6b. with offsets, delta_len bounds the stream: a longer one is DG_ERR_CAPACITY, its neighbours are served
def test_stream_longer_than_the_plan_allows(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    good = [c for c in rc.with_ranges(dg, orc) if not c[3] and len(c[4]) > 100][:3]
    reqs = [(s, 10, 50) for s in range(3)] + [(s, 0, 1 << 20) for s in range(3)]
    r = Run(torch, dg, ctx, [(c[1], c[2]) for c in good], reqs, unaligned=False)
    offs = [st[2] for st in r.streams] + [r.streams[2][2] + r.streams[2][3]]
    # stream 1 may be one byte shorter than it is; every stream's place comes from the offsets (16-byte aligned
    # arena: stream i + 1 starts where the padding after stream i ends, so stream i's span includes the padding)
    bounds = [offs[k + 1] - offs[k] for k in range(3)]
    bounds[1] -= 1
    r.plan.close()
    r.plan = dg.ReadPlan(ctx, [(ro, rl, 0, b) for (ro, rl, _, _), b in zip(r.streams, bounds)], len(reqs))
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    r.index(d_delta_offsets=d_off.data_ptr()).run()
    assert r.stream_st == [OK, 7, OK]
    r.check([c[4] for c in good], [OK, 7, OK])


# 7. the host wrappers
def test_read_ranges_equals_read_range(dg, ctx, orc):
    cases = rc.with_ranges(dg, orc)
    pick = [c for c in cases if c[3]][:3] + [c for c in cases if not c[3]][:12]
    items = [(c[1], c[2]) for c in pick]
    reqs = [(s, off, ln) for s, c in enumerate(pick) for off, ln in c[5][::7]] + [(len(pick), 0, 1)]
    got, st = dg.read_ranges(items, reqs, ctx=ctx, status=True)
    for (s, off, ln), g, code in zip(reqs, got, st):
        if s >= len(pick):
            assert code == INVALID_ARG and g == b""
        elif pick[s][3]:
            assert code == pick[s][3] and g == b""
        else:
            assert code == OK and g == dg.read_range(pick[s][1], pick[s][2], off, ln), (s, off, ln)
    with pytest.raises(dg.DeltaError):
        dg.read_ranges(items, reqs, ctx=ctx)
    assert dg.read_ranges(items, [], ctx=ctx) == []


# 8. a context closed before its read plan takes the plan along
def test_context_closed_before_its_read_plan(dg, orc, torch_cuda):
    c = dg.Context(0)
    name, R, d, _, V, _ = rc.with_ranges(dg, orc)[0]
    r = Run(torch_cuda, dg, c, [(R, d)], [(0, 10, 100)])
    r.index().run()
    r.check([V], [OK])
    c.close()
    assert c.handle is None
    r.plan.close()   # nothing left to do
    assert r.plan.handle is None


# 9. stage times of the runs
def test_stage_times(dg, ctx, orc, torch_cuda):
    name, R, d, _, V, _ = rc.with_ranges(dg, orc)[0]
    r = Run(torch_cuda, dg, ctx, [(R, d)], [(0, 0, 4096)])
    r.plan.set_timing(2)
    r.index().run()
    t = r.plan.stage_times()
    assert set(t) == {"read", "total"} and 0 < t["read"] <= t["total"] * 1.001
