"""GPU: the chunked index pass of the read plan (dg_read_plan_chunk_index,
dg_read_plan_index_chunked) leaves exactly the index the one-block pass
(dg_read_plan_index) leaves, on the streams of tests/index_cases.py, and both
equal the Python models.  Indexes are compared as dg_read_plan_index_get returns
them: the 32-byte head and, for a stream whose status is 0, every entry.

The read plan's harness (Run: arenas at unaligned offsets, guarded output
slots, the whole arena compared) is test_gpu_read.py's.
"""
from __future__ import annotations

import random

import pytest

import index_cases as ic
import read_cases as rc
from test_gpu_read import Run

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, CAPACITY, MALFORMED = 0, 1, 7, 8


class ChunkedRun(Run):
    def index_chunked(self, **kw):
        self.plan.index_chunked(self.d_delta.data_ptr(), self.d_sst.data_ptr(), stream=self.ctx.stream, **kw)
        return self

    def indexes(self):
        """Every stream's index as the last pass left it, and the stream statuses."""
        got = [self.plan.index_get(i) for i in range(self.n)]   # (synchronises the context's stream)
        self.torch.cuda.synchronize()
        return got, self.d_sst.cpu().tolist()[:self.n]


def _compare(cases, serial, chunked, streams):
    """Both passes' indexes are byte-identical and equal the model."""
    for (name, R, d, st, model), a, b, (_, _, doff, _) in zip(cases, serial, chunked, streams):
        assert a[:32] == b[:32], (name, ic.unpack_index(a)[0], ic.unpack_index(b)[0])
        head, ents, at = ic.unpack_index(b)
        assert head == model[0] and head["status"] == st, (name, head, model[0])
        assert at == doff, name
        if a != b:
            ea = ic.unpack_index(a)[1]
            k = next(k for k in range(len(ents)) if ents[k] != ea[k])
            raise AssertionError(f"{name}: entry {k} of {len(ents)}: one-block {ea[k]}, chunked {ents[k]}")
        assert ents == model[1], name


# 1. every stream of index_cases in one plan: the one-block pass, then the chunked pass over it
@pytest.mark.parametrize("chunk_bytes", [4096, 8192])
def test_both_passes_leave_the_same_index(dg, ctx, orc, torch_cuda, chunk_bytes):
    cases = ic.models(dg, orc)
    r = ChunkedRun(torch_cuda, dg, ctx, [(c[1], c[2]) for c in cases], [])
    serial, st_serial = r.index().indexes()
    r.d_sst.fill_(-1)
    r.plan.chunk_index(chunk_bytes)
    chunked, st_chunked = r.index_chunked().indexes()
    assert st_serial == [c[3] for c in cases] and st_chunked == st_serial
    _compare(cases, serial, chunked, r.streams)
    # each damaged stream sits between good neighbours, whose entries are intact (compared above, and counted here)
    bad = [k for k, c in enumerate(cases) if c[3] == MALFORMED and c[0].endswith(("chunk_0", "middle", "last"))]
    assert len(bad) == 12
    for k in bad:
        for nb in (k - 1, k + 1):
            assert cases[nb][3] == OK and len(chunked[nb]) == 32 + 8 * (len(cases[nb][2]) // 1024 + 1)


# 2. the default chunk size, one stream of about 1 MiB: the long-ADD family scaled up
def test_one_stream_of_a_megabyte(dg, ctx, orc, torch_cuda):
    rng = random.Random(91)
    R = rng.randbytes(3000)
    body = []
    for k in range(34):
        body += [("A", rng.randbytes(20000 + 517 * k))] + ic._tail(rng, 150)
    cmds, vs = rc.sequential(body)
    d = rc.stream(orc, R, cmds, version_size=vs)
    assert 1000000 < len(d) < 1300000
    model = ic.serial_index(len(R), d)
    r = ChunkedRun(torch_cuda, dg, ctx, [(R, d)], [])
    serial, _ = r.index().indexes()
    r.plan.chunk_index()
    chunked, st = r.index_chunked().indexes()
    assert st == [OK]
    _compare([("megabyte", R, d, OK, model)], serial, chunked, r.streams)
    assert model[0]["seq"] == 1


# 3. after the chunked pass the read kernel serves read_cases' ranges of every stream (test_gpu_read.py's check)
def test_reads_after_the_chunked_pass(dg, ctx, orc, torch_cuda):
    cases = ic.all_cases(dg, orc)
    items, reqs, sizes, versions = [], [], [], []
    for s, (name, R, d, st) in enumerate(cases):
        mst, V, cmds = rc.model_version(R, d)
        assert mst == st, name
        items.append((R, d))
        versions.append(V)
        for off, ln in (rc.ranges(V, cmds, len(d)) if st == OK else [(0, 16), (3, 1), (0, 0)]):
            reqs.append((s, off, ln))
            sizes.append(0 if st else len(V))
    r = ChunkedRun(torch_cuda, dg, ctx, items, [])
    r.set_requests(reqs, sizes)
    r.plan.close()
    r.plan = dg.ReadPlan(ctx, r.streams, len(reqs))
    r.plan.chunk_index(4096)
    r.index_chunked().run()
    assert r.stream_st == [c[3] for c in cases]
    r.check(versions, [c[3] for c in cases])


# 4. encode -> chunked index -> read on one stream, device-side offsets and statuses, no host step
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
    r = ChunkedRun(torch, dg, ctx, [], [])
    r.plan.close()
    r.n = n
    r.streams = [(ro, rl, 0, bound) for ro, rl in lr]   # delta_len only bounds each stream
    r.plan = dg.ReadPlan(ctx, r.streams, len(reqs))
    r.plan.chunk_index(4096)
    r.d_sst = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r.set_requests(reqs, [len(pairs[s][1]) for s, _, _ in reqs])
    r.d_ref = d_r
    r.d_delta = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    enc.run(d_r.data_ptr(), d_v.data_ptr(), r.d_delta.data_ptr(), bound, off.data_ptr(), st.data_ptr(), ctx.stream)
    r.index_chunked(d_delta_offsets=off.data_ptr(), d_delta_status=st.data_ptr())
    r.run()
    assert st.cpu().tolist() == [OK] * n and r.stream_st == [OK] * n
    r.check([p[1] for p in pairs], [OK] * n)
    # the one-block pass over the same device-side offsets leaves the same index
    chunked, _ = r.indexes()
    r.index(d_delta_offsets=off.data_ptr(), d_delta_status=st.data_ptr())
    serial, _ = r.indexes()
    assert serial == chunked


# 5. a stream longer than the plan allows is refused alone; a passed-on status comes first
def test_capacity_and_passed_on_status(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    good = [c for c in ic.new_cases(orc) if not c[3]][:3]
    versions = [rc.model_version(c[1], c[2])[1] for c in good]
    reqs = [(s, 10, 50) for s in range(3)] + [(s, 0, 1 << 20) for s in range(3)]
    r = ChunkedRun(torch, dg, ctx, [(c[1], c[2]) for c in good], reqs, unaligned=False)
    offs = [st[2] for st in r.streams] + [r.streams[2][2] + r.streams[2][3]]
    bounds = [offs[k + 1] - offs[k] for k in range(3)]
    bounds[1] -= 1   # stream 1 may be one byte shorter than it is
    r.plan.close()
    r.plan = dg.ReadPlan(ctx, [(ro, rl, 0, b) for (ro, rl, _, _), b in zip(r.streams, bounds)], len(reqs))
    r.plan.chunk_index(4096)
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    r.index_chunked(d_delta_offsets=d_off.data_ptr()).run()
    assert r.stream_st == [OK, CAPACITY, OK]
    r.check(versions, [OK, CAPACITY, OK])
    chunked, _ = r.indexes()
    serial, st = r.index(d_delta_offsets=d_off.data_ptr()).indexes()
    assert st == [OK, CAPACITY, OK] and serial == chunked
    # a status passed on from an earlier stage: that stream only, before capacity
    d_pass = torch.tensor([0, 5, 12], dtype=torch.int32, device="cuda")
    serial, st = r.index(d_delta_offsets=d_off.data_ptr(), d_delta_status=d_pass.data_ptr()).indexes()
    chunked, st2 = r.index_chunked(d_delta_offsets=d_off.data_ptr(), d_delta_status=d_pass.data_ptr()).indexes()
    assert st == [OK, 5, 12] and st2 == st and serial == chunked


# 6. the order of the calls, and the chunk size
def test_call_order_and_chunk_sizes(dg, ctx, orc, torch_cuda):
    name, R, d, _ = ic.new_cases(orc)[0]
    r = ChunkedRun(torch_cuda, dg, ctx, [(R, d)], [(0, 0, 100)])
    with pytest.raises(dg.DeltaError) as e:
        r.index_chunked()
    assert e.value.code == INVALID_ARG and "dg_read_plan_chunk_index has not run" in str(e.value)
    with pytest.raises(dg.DeltaError) as e:   # and no index has run: a read is still refused
        r.run()
    assert e.value.code == INVALID_ARG
    for bad in (1, 4095, 4097, 6144, 0xFFFFFFFF):
        with pytest.raises(dg.DeltaError) as e:
            r.plan.chunk_index(bad)
        assert e.value.code == INVALID_ARG, bad
    r.plan.chunk_index(12288)   # any multiple of 4096
    with pytest.raises(dg.DeltaError) as e:
        r.plan.chunk_index(4096)   # once per plan
    assert e.value.code == INVALID_ARG
    r.index_chunked().run()
    r.check([rc.model_version(R, d)[1]], [OK])
    r.plan.set_index_timing(2)
    r.index_chunked()
    t = r.plan.index_stage_times()
    assert list(t) == ["map", "resolve", "fill", "total"] and all(v > 0 for v in t.values())
    assert t["map"] + t["resolve"] + t["fill"] <= t["total"] * 1.001
    assert set(r.plan.stage_times()) <= {"read", "total"}   # the run's getter is as it was


# 7. the index follows the delta bytes: another valid batch of the same layout, indexed again
def test_reindex_after_the_deltas_change(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    rng = random.Random(6)
    R = rng.randbytes(3000)

    def batch(seed):
        g = random.Random(seed)
        out = []
        for k in range(4):   # the same stream lengths for every seed: 400 COPYs and 400 ADDs of 7 bytes, three chunks
            cmds, vs = rc.sequential([("C", g.randrange(0, 2900), g.randint(1, 90)) if j % 2 else ("A", g.randbytes(7))
                                      for j in range(800)])
            if k == 3:
                cmds = cmds[::-1]   # one that is not in sequence
            out.append(rc.stream(orc, R, cmds, version_size=vs))
        return out

    a, b = batch(1), batch(2)
    assert [len(x) for x in a] == [len(x) for x in b] and a != b and len(a[0]) > 2 * 4096
    va = [rc.model_version(R, d)[1] for d in a]
    vb = [rc.model_version(R, d)[1] for d in b]
    reqs = [(s, o, 300) for s in range(4) for o in (0, 1000, 2500, 6000, 20000)]
    r = ChunkedRun(torch, dg, ctx, [(R, d) for d in a], reqs)
    r.plan.chunk_index(4096)
    r.index_chunked().run()
    r.check(va, [OK] * 4)
    dl = bytearray(r.d_delta.cpu().numpy().tobytes())
    for (_, _, do, n), d in zip(r.streams, b):
        dl[do:do + n] = d
    r.d_delta.copy_(torch.frombuffer(dl, dtype=torch.uint8))
    r.d_out.copy_(torch.from_numpy(r.before))
    r.index_chunked().run()
    r.check(vb, [OK] * 4)
    got, _ = r.indexes()
    for d, raw in zip(b, got):
        head, ents, _ = ic.unpack_index(raw)
        assert (head, ents) == ic.serial_index(len(R), d)
