"""GPU: the kernels that consume command streams, at offsets and sizes in the
upper half of the u32 range, against the sparse model (tests/sparse_model.py)
on the corpus of tests/high_offset_cases.py: exact bytes, exact statuses.

The kernels keep src, dst and len in 32-bit registers and widen by hand where
two of them meet; the other GPU tests never feed them an offset above a few
MiB.  Here one reference of 2^32 - 1 - 2^20 bytes sits on the device once per
module (zeros plus the corpus's windows) and every stream names a prefix of it.
The harnesses are the siblings' (arenas at odd offsets, guard bytes, the sizing
run): ComposePlan and SplicePlan take theirs as they are; InvertPlan's and
ReadPlan's are subclassed only to take their reference from the shared arena
instead of building one from bytes.  DecodePlan and UpdatePlan are driven
directly: the update harness downloads its whole buffer after a run, which here
is the 4 GiB arena.  LineagePlan's harness is subclassed as ReadPlan's is: the
levels on R name prefixes of the arena, the others state their parent's size.
Decode and update run without CRC checks (one block would
checksum 4 GiB); the decode_large test runs with them, on a version of
2^31 + 2^20 + 3 bytes whose expected CRC comes from the model's combine.
InplacePlan is driven directly too, one batch per policy: its expected bytes
are the reference's own (tests/golden/golden_inplace_high.json), not the
model's, and dg_make_inplace is computed only to describe a difference.

Device memory: 4 GiB for R, and about 4.2 GiB more while the decode_large test
compares its output (2 GiB of output plus the compare's temporary).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import struct
import time

import numpy as np
import pytest

import high_offset_cases as hc
import sparse_model as sm
from test_gpu_compose import Run as ComposeRun
from test_gpu_index_chunked import ChunkedRun
from test_gpu_invert import Run as InvertBase
from test_gpu_lineage import LineageRun
from test_gpu_splice import Run as SpliceRun

pytestmark = pytest.mark.gpu

OK, TOO_LARGE, CAPACITY, DST_CRC = 0, 3, 7, 10
GOLD_INPLACE = {(c["name"], c["policy"]): c for c in json.load(open(os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "golden", "golden_inplace_high.json")))["cases"]}
GUARD = 0xA5
HEAD = 1 << 17   # what an update of this corpus may change of the arena: its versions are below 64 KiB


@pytest.fixture(scope="module")
def arena(torch_cuda):
    """R on the device: zeros and the corpus's windows."""
    torch = torch_cuda
    t = torch.zeros(hc.RLEN, dtype=torch.uint8, device="cuda")
    for o, b in hc.R.windows():
        t[o:o + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    yield t
    del t
    torch.cuda.empty_cache()


def _packed(r, expected):
    """A run of a transform plan: every status and size, the outputs packed without gaps, the guards intact."""
    at = 0
    for k, (name, (st, exp)) in enumerate(expected):
        assert r.status[k] == st, (name, r.status[k], st)
        assert r.offs[k] == at, name
        assert r.result(k) == exp, name
        at += len(exp)
    assert r.offs[-1] == at
    assert r.bytes[at:] == bytes([GUARD]) * (r.out_cap - at)


# 1. compose: one batch of every pair
def test_compose_plan(dg, ctx, torch_cuda):
    cases = hc.corpus()["compose"]
    pairs = [(a, b) for _, a, b, _ in cases]
    expected = [(name, sm.compose(a, b)) for name, a, b, _ in cases]
    assert [e[1][0] for e in expected] == [c[3] for c in cases]
    r = ComposeRun(torch_cuda, dg, ctx, pairs).run()
    assert r.sizing_st == [st or CAPACITY for st in r.status] and r.sizing_off == r.offs
    _packed(r, expected)


# 2. invert: one batch, every stream against a prefix of the shared reference
class InvertRun(InvertBase):
    def __init__(self, torch, dg, ctx, d_ref, items):
        """items: (ref_len, A).  The streams at odd offsets between guard bytes, the last one at the arena's end."""
        self.torch, self.dg, self.ctx, self.n = torch, dg, ctx, len(items)
        self.offsets = False
        buf, descs = bytearray([GUARD]) * 3, []
        for k, (ref_len, a) in enumerate(items):
            descs.append((0, ref_len, len(buf), len(a)))
            buf += a + (b"" if k + 1 == self.n else bytes([GUARD]) * 7)
        self.plan = dg.InvertPlan(ctx, descs)
        self.off = torch.zeros(self.n + 1, dtype=torch.int64, device="cuda")
        self.st = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.arena = [d_ref, torch.frombuffer(buf, dtype=torch.uint8).cuda()]


def test_invert_plan(dg, ctx, torch_cuda, arena):
    cases = hc.corpus()["invert"]
    expected = [(name, sm.invert(hc.R.head(ref_len), a)) for name, ref_len, a, _ in cases]
    assert [e[1][0] for e in expected] == [c[3] for c in cases]
    r = InvertRun(torch_cuda, dg, ctx, arena, [(ref_len, a) for _, ref_len, a, _ in cases])
    assert r.plan.output_bound > sum(c[1] for c in cases)   # (the bound counts every R whole: the run gets what the model needs)
    r.run(out_cap=sum(len(e[1][1]) for e in expected) + 100)
    _packed(r, expected)


# 3. splice: one batch of every group whose geometry a plan accepts; the others are refused at create
def test_splice_plan(dg, ctx, torch_cuda):
    cases = hc.corpus()["splice"]
    refused = [c for c in cases if sm.splice_geometry(c[1], c[2])]
    assert [c[5] for c in refused] == [TOO_LARGE] * 2
    for name, whole, segs, deltas, _, st in refused:
        with pytest.raises(dg.DeltaError) as e:
            dg.SplicePlan(ctx, [whole], [0, len(segs)], segments=segs, caps=[len(d) for d in deltas])
        assert e.value.code == st, name
    cases = [c for c in cases if c not in refused]
    expected = [(name, sm.splice(whole, segs, deltas, crc)) for name, whole, segs, deltas, crc, _ in cases]
    assert [e[1][0] for e in expected] == [c[5] for c in cases]
    r = SpliceRun(torch_cuda, dg, ctx, [(segs, deltas, whole, crc) for _, whole, segs, deltas, crc, _ in cases]).run()
    assert r.sizing_st == [st or CAPACITY for st in r.status] and r.sizing_off == r.offs
    _packed(r, expected)
    # the spliced header's dst_crc is the model's combine of the segments' arbitrary header values
    one = next(k for k, c in enumerate(cases) if c[0] == "one_copy_65")
    assert r.result(one)[17:25] == expected[one][1][1][17:25] != bytes(8)


# 4. read: the one-block index, then the chunked index over it, the same requests after each
class ReadRun(ChunkedRun):
    def __init__(self, torch, dg, ctx, d_ref, items, requests, sizes):
        """items: (ref_len, delta), every reference a prefix of d_ref; the streams as test_gpu_read.Run lays them out."""
        self.torch, self.dg, self.ctx, self.items = torch, dg, ctx, items
        self.n = len(items)
        dlt, self.streams = bytearray(), []
        for k, (ref_len, d) in enumerate(items):
            dlt += bytes([GUARD]) * ((1 + (3 * k) % 15) if k % 2 else (-len(dlt) % 16))
            self.streams.append((0, ref_len, len(dlt), len(d)))
            dlt += d
        self.d_ref = d_ref
        self.d_delta = torch.frombuffer(dlt + b"\0", dtype=torch.uint8).cuda()
        self.plan = dg.ReadPlan(ctx, self.streams, len(requests))
        self.d_sst = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.set_requests(requests, sizes)

    def check_model(self, cases):
        """Run.check with the sparse model: every length and status, and the output arena compared whole."""
        exp = self.before.copy()
        for j, (s, off, ln) in enumerate(self.requests):
            name, ref_len, d, _, _ = cases[s]
            st, got = sm.read(hc.R.head(ref_len), d, off, ln)
            assert self.st[j] == st, (name, off, ln, self.st[j], st)
            assert self.out_len[j] == len(got), (name, off, ln, self.out_len[j], len(got))
            o, room = self.slots[j]
            assert len(got) <= room
            exp[o:o + len(got)] = np.frombuffer(got, dtype=np.uint8)
        bad = np.flatnonzero(self.after != exp)
        if bad.size:
            at = int(bad[0])
            j = max(k for k, (o, _) in enumerate(self.slots) if o - 64 <= at)
            raise AssertionError(f"{bad.size} bytes differ, the first at {at}: {cases[self.requests[j][0]][0]} "
                                 f"{self.requests[j]}, slot at {self.slots[j]}, got {int(self.after[at])} want {int(exp[at])}")


@pytest.mark.parametrize("chunk_bytes", [4096, 65536])
def test_read_plan(dg, ctx, torch_cuda, arena, chunk_bytes):
    cases = hc.corpus()["read"]
    reqs = [(s, off, ln) for s, c in enumerate(cases) for off, ln in c[4]]
    sizes = [0 if cases[s][3] else sm.Stream.of(cases[s][2]).version_size for s, _, _ in reqs]
    r = ReadRun(torch_cuda, dg, ctx, arena, [(c[1], c[2]) for c in cases], reqs, sizes)
    serial, st_serial = r.index().indexes()
    assert st_serial == [c[3] for c in cases]
    r.run().check_model(cases)
    r.set_requests(reqs, sizes)   # a fresh output arena
    r.d_sst.fill_(-1)
    r.plan.chunk_index(chunk_bytes)
    chunked, st_chunked = r.index_chunked().indexes()
    assert st_chunked == st_serial
    for c, a, b in zip(cases, serial, chunked):
        assert a[:32] == b[:32], c[0]
        assert c[3] or (a == b and len(a) == 32 + 8 * (len(c[2]) // 1024 + 1)), c[0]
    r.run().check_model(cases)
    assert r.stream_st == st_serial


# 5. decode: standard streams whose COPYs read R's windows above 2^31
def test_decode_plan(dg, ctx, torch_cuda, arena):
    torch = torch_cuda
    cases = hc.corpus()["decode"]
    pad, descs, dlt, at = 48, [], bytearray([GUARD]) * 5, 16
    for name, ref_len, d, st in cases:
        vs = sm.Stream.of(d).version_size
        descs.append((0, ref_len, len(dlt), len(d), at, vs))
        dlt += d + bytes([GUARD]) * 3
        at += vs + pad + (-vs % 16) + 1   # odd output offsets
    plan = dg.DecodePlan(ctx, descs, ignore_hash=True)
    d_delta = torch.frombuffer(dlt, dtype=torch.uint8).cuda()
    out = torch.full((at,), GUARD, dtype=torch.uint8, device="cuda")
    lens = torch.full((len(cases),), -1, dtype=torch.int64, device="cuda")
    sts = torch.full((len(cases),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan.run(arena.data_ptr(), d_delta.data_ptr(), out.data_ptr(), lens.data_ptr(), sts.data_ptr(), ctx.stream)
    torch.cuda.synchronize()
    got, lens, sts = bytes(out.cpu().numpy()), lens.cpu().tolist(), sts.cpu().tolist()
    exp = bytearray([GUARD]) * at
    for k, (name, ref_len, d, st) in enumerate(cases):
        assert sts[k] == st == sm.decode_status(ref_len, d, descs[k][5]), (name, sts[k], st)
        if st == OK:
            vs = descs[k][5]
            assert lens[k] == vs, name
            exp[descs[k][4]:descs[k][4] + vs] = sm.replay(hc.R.head(ref_len), d, (0, vs))
            assert got[descs[k][4]:descs[k][4] + vs] == exp[descs[k][4]:descs[k][4] + vs], name
    ok = [k for k, c in enumerate(cases) if c[3] == OK]
    last = descs[ok[-1]][4] + descs[ok[-1]][5]
    assert got[:last + pad] == bytes(exp[:last + pad]), "a byte outside an output, or in a refused stream's"


# 6. update: hand-made in-place streams in the arena itself, one plan each; the arena's head is put back after each
def test_update_plan(dg, ctx, torch_cuda, arena):
    torch = torch_cuda
    cases = hc.corpus()["update"]
    head = arena[:HEAD].clone()
    before = bytes(head.cpu().numpy())
    tail = arena[hc.RLEN - 4096:].clone()
    mid = arena[hc.H - 4096:hc.H + 4096].clone()
    try:
        for name, ref_len, d, st in cases:
            plan = dg.UpdatePlan(ctx, [(0, hc.RLEN, ref_len, 0, len(d))], ignore_hash=True)
            d_delta = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
            olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            sts = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            plan.run(arena.data_ptr(), d_delta.data_ptr(), olen.data_ptr(), sts.data_ptr(), stream=ctx.stream)
            torch.cuda.synchronize()
            got = bytes(arena[:HEAD].cpu().numpy())
            arena[:HEAD].copy_(head)
            assert sts.item() == st == sm.update_status(ref_len, d, hc.RLEN), (name, sts.item(), st)
            if st == OK:
                vs = sm.Stream.of(d).version_size
                assert olen.item() == vs, name
                assert got[:vs] == sm.replay(hc.R.head(ref_len), d, (0, vs)), name
                assert got[vs:] == before[vs:], name   # (ref_len is far above: nothing of [version_size, ref_len) is touched here)
            else:
                assert olen.item() == 0 and got == before, name
            plan.close()
        assert torch.equal(arena[hc.RLEN - 4096:], tail) and torch.equal(arena[hc.H - 4096:hc.H + 4096], mid)
    finally:
        arena[:HEAD].copy_(head)
        torch.cuda.synchronize()


# 7. decode_large: a version that crosses 2^31, CRC checks on
def test_decode_large_output_crosses_2p31(dg, ctx, orc, torch_cuda):
    import random
    torch = torch_cuda
    rng = random.Random(0x2338)
    MB = 1 << 20
    B, T = rng.randbytes(MB), rng.randbytes(3)
    R = B + T
    n = 2049
    vs = n * MB + 3
    assert vs == hc.H + MB + 3
    crc_b, crc_t = (int.from_bytes(orc.crc64_xz(x), "big") for x in (B, T))
    dst_crc = sm.crc64_combine(sm.crc64_repeat(crc_b, MB, n), crc_t, 3)   # never from the device
    body = b"".join(b"\x01" + struct.pack(">III", 0, k * MB, MB) for k in range(n)) + b"\x01" + struct.pack(">III", MB, n * MB, 3)
    d = b"DLT\x03\x00" + struct.pack(">I", vs) + orc.crc64_xz(R) + dst_crc.to_bytes(8, "big") + body + b"\x00"
    assert sm.decode_status(len(R), d) == OK and sm.replay(R, d, (vs - 5, vs)) == B[-2:] + T

    def call(delta):
        out = dg._lib.Buffer()
        rc_ = dg.lib.dg_decode_large(ctx.handle, dg._lib._u8(R), len(R), dg._lib._u8(delta), len(delta), 0, 0, 0, C.byref(out))
        return rc_, out

    rc_, out = call(d)
    try:
        assert rc_ == OK and out.len == vs
        host = np.ctypeslib.as_array(C.cast(out.data, C.POINTER(C.c_uint8)), shape=(vs,))
        dev = torch.from_numpy(host).cuda()
        want = torch.frombuffer(bytearray(B), dtype=torch.uint8).cuda()
        assert bool((dev[:n * MB].view(n, MB) == want).all()), "a tile of the output is not B"
        assert bytes(dev[n * MB:].cpu().numpy()) == T
        del dev, host
    finally:
        dg.lib.dg_buffer_free(C.byref(out))
    torch.cuda.empty_cache()
    rc_, out = call(d[:20] + bytes([d[20] ^ 1]) + d[21:])   # one byte of the header's dst_crc
    dg.lib.dg_buffer_free(C.byref(out))
    assert rc_ == DST_CRC


# 8. what the read plan refuses: a length of 4 GiB at create, a stream above 2^32 - 16 bytes for the chunked index
def test_read_plan_limits(dg, ctx):
    for s in [(0, 1 << 32, 0, 100), (0, 100, 0, 1 << 32)]:
        with pytest.raises(dg.DeltaError) as e:
            dg.ReadPlan(ctx, [s], 1)
        assert e.value.code == TOO_LARGE
    p = dg.ReadPlan(ctx, [(0, (1 << 32) - 1, 0, 0xFFFFFFF1)], 1)   # accepted: its index is delta_len / 128 + 64 bytes
    with pytest.raises(dg.DeltaError) as e:
        p.chunk_index(4096)
    assert e.value.code == TOO_LARGE
    p.close()


# 9. lineage: every case in one plan, every request; the one-block index, then the chunked index over it
class HighLineageRun(LineageRun):
    def __init__(self, torch, dg, ctx, d_ref, nodes, requests, sizes):
        """nodes: (ref_len or None, delta, parent, stated ref_len or None); a level on R reads a prefix of d_ref."""
        self.torch, self.dg, self.ctx, self.items, self.nodes = torch, dg, ctx, nodes, nodes
        self.n = len(nodes)
        dlt, self.streams = bytearray(), []
        for k, (_, d, parent, _) in enumerate(nodes):
            dlt += bytes([GUARD]) * ((1 + (3 * k) % 15) if k % 2 else (-len(dlt) % 16))
            # (a level on another version: its ref_off is ignored, an odd one)
            self.streams.append((0 if parent == hc.BASE else 12345, hc.stated_ref_len(nodes, k), len(dlt), len(d)))
            dlt += d
        self.d_ref = d_ref
        self.d_delta = torch.frombuffer(dlt + b"\0", dtype=torch.uint8).cuda()
        self.max_requests = len(requests)
        self.plan = self.reads = dg.ReadPlan(ctx, self.streams, self.max_requests)
        self.lin = dg.LineagePlan(self.reads, [n[2] for n in nodes], self.max_requests)
        self.d_sst = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.set_requests(requests, sizes)

    def check_model(self, expected, names):
        """Run.check with the sparse model's results: every length and status, and the output arena compared whole."""
        exp = self.before.copy()
        for j, ((s, off, ln), (st, got, _)) in enumerate(zip(self.requests, expected)):
            assert self.st[j] == st, (names[j], s, off, ln, self.st[j], st)
            assert self.out_len[j] == len(got), (names[j], s, off, ln, self.out_len[j], len(got))
            o, room = self.slots[j]
            assert len(got) <= room
            exp[o:o + len(got)] = np.frombuffer(got, dtype=np.uint8)
        bad = np.flatnonzero(self.after != exp)
        if bad.size:
            at = int(bad[0])
            j = max(k for k, (o, _) in enumerate(self.slots) if o - 64 <= at)
            raise AssertionError(f"{bad.size} bytes differ, the first at {at}: {names[j]} {self.requests[j]}, "
                                 f"slot at {self.slots[j]}, got {int(self.after[at])} want {int(exp[at])}")


def _lineage_plan(cases):
    """One forest of all cases: (nodes, requests, sizes, expected, case name per request)."""
    nodes, reqs, sizes, expected, names = [], [], [], [], []
    for name, ns, rs, sts in cases:
        base = len(nodes)
        nodes += [(rl, d, p if p == hc.BASE else p + base, stated) for rl, d, p, stated in ns]
        for (i, off, ln), e in zip(rs, hc.LINEAGE_EXPECTED[name]):
            reqs.append((base + i, off, ln))
            sizes.append(0 if sts[i] else sm.Stream.of(ns[i][1]).version_size)
            expected.append(e)
            names.append(name)
    return nodes, reqs, sizes, expected, names


@pytest.mark.parametrize("chunk_bytes", [4096, 65536])
def test_lineage_plan(dg, ctx, torch_cuda, arena, chunk_bytes):
    cases = hc.corpus()["lineage"]
    assert dg.lineage_work_items() == hc.WORK_ITEMS   # the fan-out cases are sized for it
    nodes, reqs, sizes, expected, names = _lineage_plan(cases)
    assert len(reqs) > 3500 and {e[0] for e in expected} == {OK, sm.INVALID_ARG, sm.UNSUPPORTED, sm.MALFORMED}
    r = HighLineageRun(torch_cuda, dg, ctx, arena, nodes, reqs, sizes)
    r.index().run()
    r.check_model(expected, names)
    first, st1, len1, sst1 = r.after.copy(), list(r.st), list(r.out_len), list(r.stream_st)
    r.reset_out()
    r.d_sst.fill_(-1)
    r.reads.chunk_index(chunk_bytes)
    r.reads.index_chunked(r.d_delta.data_ptr(), r.d_sst.data_ptr(), stream=ctx.stream)
    r.run()
    r.check_model(expected, names)
    assert np.array_equal(r.after, first) and r.st == st1 and r.out_len == len1 and r.stream_st == sst1


# 10. the host wrapper on a thinned set: one lineage tree, against dg_read_lineage.  The wrapper takes host bytes
# and uploads them, so it cannot use the module's arena: one tree means one R, 4 GiB on the host and a second
# 4 GiB on the device while the call lasts.  Measured on an MI355X: 2.2 s for the whole test.
def test_read_lineage_batch_equals_read_lineage(dg, ctx, torch_cuda):
    name, ns, rs, sts = next(c for c in hc.corpus()["lineage"] if c[0] == "tree_on_edges")
    assert [n[0] for n in ns].count(hc.RLEN) == 1 and all(n[3] is None for n in ns)
    buf = np.zeros(hc.RLEN, dtype=np.uint8)
    for o, b in hc.R.windows():
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    host_r = buf.tobytes()
    del buf
    # (the wrapper sizes a slot by min(len, version_size): a length of 4 GiB on these versions would be a 4 GiB slot)
    picked = [(q, e) for k, (q, e) in enumerate(zip(rs, hc.LINEAGE_EXPECTED[name]))
              if q[2] <= 1 << 20 and (k % 4 == 0 or e[2] > 400)]   # (and every request of hundreds of pieces)
    assert len(picked) > 100 and sum(1 for _, e in picked if e[2] > 400) >= 2
    got, st = dg.read_lineage_batch([(host_r if n[0] else None, n[1]) for n in ns], [n[2] for n in ns], [q for q, _ in picked],
                                    ctx=ctx, status=True)
    torch_cuda.cuda.empty_cache()
    for k, ((i, off, ln), e) in enumerate(picked):
        assert (st[k], got[k]) == (e[0], e[1]), (i, off, ln)
        if k % 8 == 0:
            assert dg.read_lineage(host_r, hc.lineage_path(ns, i)[1], off, ln) == got[k], (i, off, ln)


# 11. in-place conversion: every case of a policy's list in one plan, against the reference's goldens
class InplaceRun:
    """items: (ref_len, standard delta), every reference a prefix of d_ref.  The streams lie at odd offsets of a
    small arena between guard bytes; the output buffer is out_cap bytes and 4 KiB of guard bytes behind them."""
    TAIL = 4096

    def __init__(self, torch, dg, ctx, d_ref, items, policy, out_cap):
        self.torch, self.ctx, self.n, self.out_cap, self.d_ref = torch, ctx, len(items), out_cap, d_ref
        buf, descs = bytearray(), []
        for k, (ref_len, d) in enumerate(items):
            buf += bytes([GUARD]) * (1 + (3 * k) % 15)
            buf += bytes([GUARD]) * (1 - len(buf) % 2)
            descs.append((0, ref_len, len(buf), len(d)))
            buf += d
        assert all(d[2] % 2 for d in descs)
        self.plan = dg.InplacePlan(ctx, descs, policy)
        self.d_delta = torch.frombuffer(buf + bytes([GUARD]), dtype=torch.uint8).cuda()
        self.out = torch.empty(out_cap + self.TAIL, dtype=torch.uint8, device="cuda")
        self.off = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.st = torch.empty(self.n, dtype=torch.int32, device="cuda")

    def run(self):
        """(statuses, offsets, the whole output buffer) of one run into buffers filled afresh."""
        torch = self.torch
        self.out.fill_(GUARD)
        self.off.fill_(-1)
        self.st.fill_(-1)
        torch.cuda.synchronize()
        self.plan.run(self.d_ref.data_ptr(), self.d_delta.data_ptr(), self.out.data_ptr(), self.out_cap, self.off.data_ptr(),
                      self.st.data_ptr(), stream=self.ctx.stream)
        torch.cuda.synchronize()
        return self.st.cpu().tolist(), self.off.cpu().tolist(), bytes(self.out.cpu().numpy())


def _host_difference(dg, name, ref_len, d, policy, got):
    """Where the device's bytes leave dg_make_inplace's: computed only when a digest differs."""
    buf = np.zeros(hc.RLEN, dtype=np.uint8)
    for o, b in hc.R.windows():
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    out = dg._lib.Buffer()
    rc_ = dg.lib.dg_make_inplace(buf.ctypes.data_as(C.POINTER(C.c_uint8)), ref_len, dg._lib._u8(d), len(d), dg._lib.POLICIES[policy],
                                 C.byref(out), None)
    exp = C.string_at(out.data, out.len) if out.len else b""
    dg.lib.dg_buffer_free(C.byref(out))
    at = next((k for k, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
    return (f"{name} ({policy}): the device's {len(got)} bytes leave dg_make_inplace's {len(exp)} (rc {rc_}) at byte {at}: "
            f"{got[at:at + 26].hex()} for {exp[at:at + 26].hex()}")


def _check_inplace(dg, policy, cases, st, offs, out, good_total):
    """Statuses, packed offsets and bytes of the accepted and refused streams at the front of a batch."""
    at = 0
    for k, (name, ref_len, d, sts) in enumerate(cases):
        assert st[k] == sts[policy], (name, st[k])
        assert offs[k] == at, name
        if sts[policy] == OK:
            g = GOLD_INPLACE[(name, policy)]
            got = out[at:at + g["len"]]
            assert offs[k + 1] - at == g["len"], (name, offs[k + 1] - at, g["len"])
            assert hashlib.sha256(got).hexdigest() == g["sha256"], _host_difference(dg, name, ref_len, d, policy, got)
            at += g["len"]
    assert at == good_total == offs[len(cases)]
    assert out[at:] == bytes([GUARD]) * (len(out) - at), "a byte behind the outputs changed"


@pytest.mark.parametrize("policy", hc.POLICIES)
def test_inplace_plan(dg, ctx, torch_cuda, arena, policy):
    cases = hc.inplace_list(policy)
    assert sum(1 for c in cases if c[3][policy] != OK) == 7
    total = sum(GOLD_INPLACE[(c[0], policy)]["len"] for c in cases if c[3][policy] == OK)
    r = InplaceRun(torch_cuda, dg, ctx, arena, [(c[1], c[2]) for c in cases], policy, total + 100)
    t0 = time.perf_counter()
    st, offs, out = r.run()
    print(f"inplace high-offset batch ({policy}): {len(cases)} streams, {time.perf_counter() - t0:.3f} s")
    _check_inplace(dg, policy, cases, st, offs, out, total)
    assert (st, offs, out) == r.run(), "a second run of the same plan differs"


# 12. out_cap decides: victims of about 2^31 bytes each behind good streams take the packed offsets past 2^32
@pytest.mark.parametrize("policy", hc.POLICIES)
def test_inplace_plan_capacity(dg, ctx, torch_cuda, arena, policy):
    good = hc.inplace_list(policy)[:24]
    while good[-1][3][policy] != OK:
        good.pop()
    assert len(good) >= 20 and sum(1 for c in good if c[3][policy] != OK) >= 3
    caps = [c for c in hc.inplace_capacity_cases() if policy in c[3]]
    assert len(caps) == {"localmin": 3, "constant": 4}[policy]
    total = sum(GOLD_INPLACE[(c[0], policy)]["len"] for c in good if c[3][policy] == OK)
    out_cap = total + 3000
    if policy == "constant":
        # one more, behind the first: the constant policy converts the first copy of an exchange whatever its length, so
        # its length can put this stream's end at 2^32 + 1500: an end kept in 32 bits would lie inside out_cap
        a = hc.U32 + 1500 - (total + caps[0][3][policy]) - 48
        d = hc.sstream([("C", hc.RLEN - a, a), ("C", 0, 8)])
        assert hc.H < a < hc.RLEN and hc.constant_victims(hc.copies_of(d)) == [0] and hc.inplace_size(d, [0]) == a + 48
        caps.insert(1, ("exchange_end_at_2p32_plus_1500", hc.RLEN, d, {policy: a + 48}))
    r = InplaceRun(torch_cuda, dg, ctx, arena, [(c[1], c[2]) for c in good + caps], policy, out_cap)
    st, offs, out = r.run()
    _check_inplace(dg, policy, good, st, offs, out, total)   # every earlier stream exact, and no byte behind them changed
    assert st[len(good):] == [CAPACITY] * len(caps)
    for k, c in enumerate(caps, len(good)):
        assert offs[k + 1] - offs[k] == c[3][policy], (c[0], offs[k + 1] - offs[k], c[3][policy])
    assert offs[-1] > hc.U32
    assert policy != "constant" or offs[len(good) + 2] - hc.U32 == 1500 < out_cap
