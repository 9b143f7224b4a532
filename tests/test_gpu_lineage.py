"""GPU: byte ranges of versions that are several deltas away from a whole
buffer (dg_lineage_plan_*, dg_read_lineage_batch), against the Python model of
tests/lineage_cases.py.

The harness is test_gpu_read.py's: the streams of a run sit in one reference
arena and one delta arena, at unaligned offsets for half of them; every
request has a slot at out_off = 0, 1, 7, 13 (mod 16) in turn, 64 guard bytes of
0xA5 between slots, the slots pre-filled with 0x5A; the expected arena is
built on the host and compared whole, so a byte written past n, into a guard
or into a failing request's slot fails the test.
"""
from __future__ import annotations

import random

import numpy as np
import pytest

import lineage_cases as lc
import read_cases as rc
from test_gpu_read import Run

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED, MALFORMED = lc.OK, lc.INVALID_ARG, lc.UNSUPPORTED, lc.MALFORMED


class LineageRun(Run):
    """A read plan and a lineage plan over nodes = (R or None, delta, parent, ref_len or None)."""

    def __init__(self, torch, dg, ctx, nodes, requests, sizes=None, max_requests=None):
        super().__init__(torch, dg, ctx, [(R or b"", d) for R, d, _, _ in nodes], [], max_requests=1)
        self.nodes = nodes
        # a stream on another states its parent's version size (its ref_off is ignored: an odd one)
        self.streams = [(ro if nodes[i][2] == lc.BASE else 12345, lc.stated_ref_len(nodes, i), do, dl)
                        for i, (ro, _, do, dl) in enumerate(self.streams)]
        self.max_requests = len(requests) if max_requests is None else max_requests
        self.plan.close()
        self.plan = self.reads = dg.ReadPlan(ctx, self.streams, self.max_requests)
        self.lin = dg.LineagePlan(self.reads, [n[2] for n in nodes], self.max_requests)
        self.set_requests(requests, sizes)

    def index_chunked(self):
        self.reads.chunk_index()
        self.reads.index_chunked(self.d_delta.data_ptr(), self.d_sst.data_ptr(), stream=self.ctx.stream)
        return self

    def reset_out(self):
        self.d_out.copy_(self.torch.from_numpy(self.before))
        self.d_st.fill_(-1)
        self.d_len.fill_(0x7FFFFFFF)
        return self

    def run(self, lineage=True):
        self.plan = self.lin if lineage else self.reads
        try:
            return super().run()
        finally:
            self.plan = self.reads


def _flatten(cases):
    """One forest of many: (nodes, statuses, versions, requests, sizes)."""
    nodes, sts, vers, reqs, sizes = [], [], [], [], []
    for f, per in cases:
        base = len(nodes)
        for (R, d, p, rl), (st, V, rs) in zip(f["nodes"], per):
            s = len(nodes)
            nodes.append((R, d, p if p == lc.BASE else p + base, rl))
            sts.append(st)
            vers.append(V)
            for off, ln in rs:
                reqs.append((s, off, ln))
                sizes.append(0 if st else len(V))
    return nodes, sts, vers, reqs, sizes


def _run_cases(torch, dg, ctx, cases):
    nodes, sts, vers, reqs, sizes = _flatten(cases)
    r = LineageRun(torch, dg, ctx, nodes, reqs, sizes)
    r.index().run()
    r.check(vers, sts)
    return r, sts, vers


# 1. the whole corpus in one plan, every range a request; the chunked index gives the same
def test_whole_corpus_after_either_index(dg, ctx, orc, torch_cuda):
    cases = lc.corpus(dg, orc)
    r, sts, vers = _run_cases(torch_cuda, dg, ctx, cases)
    assert len(r.requests) > 3000 and sts.count(OK) > 100 and len(sts) - sts.count(OK) > 80
    first, st1, len1 = r.after.copy(), list(r.st), list(r.out_len)
    r.reset_out().index_chunked().run()
    r.check(vers, sts)
    assert np.array_equal(r.after, first) and r.st == st1 and r.out_len == len1


# 2. the dense case: every level 1024 COPYs of 16 bytes, the whole version
def test_dense(dg, ctx, orc, torch_cuda):
    f, per = lc.by_name(dg, orc, "dense")
    assert len(f["nodes"]) * lc.MAX_COPIES_PER_WINDOW >= 4 * dg.lineage_work_items()
    r, sts, vers = _run_cases(torch_cuda, dg, ctx, [(f, per)])
    j = r.requests.index((len(per) - 1, 0, 16 << 10))
    assert r.st[j] == OK and r.out_len[j] == 16 << 10


# 2b. the stack's overflow: more children than the stack has room for
def test_fanout_overflows_the_stack(dg, ctx, orc, torch_cuda):
    f, per = lc.by_name(dg, orc, "fanout")
    assert lc.FANOUT_TOP - 1 + lc.FANOUT_BLOCK > dg.lineage_work_items() - len(f["nodes"])
    r, sts, vers = _run_cases(torch_cuda, dg, ctx, [(f, per)])
    j = r.requests.index((len(per) - 1, 0, len(per[-1][1])))
    assert r.st[j] == OK and r.out_len[j] == len(per[-1][1])


# 3. the fragmenting case: pieces down to single bytes
def test_fragmenting(dg, ctx, orc, torch_cuda):
    r, sts, vers = _run_cases(torch_cuda, dg, ctx, [lc.by_name(dg, orc, "fragmenting")])
    assert sts == [OK] * 5 and len(r.requests) > 300


# 3b. whole windows of zero-length commands: a continuation that moves on in the stream and not in the version
def test_windows_of_zero_length_commands(dg, ctx, orc, torch_cuda):
    f, per = lc.by_name(dg, orc, "zero_length_windows")
    r, sts, vers = _run_cases(torch_cuda, dg, ctx, [(f, per)])
    assert sts == [OK] * 3
    for s in (1, 2):   # the whole version, through every run of them, from the level that has them and from above it
        j = r.requests.index((s, 0, len(vers[s])))
        assert r.st[j] == OK and r.out_len[j] == len(vers[s])


# 4. the order of the statuses: every failing lineage beside served requests of the same launch
def test_status_order(dg, ctx, orc, torch_cuda):
    cases = [c for c in lc.corpus(dg, orc) if c[0]["name"].startswith("fail_")]
    r, sts, vers = _run_cases(torch_cuda, dg, ctx, cases)
    assert {MALFORMED, UNSUPPORTED, INVALID_ARG, OK} == set(sts)
    for (s, off, ln), st, n in zip(r.requests, r.st, r.out_len):
        assert st == sts[s] and (st == OK or n == 0)
    assert sum(1 for (s, off, ln), n in zip(r.requests, r.out_len) if sts[s] == OK and n > 0) > 100


# 5. depth-1 forests: dg_read_plan_run's arena, lengths and statuses, byte for byte
def test_depth_one_equals_the_read_plan(dg, ctx, orc, torch_cuda):
    cases = []
    for c in rc.with_ranges(dg, orc):
        st, vs, cmds = rc.parse(len(c[1]), c[2])
        if st or lc.is_sequential(cmds, vs):
            cases.append(c)
    assert len(cases) > 80 and sum(1 for c in cases if c[3]) == 10
    nodes = [(c[1], c[2], lc.BASE, None) for c in cases]
    reqs = [(s, off, ln) for s, c in enumerate(cases) for off, ln in c[5][::2]]
    sizes = [0 if cases[s][3] else len(cases[s][4]) for s, _, _ in reqs]
    r = LineageRun(torch_cuda, dg, ctx, nodes, reqs, sizes)
    r.index().run(lineage=False)
    want, st, ln = r.after.copy(), list(r.st), list(r.out_len)
    r.reset_out().run()
    assert np.array_equal(r.after, want) and r.st == st and r.out_len == ln
    r.check([c[4] for c in cases], [c[3] for c in cases])


# 6. the same plan again with other requests
def test_rerun_with_new_requests(dg, ctx, orc, torch_cuda):
    f, per = lc.by_name(dg, orc, "history_depth8")
    vers, sts = [p[1] for p in per], [p[0] for p in per]
    rng = random.Random(9)

    def some():
        reqs = [(s, rng.randrange(len(vers[s])), rng.choice([1, 100, 4096, 20000])) for s in rng.choices(range(8), k=48)]
        return reqs, [len(vers[s]) for s, _, _ in reqs]

    r = LineageRun(torch_cuda, dg, ctx, f["nodes"], *some(), max_requests=64)
    r.index().run()
    r.check(vers, sts)
    first = r.after.copy()
    r.reset_out().run()
    assert np.array_equal(r.after, first)
    r.set_requests(*some())
    r.run()
    r.check(vers, sts)


# 7. invalid shapes
def test_invalid(dg, ctx, orc, torch_cuda):
    f, per = lc.by_name(dg, orc, "history_depth3")
    vers, sts = [p[1] for p in per], [p[0] for p in per]
    r = LineageRun(torch_cuda, dg, ctx, f["nodes"], [(2, 3, 10), (3, 0, 10), (1, 5, 7)], max_requests=4)
    with pytest.raises(dg.DeltaError) as e:   # before any index
        r.run()
    assert e.value.code == INVALID_ARG and "index" in str(e.value)
    r.index().run()
    r.check(vers, sts)
    assert r.st == [OK, INVALID_ARG, OK]
    raw = bytearray(r.d_req.cpu().numpy().tobytes())   # reserved != 0: that request only
    raw[12] = 1
    r.d_req = torch_cuda.frombuffer(raw, dtype=torch_cuda.uint8).cuda()
    r.reset_out().run()
    assert r.st == [INVALID_ARG, INVALID_ARG, OK] and r.out_len[0] == 0
    with pytest.raises(dg.DeltaError) as e:   # more requests than the plan was made for
        r.lin.run(r.d_ref.data_ptr(), r.d_delta.data_ptr(), r.d_req.data_ptr(), 5, r.d_out.data_ptr(),
                  r.d_len.data_ptr(), r.d_st.data_ptr())
    assert e.value.code == INVALID_ARG
    r.lin.run(0, 0, 0, 0, 0, 0, 0)   # no requests: nothing runs, nothing is needed
    # the forest: a parent out of range, a cycle, 65 deltas down to the base
    for parents, word in (([lc.BASE, 3, 1], "parent"), ([lc.BASE, 2, 1], "cycle"), ([0, 0, 1], "cycle")):
        with pytest.raises(dg.DeltaError) as e:
            dg.LineagePlan(r.reads, parents, 4)
        assert e.value.code == INVALID_ARG and word in str(e.value), parents
    R = bytes(range(256)) * 4
    same = lc.seq_stream(orc, R, [("C", 0, 700), ("A", b"tail"), ("C", 700, 320)])   # R[:700] + b"tail" + R[700:1020]
    assert len(rc.model_version(R, same)[1]) == len(R)
    chain = lambda k: [(R if j == 0 else None, same, lc.BASE if j == 0 else j - 1, None) for j in range(k)]
    with pytest.raises(dg.DeltaError) as e:
        LineageRun(torch_cuda, dg, ctx, chain(65), [])
    assert e.value.code == INVALID_ARG and "64" in str(e.value)
    # 64 is served
    V = R
    for _ in range(64):
        V = rc.model_version(V, same)[1]
    d = LineageRun(torch_cuda, dg, ctx, chain(64), [(63, 0, 1024), (63, 690, 40), (31, 5, 2000)], [1024] * 3)
    d.index().run()
    d.check([None] * 31 + [rc.model_read(_nth(R, same, 32), 0, 1 << 20)] + [None] * 31 + [V], [OK] * 64)


def _nth(R, d, k):
    for _ in range(k):
        R = rc.model_version(R, d)[1]
    return R


# 8. the host wrappers
def test_read_lineage_batch_equals_read_lineage(dg, ctx, orc):
    cases = [c for c in lc.corpus(dg, orc) if c[0].get("host", True) and c[0].get("dense", True)]
    cases += [c for c in lc.corpus(dg, orc) if c[0]["name"].startswith("fail_") and c[0].get("host", True)][::4]
    nodes, sts, vers, reqs, _ = _flatten(cases)
    reqs = [q for k, q in enumerate(reqs) if sts[q[0]] or k % 5 == 0] + [(len(nodes), 0, 1)]
    got, st = dg.read_lineage_batch([(n[0], n[1]) for n in nodes], [n[2] for n in nodes], reqs, ctx=ctx, status=True)
    assert OK in st and MALFORMED in st and UNSUPPORTED in st
    for (s, off, ln), g, code in zip(reqs, got, st):
        if s >= len(nodes):
            assert code == INVALID_ARG and g == b""
            continue
        R, ds = lc.path(nodes, s)
        try:
            want = (OK, dg.read_lineage(R, ds, off, ln))
        except dg.DeltaError as e:
            want = (e.code, b"")
        assert (code, g) == want, (s, off, ln)
    with pytest.raises(dg.DeltaError):
        dg.read_lineage_batch([(n[0], n[1]) for n in nodes], [n[2] for n in nodes], reqs, ctx=ctx)
    assert dg.read_lineage_batch([(n[0], n[1]) for n in nodes], [n[2] for n in nodes], [], ctx=ctx) == []
    with pytest.raises(dg.DeltaError) as e:
        dg.read_lineage_batch([(None, nodes[0][1])] * 2, [1, 0], [(0, 0, 1)], ctx=ctx)
    assert e.value.code == INVALID_ARG


# 9. stage times of the runs
def test_stage_times(dg, ctx, orc, torch_cuda):
    f, per = lc.by_name(dg, orc, "history_depth3")
    r = LineageRun(torch_cuda, dg, ctx, f["nodes"], [(2, 0, 4096)], [len(per[2][1])])
    r.lin.set_timing(2)
    r.index().run()
    t = r.lin.stage_times()
    assert set(t) == {"read", "total"} and 0 < t["read"] <= t["total"] * 1.001
