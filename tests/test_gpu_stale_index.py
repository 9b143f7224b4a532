"""GPU: the containment contract of dg_read_plan_run and dg_lineage_plan_run
under a stale index (include/delta_gpu.h): a plan is indexed on batch A, the
delta arena is overwritten in place with batch B of the same layout
(tests/stale_cases.py: valid streams or a constant fill; the harness is
test_gpu_read.Run's, through ChunkedRun and LineageRun), and the plan runs
WITHOUT another index pass.

What the contract promises then, and what is asserted for every family but
"payload": every status is DG_OK or DG_ERR_MALFORMED; out_len is at most the
slot's room; a lineage request that ends MALFORMED has out_len 0; the output
arena equals its before-image everywhere outside the slots (the harness of
test_gpu_read.py: 0xA5 guards between slots pre-filled with 0x5A); the status
and length arrays beyond n_req are untouched; and an index pass plus a run
afterwards give exactly the model's results for B, so the plan is not
poisoned.  How the requests split into OK and MALFORMED is unspecified: the
split is reported in the assertion messages, not asserted.  In the "payload"
family only ADD payload bytes differ, the index depends on the framing alone,
and every request must return the model's bytes for B with DG_OK.

That every loop of both kernels terminates on arbitrary delta bytes is argued
in DESIGN.md ("Termination on arbitrary delta bytes"); tests/test_stale_cases_cpu.py
checks on the CPU that every case here is stale.
"""
from __future__ import annotations

import random

import numpy as np
import pytest

import lineage_cases as lc
import read_cases as rc
import stale_cases as sc
from test_gpu_index_chunked import ChunkedRun
from test_gpu_lineage import LineageRun

pytestmark = pytest.mark.gpu

OK, MALFORMED = 0, 8
TAIL = 8   # entries of the status and length arrays beyond n_req
STALE = ["framing", "smaller", "larger", "unordered"]


def _arm(r):
    """A fresh output arena, and status and length arrays TAIL entries longer than the run's n_req."""
    torch = r.torch
    r.d_out.copy_(torch.from_numpy(r.before))
    r.d_st = torch.full((r.m + TAIL,), -1, dtype=torch.int32, device="cuda")
    r.d_len = torch.full((r.m + TAIL,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    return r


def _overwrite(r, streams):
    """The delta arena in place: streams[i] over stream i (None: as it is), or one byte value over all of it."""
    dl = bytearray(r.d_delta.cpu().numpy().tobytes())
    if isinstance(streams, int):
        dl[:] = bytes([streams]) * len(dl)
    else:
        for (_, _, do, n), d in zip(r.streams, streams):
            if d is not None:
                assert len(d) == n
                dl[do:do + n] = d
    r.d_delta.copy_(r.torch.frombuffer(dl, dtype=r.torch.uint8))
    r.torch.cuda.synchronize()


def _contained(r, what, lineage):
    """The contract under a stale index; returns the split for the messages."""
    split = f"{what}: {r.st.count(OK)} requests OK, {r.st.count(MALFORMED)} MALFORMED"
    print(split)
    assert set(r.st) <= {OK, MALFORMED}, (split, sorted(set(r.st)))
    inside = np.zeros(len(r.after), dtype=bool)
    for j, (o, room) in enumerate(r.slots):
        inside[o:o + room] = True
        assert 0 <= r.out_len[j] <= room, (split, j, r.requests[j], r.out_len[j], room)
        assert not lineage or r.st[j] == OK or r.out_len[j] == 0, (split, j, r.requests[j], r.out_len[j])
    bad = np.flatnonzero((r.after != r.before) & ~inside)
    assert bad.size == 0, (split, f"{bad.size} bytes outside the slots changed, the first at {int(bad[0])}")
    assert r.d_st.cpu().tolist()[r.m:] == [-1] * TAIL and r.d_len.cpu().tolist()[r.m:] == [0x7FFFFFFF] * TAIL, split
    return split


# ── the read plan ──

def _read_setup(torch, dg, ctx, cases):
    """(run on A, V of every A_i, V of every B_i)"""
    rng = random.Random(0x57A20)
    va = [rc.model_version(R, a)[1] for _, R, a, _ in cases]
    vb = [va[k] if b is None else rc.model_version(R, b)[1] for k, (_, R, _, b) in enumerate(cases)]
    reqs, sizes = [], []
    for s in range(len(cases)):
        vs = max(len(va[s]), len(vb[s]))   # the slot has room for either version's bytes
        for off, ln in sc.requests(rng, vs):
            reqs.append((s, off, ln))
            sizes.append(vs)
    r = ChunkedRun(torch, dg, ctx, [(R, a) for _, R, a, _ in cases], reqs)
    r.set_requests(reqs, sizes)
    return r, va, vb


def _index(r, chunked):
    """An index pass over what the delta arena holds now (dg_read_plan_chunk_index is called once per plan)."""
    r.d_sst.fill_(-1)
    if not chunked:
        return r.index()
    if not getattr(r, "chunks_laid_out", False):
        r.plan.chunk_index(4096)
        r.chunks_laid_out = True
    r.plan.index_chunked(r.d_delta.data_ptr(), r.d_sst.data_ptr(), stream=r.ctx.stream)
    return r


@pytest.mark.parametrize("chunked", [False, True], ids=["one_block", "chunked"])
@pytest.mark.parametrize("family", ["payload"] + STALE)
def test_read_plan_after_the_deltas_change(dg, ctx, orc, torch_cuda, family, chunked):
    cases = sc.read_families(orc)[family]
    assert len(cases) >= sc.MIN_STREAMS
    for name, R, a, b in cases:   # the precondition, once more: a case that is not stale proves nothing
        assert sc.stale(len(R), a, b) == (family != "payload"), name
    r, va, vb = _read_setup(torch_cuda, dg, ctx, cases)
    n = len(cases)
    _index(r, chunked).run()
    r.check(va, [OK] * n)
    _overwrite(r, [c[3] for c in cases])
    _arm(r).run()   # no index pass
    if family == "payload":
        r.check(vb, [OK] * n)
        return
    split = _contained(r, f"read, {family}", False)
    _index(r, chunked)
    _arm(r).run()
    assert r.stream_st == [OK] * n, split
    try:
        r.check(vb, [OK] * n)
    except AssertionError as e:
        raise AssertionError(f"after a new index pass ({split}): {e}") from None


@pytest.mark.parametrize("chunked", [False, True], ids=["one_block", "chunked"])
def test_read_plan_after_the_arena_is_filled(dg, ctx, orc, torch_cuda, chunked):
    cases = sc.read_families(orc)["fills"]
    assert len(cases) >= sc.MIN_STREAMS
    r, va, _ = _read_setup(torch_cuda, dg, ctx, cases)
    n = len(cases)
    _index(r, chunked).run()
    r.check(va, [OK] * n)
    splits = []
    for f in sc.FILLS:
        _overwrite(r, f)
        _arm(r).run()   # no index pass
        splits.append(_contained(r, f"read, fill {f:#04x}", False))
    _index(r, chunked)
    _arm(r).run()
    assert r.stream_st == [MALFORMED] * n and r.st == [MALFORMED] * r.m and r.out_len == [0] * r.m, splits
    assert np.array_equal(r.after, r.before), splits
    _overwrite(r, [c[2] for c in cases])   # A again (the guards between the streams stay filled)
    _index(r, chunked)
    _arm(r).run()
    r.check(va, [OK] * n)


# ── the lineage plan ──

def _lineage_setup(torch, dg, ctx, cases, fill=None):
    """One forest of every case: (run on A, B's delta per stream or None, per stream (status, V) of A and of B)."""
    rng = random.Random(0x57A21)
    nodes, other, exp_a, exp_b, reqs, sizes = [], [], [], [], [], []
    for name, na, nb in cases:
        if fill is not None:   # nb is the level to fill
            nb = [n if i != nb else (n[0], bytes([fill]) * len(n[1]), n[2], n[3]) for i, n in enumerate(na)]
        base = len(nodes)
        ra = lc.resolve(dict(name=name, nodes=na, host=False, dense=False))
        rb = lc.resolve(dict(name=name, nodes=nb, host=False, dense=False))
        assert all(st == OK for st, _, _ in ra), name
        changed = [i for i, (a, b) in enumerate(zip(na, nb)) if a[1] != b[1]]
        assert len(changed) == 1, name   # one level at a time
        for i, (a, b) in enumerate(zip(na, nb)):
            nodes.append((a[0], a[1], a[2] if a[2] == lc.BASE else a[2] + base, a[3]))
            other.append(b[1] if i in changed else None)
            exp_a.append((ra[i][0], ra[i][1]))
            exp_b.append((rb[i][0], rb[i][1]))
        for i in sorted({changed[0], (changed[0] + len(na)) // 2, len(na) - 1}):   # the level itself and levels that read through it
            vs = max(len(ra[i][1]), len(rb[i][1] or b""), lc.header_size(nb[i][1]) or 0)
            for off, ln in sc.requests(rng, vs)[:6]:
                reqs.append((base + i, off, ln))
                sizes.append(vs)
    r = LineageRun(torch, dg, ctx, nodes, reqs, sizes)
    return r, other, exp_a, exp_b


@pytest.mark.parametrize("chunked", [False, True], ids=["one_block", "chunked"])
@pytest.mark.parametrize("family", ["payload"] + STALE)
def test_lineage_plan_after_the_deltas_change(dg, ctx, orc, torch_cuda, family, chunked):
    cases = sc.lineage_families(dg, orc)[family]
    assert len(cases) >= sc.MIN_STREAMS
    for ref_len, a, b in sc.lineage_streams(cases):
        assert sc.stale(ref_len, a, b) == (family != "payload")
    r, other, exp_a, exp_b = _lineage_setup(torch_cuda, dg, ctx, cases)
    _index(r, chunked).run()
    r.check([v for _, v in exp_a], [st for st, _ in exp_a])
    _overwrite(r, other)
    _arm(r).run()   # no index pass
    if family == "payload":
        assert [st for st, _ in exp_b] == [OK] * r.n
        r.check([v for _, v in exp_b], [OK] * r.n)
        return
    split = _contained(r, f"lineage, {family}", True)
    _index(r, chunked)
    _arm(r).run()
    try:
        r.check([v for _, v in exp_b], [st for st, _ in exp_b])
    except AssertionError as e:
        raise AssertionError(f"after a new index pass ({split}): {e}") from None


@pytest.mark.parametrize("chunked", [False, True], ids=["one_block", "chunked"])
def test_lineage_plan_after_a_level_is_filled(dg, ctx, orc, torch_cuda, chunked):
    cases = sc.lineage_families(dg, orc)["fills"]
    assert len(cases) == 7   # depth 1, 3 and 8: the top, the middle and the base level of each
    splits = []
    for f in sc.FILLS:
        r, other, exp_a, exp_b = _lineage_setup(torch_cuda, dg, ctx, cases, fill=f)
        _index(r, chunked).run()
        r.check([v for _, v in exp_a], [st for st, _ in exp_a])
        _overwrite(r, other)
        _arm(r).run()   # no index pass
        splits.append(_contained(r, f"lineage, fill {f:#04x}", True))
        _index(r, chunked)
        _arm(r).run()
        assert MALFORMED in [st for st, _ in exp_b], splits
        r.check([v for _, v in exp_b], [st for st, _ in exp_b])
    # the whole arena filled, every stream and the bytes between them, under the index of A
    _overwrite(r, [n[1] for n in r.nodes])
    _index(r, chunked)
    _arm(r).run()
    r.check([v for _, v in exp_a], [st for st, _ in exp_a])
    for f in sc.FILLS:
        _overwrite(r, f)
        _arm(r).run()   # no index pass
        _contained(r, f"lineage, arena {f:#04x}", True)
    _index(r, chunked)
    _arm(r).run()
    assert r.st == [MALFORMED] * r.m and r.out_len == [0] * r.m and np.array_equal(r.after, r.before), splits
