"""GPU: dg_sketch_plan_*, dg_sketch_match_device, dg_sketch_batch and pick_bases
(csrc/dg_sketch_dev.hip) produce word for word what the Python model of
tests/sketch_cases.py produces, which tests/test_sketch_cpu.py also pins the
host functions to.

The sketch sweep at every (p, K): all spans of one sweep in one arena, so a read
past a span meets other bytes; buffers whose minimum sits on a chunk seam; guard
words around the output; a re-run on other bytes; the empty plan.  The match
cases on the device against the model and the host function.  Then the chain
sketch plan -> match -> pairs -> encode plan -> decode on a family of bases and
versions.
"""
from __future__ import annotations

import numpy as np
import pytest

import sketch_cases as sc
from stage_timing import check_ring_phases

pytestmark = pytest.mark.gpu

GUARD = 0x5AA55AA55AA55AA5
GUARD_WORDS = 8


def words(t):
    """A device int64 tensor as a list of unsigned words."""
    return t.cpu().numpy().view(np.uint64).tolist()


class Sketches:
    """One plan over `spans` of an arena; the output between guard words."""

    def __init__(self, torch, dg, ctx, spans, p, k):
        self.torch, self.ctx, self.n, self.k = torch, ctx, len(spans), k
        self.plan = dg.SketchPlan(ctx, spans, p=p, k=k)
        self.out = torch.full((self.n * k + 2 * GUARD_WORDS,), GUARD, dtype=torch.int64, device="cuda")

    def run(self, arena: bytes):
        torch = self.torch
        d = torch.frombuffer(bytearray(arena) or bytearray(1), dtype=torch.uint8).cuda()
        assert d.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        self.plan.run(d.data_ptr(), self.out.data_ptr() + 8 * GUARD_WORDS, stream=self.ctx.stream)
        torch.cuda.synchronize()
        w = words(self.out)
        assert w[:GUARD_WORDS] == [GUARD] * GUARD_WORDS and w[-GUARD_WORDS:] == [GUARD] * GUARD_WORDS, "a word outside the n K outputs"
        body = w[GUARD_WORDS:-GUARD_WORDS] if self.n else []
        return [body[i * self.k:(i + 1) * self.k] for i in range(self.n)]


def chunk_bytes(dg, ctx):
    return dg.SketchPlan(ctx, [], p=16, k=16).chunk_bytes


# 1. the sweep: every length, offset residue and content at every (p, K)
@pytest.mark.parametrize("p", sc.SEEDS)
def test_sweep_equals_model(dg, ctx, torch_cuda, p):
    c = chunk_bytes(dg, ctx)
    assert c % 1024 == 0
    bufs = sc.sweep_buffers(p, c)
    assert {len(b) for _, b in bufs} >= set(sc.sweep_lengths(p, c))
    arena, spans = sc.pack([b for _, b in bufs])
    assert {off % 16 for off, _ in spans} == set(range(16))
    assert len(arena) < 1 << 20
    for k in sc.BINS:
        s = Sketches(torch_cuda, dg, ctx, spans, p, k)
        assert s.plan.chunk_bytes == c
        got = s.run(arena)
        for (name, b), g in zip(bufs, got):
            assert g == sc.sketch(b, p, k), (p, k, name)
        assert bufs[0][1] == b"" and got[0] == [sc.EMPTY] * k   # shorter than the seed: every bin empty
        by = {name: g for (name, _), g in zip(bufs, got)}
        assert sum(w != sc.EMPTY for w in by["zeros_%d" % (c + 1)]) == 1


# 2. chunk seams: a bin whose minimum only a window across the chunk boundary attains
@pytest.mark.parametrize("p,k", [(16, 1024), (64, 256), (17, 64)])
def test_chunk_seams(dg, ctx, torch_cuda, p, k):
    c = chunk_bytes(dg, ctx)
    bufs = sc.seam_buffers(p, k, c, count=4)
    assert len(bufs) >= 4
    arena, spans = sc.pack(bufs, first=9)
    got = Sketches(torch_cuda, dg, ctx, spans, p, k).run(arena)
    for i, (b, g) in enumerate(zip(bufs, got)):
        assert g == sc.sketch(b, p, k), (p, k, i)


# 3. a re-run of one plan and one output on other bytes keeps nothing; the empty plan touches nothing
def test_rerun_and_empty_plan(dg, ctx, torch_cuda):
    import random
    torch = torch_cuda
    p, k = 16, 256
    c = chunk_bytes(dg, ctx)
    rng = random.Random(5)
    lens = [c + 300, 40, 0, 2 * c + 1, 15, 700]
    A = [rng.randbytes(n) for n in lens]
    B = [rng.randbytes(n) for n in lens]
    B[1] = bytes(40)   # fewer non-empty bins than A's: a kept minimum would show
    arena_a, spans = sc.pack(A, first=2)
    arena_b, spans_b = sc.pack(B, first=2)
    assert spans == spans_b
    s = Sketches(torch, dg, ctx, spans, p, k)
    assert s.run(arena_a) == [sc.sketch(b, p, k) for b in A]
    got = s.run(arena_b)
    assert got == [sc.sketch(b, p, k) for b in B]
    assert got != [sc.sketch(b, p, k) for b in A]
    # stage times, the ring grown and shrunk; the words stay
    t_names = ["sketch", "total"]
    check_ring_phases(s.plan, lambda: s.run(arena_b), t_names)
    assert s.run(arena_b) == got
    # n == 0: nothing is written, with or without pointers
    e = Sketches(torch, dg, ctx, [], p, k)
    assert e.run(b"") == [] and e.plan.n == 0
    e.plan.run(0, 0, stream=ctx.stream)
    torch.cuda.synchronize()
    # spans shorter than the seed only: no kernel, every bin empty
    z = Sketches(torch, dg, ctx, [(0, 3), (3, 15)], p, k)
    assert z.run(bytes(18)) == [[sc.EMPTY] * k] * 2
    for bad in [dict(p=0), dict(p=65), dict(k=8), dict(k=2048), dict(k=100)]:
        with pytest.raises(dg.DeltaError) as err:
            dg.SketchPlan(ctx, [(0, 10)], **{**dict(p=16, k=256), **bad})
        assert err.value.code == 1
    with pytest.raises(dg.DeltaError) as err:
        dg.SketchPlan(ctx, [(0, 1 << 32)])
    assert err.value.code == 3
    with pytest.raises(dg.DeltaError) as err:   # the arena must be 16-byte aligned
        d = torch.zeros(64, dtype=torch.uint8, device="cuda")
        dg.SketchPlan(ctx, [(0, 20)]).run(d.data_ptr() + 4, s.out.data_ptr())
    assert err.value.code == 1


# 4. the match cases on the device: equal to the model and to the host function
def test_match_equals_model_and_host(dg, ctx, torch_cuda):
    torch = torch_cuda
    pad = 4   # guard dg_match_t in front and behind; the output starts at a 4-byte boundary only
    for name, T, Cd, k, mode, base, min_equal in sc.match_cases():
        n_t, n_c = len(T), len(Cd)
        up = lambda S: torch.from_numpy(np.array([w for s in S for w in s] or [0], dtype=np.uint64).view(np.int64)).cuda()
        d_t, d_c = up(T), up(Cd)
        out = torch.full((4 * (n_t + 2 * pad) + 1,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dg.match_sketches_device(ctx, d_t.data_ptr(), n_t, d_c.data_ptr(), n_c, out.data_ptr() + 4 + 16 * pad,
                                 k=k, mode=mode, target_base=base, min_equal=min_equal, stream=ctx.stream)
        torch.cuda.synchronize()
        w = (out.cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
        guard = (-7) & 0xFFFFFFFF
        assert w[:1 + 4 * pad] == [guard] * (1 + 4 * pad) and w[1 + 4 * (pad + n_t):] == [guard] * (4 * pad), name
        body = w[1 + 4 * pad:1 + 4 * (pad + n_t)]
        got = [tuple(body[4 * t:4 * t + 3]) for t in range(n_t)]
        assert all(body[4 * t + 3] == 0 for t in range(n_t)), name
        assert got == sc.select(T, Cd, mode, base, min_equal), name
        assert got == dg.match_sketches(T, Cd, k, mode, base, min_equal), name
    for bad in [dict(k=8), dict(mode=3), dict(min_equal=0)]:
        with pytest.raises(dg.DeltaError) as err:
            dg.match_sketches_device(ctx, d_t.data_ptr(), 1, d_c.data_ptr(), 1, out.data_ptr(), **{**dict(k=16), **bad})
        assert err.value.code == 1


# 5. end to end: sketch plan -> match -> pairs -> encode plan -> decode
def test_family_picks_its_bases(dg, ctx, orc, torch_cuda):
    torch = torch_cuda
    p, k = 16, 64
    bases, versions = sc.family()
    nb, nv = len(bases), len(versions)
    # the family has the property, by the model: a right pick everywhere, own equal above every other
    sb, sv = [sc.sketch(b, p, k) for b in bases], [sc.sketch(v, p, k) for v in versions]
    want = sc.select(sv, sb)
    for j, v in enumerate(sv):
        eq = [sc.score(v, b)[0] for b in sb]
        assert want[j][0] == j % nb and eq[j % nb] >= 31 and all(e == 0 for i, e in enumerate(eq) if i != j % nb), j

    def arena(bufs):   # 16-byte aligned spans
        lay, buf = [], bytearray()
        for b in bufs:
            lay.append((len(buf), len(b)))
            buf += b + bytes(-len(b) % 16)
        return torch.frombuffer(buf, dtype=torch.uint8).cuda(), lay

    d_r, lr = arena(bases)
    d_v, lv = arena(versions)
    s = ctx.stream
    pr, pv = dg.SketchPlan(ctx, lr, p=p, k=k), dg.SketchPlan(ctx, lv, p=p, k=k)
    d_sb = torch.zeros(nb * k, dtype=torch.int64, device="cuda")
    d_sv = torch.zeros(nv * k, dtype=torch.int64, device="cuda")
    d_m = torch.zeros(nv * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pr.run(d_r.data_ptr(), d_sb.data_ptr(), stream=s)
    pv.run(d_v.data_ptr(), d_sv.data_ptr(), stream=s)
    dg.match_sketches_device(ctx, d_sv.data_ptr(), nv, d_sb.data_ptr(), nb, d_m.data_ptr(), k=k, stream=s)
    torch.cuda.synchronize()
    assert [words(d_sb)[i * k:(i + 1) * k] for i in range(nb)] == sb
    got = [tuple(r[:3]) for r in d_m.cpu().view(nv, 4).tolist()]
    assert got == want

    def encode_all(pick):
        pairs = [(*lr[pick[j]], *lv[j]) for j in range(nv)]
        enc = dg.EncodePlan(ctx, "onepass", pairs, p=p)
        out = torch.zeros(max(enc.output_bound, 1), dtype=torch.uint8, device="cuda")
        off = torch.zeros(nv + 1, dtype=torch.int64, device="cuda")
        st = torch.full((nv,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        enc.run(d_r.data_ptr(), d_v.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * nv
        o, raw = off.cpu().tolist(), bytes(out.cpu().numpy())
        return [raw[o[j]:o[j + 1]] for j in range(nv)]

    picked = encode_all([g[0] for g in got])
    for j, d in enumerate(picked):
        assert dg.decode(bases[got[j][0]], d, ctx=ctx) == versions[j], j
    against_first = encode_all([0] * nv)
    assert sum(map(len, picked)) < sum(map(len, against_first))


# 6. pick_bases and sketch_batch
def test_pick_bases_and_sketch_batch(dg, ctx, torch_cuda):
    p, k = 16, 64
    bases, versions = sc.family()
    everything = list(bases) + list(versions)
    model = [sc.sketch(b, p, k) for b in everything]
    assert dg.sketch_batch(everything, p=p, k=k, ctx=ctx) == model
    assert dg.sketch_batch([], ctx=ctx) == [] and dg.sketch_batch([b"", b"abc"], k=16, ctx=ctx) == [[sc.EMPTY] * 16] * 2
    got = dg.pick_bases(everything, mode="earlier", p=p, k=k, ctx=ctx)
    want = [(None if b == sc.NONE else b, e, u) for b, e, u in sc.select(model, model, sc.EARLIER)]
    assert got == want
    for i, (b, _, _) in enumerate(got):
        assert b is None or b < i
        if i < len(bases):
            assert b is None                       # nothing earlier resembles a base
        else:
            assert b % len(bases) == i % len(bases)   # its base, or an earlier version of the same base
    got = dg.pick_bases(everything, mode="not_self", p=p, k=k, min_equal=5, ctx=ctx)
    assert got == [(None if b == sc.NONE else b, e, u) for b, e, u in sc.select(model, model, sc.NOT_SELF, 0, 5)]
    assert all(b is not None and b != i for i, (b, _, _) in enumerate(got))
    assert dg.pick_bases([], ctx=ctx) == []
