"""The GPU greedy encoder (dg_greedy.hip) through every entry point, byte for
byte against the hash-free model of src/c/greedy.c:88-267 (tests/greedy_cases.py,
itself pinned to the reference by tests/test_greedy_model_cpu.py) and against
the reference's own deltas (tests/golden/golden_greedy.json), for both
tie-breaks (hash table: the largest offset among the longest matches;
--splay: the smallest).  Every delta is decoded back on the GPU.

Pairs are grouped into one batch or plan per (p, splay), so mixed sizes share
a plan.  The shapes are the smallest at which the kernels can go wrong: the
64-position stride of the miss run, the 64-candidate tiles of a bucket, the
lane / wave hand-over of the match extension, the 64-record tiles and the three
payload paths of the serialiser.
"""
from __future__ import annotations

import hashlib
import json
import os
import random
import subprocess

import pytest

import greedy_cases as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "delta")
GREEDY = 0
MODES = [False, True]


def _mode_id(s):
    return "splay" if s else "table"


def _check_batch(dg, ctx, orc, items, p, splay):
    """items: (name, R, V); one encode_batch; each delta = the model's, decodes to V."""
    got = dg.encode_batch([(R, V) for _, R, V in items], "greedy", p=p, splay=splay, ctx=ctx)
    for (name, R, V), d in zip(items, got):
        assert d == G.model_delta(orc, R, V, p, splay), (name, p, splay)
        assert dg.decode(R, d, ctx=ctx) == V, (name, p, splay)
    return got


def _by_p(cases):
    groups = {}
    for name, R, V, p in cases:
        groups.setdefault(p, []).append((name, R, V))
    return groups


# 1. random small pairs over small alphabets
@pytest.mark.parametrize("splay", MODES, ids=_mode_id)
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8, 16, 17, 32])
def test_random_small_pairs(dg, ctx, orc, p, splay):
    items = [(f"rand{i}", R, V) for i, (R, V) in enumerate(G.random_pairs(0x6EED0 + p, 40))]
    _check_batch(dg, ctx, orc, items, p, splay)


# 2-8. edges, ties, match lengths, gap lengths, > 128 records, long buckets
@pytest.mark.parametrize("splay", MODES, ids=_mode_id)
@pytest.mark.parametrize("group", ["edge_cases", "tie_cases", "match_length_cases", "gap_cases",
                                   "record_cases", "bucket_cases"])
def test_named_cases(dg, ctx, orc, group, splay):
    for p, items in _by_p(getattr(G, group)()).items():
        got = _check_batch(dg, ctx, orc, items, p, splay)
        cmds = {name: G.parse(d) for (name, _, _), d in zip(items, got)}
        if group == "tie_cases":
            assert cmds["tie_xx"] == [("C", 0 if splay else 300, 300)]
            assert cmds["longest_late"] == [("C", 90, 500)]
            assert cmds["longest_early"] == [("C", 0, 500)]
        if group == "edge_cases":
            if p == 16:
                assert cmds["v_empty"] == [] and cmds["eq_p"] == [("C", 0, 16)]
                assert cmds["last_seed"][1] == ("C", 34, 16)
                assert [c[0] for c in cmds["tail_pm1"]] == ["A"]
            else:
                assert cmds["v_lt4_gap"] == [("A", b"x"), ("C", 0, 2)]
        if group == "record_cases":
            assert sum(c[0] == "C" for c in cmds["blocks130"]) >= 130
        if group == "bucket_cases" and p == 16:
            assert cmds["zeros_p16"] == [("C", 0, 4096)]
            assert cmds["motif200"][0][:2] == ("C", 24 * 137)


# ── plans over torch buffers ─────────────────────────────────────────────────

def _plan_run(torch, ctx, plan, ref_t, ver_t):
    n = plan.n
    out = torch.empty(max(plan.output_bound, 1), dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan.run(ref_t.data_ptr(), ver_t.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(),
             st.data_ptr(), ctx.stream)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    offs = off.cpu().tolist()
    outc = bytes(out.cpu().numpy())
    return [outc[offs[i]:offs[i + 1]] for i in range(n)]


def _arena(torch, chunks, size):
    buf = bytearray(size)
    for o, b in chunks:
        buf[o:o + len(b)] = b
    t = torch.empty(max(size, 1), dtype=torch.uint8, device="cuda")
    if size:
        t[:size] = torch.frombuffer(buf, dtype=torch.uint8)
    return t


# 9. layout: odd offsets, shared R, the last pair ends at the last byte of both arenas
@pytest.mark.parametrize("splay", MODES, ids=_mode_id)
def test_plan_layout_unaligned(dg, ctx, orc, torch_cuda, splay):
    rng = random.Random(99)
    pairs = G.random_pairs(0x1A7, 12)
    shared = bytes(rng.randrange(4) for _ in range(173))
    vs8 = [shared[rng.randrange(100):][:rng.randrange(20, 70)] + bytes(rng.randrange(4) for _ in range(i + 1))
           for i in range(8)]
    X = rng.randbytes(333)
    last = (rng.randbytes(21) + X, rng.randbytes(3) + X)   # its match ends at the last byte of both arenas
    lay, rch, vch = [], [], []
    rt, vt = 1, 3   # odd offsets throughout

    def odd(x):
        return x | 1

    for R, V in pairs:
        lay.append((rt, len(R), vt, len(V)))
        rch.append((rt, R))
        vch.append((vt, V))
        rt, vt = odd(rt + len(R)), odd(vt + len(V))
    r_shared = rt
    rch.append((rt, shared))
    rt = odd(rt + len(shared))
    for V in vs8:   # eight pairs share one r_off
        lay.append((r_shared, len(shared), vt, len(V)))
        vch.append((vt, V))
        vt = odd(vt + len(V))
    lay.append((rt, len(last[0]), vt, len(last[1])))
    rch.append((rt, last[0]))
    vch.append((vt, last[1]))
    rt, vt = rt + len(last[0]), vt + len(last[1])   # the arenas end here, to the byte
    inputs = pairs + [(shared, V) for V in vs8] + [last]
    ref_t, ver_t = _arena(torch_cuda, rch, rt), _arena(torch_cuda, vch, vt)
    assert ref_t.numel() == rt and ver_t.numel() == vt
    plan = dg.EncodePlan(ctx, "greedy", lay, p=4, splay=splay)
    assert plan.table_size(0) == 0 and not plan.members
    got = _plan_run(torch_cuda, ctx, plan, ref_t, ver_t)
    for i, ((R, V), d) in enumerate(zip(inputs, got)):
        assert d == G.model_delta(orc, R, V, 4, splay), i
        assert dg.decode(R, d, ctx=ctx) == V


def _fixed_shape_pairs(seed, n):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        R = bytes(rng.randrange(4) for _ in range(150))
        V = bytearray(rng.randrange(4) for _ in range(180))
        a, at = rng.randrange(90), rng.randrange(120)
        V[at:at + 60] = R[a:a + 60]
        out.append((R, bytes(V)))
    return out


# 10. re-run: same bytes twice, then other bytes in the same layout (no stale index)
def test_plan_rerun(dg, ctx, orc, torch_cuda):
    n = 16
    A, B = _fixed_shape_pairs(1, n), _fixed_shape_pairs(2, n)
    lay = [(160 * i, 150, 192 * i, 180) for i in range(n)]
    plan = dg.EncodePlan(ctx, "greedy", lay, p=8)

    def run(pairs):
        ref_t = _arena(torch_cuda, [(160 * i, R) for i, (R, _) in enumerate(pairs)], 160 * n)
        ver_t = _arena(torch_cuda, [(192 * i, V) for i, (_, V) in enumerate(pairs)], 192 * n)
        return _plan_run(torch_cuda, ctx, plan, ref_t, ver_t)

    a1, a2 = run(A), run(A)
    assert a1 == a2
    assert a1 == [G.model_delta(orc, R, V, 8) for R, V in A]
    assert run(B) == [G.model_delta(orc, R, V, 8) for R, V in B]
    assert run(A) == a1


# 11. mid-size pairs against the reference's deltas (goldens; the library where built)
@pytest.mark.parametrize("splay", MODES, ids=_mode_id)
def test_midsize_golden(dg, ctx, orc, splay):
    import oracle as O
    golden = {(c["name"], c["splay"]): c
              for c in json.load(open(os.path.join(HERE, "golden", "golden_greedy.json")))["cases"]
              if not c.get("inplace")}
    specs = G.midsize_specs()
    ins = [G.spec_inputs(orc, s) for s in specs]
    got = dg.encode_batch(ins, "greedy", p=16, splay=splay, ctx=ctx)
    ref = O.Reference() if O.reference_available() and not splay else None
    for s, (R, V), d in zip(specs, ins, got):
        c = golden[(s["name"], splay)]
        assert len(d) == c["delta_len"], s["name"]
        assert hashlib.sha256(d).hexdigest() == c["delta_sha256"], s["name"]
        assert dg.decode(R, d, ctx=ctx) == V
        if ref is not None:   # (the library has no --splay switch: ref_encode_pair passes no flags)
            assert d == ref.encode(GREEDY, R, V, p=16), s["name"]


# 12. surfaces
def _model_cmds(dg, R, V, p, splay):
    return [dg.CopyCmd(c[1], c[2]) if c[0] == "C" else dg.AddCmd(c[1]) for c in G.greedy_model(R, V, p, splay)]


def test_diff_surfaces(dg, ctx):
    for p, (R, V) in zip((2, 4, 16, 16), G.random_pairs(0xD1FF, 4)):
        for splay in MODES:
            want = _model_cmds(dg, R, V, p, splay)
            assert dg.diff(R, V, "greedy", p=p, splay=splay, ctx=ctx) == want
            assert dg.diff_greedy(R, V, p, splay, ctx=ctx) == want
    name, R, V, p = G.tie_cases()[0]
    assert dg.diff_greedy(R, V, p, ctx=ctx) == [dg.CopyCmd(300, 300)]
    assert dg.diff_greedy(R, V, p, splay=True, ctx=ctx) == [dg.CopyCmd(0, 300)]


@pytest.mark.parametrize("splay", MODES, ids=_mode_id)
def test_pipelined_equals_batch(dg, ctx, splay):
    pairs = G.random_pairs(0x919E, 30) + [(R, V) for _, R, V, p in G.gap_cases()]
    want = dg.encode_batch(pairs, "greedy", p=16, splay=splay, ctx=ctx)
    assert dg.encode_pipelined(pairs, "greedy", p=16, splay=splay, chunk_bytes=4096, ctx=ctx) == want
    assert dg.encode_pipelined(pairs, "greedy", p=16, splay=splay, align=1, ctx=ctx) == want


def test_inplace_equals_reference(dg, ctx, orc):
    import oracle as O
    cases = [c for c in json.load(open(os.path.join(HERE, "golden", "golden_greedy.json")))["cases"]
             if c.get("inplace")]
    assert len(cases) >= 8
    ref = O.Reference() if O.reference_available() else None
    for c in cases:
        R, V = G.spec_inputs(orc, c)
        d = dg.encode(R, V, "greedy", p=c["p"], inplace=True, policy=("localmin", "constant")[c["policy"]], ctx=ctx)
        assert len(d) == c["delta_len"] and hashlib.sha256(d).hexdigest() == c["delta_sha256"], c["name"]
        assert dg.decode(R, d, ctx=ctx) == V
        if ref is not None:
            assert d == ref.encode_inplace(GREEDY, R, V, p=c["p"], policy=c["policy"])


@pytest.mark.parametrize("dominant", [False, True])
def test_stage_times(dg, ctx, torch_cuda, dominant):
    pairs = _fixed_shape_pairs(3, 8)
    lay = [(160 * i, 150, 192 * i, 180) for i in range(8)]
    plan = dg.EncodePlan(ctx, "greedy", lay, p=16)
    plan.set_timing(1, dominant_only=dominant)
    ref_t = _arena(torch_cuda, [(160 * i, R) for i, (R, _) in enumerate(pairs)], 160 * 8)
    ver_t = _arena(torch_cuda, [(192 * i, V) for i, (_, V) in enumerate(pairs)], 192 * 8)
    _plan_run(torch_cuda, ctx, plan, ref_t, ver_t)
    t = plan.stage_times()
    assert t["greedy_build"] > 0 and t["greedy_scan"] > 0
    assert "corr_build" not in t and "corr_scan" not in t
    if dominant:
        assert set(t) == {"diff", "greedy_build", "greedy_scan"}


def test_splay_still_unsupported_elsewhere(dg, ctx):
    R, V = G.random_pairs(5, 1)[0]
    for algo in ("onepass", "correcting"):
        with pytest.raises(dg.DeltaError) as e:
            dg.encode(R, V, algo, splay=True, ctx=ctx)
        assert e.value.code == 2   # DG_ERR_UNSUPPORTED
        with pytest.raises(dg.DeltaError) as e:
            dg.EncodePlan(ctx, algo, [(0, 10, 0, 10)], splay=True)
        assert e.value.code == 2
    with pytest.raises(dg.DeltaError) as e:   # in-place stays a host step after the plan
        dg.EncodePlan(ctx, "greedy", [(0, 10, 0, 10)], inplace=True)
    assert e.value.code == 2


# 13. the command line against the reference's
@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="reference CLI not built (oracle/_ref)")
@pytest.mark.parametrize("extra", [[], ["--splay"], ["--seed-len", "4"], ["--verbose"], ["--inplace"],
                                   ["--splay", "--inplace", "--verbose"]], ids=lambda e: "_".join(e) or "plain")
def test_cli_equals_reference(tmp_path, extra):
    rng = random.Random(13)
    X = bytes(rng.randrange(4) for _ in range(3000))
    R = X + rng.randbytes(500) + X[:1000]
    V = X[1500:] + rng.randbytes(7) + X[:1500] + R[3000:3400]
    rp, vp = tmp_path / "r", tmp_path / "v"
    rp.write_bytes(R)
    vp.write_bytes(V)
    ours = subprocess.run([CLI, "encode", "greedy", str(rp), str(vp), str(tmp_path / "d")] + extra,
                          capture_output=True, text=True)
    ref = subprocess.run([REF_CLI, "encode", "greedy", str(rp), str(vp), str(tmp_path / "e")] + extra,
                         capture_output=True, text=True)
    assert ours.returncode == ref.returncode == 0, (ours.stderr, ref.stderr)
    assert (tmp_path / "d").read_bytes() == (tmp_path / "e").read_bytes()

    def lines(s, a, b):   # stdout but the Time: line; the delta's path differs by design of the test
        return [ln.replace(str(tmp_path / a), str(tmp_path / b)) for ln in s.splitlines() if not ln.startswith("Time:")]

    assert lines(ours.stdout, "d", "e") == lines(ref.stdout, "e", "e")
    assert ours.stderr == ref.stderr


def test_cli_greedy_runs_and_splay_rejected_elsewhere(tmp_path, dg, ctx, orc):
    name, R, V, p = G.tie_cases()[0]
    rp, vp, dp = tmp_path / "r", tmp_path / "v", tmp_path / "d"
    rp.write_bytes(R)
    vp.write_bytes(V)
    for extra, splay in (([], False), (["--splay"], True)):
        r = subprocess.run([CLI, "encode", "greedy", str(rp), str(vp), str(dp)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert dp.read_bytes() == G.model_delta(orc, R, V, 16, splay)
        assert r.stdout.splitlines()[0] == "Algorithm:    greedy" + (" [splay]" if splay else "")
    r = subprocess.run([CLI, "encode", "greedy", str(rp), str(vp), str(dp), "--splay", "--inplace"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "Algorithm:    greedy [splay] + in-place (localmin)"
    for algo in ("onepass", "correcting"):
        r = subprocess.run([CLI, "encode", algo, str(rp), str(vp), str(dp), "--splay"], capture_output=True, text=True)
        assert r.returncode == 1 and "--splay is not provided by the MI355X build" in r.stderr
