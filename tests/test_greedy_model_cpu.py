"""Pins the checker of the greedy tests: the hash-free model of
src/c/greedy.c:88-267 (tests/greedy_cases.py) against a plain brute force and
against the reference's own greedy deltas (tests/golden/golden_greedy.json,
both tie-breaks), and, where the reference is built (oracle/_ref), against the
reference directly on a few hundred small pairs.  No GPU; passes with or
without the GPU encoder.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess

import pytest

import greedy_cases as G

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "golden_greedy.json")
GREEDY = 0


def brute(R: bytes, V: bytes, p: int, splay: bool) -> list:
    """The specification, offset by offset: candidates are the offsets a with
    R[a:a+p] == V[vc:vc+p]; the longest match wins; among the longest the
    largest offset (hash table) or, with --splay, the smallest."""
    cmds, vc, vs = [], 0, 0
    while vc + p <= len(V):
        best_len, best_a = 0, 0
        for a in range(len(R) - p + 1):
            if R[a:a + p] != V[vc:vc + p]:
                continue
            ml = p
            while vc + ml < len(V) and a + ml < len(R) and V[vc + ml] == R[a + ml]:
                ml += 1
            if ml > best_len or (ml == best_len and not splay):
                best_len, best_a = ml, a
        if best_len == 0:
            vc += 1
            continue
        if vs < vc:
            cmds.append(("A", V[vs:vc]))
        cmds.append(("C", best_a, best_len))
        vs = vc = vc + best_len
    if vs < len(V):
        cmds.append(("A", V[vs:]))
    return cmds


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


def test_model_equals_brute_force():
    differ = 0
    for p in (1, 2, 3, 4, 5, 8, 16):
        for R, V in G.random_pairs(0xB207E + p, 60):
            a, b = brute(R, V, p, False), brute(R, V, p, True)
            assert G.greedy_model(R, V, p, False) == a
            assert G.greedy_model(R, V, p, True) == b
            assert G.apply(R, a) == V and G.apply(R, b) == V
            differ += a != b
    assert differ > 50   # the tie-break matters on these inputs
    for name, R, V, p in G.edge_cases() + G.tie_cases() + G.gap_cases()[:6]:
        for splay in (False, True):
            assert G.greedy_model(R, V, p, splay) == brute(R, V, p, splay), (name, splay)


def test_model_equals_golden(orc, golden):
    """Every reference delta: the parsed command list where the bytes are
    inline, the whole delta (length and sha256) always."""
    assert len(golden) > 200
    assert {c["splay"] for c in golden} == {False, True}
    for c in golden:
        if c.get("inplace"):
            continue
        R, V = G.spec_inputs(orc, c)
        assert hashlib.sha256(R).hexdigest() == c["r_sha256"], c["name"]
        assert hashlib.sha256(V).hexdigest() == c["v_sha256"], c["name"]
        cmds = G.greedy_model(R, V, c["p"], c["splay"])
        if "delta_hex" in c:
            assert cmds == G.parse(bytes.fromhex(c["delta_hex"])), (c["name"], c["splay"])
        d = G.serialize(cmds, len(V), orc.crc64_xz(R), orc.crc64_xz(V))
        assert len(d) == c["delta_len"], (c["name"], c["splay"])
        assert hashlib.sha256(d).hexdigest() == c["delta_sha256"], (c["name"], c["splay"])


def test_golden_tie_break_has_teeth(golden):
    by = {}
    for c in golden:
        if not c.get("inplace"):
            by.setdefault((c["name"], c["p"]), {})[c["splay"]] = c["delta_sha256"]
    assert sum(1 for v in by.values() if v[False] != v[True]) >= 20
    tie = by[("tie_xx", 16)]
    assert tie[False] != tie[True]


def test_model_equals_reference(orc, ref, tmp_path):
    import oracle as O
    n = 0
    for p in (1, 2, 3, 4, 5, 8, 16):
        for R, V in G.random_pairs(0x4EF + p, 40):
            assert G.model_delta(orc, R, V, p) == ref.encode(GREEDY, R, V, p=p), (p, n)
            n += 1
    rp, vp, dp = tmp_path / "r", tmp_path / "v", tmp_path / "d"
    for p in (1, 3, 16):
        for R, V in G.random_pairs(0x5B1A7 + p, 25):   # --splay: the reference CLI
            rp.write_bytes(R)
            vp.write_bytes(V)
            subprocess.run([O.REF_CLI, "encode", "greedy", str(rp), str(vp), str(dp), "--splay",
                            "--seed-len", str(p)], check=True, capture_output=True)
            assert G.model_delta(orc, R, V, p, True) == dp.read_bytes(), p
