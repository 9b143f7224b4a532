"""CPU: dg.compose (dg_compose, csrc/dg_compose.cpp) joins delta(R -> V1) and
delta(V1 -> V2) into delta(R -> V2) in the normal form of include/delta_gpu.h.

Every case must equal the Python model (tests/compose_cases.py, which run-length
encodes the byte-provenance map) byte for byte, and the oracle must decode the
result against R to V2 with both CRC checks on.  Then the laws that follow from
the normal form being a function of the provenance map (associativity, the
identity), every failure status in its precedence, and the CLI.
"""
from __future__ import annotations

import os
import random
import subprocess

import pytest

import compose_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")


def check(dg, orc, c):
    name, R, V1, V2, A, B = c
    C = dg.compose(A, B)
    assert C == cc.model_compose(dg, A, B), name
    rc, out = orc.decode(R, C)
    assert rc == 0 and out == V2, name
    return C


def test_model_is_not_vacuous(dg, orc):
    """The model against hand-written normal forms."""
    R = bytes(range(200))
    _, _, _, _, A, B = cc.case(dg, orc, "x", R, [("C", 10, 20), ("C", 30, 20), ("A", b"lit")], [("C", 5, 30), ("C", 35, 8), ("A", b"!")])
    cmds, inplace, vs, src_crc, dst_crc = dg.decode_delta(cc.model_compose(dg, A, B))
    assert [(type(c).__name__, c.dst) for c in cmds] == [("PlacedCopy", 0), ("PlacedAdd", 35)]
    assert (cmds[0].src, cmds[0].length, bytes(cmds[1].data)) == (15, 35, b"lit!")
    assert (inplace, vs, src_crc, dst_crc) == (False, 39, orc.crc64_xz(R), dg.decode_delta(B)[4])


def test_random_small_pairs(dg, orc):
    for c in cc.random_cases(dg, orc):
        check(dg, orc, c)


def test_command_counts(dg, orc):
    for c in cc.count_cases(dg, orc):
        check(dg, orc, c)


def test_shaped_cases(dg, orc):
    got = {c[0]: check(dg, orc, c) for c in cc.shaped_cases(dg, orc)}

    def shape(name):
        return [(type(c).__name__[6:], c.length if hasattr(c, "length") else len(c.data)) for c in dg.decode_delta(got[name])[0]]

    assert shape("merge_across_b") == [("Copy", 100)]
    assert shape("merge_across_a") == [("Copy", 40)]
    assert shape("merge_many_whole_copies") == [("Copy", 300)]
    assert shape("no_merge_over_add") == [("Copy", 50), ("Add", 3), ("Copy", 50)]
    assert shape("no_merge_gap") == [("Copy", 50), ("Copy", 49)]
    assert shape("seventy_adds") == [("Copy", 10), ("Add", 70), ("Copy", 20)]
    assert shape("seventy_literal_copies") == [("Add", 142)]
    assert shape("empty_v2") == [] and len(got["empty_v2"]) == 26
    assert shape("three_times")[:1] == [("Copy", 10)]
    assert dg.info(got["three_times"])["version_size"] == 270


def test_realistic_streams(dg, orc):
    for c in cc.realistic_cases(dg, orc):
        check(dg, orc, c)


def test_associativity_and_identity(dg, orc):
    rng = random.Random(21)
    for k in range(25):
        alpha = b"ab" if k % 2 else bytes(range(256))
        R = bytes(rng.choice(alpha) for _ in range(rng.randint(1, 80)))
        a = cc.random_cmds(rng, len(R), rng.randint(0, 15), alpha, zero=0.1)
        V1 = cc.apply(a, R)
        b = cc.random_cmds(rng, len(V1), rng.randint(0, 15), alpha, zero=0.1)
        V2 = cc.apply(b, V1)
        c = cc.random_cmds(rng, len(V2), rng.randint(0, 15), alpha, zero=0.1)
        V3 = cc.apply(c, V2)
        A, B, Cd = cc.make_delta(dg, orc, a, R), cc.make_delta(dg, orc, b, V1), cc.make_delta(dg, orc, c, V2)
        left = dg.compose(dg.compose(A, B), Cd)
        assert left == dg.compose(A, dg.compose(B, Cd))
        assert orc.decode(R, left) == (0, V3)
        # the identity law: A's own normal form, on either side, and idempotent
        norm = dg.compose(A, cc.identity_delta(dg, orc, V1))
        assert norm == cc.model_compose(dg, A, cc.identity_delta(dg, orc, V1))
        assert dg.compose(cc.identity_delta(dg, orc, R), A) == norm
        assert dg.compose(norm, cc.identity_delta(dg, orc, V1)) == norm
        assert orc.decode(R, norm) == (0, V1)


def test_statuses_in_precedence(dg, orc):
    (R, V1, V2, A, B), bad = cc.damaged(dg, orc)
    assert orc.decode(R, dg.compose(A, B)) == (0, V2)
    for name, a, b, status in bad:
        with pytest.raises(dg.DeltaError) as e:
            dg.compose(a, b)
        assert e.value.code == status, name


def test_ignore_hash(dg, orc):
    (R, V1, V2, A, B), bad = cc.damaged(dg, orc)
    _, a, b, _ = next(x for x in bad if x[0] == "crc_mismatch")
    C = dg.compose(a, b, ignore_hash=True)
    assert C == dg.compose(A, B)
    # ignore_hash skips that check alone
    _, a, b, status = next(x for x in bad if x[0] == "not_sequential_and_crc")
    with pytest.raises(dg.DeltaError) as e:
        dg.compose(a, b, ignore_hash=True)
    assert e.value.code == status


def test_copy_of_a_past_r_passes_through(dg, orc):
    """The composer never sees R: decode rejects C as it would reject A."""
    R = bytes(100)
    A = dg.encode_delta([dg.PlacedCopy(src=90, dst=0, length=20)], inplace=False, version_size=20,
                        src_crc=orc.crc64_xz(R), dst_crc=orc.crc64_xz(bytes(20)))
    C = dg.compose(A, cc.identity_delta(dg, orc, bytes(20)))
    assert C == A
    assert orc.decode(R, A)[0] != 0 and orc.decode(R, C)[0] == orc.decode(R, A)[0]


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_compose(dg, orc, tmp_path):
    import oracle as O
    (R, V1, V2, A, B), bad = cc.damaged(dg, orc)
    pa, pb, pc = tmp_path / "ab.delta", tmp_path / "bc.delta", tmp_path / "ac.delta"
    pa.write_bytes(A)
    pb.write_bytes(B)
    r = run_cli("compose", str(pa), str(pb), str(pc))
    assert r.returncode == 0, r.stderr
    assert pc.read_bytes() == dg.compose(A, B)
    lines = r.stdout.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["Input delta", "Input delta", "Output delta", "Commands", "Copy bytes",
                                                   "Add bytes", "Src CRC", "Dst CRC", "Time"]
    inf = dg.info(pc.read_bytes())
    assert lines[3].split(":")[1].strip() == f"{inf['num_copies']} copies, {inf['num_adds']} adds"
    assert lines[6].split(":")[1].strip() == orc.crc64_xz(R).hex() and lines[7].split(":")[1].strip() == orc.crc64_xz(V2).hex()
    if os.path.exists(O.REF_CLI):   # the reference's own decoder accepts the result
        pr, po = tmp_path / "r.bin", tmp_path / "out.bin"
        pr.write_bytes(R)
        rr = subprocess.run([O.REF_CLI, "decode", str(pr), str(pc), str(po)], capture_output=True, text=True)
        assert rr.returncode == 0, rr.stderr
        assert po.read_bytes() == V2
    by = {x[0]: x for x in bad}
    for name, msg in [("a_magic", "not a delta file"), ("b_empty", "not a delta file"), ("crc_mismatch", "not against"),
                      ("b_inplace_flag", "unsupported"), ("a_not_sequential", "unsupported"),
                      ("b_unknown_command", "")]:
        _, a, b, _ = by[name]
        pa.write_bytes(a)
        pb.write_bytes(b)
        pc.unlink(missing_ok=True)
        r = run_cli("compose", str(pa), str(pb), str(pc))
        assert r.returncode == 1 and msg in r.stderr and r.stderr and not pc.exists(), name
    _, a, b, _ = by["crc_mismatch"]
    pa.write_bytes(a)
    pb.write_bytes(b)
    r = run_cli("compose", str(pa), str(pb), str(pc), "--ignore-hash")
    assert r.returncode == 0 and pc.read_bytes() == dg.compose(A, B)
    assert "compose" in run_cli().stderr
