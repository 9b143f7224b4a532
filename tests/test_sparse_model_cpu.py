"""CPU: the sparse model (tests/sparse_model.py) gives the dense models' bytes
and statuses on every case of the existing corpora, and its CRC-64/XZ combine
equals the oracle's CRC of the concatenation.

This is what entitles the sparse model to be the reference where the dense
models cannot go: offsets and sizes above 2^31 (tests/high_offset_cases.py).
"""
from __future__ import annotations

import random

import pytest

import compose_cases as cc
import invert_cases as ivc
import read_cases as rc
import sparse_model as sm
import splice_cases as sc
import update_cases as uc

LENGTHS = [0, 1, 7, 8, 9, 65537]


def test_sparse_bytes():
    s = sm.SparseBytes(1 << 33, {5: b"abc", (1 << 32) + 7: b"xyz"})
    assert s[0:10] == b"\0" * 5 + b"abc" + b"\0\0" and s[6:7] == b"b" and s[8:8] == b""
    assert s[(1 << 32) + 6:(1 << 32) + 12] == b"\0xyz\0\0" and len(s) == 1 << 33
    assert s[(1 << 33) - 2:(1 << 33) + 9] == b"\0\0"
    assert s.head(7)[0:7] == b"\0" * 5 + b"ab" and len(s.head(7)) == 7
    with pytest.raises(AssertionError):
        s[0:(1 << 20) + 1]
    with pytest.raises(AssertionError):
        sm.SparseBytes(10, {0: b"abcd", 3: b"x"})


def test_crc_combine_equals_the_oracle(orc):
    rng = random.Random(5)
    bufs = [rng.randbytes(n) for n in LENGTHS]
    crc = {b: int.from_bytes(orc.crc64_xz(b), "big") for b in bufs}
    for x in bufs:
        assert sm.crc64(x) == crc[x]
        for y in bufs:
            assert sm.crc64_combine(crc[x], crc[y], len(y)) == int.from_bytes(orc.crc64_xz(x + y), "big"), (len(x), len(y))
        for k in (0, 1, 2, 3, 7, 64, 65):
            if k * len(x) <= 1 << 20:
                assert sm.crc64_repeat(crc[x], len(x), k) == int.from_bytes(orc.crc64_xz(x * k), "big"), (len(x), k)
    s = sm.SparseBytes(70000, {1: bufs[3], 60001: bufs[4], 69999: b"\x07"})
    assert sm.crc64_sparse(s) == int.from_bytes(orc.crc64_xz(s[0:70000]), "big")


def test_compose_equals_the_dense_model(dg, orc):
    for name, _, _, _, A, B in cc.all_cases(dg, orc):
        assert sm.compose(A, B) == (sm.OK, cc.model_compose(dg, A, B)), name
    _, bad = cc.damaged(dg, orc)
    for name, a, b, status in bad:
        assert sm.compose(a, b) == (status, b""), name
    by = {x[0]: x for x in bad}
    assert sm.compose(by["crc_mismatch"][1], by["crc_mismatch"][2], ignore_hash=True)[0] == sm.OK
    assert sm.compose(by["not_sequential_and_crc"][1], by["not_sequential_and_crc"][2], ignore_hash=True)[0] == sm.UNSUPPORTED


def test_invert_equals_the_dense_model(dg, orc):
    for name, R, _, A in ivc.all_cases(dg, orc):
        assert sm.invert(R, A) == (sm.OK, ivc.model_invert(dg, R, A)), name
    (R, _, _), bad = ivc.damaged(dg, orc)
    for name, a, status in bad:
        assert sm.invert(R, a) == (status, b""), name


def test_splice_equals_the_dense_model(dg, orc):
    for c in sc.all_cases(dg, orc):
        name, R, V, whole, segs, deltas = c
        assert sm.splice(whole, segs, deltas, orc.crc64_xz(R)) == (sm.OK, sc.expected(dg, orc, c)), name
    (R, V, whole, _, _), bad = sc.damaged(dg, orc)
    for name, segs, deltas, seg_status, status in bad:
        assert sm.splice(whole, segs, deltas, orc.crc64_xz(R), seg_status) == (status, b""), name
    # geometry: what test_splice_cpu.py pins of dg_splice
    assert sm.splice_geometry((0, 100, 0, 50), [(0, 100, 0, 20), (0, 100, 21, 29)]) == sm.INVALID_ARG
    assert sm.splice_geometry((0, 100, 0, 50), [(0, 100, 0, 20)]) == sm.INVALID_ARG
    assert sm.splice_geometry((0, 100, 0, 50), [(1, 100, 0, 50)]) == sm.INVALID_ARG
    assert sm.splice_geometry((0, 100, 0, 50), []) == sm.INVALID_ARG
    assert sm.splice_geometry((0, sm.PLAN_LIMIT, 0, 0), [(0, 0, 0, 0)]) == sm.TOO_LARGE
    assert sm.splice_geometry((0, sm.PLAN_LIMIT - 1, 0, sm.PLAN_LIMIT - 1), [(0, 0, 0, sm.PLAN_LIMIT - 1)]) == sm.OK


def test_read_equals_the_dense_model(dg, orc):
    n = 0
    for name, R, d, st, V, rs in rc.with_ranges(dg, orc):
        if st != rc.UNSUPPORTED:   # (a read plan's stream status is decode's for a standard stream)
            assert sm.decode_status(len(R), d) == st, name
        for off, ln in rs:
            assert sm.read(R, d, off, ln) == (st, b"" if st else rc.model_read(V, off, ln)), (name, off, ln)
            n += 1
    assert n > 10000


def test_lineage_read_equals_the_dense_model(dg, orc):
    """Every forest of lineage_cases whose statuses the host can express (a
    stated ref_len that is not the parent's size exists on the device only; those
    forests are pinned to lineage_cases.node_status instead), every node, every
    range: lc.model_lineage_read's status and bytes.  The dense model rebuilds
    every level per call, so it is called once per node (and for every range of a
    failing one); the other ranges are slices of the version it built, which
    lineage_cases.resolve keeps."""
    import lineage_cases as lc
    n = stated = 0
    for f, per in lc.corpus(dg, orc):
        nodes = f["nodes"]
        for i, (st, V, rs) in enumerate(per):
            R, ds = lc.path(nodes, i)
            refs = None
            if f.get("host", True):
                for off, ln in rs if st else rs[:1]:
                    assert sm.lineage_read(R, ds, off, ln) == lc.model_lineage_read(R, ds, off, ln), (f["name"], i, off, ln)
            else:
                chain = [i]
                while nodes[chain[-1]][2] != lc.BASE:
                    chain.append(nodes[chain[-1]][2])
                refs = [nodes[k][3] for k in chain[::-1]]
                stated += st == sm.INVALID_ARG
            for off, ln in rs:
                want = (st, b"") if st else (sm.OK, rc.model_read(V, off, ln))
                assert sm.lineage_read(R, ds, off, ln, stated=refs) == want, (f["name"], i, off, ln)
                n += 1
            assert st or sm.lineage_pieces(R, ds, 0, len(V), stated=refs) >= (len(V) > 0)
    assert n > 3000 and stated >= 4
    # a piece count by hand: 3 bytes of payload, then 2 pieces of R through a level that cuts the range once
    R = bytes(range(200))
    import high_offset_cases as hc
    d1 = hc.sstream([("C", 100, 50), ("C", 0, 50)])
    d2 = hc.sstream([("A", b"abc"), ("C", 40, 30)])
    assert sm.lineage_read(R, [d1, d2], 0, 99) == (sm.OK, b"abc" + R[140:150] + R[0:20])
    assert sm.lineage_pieces(R, [d1, d2], 0, 99) == 3 and sm.lineage_pieces(R, [d1, d2], 3, 10) == 1


def test_replay_equals_the_oracle_on_inplace_streams(dg, orc):
    """update_cases' families, in-place: memmove order, overwrites, zeros in an
    uncovered grown tail.  Read whole and as three windows."""
    cases = []
    for k, kind in enumerate(uc.ORDER_KINDS):
        rng = random.Random(3000 + k)
        cases.append((kind, ) + uc.order_case(dg, rng, kind))
        cases.append((kind + "_small", ) + uc.order_case(dg, rng, kind, n_r=3000, n_cmds=rng.randint(2, 110)))
    for k, kind in enumerate(uc.MOVE_KINDS):
        rng = random.Random(4000 + k)
        cases.append((kind, ) + uc.moves_case(dg, rng, kind, 9000))
    for name, R, cmds, vs in cases:
        d, V = uc.make_delta(dg, orc, R, cmds, vs)
        bsz = max(len(R), vs)
        assert sm.update_status(len(R), d, bsz) == sm.OK and sm.decode_status(len(R), d, bsz) == sm.OK, name
        assert sm.update_status(len(R), d, bsz - 1) == sm.CAPACITY, name
        assert sm.replay(R, d, (0, vs)) == V, name
        cuts = [0, vs // 3, vs // 3 + 1, vs]
        assert b"".join(sm.replay(R, d, (a, b)) for a, b in zip(cuts[:-1], cuts[1:])) == V, name
    # the damages of a three-window stream, except the one the model has no means for (a CRC over R)
    R, d, V = uc.three_window_stream(dg, orc, random.Random(77))
    assert sm.replay(R, d, (0, len(V))) == V
    for how in uc.DAMAGES:
        if how == "src_crc":
            continue
        bad, cap, status = uc.damage(d, R, how)
        assert sm.update_status(len(R), bad, max(len(R), uc.version_size(bad)) if cap is None else cap) == status, how
        if how in uc.DECODE_AGREES:
            assert sm.decode_status(len(R), bad) == status, how
