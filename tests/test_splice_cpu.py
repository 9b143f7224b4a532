"""CPU: the host splice (dg_splice, csrc/dg_splice.cpp), the segmentation rule
(dg_segment_pairs) and the plan's geometry checks, against the Python model of
tests/splice_cases.py and the decoders.  No GPU: segment deltas come from the
oracle's encoders and from hand-made command lists.
"""
from __future__ import annotations

import os
import random
import subprocess

import pytest

import compose_cases as cc
import splice_cases as sc

OK, INVALID, UNSUPPORTED, TOO_LARGE, CAPACITY, MALFORMED = 0, 1, 2, 3, 7, 8


def splice_of(dg, orc, c):
    return dg.splice(c[4], c[5], c[3], orc.crc64_xz(c[1]))


def status_of(dg, fn, *a):
    try:
        fn(*a)
        return OK
    except dg.DeltaError as e:
        return e.code


def test_equals_the_model_on_the_corpus(dg, orc):
    cases = sc.all_cases(dg, orc)
    assert len(cases) > 90
    for c in cases:
        assert splice_of(dg, orc, c) == sc.expected(dg, orc, c), c[0]


def test_oracle_decodes_every_result_with_both_crc_checks(dg, orc):
    for c in sc.all_cases(dg, orc):
        assert orc.decode(c[1], splice_of(dg, orc, c)) == (0, c[2]), c[0]


def test_reference_cli_decodes_a_sample(dg, orc, tmp_path):
    import oracle as O
    if not os.path.exists(O.REF_CLI):
        pytest.skip("oracle/_ref/delta is not built")
    pr, pd, po = tmp_path / "r", tmp_path / "d", tmp_path / "o"
    for c in sc.all_cases(dg, orc)[::5]:
        pr.write_bytes(c[1])
        pd.write_bytes(splice_of(dg, orc, c))
        po.unlink(missing_ok=True)
        p = subprocess.run([O.REF_CLI, "decode", str(pr), str(pd), str(po)], capture_output=True, text=True)
        assert p.returncode == 0, (c[0], p.stderr)
        assert po.read_bytes() == c[2], c[0]


def test_consequences_of_the_normal_form(dg, orc):
    by = {c[0]: c for c in sc.all_cases(dg, orc)}
    # R == V in any number of segments whose windows contain them: one COPY, 25 + 13 + 1 bytes
    for name in ("identical", "identical_correcting", "one_copy_130", "windows_differ_copies_merge"):
        d = splice_of(dg, orc, by[name])
        cmds = dg.decode_delta(d)[0]
        assert len(d) == 39 and len(cmds) == 1 and isinstance(cmds[0], dg.PlacedCopy) and cmds[0].src == 0, name
    # a V unrelated to R: one ADD of |V|
    for name in ("unrelated", "one_add_70", "empty_r"):
        c = by[name]
        cmds = dg.decode_delta(splice_of(dg, orc, c))[0]
        assert len(cmds) == 1 and bytes(cmds[0].data) == c[2], name
    # a block deleted exactly at a seam: two adjacent COPYs that must not merge
    for name in ("deleted_at_seam", "seam_copy_copy_gap"):
        cmds = dg.decode_delta(splice_of(dg, orc, by[name]))[0]
        assert [type(x).__name__ for x in cmds] == ["PlacedCopy", "PlacedCopy"], name
        assert cmds[0].src + cmds[0].length != cmds[1].src, name
    # one byte off the seam: the byte after the seam is shorter than a seed, a literal between the two COPYs
    cmds = dg.decode_delta(splice_of(dg, orc, by["deleted_off_seam"]))[0]
    assert [type(x).__name__ for x in cmds] == ["PlacedCopy", "PlacedAdd", "PlacedCopy"] and len(cmds[1].data) == 1
    assert len(splice_of(dg, orc, by["empty_v"])) == 26 and len(splice_of(dg, orc, by["empty_v_empty_r"])) == 26


def test_one_segment_over_all_of_r_is_compose_with_identity(dg, orc):
    import oracle as O
    rng = random.Random(5)
    cases = [(c[1], c[2], d) for c in cc.shaped_cases(dg, orc)[:12] for d in [c[4]]]   # (R, V1, A) with hand-made A
    R, V = orc.synth_pair(77, 20000, 200)
    cases.append((R, V, orc.encode(O.CORRECTING, R, V, p=16, q=1)))
    cases.append((R, V, cc.make_delta(dg, orc, cc.random_cmds(rng, len(R), 300, b"ab", max_len=4, zero=0.2), R)))
    for R, _, A in cases:
        vs = dg.decode_delta(A)[2]
        V = orc.decode(R, A, ignore_hash=True)[1] or b""
        got = dg.splice([(0, len(R), 0, vs)], [A], (0, len(R), 0, vs), orc.crc64_xz(R))
        assert got == dg.compose(A, cc.identity_delta(dg, orc, V))


def test_combined_dst_crc_on_ragged_and_empty_segments(dg, orc):
    rng = random.Random(6)
    R = rng.randbytes(100)
    for sizes in ([0], [1], [0, 0, 0], [1, 0, 1], [0, 7, 0, 0, 300, 1, 0], [5000, 1, 0, 2, 64, 63, 65, 0], [3] * 131):
        V = rng.randbytes(sum(sizes))
        segs = [(0, 100, a, b) for a, b in sc.tile(len(V), sizes)][:len(sizes)]
        deltas = [cc.make_delta(dg, orc, [("A", V[a:a + b])] if b else [], R) for _, _, a, b in segs]
        d = dg.splice(segs, deltas, (0, 100, 0, len(V)), orc.crc64_xz(R))
        assert dg.info(d)["dst_crc"] == orc.crc64_xz(V), sizes
        assert orc.decode(R, d) == (0, V)


def test_segment_pairs_rule_at_the_clipping_edges(dg):
    def rule(r_len, v_len, S, W):
        out = []
        for j in range(max(1, -(-v_len // S))):
            lo = min(j * S, r_len)
            a = lo - min(lo, W)
            b = min(r_len, j * S + S + W)
            out.append((a, max(a, b) - a, min(j * S, v_len), min((j + 1) * S, v_len) - min(j * S, v_len)))
        return out

    for r_len, v_len, S, W in [(0, 0, 16, 0), (0, 100, 16, 16), (100, 0, 16, 16), (1000, 1000, 256, 0), (1000, 1000, 256, 256),
                               (1000, 1001, 256, 4096), (100, 5000, 1024, 512), (5000, 100, 1024, 512), (4096, 4096, 4096, 16),
                               (4097, 4097, 4096, 16), (300, 2000, 256, 128), (1 << 20, (1 << 20) + 1, 1 << 16, 1 << 16)]:
        segs, first = dg.segment_pairs((0, r_len, 0, v_len), S, W)
        assert segs == rule(r_len, v_len, S, W) and first == [0, len(segs)], (r_len, v_len, S, W)
        assert all(a + n <= r_len for a, n, _, _ in segs) and sum(s[3] for s in segs) == v_len
    # offsets carry over, groups follow each other, aligned wholes give aligned segments
    segs, first = dg.segment_pairs([(160, 1000, 32, 600), (4000, 10, 8000, 0), (0, 0, 9000, 700)], 256, 256)
    assert first == [0, 3, 4, 7]
    assert segs[:3] == [(160 + a, n, 32 + c, d) for a, n, c, d in rule(1000, 600, 256, 256)]
    assert segs[3] == (4000, 10, 8000, 0) and segs[4:] == [(0, 0, 9000 + c, d) for _, _, c, d in rule(0, 700, 256, 256)]
    assert all(x % 16 == 0 for s in segs[:3] for x in (s[0], s[2]))
    for args, code in [(((0, 10, 0, 10), 0, 0), INVALID), (((0, 10, 0, 10), 24, 16), INVALID), (((0, 10, 0, 10), 16, 8), INVALID),
                       (((0, (1 << 32) - (1 << 20), 0, 10), 16, 16), TOO_LARGE), (((0, 10, 0, (1 << 32) - (1 << 20)), 1 << 20, 16), TOO_LARGE)]:
        assert status_of(dg, dg.segment_pairs, *args) == code, args
    assert len(dg.segment_pairs((0, 10, 0, (1 << 32) - (1 << 20) - 1), 1 << 20, 1 << 20)[0]) == 4095


def test_geometry_errors(dg, orc):
    R = bytes(100)
    e = cc.make_delta(dg, orc, [], R)
    crc = orc.crc64_xz(R)
    whole = (50, 100, 20, 60)
    d30 = cc.make_delta(dg, orc, [("C", 0, 30)], R)
    good = [(50, 100, 20, 30), (60, 90, 50, 30)]
    assert len(dg.splice(good, [d30, d30], whole, crc)) == 26 + 26
    for segs, code in [
        ([(50, 100, 20, 30), (60, 90, 51, 29)], INVALID),      # a gap in V
        ([(50, 100, 20, 30), (60, 90, 49, 31)], INVALID),      # an overlap in V
        ([(60, 90, 50, 30), (50, 100, 20, 30)], INVALID),      # out of order
        ([(50, 100, 20, 30), (60, 90, 50, 29)], INVALID),      # V not covered
        ([(50, 100, 20, 30), (60, 90, 50, 31)], INVALID),      # past V's end
        ([(49, 100, 20, 30), (60, 90, 50, 30)], INVALID),      # a window before R
        ([(50, 100, 20, 30), (60, 91, 50, 30)], INVALID),      # a window past R's end
        ([(50, 100, 20, 30), (151, 0, 50, 30)], INVALID),      # an empty window outside R
    ]:
        assert status_of(dg, dg.splice, segs, [d30, d30], whole, crc) == code, segs
    assert status_of(dg, dg.splice, [], [], whole, crc) == INVALID
    big = (1 << 32) - (1 << 20)
    assert status_of(dg, dg.splice, [(0, big, 0, 0)], [e], (0, big, 0, 0), crc) == TOO_LARGE
    assert status_of(dg, dg.splice, [(0, 0, 0, big)], [e], (0, 0, 0, big), crc) == TOO_LARGE
    # an empty window at R's very end is inside R
    assert len(dg.splice([(50, 100, 20, 30), (150, 0, 50, 30)], [d30, cc.make_delta(dg, orc, [("A", bytes(30))], b"")], whole, crc)) > 26


def test_every_status_from_a_damaged_segment(dg, orc):
    (R, V, whole, segs, good), bad = sc.damaged(dg, orc)
    crc = orc.crc64_xz(R)
    want = sc.model_splice(dg, orc, segs, good, whole, crc, V)
    assert dg.splice(segs, good, whole, crc) == want
    assert {x[4] for x in bad} >= {MALFORMED, UNSUPPORTED, 11, 6, 5}
    for name, sg, ds, st, code in bad:
        assert status_of(dg, dg.splice, sg, ds, whole, crc, st) == code, name
        assert dg.splice(segs, good, whole, crc, [0, 0, 0]) == want   # the good group between them


def test_sketch_chosen_windows_answer_drift(dg, orc):
    """Drift: V = 3 S random bytes || R, so segment j's content sits 3 S before
    its own offset in R and the fixed rule's windows (W = S / 2) never reach it;
    windows chosen by resemblance find it.  The bounds are the issue's."""
    import oracle as O
    S, W = 4096, 2048
    rng = random.Random(7)
    R = rng.randbytes(13 * S)
    V = rng.randbytes(3 * S) + R
    whole = (0, len(R), 0, len(V))
    crc = orc.crc64_xz(R)
    sizes = {}
    for rule in ("fixed", "sketch_host"):
        segs = dg.segment_pairs(whole, S, W)[0] if rule == "fixed" else dg.sketch_windows(R, V, S, W, host=True)
        assert [(s[2], s[3]) for s in segs] == [(j * S, S) for j in range(16)]
        deltas = sc.encoded(orc, O.ONEPASS, R, V, segs)
        d = dg.splice(segs, deltas, whole, crc)
        assert orc.decode(R, d) == (0, V), rule
        sizes[rule] = len(d)
    print("spliced sizes", sizes, "of", len(V))
    assert sizes["fixed"] > 0.95 * len(V)
    assert sizes["sketch_host"] < 0.5 * len(V)   # the literal floor is 3/16 of V
