"""Inputs of tests/test_splice_cpu.py, tests/test_splice_sanitize_cpu.py and
tests/test_gpu_splice.py, and the Python model of the splice.

A case is (name, R, V, whole, segments, deltas): whole = (r_off, r_len, v_off,
v_len) and segments (the same four per segment) are spans of two arenas in which
R and V sit at whole's offsets; deltas[j] is a standard delta of segment j of V
against its window of R.  Segment deltas come from the oracle's onepass and
correcting encoders at a small table size and from hand-made command lists
(compose_cases.make_delta), which cover what encoders never emit: adjacent
mergeable commands inside a stream, zero-length commands, a COPY ending exactly
at its window's end.  Nothing here needs a GPU.

The model does not walk commands as the library does: it computes the byte-
provenance map of V (for each position a literal, or an offset of R) and
run-length encodes it, which is the definition of the normal form
(include/delta_gpu.h).  Its dst_crc is the CRC of V itself, so the library's
combination of the segments' CRCs is checked against the real thing.
"""
from __future__ import annotations

import random

import numpy as np

import compose_cases as cc

OK, UNSUPPORTED, TOO_LARGE, CAPACITY, MALFORMED, INVALID = 0, 2, 3, 7, 8, 1
GROUP_COUNTS = [1, 2, 63, 64, 65, 130]   # the resolve wave's batch edges


# ── the model ──

def model_splice(dg, orc, segments, deltas, whole, src_crc, V) -> bytes:
    """The spliced delta in normal form, from the provenance map of V."""
    ro, rl, vo, vl = whole
    prov = np.full(vl, -2, dtype=np.int64)   # -1: a literal; >= 0: that offset of R
    lit = np.zeros(vl, dtype=np.uint8)
    for (sro, srl, svo, svl), A in zip(segments, deltas):
        cmds, inplace, vs, _, _ = dg.decode_delta(A)
        assert not inplace and vs == svl
        base = svo - vo
        for c in cmds:
            if isinstance(c, dg.PlacedCopy):
                assert c.src + c.length <= srl
                prov[base + c.dst:base + c.dst + c.length] = np.arange(c.src, c.src + c.length, dtype=np.int64) + (sro - ro)
            else:
                prov[base + c.dst:base + c.dst + len(c.data)] = -1
                lit[base + c.dst:base + c.dst + len(c.data)] = np.frombuffer(bytes(c.data), dtype=np.uint8)
    assert (prov != -2).all(), "not an exact cover"
    out = []
    if vl:
        cont = np.zeros(vl, dtype=bool)   # position k continues the run of k - 1
        cont[1:] = ((prov[1:] == -1) & (prov[:-1] == -1)) | ((prov[1:] >= 0) & (prov[:-1] >= 0) & (prov[1:] == prov[:-1] + 1))
        starts = np.flatnonzero(~cont).tolist() + [vl]
        for s, e in zip(starts[:-1], starts[1:]):
            if prov[s] < 0:
                out.append(dg.PlacedAdd(dst=s, data=lit[s:e].tobytes()))
            else:
                out.append(dg.PlacedCopy(src=int(prov[s]), dst=s, length=e - s))
    return dg.encode_delta(out, inplace=False, version_size=vl, src_crc=src_crc, dst_crc=orc.crc64_xz(V))


# ── builders ──

def tile(v_len, sizes):
    """V cut into consecutive pieces of the given sizes (the last takes the rest)."""
    out, at = [], 0
    for s in sizes:
        out.append((at, min(s, v_len - at)))
        at += out[-1][1]
    if at < v_len or not out:
        out.append((at, v_len - at))
    return out


def encoded(orc, algo, R, V, segs):
    return [orc.encode(algo, R[a:a + b], V[c:c + d], p=16, q=1) for a, b, c, d in segs]


def case(dg, orc, name, R, V, segs, deltas=None, algo=None, ro=0, vo=0):
    """segs: (r_off, r_len, v_off, v_len) relative to R and V themselves; the
    case places R and V at ro and vo of their arenas."""
    import oracle as O
    if deltas is None:
        deltas = encoded(orc, O.ONEPASS if algo is None else algo, R, V, segs)
    return (name, R, V, (ro, len(R), vo, len(V)), [(a + ro, b, c + vo, d) for a, b, c, d in segs], deltas)


def fixed(dg, r_len, v_len, S, W):
    return dg.segment_pairs((0, r_len, 0, v_len), S, W)[0]


def hand(dg, orc, R, V, segs, cmd_lists):
    """Segment deltas from command lists; checks that they rebuild the segment."""
    out = []
    for (a, b, c, d), cmds in zip(segs, cmd_lists):
        win = R[a:a + b]
        assert cc.apply(cmds, win) == V[c:c + d], "the command list does not build its segment"
        out.append(cc.make_delta(dg, orc, cmds, win))
    return out


def family_cases(dg, orc, seed=21):
    import oracle as O
    rng = random.Random(seed)
    out = []
    R = rng.randbytes(5000)
    out.append(case(dg, orc, "identical", R, R, fixed(dg, 5000, 5000, 1024, 512)))
    out.append(case(dg, orc, "identical_correcting", R, R, fixed(dg, 5000, 5000, 256, 256), algo=O.CORRECTING, ro=48, vo=16))
    V = rng.randbytes(4100)
    out.append(case(dg, orc, "unrelated", R, V, fixed(dg, 5000, 4100, 1024, 1024)))
    for k, algo in enumerate([O.ONEPASS, O.CORRECTING]):
        r, v = orc.synth_pair(0x5EC0 + k, 32768, 327)
        out.append(case(dg, orc, f"edits{k}", r, v, fixed(dg, len(r), len(v), 4096, 4096), algo=algo))
    S = 512
    v = b"".join(R[j * S:(j + 1) * S] if j % 2 == 0 else rng.randbytes(S) for j in range(9))
    out.append(case(dg, orc, "alternating", R, v, fixed(dg, len(R), len(v), S, 256)))
    S = 1024
    v = R[:S] + R[S + 200:]
    out.append(case(dg, orc, "deleted_at_seam", R, v, fixed(dg, len(R), len(v), S, S)))
    v = R[:S + 1] + R[S + 201:]
    out.append(case(dg, orc, "deleted_off_seam", R, v, fixed(dg, len(R), len(v), S, S)))
    v = R[:3000]
    out.append(case(dg, orc, "windows_differ_copies_merge", R, v, [(0, 1500, 0, 1000), (700, 2300, 1000, 1200), (2000, 3000, 2200, 800)]))
    out.append(case(dg, orc, "empty_v", R, b"", [(0, len(R), 0, 0)]))
    out.append(case(dg, orc, "empty_v_empty_r", b"", b"", [(0, 0, 0, 0)]))
    v = rng.randbytes(700)
    out.append(case(dg, orc, "empty_r", b"", v, [(0, 0, a, b) for a, b in tile(700, [256, 256])], vo=32))
    v = R[:2048]
    out.append(case(dg, orc, "empty_segments", R, v,
                    [(0, 0, 0, 0), (0, 0, 0, 0), (0, 1500, 0, 1024), (0, 5000, 1024, 0), (17, 0, 1024, 0), (512, 2000, 1024, 1024),
                     (5000, 0, 2048, 0)]))
    v = R[:4 * 256 + 1]
    out.append(case(dg, orc, "last_segment_one_byte", R, v, fixed(dg, len(R), len(v), 256, 256)))
    v = R[100:400] + rng.randbytes(30) + R[400:500]
    out.append(case(dg, orc, "shorter_than_seed", R, v, [(0, 5000, a, b) for a, b in tile(len(v), [7] * 20 + [300, 5, 5])]))
    for n in GROUP_COUNTS:
        vl = n * 256 - 100
        r = rng.randbytes(vl + 300)
        v = bytearray(r[:vl])
        for _ in range(max(1, n // 3)):
            x, ln = rng.randrange(vl), rng.randint(1, 40)
            v[x:x + ln] = rng.randbytes(len(v[x:x + ln]))
        v = bytes(v)
        out.append(case(dg, orc, f"group{n}", r, v, fixed(dg, len(r), len(v), 256, 256), algo=O.CORRECTING if n == 65 else None))
    # one run through 130 segments, and one ADD through 70
    r = rng.randbytes(130 * 256)
    out.append(case(dg, orc, "one_copy_130", r, r, fixed(dg, len(r), len(r), 256, 0)))
    v = rng.randbytes(70 * 256)
    out.append(case(dg, orc, "one_add_70", r, v, fixed(dg, len(r), len(v), 256, 256)))
    return out


def shaped_cases(dg, orc, seed=22):
    """Hand-made segment streams."""
    rng = random.Random(seed)
    R = rng.randbytes(600)
    lit = rng.randbytes
    out = []

    def shaped(name, segs, cmd_lists, ro=0, vo=0):
        V = b"".join(cc.apply(cmds, R[a:a + b]) for (a, b, _, _), cmds in zip(segs, cmd_lists))
        at, placed = 0, []
        for (a, b, _, _), cmds in zip(segs, cmd_lists):
            n = len(cc.apply(cmds, R[a:a + b]))
            placed.append((a, b, at, n))
            at += n
        out.append(case(dg, orc, name, R, V, placed, hand(dg, orc, R, V, placed, cmd_lists), ro=ro, vo=vo))

    W = (0, 600, 0, 0)
    shaped("mergeable_inside", [W], [[("C", 0, 50), ("C", 50, 50), ("A", lit(5)), ("A", lit(6)), ("C", 100, 10), ("C", 111, 9)]])
    shaped("zero_lengths", [W, W],
           [[("C", 7, 0), ("C", 0, 30), ("A", b""), ("C", 30, 30), ("C", 599, 0), ("C", 600, 0), ("A", lit(5)), ("A", b""), ("A", lit(5))],
            [("A", b""), ("A", lit(3)), ("C", 3, 0), ("C", 50, 20), ("A", b""), ("C", 0, 0)]])
    shaped("only_zero_lengths", [W, W, W], [[("C", 0, 60)], [("C", 60, 0), ("A", b"")], [("C", 60, 40)]])
    shaped("copy_ends_at_window_end", [(100, 200, 0, 0), (300, 300, 0, 0)], [[("C", 150, 50)], [("C", 0, 300)]], ro=16, vo=64)
    shaped("seam_copy_copy_merge", [(0, 300, 0, 0), (200, 400, 0, 0)], [[("A", lit(4)), ("C", 10, 250)], [("C", 60, 100), ("A", lit(2))]])
    shaped("seam_copy_copy_gap", [(0, 300, 0, 0), (200, 400, 0, 0)], [[("C", 10, 250)], [("C", 61, 100)]])
    shaped("seam_add_add", [W, W], [[("C", 0, 10), ("A", lit(70))], [("A", lit(100)), ("C", 5, 5)]])
    shaped("seam_add_copy", [W, W], [[("A", lit(9))], [("C", 0, 9)]])
    shaped("single_runs_chain", [W] * 6,
           [[("C", 0, 10)], [("C", 10, 10), ("C", 20, 5)], [], [("C", 25, 75)], [("A", lit(3))], [("A", lit(200)), ("A", lit(1))]])
    shaped("merged_first_then_more", [W] * 3,
           [[("A", lit(5)), ("C", 0, 100)], [("C", 100, 50), ("A", lit(80)), ("C", 3, 3)], [("C", 6, 10), ("C", 16, 4), ("A", lit(1))]])
    shaped("long_payloads", [W] * 2, [[("A", lit(65)), ("C", 1, 1), ("A", lit(64)), ("C", 1, 1), ("A", lit(5000))],
                                      [("A", lit(17)), ("C", 0, 600), ("A", lit(1500))]], vo=3, ro=1)
    # a command header cut by the 1 KiB parse window (which starts at byte 25), and more commands than one window holds
    many = [("A", lit(1011)), ("C", 0, 100)] + cc.random_cmds(rng, len(R), 300, bytes(range(256)), max_len=40)
    shaped("window_cut", [W, W], [many, [("C", 0, 1)] + cc.random_cmds(rng, len(R), 200, b"ab", max_len=3, zero=0.2)])
    return out


def random_cases(dg, orc, n=60, seed=23):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        alpha = b"ab" if k % 2 else b"xyz"
        R = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 60)))
        segs, lists, at = [], [], 0
        for _ in range(rng.randint(1, 7)):
            a = rng.randint(0, len(R))
            b = rng.randint(0, len(R) - a)
            cmds = cc.random_cmds(rng, b, rng.choice([0, 0, 1, 2, 5, 9]), alpha, zero=0.15)
            n_v = len(cc.apply(cmds, R[a:a + b]))
            segs.append((a, b, at, n_v))
            lists.append(cmds)
            at += n_v
        V = b"".join(cc.apply(c, R[a:a + b]) for (a, b, _, _), c in zip(segs, lists))
        out.append(case(dg, orc, f"random{k}", R, V, segs, hand(dg, orc, R, V, segs, lists), ro=rng.choice([0, 5]), vo=rng.choice([0, 9])))
    return out


_cache = {}


def all_cases(dg, orc):
    """Every OK case, built once per session and never changed."""
    if "all" not in _cache:
        _cache["all"] = family_cases(dg, orc) + shaped_cases(dg, orc) + random_cases(dg, orc)
    return _cache["all"]


def expected(dg, orc, c):
    """The model's splice of a case, computed once."""
    key = ("model", c[0])
    if key not in _cache:
        name, R, V, whole, segs, deltas = c
        _cache[key] = model_splice(dg, orc, segs, deltas, whole, orc.crc64_xz(R), V)
    return _cache[key]


# ── damage: (name, segments, deltas, seg_status | None, status); one good group, damaged in one segment ──

def damaged(dg, orc):
    rng = random.Random(24)
    R = rng.randbytes(400)
    segs = [(0, 300, 0, 100), (100, 300, 100, 59), (0, 400, 159, 60)]
    lists = [[("C", 10, 50), ("A", rng.randbytes(30)), ("C", 200, 20)], [("C", 5, 50), ("A", rng.randbytes(9))], [("C", 340, 60)]]
    V = b"".join(cc.apply(c, R[a:a + b]) for (a, b, _, _), c in zip(segs, lists))
    good = hand(dg, orc, R, V, segs, lists)
    whole = (0, len(R), 0, len(V))

    def patch(d, at, val):
        return d[:at] + bytes(val) + d[at + len(val):]

    def with_seg(j, d):
        return [d if k == j else x for k, x in enumerate(good)]

    def nonseq(j):
        placed, size = cc.place(dg, lists[j])
        c = placed[1]
        placed[1] = dg.PlacedCopy(src=c.src, dst=c.dst + 1, length=c.length) if isinstance(c, dg.PlacedCopy) \
            else dg.PlacedAdd(dst=c.dst + 1, data=c.data)
        a, b, _, _ = segs[j]
        return dg.encode_delta(placed, inplace=False, version_size=size, src_crc=orc.crc64_xz(R[a:a + b]),
                               dst_crc=orc.crc64_xz(cc.apply(lists[j], R[a:a + b])))

    past = cc.make_delta(dg, orc, [("C", 5, 50), ("A", bytes(9))], R[100:400] + bytes(8))
    past = past[:26] + (251).to_bytes(4, "big") + past[30:]   # COPY(251, 50): one byte past the window of 300
    out = [
        ("incoming_status", segs, good, [0, 11, 0], 11),
        ("incoming_first_wins", segs, with_seg(0, b"junk"), [0, 6, 12], 6),
        ("magic", segs, with_seg(1, patch(good[1], 0, b"X")), None, MALFORMED),
        ("short", segs, with_seg(2, good[2][:24]), None, MALFORMED),
        ("empty_stream", segs, with_seg(0, b""), None, MALFORMED),
        ("truncated_header", segs, with_seg(0, good[0][:25 + 13 + 4]), None, MALFORMED),
        ("truncated_payload", segs, with_seg(1, good[1][:25 + 13 + 9 + 4]), None, MALFORMED),
        ("unknown_command", segs, with_seg(1, patch(good[1], 25, b"\x07")), None, MALFORMED),
        ("copy_past_window", segs, with_seg(1, past), None, MALFORMED),
        ("inplace_flag", segs, with_seg(2, patch(good[2], 4, b"\x01")), None, UNSUPPORTED),
        ("not_sequential", segs, with_seg(0, nonseq(0)), None, UNSUPPORTED),
        ("sum_short", segs, with_seg(1, patch(good[1], 5, (60).to_bytes(4, "big"))), None, UNSUPPORTED),
        ("version_size_is_not_the_segments", segs, with_seg(2, cc.make_delta(dg, orc, [("C", 340, 59)], R)), None, UNSUPPORTED),
        # mixed defects: the kind decides, not the position
        ("unsupported_then_malformed", segs, [nonseq(0), good[1], good[2][:30]], None, MALFORMED),
        ("malformed_and_incoming", segs, with_seg(0, b"junk"), [0, 0, 5], 5),
    ]
    return (R, V, whole, segs, good), out
