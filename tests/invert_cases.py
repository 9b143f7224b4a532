"""Inputs of tests/test_invert_cpu.py and tests/test_gpu_invert.py, and the
Python model of delta inversion.

A case is (name, R, V, A): A = delta(R -> V).  Adversarial streams are built
from command lists with the helpers of tests/compose_cases.py; the realistic
ones are the oracle's onepass and correcting deltas.  Nothing here needs a GPU.

The model does not sort and sweep as the library does: it paints the map "for
each position of R a literal, or an offset of V" COPY by COPY in reverse key
order, so that the first COPY in key order wins, and run-length encodes it,
which is the definition of the normal form (include/delta_gpu.h).
"""
from __future__ import annotations

import random

import numpy as np

import compose_cases as cc

COUNTS = [0, 1, 63, 64, 65, 128, 129, 300]
SPANS = [1, 15, 16, 17, 63, 64, 65, 5000]
ORDERS = ["key", "reversed", "shuffled"]


# ── the model ──

def model_invert(dg, R: bytes, A: bytes) -> bytes:
    """invert(R, A) in normal form, from the provenance map of R."""
    cmds, inplace, _, src_crc, dst_crc = dg.decode_delta(A)
    assert not inplace
    n = len(R)
    copies = [(c.src, -c.length, k, c) for k, c in enumerate(cmds) if isinstance(c, dg.PlacedCopy) and c.length]
    prov = np.full(n, -1, dtype=np.int64)   # -1: a literal; >= 0: that offset of V
    for _, _, _, c in sorted(copies, key=lambda t: t[:3], reverse=True):
        assert c.src + c.length <= n
        prov[c.src:c.src + c.length] = np.arange(c.dst, c.dst + c.length, dtype=np.int64)
    out = []
    if n:
        cont = np.zeros(n, dtype=bool)   # position k continues the run of k - 1
        cont[1:] = ((prov[1:] == -1) & (prov[:-1] == -1)) | ((prov[1:] >= 0) & (prov[:-1] >= 0) & (prov[1:] == prov[:-1] + 1))
        starts = np.flatnonzero(~cont).tolist() + [n]
        for s, e in zip(starts[:-1], starts[1:]):
            if prov[s] < 0:
                out.append(dg.PlacedAdd(dst=s, data=R[s:e]))
            else:
                out.append(dg.PlacedCopy(src=int(prov[s]), dst=s, length=e - s))
    return dg.encode_delta(out, inplace=False, version_size=n, src_crc=dst_crc, dst_crc=src_crc)


def case(dg, orc, name, R, cmds):
    return (name, R, cc.apply(cmds, R), cc.make_delta(dg, orc, cmds, R))


def covers_all(dg, R, A) -> bool:
    """A's COPYs read every byte of R."""
    seen = np.zeros(len(R), dtype=bool)
    for c in dg.decode_delta(A)[0]:
        if isinstance(c, dg.PlacedCopy):
            seen[c.src:c.src + c.length] = True
    return bool(seen.all())


# ── builders ──

def random_cases(dg, orc, n=40, seed=71):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        alpha = b"ab" if k % 2 else b"xyz"
        R = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 60)))
        out.append(case(dg, orc, f"random{k}", R, cc.random_cmds(rng, len(R), rng.randint(0, 12), alpha, zero=0.1)))
    return out


def count_cases(dg, orc, seed=72):
    """n COPYs (the tile edges of the sweep and of a sort pass) in key order,
    reversed and shuffled, an ADD after every seventh."""
    rng = random.Random(seed)
    R = rng.randbytes(2000)
    out = []
    for n in COUNTS:
        copies = sorted(((rng.randrange(0, 1900), rng.randint(1, 40)) for _ in range(n)), key=lambda c: (c[0], -c[1]))
        for order in ORDERS:
            cs = list(copies)
            if order == "reversed":
                cs.reverse()
            elif order == "shuffled":
                rng.shuffle(cs)
            cmds = []
            for k, (s, ln) in enumerate(cs):
                cmds.append(("C", s, ln))
                if k % 7 == 6:
                    cmds.append(("A", rng.randbytes(rng.randint(1, 5))))
            out.append(case(dg, orc, f"count{n}_{order}", R, cmds))
    return out


def shaped_cases(dg, orc, seed=73):
    rng = random.Random(seed)
    R = rng.randbytes(400)
    lit = rng.randbytes
    out = [
        case(dg, orc, "nested", R, [("C", 10, 100), ("A", lit(3)), ("C", 30, 20)]),
        case(dg, orc, "nested_inner_first", R, [("C", 30, 20), ("A", lit(3)), ("C", 10, 100)]),
        case(dg, orc, "overlap_chain", R, [("C", 10 * k, 25) for k in range(12)]),
        case(dg, orc, "overlap_chain_backwards", R, [("C", 10 * k, 25) for k in reversed(range(12))]),
        case(dg, orc, "equal_src", R, [("C", 50, 10), ("C", 50, 30), ("C", 50, 20)]),
        case(dg, orc, "equal_src_and_len", R, [("C", 50, 30), ("A", lit(2)), ("C", 50, 30)]),
        case(dg, orc, "touching_merge", R, [("C", 10, 20), ("C", 30, 20)]),
        case(dg, orc, "touching_no_merge", R, [("C", 30, 20), ("C", 10, 20)]),
        case(dg, orc, "touching_add_between", R, [("C", 10, 20), ("A", lit(1)), ("C", 30, 20)]),
        case(dg, orc, "three_times", R, [("C", 40, 50), ("C", 40, 50), ("C", 40, 50)]),
        case(dg, orc, "gap_at_start", R, [("C", 7, 393)]),
        case(dg, orc, "gap_in_middle", R, [("C", 0, 100), ("C", 131, 269)]),
        case(dg, orc, "gap_at_end", R, [("C", 0, 399)]),
        case(dg, orc, "gaps_everywhere", R, [("C", 300, 50), ("A", lit(9)), ("C", 3, 100), ("C", 120, 100)]),
        case(dg, orc, "fully_covered", R, [("C", 200, 200), ("A", lit(5)), ("C", 0, 200)]),
        case(dg, orc, "identity", R, [("C", 0, 400)]),
        case(dg, orc, "not_covered", R, [("A", lit(33))]),
        case(dg, orc, "empty_r", b"", [("A", lit(20))]),
        case(dg, orc, "empty_v", R, []),
        case(dg, orc, "empty_both", b"", []),
        case(dg, orc, "zero_lengths", R,
             [("C", 7, 0), ("C", 0, 30), ("A", b""), ("C", 30, 30), ("C", 400, 0), ("A", lit(5)), ("A", b""), ("C", 100, 0),
              ("C", 90, 10)]),
    ]
    # src values that differ in one byte only, and lengths likewise: most
    # passes of a radix sort find one digit, one pass does not
    order = list(range(200))
    rng.shuffle(order)
    out.append(case(dg, orc, "src_low_byte", R, [("C", k, 7) for k in order]))
    out.append(case(dg, orc, "len_low_byte", R, [("C", 9, 1 + k) for k in order]))
    big = rng.randbytes(2 * 65536 + 300)
    o40 = list(range(40))
    rng.shuffle(o40)
    out.append(case(dg, orc, "src_second_byte", big, [("C", 256 * k + 5, 300) for k in o40]))
    out.append(case(dg, orc, "len_second_byte", big, [("C", 5, 256 * (k + 1)) for k in o40[:12]]))
    out.append(case(dg, orc, "src_third_byte", big, [("C", 65536 * k + 5, 100) for k in (2, 0, 1)]))
    # literal gaps at odd offsets of R, a 3-byte COPY between them
    cmds, at = [], 0
    for n in SPANS:
        at += n
        cmds.append(("C", at, 3))
        at += 3
    spans_r = rng.randbytes(at + 1)
    out.append(case(dg, orc, "literal_spans", spans_r, cmds))
    out.append(case(dg, orc, "literal_spans_shifted", b"\x07" + spans_r, [("C", s + 1, n) for _, s, n in cmds]))
    # a command header cut by the 1 KiB parse window (which starts at byte 25):
    # the second command starts 4 bytes before the window's end
    out.append(case(dg, orc, "window_cut", R,
                    [("A", lit(1011)), ("C", 0, 100)] + cc.random_cmds(rng, len(R), 200, bytes(range(256)), max_len=40)))
    return out


def realistic_cases(dg, orc):
    import oracle as O
    out = []
    for k, n in enumerate([16384, 3000]):
        R, V = orc.synth_pair(0x1A0 + k, n, n // 100)
        for algo, nm in ((O.ONEPASS, "onepass"), (O.CORRECTING, "correcting")):
            out.append((f"{nm}{n}", R, V, orc.encode(algo, R, V, p=16, q=1)))
    # block transpositions: the correcting encoder's COPYs jump back and forth in R
    R, V = orc.synth_transpose(0x7A5, 16, 1024)
    out.append(("transposed_correcting", R, V, orc.encode(O.CORRECTING, R, V, p=16, q=1)))
    out.append(("transposed_onepass", R, V, orc.encode(O.ONEPASS, R, V, p=16, q=1)))
    return out


_cache = {}


def all_cases(dg, orc):
    """Every OK case, built once per session."""
    if "all" not in _cache:
        _cache["all"] = random_cases(dg, orc) + count_cases(dg, orc) + shaped_cases(dg, orc) + realistic_cases(dg, orc)
    return _cache["all"]


def in_key_order(dg, A) -> bool:
    keys = [(c.src, -c.length) for c in dg.decode_delta(A)[0] if isinstance(c, dg.PlacedCopy) and c.length]
    return keys == sorted(keys)


# ── damage: (name, A, status) against R, one kind of defect each unless stated ──

def damaged(dg, orc):
    rng = random.Random(75)
    R = rng.randbytes(300)
    a = [("C", 10, 50), ("A", rng.randbytes(30)), ("C", 200, 40)]
    V = cc.apply(a, R)
    A = cc.make_delta(dg, orc, a, R)

    def patch(d, at, val):
        return d[:at] + bytes(val) + d[at + len(val):]

    def nonseq(cmds, src):   # the second command's dst off by one
        placed, size = cc.place(dg, cmds)
        placed[1] = dg.PlacedAdd(dst=placed[1].dst + 1, data=placed[1].data)
        return dg.encode_delta(placed, inplace=False, version_size=size, src_crc=orc.crc64_xz(src),
                               dst_crc=orc.crc64_xz(cc.apply(cmds, src)))

    past = cc.make_delta(dg, orc, [("C", 10, 50), ("C", 280, 21)], R + b"\0")   # reads one byte past R
    MAL, UNS = 8, 2
    out = [
        ("magic", patch(A, 0, b"X"), MAL),
        ("version", patch(A, 3, b"\x02"), MAL),
        ("short", A[:24], MAL),
        ("empty", b"", MAL),
        ("truncated_header", A[:25 + 13 + 4], MAL),
        ("truncated_payload", A[:25 + 13 + 9 + 4], MAL),
        ("unknown_command", patch(A, 25, b"\x07"), MAL),
        ("unknown_command_later", patch(A, 25 + 13 + 9 + 30, b"\x03"), MAL),
        ("copy_past_ref", past, MAL),
        ("copy_past_4g", patch(A, 26, b"\xff\xff\xff\xf0"), MAL),
        ("inplace_flag", patch(A, 4, b"\x01"), UNS),
        ("not_sequential", nonseq(a, R), UNS),
        ("sum_short", patch(A, 5, (121).to_bytes(4, "big")), UNS),
        ("sum_long", patch(A, 5, (5).to_bytes(4, "big")), UNS),
        # mixed defects: the kind decides, not the position
        ("not_sequential_then_malformed", nonseq(a, R)[:-1 - 13 + 5], MAL),
        ("flag_and_malformed", patch(patch(A, 4, b"\x01"), 25 + 13, b"\x09"), MAL),
        ("flag_and_copy_past_ref", patch(past, 4, b"\x01"), MAL),
        ("sum_short_and_copy_past_ref", patch(past, 5, (99).to_bytes(4, "big")), MAL),
        ("flag_and_not_sequential", patch(nonseq(a, R), 4, b"\x01"), UNS),
    ]
    return (R, V, A), out
