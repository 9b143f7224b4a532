"""Inputs of tests/test_compose_cpu.py and tests/test_gpu_compose.py, and the
Python model of delta composition.

A case is (name, R, V1, V2, A, B): A = delta(R -> V1), B = delta(V1 -> V2).
Adversarial streams are built from command lists with dg.encode_delta; the
realistic ones are the oracle's onepass and correcting deltas.  Nothing here
needs a GPU.

The model does not walk pieces as the library does: it computes the byte-
provenance map of V2 (for each position a literal, or an offset of R) and
run-length encodes it, which is the definition of the normal form
(include/delta_gpu.h).
"""
from __future__ import annotations

import random

import numpy as np

COUNTS = [0, 1, 63, 64, 65, 128, 129, 300]
SPANS = [1, 15, 16, 17, 63, 64, 65, 5000]


# ── command lists: ("C", src, len) or ("A", bytes), placed sequentially ──

def place(dg, cmds):
    out, dst = [], 0
    for c in cmds:
        if c[0] == "C":
            out.append(dg.PlacedCopy(src=c[1], dst=dst, length=c[2]))
            dst += c[2]
        else:
            out.append(dg.PlacedAdd(dst=dst, data=bytes(c[1])))
            dst += len(c[1])
    return out, dst


def apply(cmds, src: bytes) -> bytes:
    out = bytearray()
    for c in cmds:
        if c[0] == "C":
            assert c[1] + c[2] <= len(src)
            out += src[c[1]:c[1] + c[2]]
        else:
            out += c[1]
    return bytes(out)


def make_delta(dg, orc, cmds, src: bytes, *, src_crc=None, dst_crc=None, inplace=False, version_size=None) -> bytes:
    placed, size = place(dg, cmds)
    ver = apply(cmds, src)
    return dg.encode_delta(placed, inplace=inplace, version_size=size if version_size is None else version_size,
                           src_crc=src_crc or orc.crc64_xz(src), dst_crc=dst_crc or orc.crc64_xz(ver))


def case(dg, orc, name, R, a_cmds, b_cmds):
    V1 = apply(a_cmds, R)
    V2 = apply(b_cmds, V1)
    return (name, R, V1, V2, make_delta(dg, orc, a_cmds, R), make_delta(dg, orc, b_cmds, V1))


# ── the model ──

def model_compose(dg, A: bytes, B: bytes) -> bytes:
    """compose(A, B) in normal form, from the provenance map of V2."""
    ca, ia, vsa, src_crc, _ = dg.decode_delta(A)
    cb, ib, vsb, _, dst_crc = dg.decode_delta(B)
    assert not ia and not ib

    def provenance(cmds, size, prov_in, lit_in):
        prov = np.full(size, -2, dtype=np.int64)   # -1: a literal; >= 0: that offset of R
        lit = np.zeros(size, dtype=np.uint8)
        for c in cmds:
            if isinstance(c, dg.PlacedCopy):
                prov[c.dst:c.dst + c.length] = prov_in(c.src, c.length)
                lit[c.dst:c.dst + c.length] = lit_in(c.src, c.length)
            else:
                prov[c.dst:c.dst + len(c.data)] = -1
                lit[c.dst:c.dst + len(c.data)] = np.frombuffer(bytes(c.data), dtype=np.uint8)
        assert (prov != -2).all(), "not an exact cover"
        return prov, lit

    p1, l1 = provenance(ca, vsa, lambda s, n: np.arange(s, s + n, dtype=np.int64), lambda s, n: 0)
    p2, l2 = provenance(cb, vsb, lambda s, n: p1[s:s + n], lambda s, n: l1[s:s + n])
    out = []
    if vsb:
        cont = np.zeros(vsb, dtype=bool)   # position k continues the run of k - 1
        cont[1:] = ((p2[1:] == -1) & (p2[:-1] == -1)) | ((p2[1:] >= 0) & (p2[:-1] >= 0) & (p2[1:] == p2[:-1] + 1))
        starts = np.flatnonzero(~cont).tolist() + [vsb]
        for s, e in zip(starts[:-1], starts[1:]):
            if p2[s] < 0:
                out.append(dg.PlacedAdd(dst=s, data=l2[s:e].tobytes()))
            else:
                out.append(dg.PlacedCopy(src=int(p2[s]), dst=s, length=e - s))
    return dg.encode_delta(out, inplace=False, version_size=vsb, src_crc=src_crc, dst_crc=dst_crc)


def identity_delta(dg, orc, V: bytes) -> bytes:
    crc = orc.crc64_xz(V)
    cmds = [dg.PlacedCopy(src=0, dst=0, length=len(V))] if V else []
    return dg.encode_delta(cmds, inplace=False, version_size=len(V), src_crc=crc, dst_crc=crc)


# ── builders ──

def random_cmds(rng, src_len, n, alphabet, max_len=6, zero=0.0):
    cmds = []
    for _ in range(n):
        ln = 0 if rng.random() < zero else rng.randint(1, max_len)
        if src_len and rng.random() < 0.6:
            ln = min(ln, src_len)
            cmds.append(("C", rng.randint(0, src_len - ln), ln))
        else:
            cmds.append(("A", bytes(rng.choice(alphabet) for _ in range(ln))))
    return cmds


def random_cases(dg, orc, n=40, seed=11):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        alpha = b"ab" if k % 2 else b"xyz"
        R = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 60)))
        a = random_cmds(rng, len(R), rng.randint(0, 12), alpha, zero=0.1)
        b = random_cmds(rng, len(apply(a, R)), rng.randint(0, 12), alpha, zero=0.1)
        out.append(case(dg, orc, f"random{k}", R, a, b))
    return out


def count_cases(dg, orc, seed=12):
    rng = random.Random(seed)
    R = rng.randbytes(700)
    out = []
    for na in COUNTS:
        a = random_cmds(rng, len(R), na, bytes(range(256)), max_len=5)
        v1 = len(apply(a, R))
        for nb in COUNTS:
            b = random_cmds(rng, v1, nb, bytes(range(256)), max_len=5)
            out.append(case(dg, orc, f"count{na}x{nb}", R, a, b))
    return out


def shaped_cases(dg, orc, seed=13):
    rng = random.Random(seed)
    R = rng.randbytes(400)
    lit = rng.randbytes
    a3 = [("C", 10, 50), ("A", lit(30)), ("C", 200, 40)]   # V1: [0,50) R, [50,80) literal, [80,120) R
    out = [
        case(dg, orc, "inside_copy", R, a3, [("C", 5, 20)]),
        case(dg, orc, "inside_add", R, a3, [("C", 55, 20)]),
        case(dg, orc, "starts_at_boundary", R, a3, [("C", 50, 40)]),
        case(dg, orc, "ends_at_boundary", R, a3, [("C", 20, 30)]),
        case(dg, orc, "exactly_one", R, a3, [("C", 50, 30)]),
        case(dg, orc, "covers_all", R, a3, [("C", 0, 120)]),
        case(dg, orc, "three_times", R, a3, [("C", 40, 50), ("C", 40, 50), ("C", 40, 50), ("C", 0, 120)]),
        case(dg, orc, "empty_v1", R, [], [("A", lit(7)), ("A", lit(3))]),
        case(dg, orc, "empty_v1_v2", R, [], []),
        case(dg, orc, "empty_v2", R, a3, []),
        case(dg, orc, "empty_r", b"", [("A", lit(20))], [("C", 3, 10), ("A", lit(2)), ("C", 0, 20)]),
        case(dg, orc, "zero_lengths", R,
             [("C", 7, 0), ("C", 0, 30), ("A", b""), ("C", 30, 30), ("C", 99, 0), ("A", lit(5)), ("A", b""), ("A", lit(5))],
             [("A", b""), ("C", 10, 40), ("C", 3, 0), ("C", 50, 20), ("A", b""), ("A", lit(4)), ("C", 0, 0), ("A", lit(4))]),
        case(dg, orc, "seventy_adds", R, a3, [("C", 0, 10)] + [("A", lit(1)) for _ in range(70)] + [("C", 100, 20)]),
        case(dg, orc, "seventy_literal_copies", R, [("A", lit(300))],
             [("C", 3 * k, 1) for k in range(70)] + [("A", lit(2))] + [("C", 100 + k, 1) for k in range(70)]),
        case(dg, orc, "merge_across_b", R, [("C", 0, 100)], [("C", 0, 50), ("C", 50, 50)]),
        case(dg, orc, "merge_across_a", R, [("C", 10, 20), ("C", 30, 20)], [("C", 0, 40)]),
        case(dg, orc, "merge_across_both", R, [("C", 10, 20), ("C", 30, 20), ("C", 50, 5)], [("C", 5, 20), ("C", 25, 18)]),
        case(dg, orc, "merge_many_whole_copies", R, [("C", 0, 400)], [("C", 2 * k, 2) for k in range(150)]),
        case(dg, orc, "no_merge_over_add", R, [("C", 0, 100)], [("C", 0, 50), ("A", lit(3)), ("C", 50, 50)]),
        case(dg, orc, "no_merge_gap", R, [("C", 0, 100)], [("C", 0, 50), ("C", 51, 49)]),
        case(dg, orc, "adds_of_a_and_b_merge", R, [("C", 0, 10), ("A", lit(10)), ("C", 10, 10)],
             [("A", lit(3)), ("C", 10, 10), ("A", lit(3)), ("C", 12, 5), ("C", 0, 30)]),
    ]
    # payload spans at odd source and destination offsets, from A's literals and from B's
    big = lit(3 + sum(SPANS) + len(SPANS))
    b, at = [("A", b"\x01")], 3
    for n in SPANS:
        b += [("C", at, n), ("C", 0, 1), ("A", lit(n))]
        at += n + 1
    out.append(case(dg, orc, "payload_spans", R, [("C", 0, 1), ("A", big), ("C", 1, 2)], b))
    # a command header cut by the 1 KiB parse window (which starts at byte 25): the
    # second command starts 4 bytes before the window's end, in both streams
    a = [("A", lit(1011)), ("C", 0, 100)] + random_cmds(rng, len(R), 200, bytes(range(256)), max_len=40)
    v1 = len(apply(a, R))
    b = [("A", lit(1011)), ("C", 500, 1000)] + random_cmds(rng, v1, 260, bytes(range(256)), max_len=40)
    out.append(case(dg, orc, "window_cut", R, a, b))
    return out


def realistic_cases(dg, orc, seed=14):
    import oracle as O
    rng = random.Random(seed)
    out = []
    for k, algo in enumerate([O.ONEPASS, O.CORRECTING, O.ONEPASS]):
        n = [16384, 16384, 3000][k]
        R, V1 = orc.synth_pair(0xC0A0 + k, n, n // 100)
        v2 = bytearray(V1)
        for _ in range(n // 100):
            p = rng.randrange(len(v2))
            if rng.random() < 0.5:
                v2[p] ^= 0x55
            elif rng.random() < 0.5:
                v2[p:p] = rng.randbytes(rng.randint(1, 9))
            else:
                del v2[p:p + rng.randint(1, 9)]
        V2 = bytes(v2)
        out.append((f"realistic{k}", R, V1, V2, orc.encode(algo, R, V1, p=16, q=1), orc.encode(algo, V1, V2, p=16, q=1)))
    return out


_cache = {}


def all_cases(dg, orc):
    """Every OK case, built once per session."""
    if "all" not in _cache:
        _cache["all"] = random_cases(dg, orc) + count_cases(dg, orc) + shaped_cases(dg, orc) + realistic_cases(dg, orc)
    return _cache["all"]


# ── damage: (name, A, B, status), one kind of defect each unless stated ──

def damaged(dg, orc):
    rng = random.Random(15)
    R = rng.randbytes(300)
    a = [("C", 10, 50), ("A", rng.randbytes(30)), ("C", 200, 40)]
    V1 = apply(a, R)
    b = [("C", 5, 60), ("A", rng.randbytes(9)), ("C", 0, 120)]
    A, B = make_delta(dg, orc, a, R), make_delta(dg, orc, b, V1)
    crc1 = orc.crc64_xz(V1)

    def patch(d, at, val):
        return d[:at] + bytes(val) + d[at + len(val):]

    def nonseq(cmds, src):   # the second command's dst off by one
        placed, size = place(dg, cmds)
        placed[1] = dg.PlacedCopy(src=placed[1].src, dst=placed[1].dst + 1, length=placed[1].length) \
            if isinstance(placed[1], dg.PlacedCopy) else dg.PlacedAdd(dst=placed[1].dst + 1, data=placed[1].data)
        return dg.encode_delta(placed, inplace=False, version_size=size, src_crc=orc.crc64_xz(src),
                               dst_crc=orc.crc64_xz(apply(cmds, src)))

    MAL, UNS, CRC = 8, 2, 9
    out = [
        ("a_magic", patch(A, 0, b"X"), B, MAL),
        ("b_magic", A, patch(B, 3, b"\x02"), MAL),
        ("a_short", A[:24], B, MAL),
        ("b_empty", A, b"", MAL),
        ("a_truncated_header", A[:25 + 13 + 4], B, MAL),
        ("b_truncated_payload", A, B[:25 + 13 + 9 + 4], MAL),
        ("a_unknown_command", patch(A, 25, b"\x07"), B, MAL),
        ("b_unknown_command", A, patch(B, 25 + 13, b"\x03"), MAL),
        ("b_copy_past_v1", A, make_delta(dg, orc, [("C", 100, 21)], V1 + b"\0"), MAL),
        ("a_copy_past_4g", make_delta(dg, orc, [("C", 10, 50)], R)[:26] + b"\xff\xff\xff\xf0" +
         make_delta(dg, orc, [("C", 10, 50)], R)[30:], identity_delta(dg, orc, R[10:60]), MAL),
        ("a_inplace_flag", patch(A, 4, b"\x01"), B, UNS),
        ("b_inplace_flag", A, patch(B, 4, b"\x01"), UNS),
        ("a_not_sequential", nonseq(a, R), B, UNS),
        ("b_not_sequential", A, nonseq(b, V1), UNS),
        ("a_sum_short", patch(A, 5, (121).to_bytes(4, "big")), make_delta(dg, orc, b, V1 + b"\0", src_crc=crc1), UNS),
        ("b_sum_long", A, patch(B, 5, (5).to_bytes(4, "big")), UNS),
        ("crc_mismatch", A, patch(B, 9, bytes(8)), CRC),
        # mixed defects: the kind decides, not the position
        ("malformed_and_not_sequential", nonseq(a, R), B[:25 + 13 + 9 + 4], MAL),
        ("not_sequential_then_malformed", nonseq(a, R)[:-1 - 13 + 5], B, MAL),
        ("flag_and_malformed", patch(A, 4, b"\x01"), patch(B, 25 + 13, b"\x09"), MAL),
        ("flag_and_copy_past_v1", patch(A, 4, b"\x01"), make_delta(dg, orc, [("C", 100, 21)], V1 + b"\0"), MAL),
        ("not_sequential_and_crc", nonseq(a, R), patch(B, 9, bytes(8)), UNS),
    ]
    return (R, V1, apply(b, V1), A, B), out
