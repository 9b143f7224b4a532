"""Greedy (src/c/greedy.c:88-267): a hash-free model and the shared test inputs.

Greedy's output does not depend on its hash table: at every position v_c the
candidates are exactly the offsets of R whose p-byte seed equals V's, the
longest match wins, and ties go to the largest offset (hash table) or, with
--splay, the smallest.  ``greedy_model`` computes that with a dictionary keyed
on the seed bytes (so mid-size inputs stay quick); tests/test_greedy_model_cpu.py
pins it against a plain brute force and against the reference's own deltas
(tests/golden/golden_greedy.json).

Commands are tuples: ("C", offset_in_R, length) and ("A", bytes).
"""
from __future__ import annotations

import random
import struct

from cases import small_cases


def _prefix(R: bytes, a: int, V: bytes, v: int) -> int:
    """Common-prefix length of R[a:] and V[v:]."""
    n = min(len(R) - a, len(V) - v)
    lo, step = 0, 64
    while lo < n:
        s = min(step, n - lo)
        if R[a + lo:a + lo + s] == V[v + lo:v + lo + s]:
            lo += s
            step = min(2 * step, 1 << 16)
            continue
        l, h = 0, s   # the first l bytes of the piece are equal, the first h are not
        while h - l > 1:
            m = (l + h) // 2
            if R[a + lo:a + lo + m] == V[v + lo:v + lo + m]:
                l = m
            else:
                h = m
        return lo + l
    return n


def greedy_model(R: bytes, V: bytes, p: int, splay: bool = False) -> list:
    index = {}
    for a in range(len(R) - p + 1):
        index.setdefault(R[a:a + p], []).append(a)   # ascending
    cmds, vc, vs = [], 0, 0
    while vc + p <= len(V):
        cand = index.get(V[vc:vc + p])
        if not cand:
            vc += 1
            continue
        best_len, best_a = 0, 0
        for a in (cand if splay else reversed(cand)):   # the first of the longest wins
            ml = _prefix(R, a, V, vc)
            if ml > best_len:
                best_len, best_a = ml, a
        if vs < vc:
            cmds.append(("A", V[vs:vc]))
        cmds.append(("C", best_a, best_len))
        vs = vc = vc + best_len
    if vs < len(V):
        cmds.append(("A", V[vs:]))
    return cmds


def serialize(cmds: list, v_len: int, src_crc: bytes, dst_crc: bytes) -> bytes:
    """The standard DLT\\x03 delta of a command list (src/c/encoding.c:39-90)."""
    out = [b"DLT\x03\x00", struct.pack(">I", v_len), src_crc, dst_crc]
    dst = 0
    for c in cmds:
        if c[0] == "C":
            out.append(b"\x01" + struct.pack(">III", c[1], dst, c[2]))
            dst += c[2]
        else:
            out.append(b"\x02" + struct.pack(">II", dst, len(c[1])) + c[1])
            dst += len(c[1])
    out.append(b"\x00")
    return b"".join(out)


def parse(delta: bytes) -> list:
    """The command list of a standard delta, in stream order."""
    assert delta[:4] == b"DLT\x03" and delta[4] == 0
    cmds, i = [], 25
    while True:
        t = delta[i]
        if t == 0:
            assert i + 1 == len(delta)
            return cmds
        if t == 1:
            src, _, n = struct.unpack(">III", delta[i + 1:i + 13])
            cmds.append(("C", src, n))
            i += 13
        else:
            assert t == 2
            _, n = struct.unpack(">II", delta[i + 1:i + 9])
            cmds.append(("A", delta[i + 9:i + 9 + n]))
            i += 9 + n


def model_delta(orc, R: bytes, V: bytes, p: int, splay: bool = False) -> bytes:
    return serialize(greedy_model(R, V, p, splay), len(V), orc.crc64_xz(R), orc.crc64_xz(V))


def apply(R: bytes, cmds: list) -> bytes:
    return b"".join(R[c[1]:c[1] + c[2]] if c[0] == "C" else c[1] for c in cmds)


# ── inputs ───────────────────────────────────────────────────────────────────

def random_pairs(seed: int, n: int) -> list:
    """Small pairs over small alphabets (many equal seeds, many ties): lengths
    0-199, alphabets of 2, 3, 4 and 16 symbols, half with a slice of R spliced
    into V."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        alpha = rng.choice([2, 3, 4, 16])
        R = bytes(rng.randrange(alpha) for _ in range(rng.randrange(200)))
        V = bytearray(rng.randrange(alpha) for _ in range(rng.randrange(200)))
        if rng.random() < 0.5 and R:
            a = rng.randrange(len(R))
            at = rng.randrange(len(V) + 1)
            V[at:at] = R[a:a + rng.randrange(1, 120)]
            del V[199:]
        out.append((R, bytes(V)))
    return out


MATCH_LENGTHS = (15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 70000)
GAP_LENGTHS = (0, 1, 4, 5, 32, 33, 63, 64, 65, 127, 128, 129, 4097)


def edge_cases() -> list:
    """(name, R, V, p)."""
    rng = random.Random(0x6ED6E)
    rb = rng.randbytes
    R40, R50, R16 = rb(40), rb(50), rb(16)
    return [
        ("v_empty", R40, b"", 16),
        ("r_empty", b"", rb(40), 16),
        ("both_empty", b"", b"", 16),
        ("r_short", R40[:15], R40[:15] + rb(20), 16),
        ("v_short", R40, R40[:15], 16),
        ("eq_p", R16, R16, 16),
        ("diff_last", R16, R16[:15] + bytes([R16[15] ^ 1]), 16),
        ("last_seed", R50, rb(7) + R50[34:] + rb(5), 16),          # R's last seed, ended by R
        ("tail_pm1", R50, rb(30) + R50[10:25], 16),                # 15 equal bytes at V's end: no seed
        ("v_lt4", R40, R40[5:8], 2),                               # |V| < 4: one COPY
        ("v_lt4_gap", b"abcd", b"xab", 2),                           # |V| < 4: a 1-byte gap, then a COPY
    ]


def tie_cases() -> list:
    rng = random.Random(0x71E)
    X = rng.randbytes(300)
    Y = rng.randbytes(500)
    junk = rng.randbytes(50)
    return [
        ("tie_xx", X + X, X, 16),                                  # default: COPY from 300; --splay: from 0
        ("longest_late", Y[:40] + junk + Y, Y, 16),                # the longest wins, wherever it lies
        ("longest_early", Y + junk + Y[:40], Y, 16),
    ]


def match_length_cases() -> list:
    rng = random.Random(0x3A7C4)
    rb = rng.randbytes
    out = []
    for L in MATCH_LENGTHS:
        M = rb(L)
        x = rng.randrange(256)
        out.append((f"len{L}_byte", rb(20) + M + bytes([x]) + rb(20), rb(10) + M + bytes([x ^ 0x55]) + rb(10), 16))
        out.append((f"len{L}_end_r", rb(20) + M, rb(10) + M + rb(10), 16))
        out.append((f"len{L}_end_v", rb(20) + M + rb(20), rb(10) + M, 16))
    return out


def gap_cases() -> list:
    """A gap of g bytes before each of two matches (g = 0: two COPYs back to
    back, and no leading ADD)."""
    rng = random.Random(0x6A9)
    rb = rng.randbytes
    out = []
    for g in GAP_LENGTHS:
        A, B = rb(40), rb(40)
        out.append((f"gap{g}", B + rb(30) + A, rb(g) + A + rb(g) + B, 16))
    return out


def record_cases() -> list:
    """More than 64 and more than 128 COPY records: 130 blocks of 48 bytes of R
    in permuted order, each followed by one junk byte."""
    rng = random.Random(0x4EC)
    R = rng.randbytes(130 * 48)
    order = list(range(130))
    rng.shuffle(order)
    V = b"".join(R[48 * i:48 * i + 48] + rng.randbytes(1) for i in order)
    return [("blocks130", R, V, 16)]


def bucket_cases() -> list:
    """Buckets of more than 64 and more than 128 equal seeds."""
    rng = random.Random(0xB0C)
    motif = rng.randbytes(20)
    R = b"".join(motif + struct.pack(">I", 0x01000000 + 7919 * i) for i in range(200))
    V = motif + struct.pack(">I", 0x01000000 + 7919 * 137) + rng.randbytes(50)
    P3 = bytes([0, 1, 2]) * 1365
    Z = bytes(4096)
    return [
        ("motif200", R, V, 16),                                    # one best among 200 equal seeds
        ("period3", P3, P3[1:] + b"\x07" + P3[:100], 4),
        ("zeros_p16", Z, Z, 16),
        ("zeros_p1", Z, Z, 1),
    ]


def named_cases() -> list:
    return (edge_cases() + tie_cases() + match_length_cases() + gap_cases() + record_cases() + bucket_cases())


def midsize_specs() -> list:
    """Generator specs of the mid-size pairs (p = 16), built by ``spec_inputs``."""
    out = [dict(name=f"c2_{i}", kind="synth_edits", seed=0xC2000000 + i, pair_len=65536, n_edits=655)
           for i in range(4)]
    out += [dict(name=f"c4_{i}", kind="synth_transpose", seed=0xC4000000 + i, num_blocks=8 + i,
                 mean=262144 // (8 + i), pct=50) for i in range(2)]
    out.append(dict(name="shift_64k", kind="synth_shift", seed=0xC3510000, pair_len=65536, n_edits=300,
                    indel_pct=50))
    return out


_NAMED = None


def spec_inputs(orc, c: dict):
    """(R, V) of a golden entry or a mid-size spec, from its generator fields."""
    global _NAMED
    k = c["kind"]
    if k == "synth_edits":
        return orc.synth_pair(c["seed"], c["pair_len"], c["n_edits"])
    if k == "synth_transpose":
        return orc.synth_transpose(c["seed"], c["num_blocks"], c["mean"], c["pct"])
    if k == "synth_shift":
        return orc.synth_shift(c["seed"], c["pair_len"], c["n_edits"], c["indel_pct"])
    if k == "greedy_random":
        return random_pairs(c["seed"], c["index"] + 1)[c["index"]]
    if _NAMED is None:
        _NAMED = {("small", n): (R, V) for n, R, V, _, _ in small_cases()}
        _NAMED.update({("greedy_named", n): (R, V) for n, R, V, _ in named_cases()})
    return _NAMED[(k, c["name"])]
