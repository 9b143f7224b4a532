"""The Python model of the resemblance sketch, the score and the selection
(include/delta_gpu.h, "reference selection"), in plain int arithmetic, and the
builders of the cases the sketch tests share.

    fp_a    = Horner base 263 mod 2^61 - 1 over X[a .. a + p)
    h_a     = mix(fp_a), the splitmix64 finaliser mod 2^64
    sketch  = per bin h >> (64 - log2 K) the minimum h, EMPTY where none

The model rolls the fingerprint from window to window, which is exact in
Python's integers; check_fingerprints compares it with the oracle's
delta_fingerprint restatement window by window.
"""
from __future__ import annotations

import functools
import random

M61 = (1 << 61) - 1
M64 = (1 << 64) - 1
BASE = 263
EMPTY = M64
NONE = 0xFFFFFFFF
ALL, NOT_SELF, EARLIER = 0, 1, 2

SEEDS = (1, 4, 16, 17, 64)
BINS = (16, 64, 256, 1024)


def fingerprint(data: bytes, a: int, p: int) -> int:
    fp = 0
    for b in data[a:a + p]:
        fp = (fp * BASE + b) % M61
    return fp


def mix(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fingerprints(data: bytes, p: int) -> list:
    """fp_a for a = 0 .. n - p, rolled."""
    n = len(data)
    if n < p:
        return []
    top = pow(BASE, p - 1, M61)
    fp = fingerprint(data, 0, p)
    out = [fp]
    for a in range(n - p):
        fp = ((fp - data[a] * top) * BASE + data[a + p]) % M61
        out.append(fp)
    return out


@functools.lru_cache(maxsize=None)
def hashes(data: bytes, p: int) -> tuple:
    return tuple(mix(f) for f in fingerprints(data, p))


def sketch_of_hashes(hs, k: int) -> list:
    shift = 64 - (k.bit_length() - 1)
    out = [EMPTY] * k
    for h in hs:
        b = h >> shift
        if h < out[b]:
            out[b] = h
    return out


def sketch(data: bytes, p: int = 16, k: int = 256) -> list:
    return sketch_of_hashes(hashes(bytes(data), p), k)


def score(a, b):
    equal = used = 0
    for x, y in zip(a, b):
        if x != y:
            used += 1   # one of them is not EMPTY
        elif x != EMPTY:
            equal += 1
            used += 1
    return equal, used


def select(targets, cands, mode=ALL, target_base=0, min_equal=1) -> list:
    """(best, equal, used) per target; (NONE, 0, 0) when nothing is eligible."""
    out = []
    for t, T in enumerate(targets):
        me = target_base + t
        best = (NONE, 0, 0)
        for c, Cd in enumerate(cands):
            if (mode == NOT_SELF and c == me) or (mode == EARLIER and c >= me):
                continue
            eq, us = score(T, Cd)
            # ascending c: only a strictly higher score replaces the best so far
            if eq >= min_equal and (best[0] == NONE or eq * best[2] > best[1] * us):
                best = (c, eq, us)
        out.append(best)
    return out


def check_fingerprints(orc):
    """The model's rolled fingerprints against the oracle's, window by window."""
    rng = random.Random(0x5EED)
    data = rng.randbytes(140)
    n = 0
    for p in SEEDS:
        fps = fingerprints(data, p)
        assert len(fps) == len(data) - p + 1
        for a, f in enumerate(fps):
            assert f == orc.fingerprint(data, a, p) == fingerprint(data, a, p), (p, a)
        n += len(fps)
    return n


# ── the sketch sweep ──

def sweep_lengths(p: int, c: int) -> list:
    """Around the seed length, around a wave's width, around the chunk size c."""
    return sorted({0, 1, p - 1, p, p + 1, 63, 64, 65, c - 1, c, c + 1, c + p - 2, c + p - 1, 2 * c + 7})


@functools.lru_cache(maxsize=None)
def sweep_buffers(p: int, c: int) -> tuple:
    """(name, bytes): random bytes at every length of the sweep; zeros, one byte
    repeated and a 256-byte period at the lengths that matter to them; a random
    buffer and its copy shifted by three bytes."""
    rng = random.Random(1000 * p + 7)
    out = [("random_%d" % n, rng.randbytes(n)) for n in sweep_lengths(p, c)]
    for n in (p, 65, c + 1):
        out.append(("zeros_%d" % n, bytes(n)))
        out.append(("period1_%d" % n, b"\x5a" * n))
    for n in (65, 300, c + p - 1):
        out.append(("period256_%d" % n, (bytes(range(256)) * (n // 256 + 1))[:n]))
    base = rng.randbytes(c + 40)
    out += [("base", base), ("shifted", rng.randbytes(3) + base)]
    return tuple(out)


def pack(buffers, first=0):
    """The buffers in one arena from offset `first`, nothing between them but the
    0 .. 15 filler bytes that steer the start offsets through every residue
    mod 16 (a read past a span meets filler or the next span's bytes, neither
    of which the model saw).  Returns (arena bytes, [(off, len)])."""
    arena = bytearray(b"\xee" * first)
    spans = []
    for i, b in enumerate(buffers):
        want = (first + 5 * i) % 16   # 5 is odd: sixteen buffers in a row cover every residue
        arena += b"\xee" * ((want - len(arena)) % 16)
        spans.append((len(arena), len(b)))
        arena += b
    return bytes(arena), spans


def seam_buffers(p: int, k: int, c: int, count: int = 4) -> list:
    """Buffers of a little more than one chunk in which some bin's minimum is
    attained only by a window that starts in chunk 0 and reads into chunk 1."""
    out, seed = [], 0
    while len(out) < count:
        seed += 1
        assert seed < 200, "no seam buffer found"
        data = random.Random(0xC0FFEE + seed).randbytes(c + 2 * p)
        hs = hashes(data, p)
        sk = sketch_of_hashes(hs, k)
        straddle = range(c - p + 1, c)   # a < c < a + p
        mins = set(sk)
        if any(hs[a] in mins and hs.count(hs[a]) == 1 for a in straddle):
            out.append(data)
    return out


# ── the match cases ──

def planted_sketches(rng, n: int, k: int, pool) -> list:
    """n sketches of k words: random words, words planted from a shared pool at
    their own bins (so that sketches agree there), and EMPTY bins."""
    out = []
    for _ in range(n):
        s = []
        for b in range(k):
            r = rng.random()
            s.append(EMPTY if r < 0.15 else pool[b] if r < 0.45 else rng.getrandbits(64) & ~1)
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def match_cases() -> tuple:
    """(name, targets, cands, k, mode, target_base, min_equal)."""
    out = []
    rng = random.Random(77)
    sizes = (0, 1, 3, 65, 130)
    for k in (16, 256):
        pool = [rng.getrandbits(64) | 1 for _ in range(k)]
        for i, n_t in enumerate(sizes):
            for j, n_c in enumerate(sizes):
                mode = (ALL, NOT_SELF, EARLIER)[(i + j) % 3]
                base = (0, 2, 60)[(i + 2 * j) % 3]
                min_equal = (1, 5)[(i * 5 + j) % 2]
                out.append(("planted_k%d_%dx%d" % (k, n_t, n_c), planted_sketches(rng, n_t, k, pool),
                            planted_sketches(rng, n_c, k, pool), k, mode, base, min_equal))
        # one set against itself in every mode, with a window of it as the targets
        S = planted_sketches(rng, 70, k, pool)
        for mode in (ALL, NOT_SELF, EARLIER):
            out.append(("self_k%d_mode%d" % (k, mode), S, S, k, mode, 0, 1))
            out.append(("window_k%d_mode%d" % (k, mode), S[40:], S, k, mode, 40, 1))
        # duplicates: candidates 2, 5 and 9 are one sketch, equal to the target
        T = planted_sketches(rng, 1, k, pool)
        C_ = planted_sketches(rng, 12, k, pool)
        C_[2] = C_[5] = C_[9] = list(T[0])
        out.append(("duplicates_k%d" % k, T, C_, k, ALL, 0, 1))
        # rational ties: 2/4 at candidate 3 against 1/2 at candidate 1 and again at 4
        t = [EMPTY] * k
        t[0], t[1] = 11, 22
        half = [11, 33] + [EMPTY] * (k - 2)          # equal 1, used 2
        two4 = [11, 22, 44, 55] + [EMPTY] * (k - 4)  # equal 2, used 4
        none = [99] + [EMPTY] * (k - 1)              # equal 0
        out.append(("tie_k%d" % k, [t], [none, half, none, two4, half], k, ALL, 0, 1))
        out.append(("tie_swapped_k%d" % k, [t], [none, two4, none, half], k, ALL, 0, 1))
        out.append(("tie_min2_k%d" % k, [t], [none, half, none, two4, half], k, ALL, 0, 2))
        # nothing eligible: no equal bin; all empty; every candidate inadmissible
        out.append(("nothing_k%d" % k, [t, [EMPTY] * k], [none, [EMPTY] * k], k, ALL, 0, 1))
        out.append(("first_of_set_k%d" % k, [t], [t, t], k, EARLIER, 0, 1))
        out.append(("min5_k%d" % k, [t], [two4, half], k, ALL, 0, 5))
    return tuple(out)


# ── the end-to-end family ──

@functools.lru_cache(maxsize=None)
def family():
    """8 random bases of 4096 bytes and 16 versions: version j is base j mod 8
    with 2 % of its bytes substituted and one 3-byte insertion."""
    rng = random.Random(2725)
    bases = [rng.randbytes(4096) for _ in range(8)]
    versions = []
    for j in range(16):
        v = bytearray(bases[j % 8])
        for at in rng.sample(range(len(v)), len(v) * 2 // 100):
            v[at] ^= rng.randrange(1, 256)
        at = rng.randrange(len(v))
        v[at:at] = rng.randbytes(3)
        versions.append(bytes(v))
    return bases, versions
