"""Inputs of the encode plan's contract tests (tests/test_gpu_encode_plan.py).

Pure Python, no GPU.  tests/test_encode_plan_cases_cpu.py proves from the
oracle's own deltas that every pair below has the shape its name claims, so a
generator that stops producing a shape fails there, on the CPU.

* ``small_layout_cases()``  named pairs (name, R, V), each buffer at most
  64 KiB, the two arenas together well under the 8 x 160 KiB layout;
* ``layout(pairs, align)``  the pairs packed into two arenas that end at the
  last pair's last byte, at 16-byte aligned or at odd offsets;
* ``rerun_lengths()`` / ``auto_lengths()`` / ``datasets(lengths, seed)``
  several contents of one fixed layout.

The matches are built so that the one-pass scan finds them whatever the table
size: a match on the current diagonal (V = R with bytes substituted, or V = a
prefix + R) hashes R's and V's seed into the same slot one step after the
substituted byte, and the tables are empty after every match.
"""
from __future__ import annotations

import random
from collections import namedtuple

from test_gpu_serialize_tiles import _cases as _tile_cases
from test_gpu_serialize_tiles import _pair as _tile_pair

P = 16                 # the seed length every test here uses
CHUNK = 2048           # positions per member chunk (dg_layout.h kMemChunk)
MAX_LEN = 64 << 10     # per buffer
MAX_ARENA = 8 * (160 << 10)

CHUNK_EDGE_LENGTHS = [2032, 2047, 2048, 2049, 2064, 4095, 4096, 4097, 2040, 3001, 6151]
COPY_COUNTS = [1, 63, 64, 65, 128, 129]
DENSE_K = [17, 20, 24, 31, 32, 33]


def _other(rng, b):
    """A byte that differs from b."""
    return (b + rng.randrange(1, 256)) & 0xFF


def substituted(rng, R, positions):
    V = bytearray(R)
    for x in positions:
        V[x] = _other(rng, V[x])
    return bytes(V)


def replaced(rng, R, spans):
    """R with every [a, b) of spans replaced by bytes that differ at a and b - 1."""
    V = bytearray(R)
    for a, b in spans:
        V[a:b] = rng.randbytes(b - a)
        V[a] = _other(rng, R[a])
        V[b - 1] = _other(rng, R[b - 1])
    return bytes(V)


def copies_pair(rng, n, shift=0, step=40):
    """A delta of exactly n COPYs: V = R with n - 1 substituted bytes, `step`
    apart; shift > 0 puts `shift` bytes in front of V, so that the matches leave
    diagonal 0 (the member chain then keeps none of them: the plain records)."""
    R = rng.randbytes(step * n)
    V = substituted(rng, R, [step * k - 1 for k in range(1, n)])
    return R, rng.randbytes(shift) + V


def gap_pair(rng, gaps, piece=64, shift=0):
    """V = R with a replaced stretch of each length in gaps, `piece` kept bytes
    before each; the kept tail leaves the last gap before a COPY."""
    R = rng.randbytes(sum(gaps) + piece * (len(gaps) + 1))
    spans, at = [], 0
    for g in gaps:
        at += piece
        spans.append((at, at + g))
        at += g
    return R, rng.randbytes(shift) + replaced(rng, R, spans)


def tail_add_pair(rng, n, tail):
    """A trailing ADD of `tail` bytes after n kept bytes."""
    R = rng.randbytes(n + tail)
    return R, R[:n] + bytes(_other(rng, b) for b in R[n:])


def window_pair(rng, n, gap, last):
    """A gap of `gap` >= 5 bytes, then a COPY of `last` < 32 bytes that ends V:
    the 32 bytes from the gap's start cross |V|."""
    R = rng.randbytes(n + gap + last)
    return R, replaced(rng, R, [(n, n + gap)])


def dense_pair(rng, k, n=3 * CHUNK + 100):
    """One substituted byte every k bytes: COPYs of k - 1 bytes on diagonal 0."""
    R = rng.randbytes(n)
    return R, substituted(rng, R, range(k - 1, n, k))


def alternating_pair(rng, keep, drop, n=3 * CHUNK + 100):
    """`keep` kept bytes, `drop` replaced ones, and so on."""
    R = rng.randbytes(n)
    spans = [(a + keep, min(a + keep + drop, n)) for a in range(0, n - keep - 2, keep + drop)]
    return R, replaced(rng, R, spans)


def command_dense_pair(rng, n=1000):
    """V = 16-byte pieces of R at scattered (increasing) offsets, one literal
    byte between them: 23 delta bytes per 17 of V, next to the plan's bound."""
    R = bytearray(rng.randbytes(MAX_LEN))
    V, at = bytearray(), rng.randrange(1, 9)
    for _ in range(n):
        V += R[at:at + 16]
        nxt = at + 16 + rng.randrange(1, 9)
        # the literal: no match grows into it, forwards or backwards
        V.append(rng.choice([b for b in range(256) if b not in (R[at + 16], R[nxt - 1])]))
        at = nxt
    return bytes(R[:at + 64]), bytes(V)


_SMALL = None


def small_layout_cases():
    """(name, R, V); the same list on every call."""
    global _SMALL
    if _SMALL is not None:
        return _SMALL
    rng = random.Random(0xE7C0DE)
    rb = rng.randbytes
    out = []
    # stream edges
    X = rb(300)
    out += [("v_empty", rb(100), b""), ("r_empty", b"", rb(100)), ("both_empty", b"", b""),
            ("v_lt5", X, X[:3]), ("v_lt_p", X, X[:11]), ("v_eq_p", X, X[:16]),
            ("r_longer", X, X[:120] + rb(9) + X[150:260]), ("v_longer", X[:200], X[:90] + rb(33) + X[90:] + rb(7))]
    # chunk edges: min(|R|, |V|) on and around the chunk and the 16-byte piece boundaries
    for i, n in enumerate(CHUNK_EDGE_LENGTHS):
        R = rb(n)
        V = substituted(rng, R, range(97 + i, n - 20, 331))   # kept up to the last byte
        if i % 3 == 1:
            R += rb(5 + i)            # |R| > |V|
        elif i % 3 == 2:
            V += rb(3 + 2 * i)        # |V| > |R|
        out.append((f"edge_{n}", R, V))
    # record counts: exact ones on diagonal 0 and off it, and the tile pairs
    for n in COPY_COUNTS:
        out.append((f"copies_{n}", *copies_pair(rng, n)))
    for n in (63, 64, 65, 129):
        out.append((f"copies_{n}_shift", *copies_pair(rng, n, shift=7)))
    tiles = {name: (R, V) for name, R, V in _tile_cases(1)}
    for name in ("records_64_mixed", "records_129", "direct_tiles", "no_records"):
        out.append((name, *tiles[name]))
    # (the tile test's own all_direct has a V of 395 KB: the same generator, 21 pieces)
    out.append(("all_direct", *_tile_pair(rng, 21, [3000])))
    # 64 records of 13 + 9 + 80 bytes: one plain tile over the 4 KiB stage, then a staged one
    out.append(("direct_tile_shift", *gap_pair(rng, [80] * 70, shift=5)))
    # ADD payload classes, before a COPY and as the trailing ADD
    out.append(("gaps_small", *gap_pair(rng, [1, 2, 3, 4, 5, 6, 8, 15, 16, 17, 31, 32, 33, 34, 64, 65, 100, 255])))
    out.append(("gaps_small_shift", *gap_pair(rng, [4, 1, 5, 32, 3, 33, 2, 255, 7], shift=3)))
    out.append(("gaps_large", *gap_pair(rng, [256, 257, 300, 511, 512, 513, 700, 1500], piece=200)))
    out.append(("gaps_large_shift", *gap_pair(rng, [256, 700, 513], piece=200, shift=9)))
    for t in (1, 4, 5, 32, 33, 255, 256, 900):
        out.append((f"tail_{t}", *tail_add_pair(rng, 400 + t, t)))
    for gap, last in ((5, 16), (9, 20), (15, 16)):
        out.append((f"window_{gap}_{last}", *window_pair(rng, 1000 + gap, gap, last)))
    # member density
    for k in DENSE_K:
        out.append((f"dense_{k}", *dense_pair(rng, k)))
    out.append(("alternating_18_30", *alternating_pair(rng, 18, 30)))
    out.append(("alternating_17_34", *alternating_pair(rng, 17, 34)))
    # command density
    out.append(("command_dense", *command_dense_pair(rng)))
    _SMALL = out
    return out


Layout = namedtuple("Layout", "lay r_size v_size align")


def layout(pairs, align):
    """pairs: (R, V) or (r_len, v_len).  align=16: every offset a multiple of
    16; align=1: every offset odd.  The arenas end at the last pair's last byte."""
    assert align in (1, 16)
    lens = [(len(a), len(b)) if not isinstance(a, int) else (a, b) for a, b in pairs]

    def nxt(x):
        return (x | 1) if align == 1 else (x + 15) & ~15

    lay = []
    rt, vt = (1, 3) if align == 1 else (0, 0)
    for k, (rl, vl) in enumerate(lens):
        lay.append((rt, rl, vt, vl))
        last = k + 1 == len(lens)
        rt, vt = (rt + rl, vt + vl) if last else (nxt(rt + rl), nxt(vt + vl))
    return Layout(lay, rt, vt, align)


def arenas(lay, pairs, fill=0):
    """The two arenas' bytes of `pairs` laid out by `lay`."""
    r, v = bytearray([fill]) * lay.r_size, bytearray([fill]) * lay.v_size
    for (ro, rl, vo, vl), (R, V) in zip(lay.lay, pairs):
        assert (rl, vl) == (len(R), len(V))
        r[ro:ro + rl] = R
        v[vo:vo + vl] = V
    return bytes(r), bytes(v)


# ── several contents of one layout ──────────────────────────────────────────

STRETCH = 4500       # an unmatched stretch of more than 4096 bytes ...
STRETCH_MIN = 8192   # ... in every pair at least this long, followed by a match
# In a pair this long, `edits` and `shift` substitute a byte every 24: matches of
# 23 bytes, which a correcting index that lost a few seeds to stale entries no
# longer finds whole (a long match is found from any of its seeds and grown
# backwards, so sparse edits alone would not show a stale index).  With a table
# of 65537 entries the pair's index is half full.
DENSE_MIN = 64 << 10
DENSE_STEP = 24


def rerun_lengths():
    """(r_len, v_len) of the small re-run layout: the chunk edges, some with
    |R| != |V|, and one pair of 64 KiB: densely edited, and long enough for the
    unmatched stretch (a one-pass table of |R| / 16 slots that 4500 unmatched
    seeds do not fill, so the match after them is found at every q)."""
    out = []
    for i, n in enumerate(CHUNK_EDGE_LENGTHS + [1000, 16]):
        out.append((n + (11 if i % 4 == 1 else 0), n + (23 if i % 4 == 3 else 0)))
    out.append((DENSE_MIN, DENSE_MIN))   # (its table of |R| / 16 slots is not yet full after the stretch)
    return out


def auto_lengths():
    """8 pairs of 160 KiB: a mean above the 128 KiB at which automatic mode picks members."""
    return [(160 << 10, 160 << 10)] * 8


DATASETS = ("edits", "unrelated", "same", "shift")


def datasets(lengths, seed=1):
    """name -> [(R, V)] of identical lengths: sparse substitutions, V random, V =
    R cut or extended, V = R moved by 1..8 bytes.  Every dataset has its own R.
    In pairs of STRETCH_MIN bytes or more, V starts with STRETCH unmatched bytes
    and a match follows them."""
    out = {}
    for d, name in enumerate(DATASETS):
        rng = random.Random(1000 * seed + d)
        pairs = []
        for i, (rl, vl) in enumerate(lengths):
            R = rng.randbytes(rl)
            base = (R + rng.randbytes(max(vl - rl, 0)))[:vl]
            if name == "edits":
                V = substituted(rng, base, range(50 + i, vl, 311))
            elif name == "unrelated":
                V = rng.randbytes(vl)
            elif name == "same":
                V = base
            else:
                s = 1 + (i + d) % 8
                V = (rng.randbytes(s) + R + rng.randbytes(max(vl - rl - s, 0)))[:vl]
            if min(rl, vl) >= DENSE_MIN and name in ("edits", "shift"):
                V = substituted(rng, V, range(DENSE_STEP - 1, vl, DENSE_STEP))
            if min(rl, vl) >= STRETCH_MIN:
                V = bytearray(V)
                V[:STRETCH] = rng.randbytes(STRETCH)
                if name == "unrelated":
                    V[STRETCH:STRETCH + 3000] = R[STRETCH:STRETCH + 3000]
                V = bytes(V)
            pairs.append((R, V))
        out[name] = pairs
    return out
