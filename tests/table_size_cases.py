"""Pairs that tell a wrong table slot from a right one at a given table size.

Every encoder kernel turns a fingerprint into `fp % q`, by FP64 below 2^23 and
by a 64-bit Barrett reduction from there on, and the window chain's
first-writer search changes at 2^25.  A slot function that is wrong but
deterministic still sends equal windows to equal slots, so on random data the
delta changes only where two different windows share a slot inside one epoch:
at q >= 2^20 that almost never happens by itself.  The pairs here plant such
collisions for one q: 16-byte windows found by a birthday search that share a
slot at that q and at none of the other sizes under test, laid out so that the
first writer of the slot (onepass.c:141-166) blocks a lookup that would
otherwise hit.  Each planted collision costs exactly one byte of delta (the
COPY starts one byte later), so the delta at the planted q differs from the
delta at every other q.

Pure Python, fixed seeds, p = 16; shared by the CPU tests (which prove the
above), the golden minting script and the GPU tests.
"""
from __future__ import annotations

import functools
import random

M61 = (1 << 61) - 1
BASE = 263
P = 16

Q_DEFAULT = 1048573                      # the CLI's --table-size default
Q_BELOW_23, Q_ABOVE_23 = 8388593, 8388617    # the primes around 2^23
Q_BELOW_25, Q_ABOVE_25 = 33554393, 33554467  # the primes around 2^25
QS = (Q_DEFAULT, Q_BELOW_23, Q_ABOVE_23, Q_BELOW_25, Q_ABOVE_25)

FAMILIES = ("offdiag_v", "offdiag_r", "diagonal")
GAPS = (48, 300, 900, 3000)
SHORT_RUNS = (5, 9)                      # mismatch runs of the short diagonal family
N_PAIRS, N_TRIPLES = 8, 6
SKEW = 37                                # how much longer j2 is than j1

# correcting: (r_len, q, max_table) -> (cap, |F|, m); |F| = next_prime(2 seeds)
# is the last prime below 2^23 at 4 MiB and the first above it 8 bytes later
MAX_TABLE = 1073741827
CORRECTING_ROWS = (
    (4194304, 1, MAX_TABLE, (524287, 8388581, 16)),
    (4194304, 1048573, MAX_TABLE, (1048573, 8388581, 8)),
    (4194304, 1, 4096, (4099, 8388581, 2047)),
    (4194312, 1, MAX_TABLE, (524287, 8388617, 17)),
    (4194312, 1048573, MAX_TABLE, (1048573, 8388617, 9)),
    (4194312, 1, 4096, (4099, 8388617, 2047)),
)

BUF_CAP_1_ROW = (4194312, 1, 4096)       # also encoded with a lookback buffer of 1


def correcting_name(r_len, q, max_table, buf_cap=256):
    return f"correcting_r{r_len}_q{q}_mt{max_table}" + (f"_buf{buf_cap}" if buf_cap != 256 else "")


def golden():
    """{name: case} of golden/golden_table_size.json (minted from the
    reference by golden/make_golden.py)."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_table_size.json")
    with open(path) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


# onepass at its natural size: q = next_prime(seeds / 16) passes 2^23 here
NATURAL_LEN = (128 << 20) + 4096
NATURAL_Q = 8388881
NATURAL_SEED = 0x7AB1E128


def fingerprint(w: bytes) -> int:
    """sum(w[i] * 263**(15 - i)) mod (2**61 - 1) (hash.c), by Horner."""
    h = 0
    for b in w:
        h = (h * BASE + b) % M61
    return h


def _distinct_elsewhere(ws, q) -> bool:
    fps = [fingerprint(w) for w in ws]
    for o in QS:
        if o != q and len({f % o for f in fps}) != len(fps):
            return False
    return True


def _windows(rng, nh: int, nt: int):
    """An endless stream of distinct (bytes, fingerprint) of nh + nt bytes: a
    random head followed by a random tail, fp = fp(head) 263^nt + fp(tail),
    so the n-th head and tail add 2n - 1 windows for two short fingerprints."""
    bt = pow(BASE, nt, M61)
    heads, tails = [], []
    seen_h, seen_t = set(), set()
    while True:
        hb, tb = rng.randbytes(nh), rng.randbytes(nt)
        if hb in seen_h or tb in seen_t:
            continue
        seen_h.add(hb)
        seen_t.add(tb)
        fh, ft = fingerprint(hb) * bt % M61, fingerprint(tb)
        for tb2, ft2 in tails:
            yield hb + tb2, (fh + ft2) % M61
        heads.append((hb, fh))
        tails.append((tb, ft))
        for hb2, fh2 in heads:
            yield hb2 + tb, (fh2 + ft) % M61


@functools.lru_cache(maxsize=None)
def collisions(q: int):
    """(pairs, triples): N_PAIRS tuples (A, B) and N_TRIPLES tuples
    (A1, A2, B) of distinct random 16-byte windows with equal fp % q and
    pairwise unequal slots at every other q of QS.  Birthday search, bucketed
    by slot."""
    buckets = {}
    pairs, triples = [], []
    for w, f in _windows(random.Random(0x51075 ^ q), 8, 8):
        b = buckets.setdefault(f % q, [])
        if len(b) >= 3:
            continue
        b.append(w)
        if len(b) == 1:
            continue
        if not _distinct_elsewhere(b, q):
            b.pop()
        elif len(b) == 2 and len(pairs) < N_PAIRS:
            pairs.append((b[0], b[1]))
        elif len(b) == 3 and len(triples) < N_TRIPLES:
            triples.append((b[0], b[1], b[2]))
        if len(pairs) == N_PAIRS and len(triples) == N_TRIPLES:
            return tuple(pairs), tuple(triples)


@functools.lru_cache(maxsize=None)
def short_triples(q: int, k: int):
    """(P, [(X1, X2, Y)]): a 16 - k byte string P and N_TRIPLES tuples of k-byte
    strings such that the windows X1 + P, X2 + P and P + Y share a slot at q
    (and at no other q of QS), X1 and X2 differing in their first and last
    bytes.  In R = .. X1 P Y .. and V = .. X2 P Y .. the mismatch run is k
    bytes long, its first windows are X1 + P and X2 + P and the first equal
    window is P + Y: overlapping windows, found by the same birthday search
    over the k free bytes on either side of P."""
    rng = random.Random(0x5407 ^ q ^ (k << 40))
    Pb = rng.randbytes(P - k)
    fP = fingerprint(Pb)
    bx, by = pow(BASE, P - k, M61), pow(BASE, k, M61)
    xs, ys, out = {}, {}, []
    done = set()

    def close(s):
        if s in done or s not in ys:
            return
        X = xs.get(s, [])
        for i in range(len(X)):
            for j in range(i):
                X1, X2, Y = X[j], X[i], ys[s][0]
                if X1[0] != X2[0] and X1[-1] != X2[-1] and \
                        _distinct_elsewhere([X1 + Pb, X2 + Pb, Pb + Y], q):
                    out.append((X1, X2, Y))
                    done.add(s)
                    return

    for (X, fx), (Y, fy) in zip(_windows(rng, k // 2, k - k // 2), _windows(rng, k // 2, k - k // 2)):
        sa = (fx * bx + fP) % M61 % q
        sb = (fP * by + fy) % M61 % q
        xs.setdefault(sa, []).append(X)
        ys.setdefault(sb, []).append(Y)
        close(sa)
        close(sb)
        if len(out) >= N_TRIPLES:
            return Pb, tuple(out[:N_TRIPLES])


def _offdiag(rng, q, gap, blocker_in_v):
    """V = j1 + S and R = j2 + S per collision (roles swapped for the R
    table): j1 holds A `gap` bytes before S = B + 300 random bytes and j2 is
    SKEW bytes longer.  A is the first writer of B's slot in the table of its
    own stream, so the other stream's lookup of B, SKEW steps later, finds A
    and fails; the window one byte on hits."""
    first, second = bytearray(), bytearray()
    for i, (A, B) in enumerate(collisions(q)[0]):
        # every other blocker of a long epoch sits past the steps the chain
        # keeps in registers (64 kHistChunks = 384), i.e. in the table tier
        lead = rng.randrange(20, 60) + (rng.randrange(400, 700) if i % 2 and gap >= 900 else 0)
        j1 = rng.randbytes(lead) + A + rng.randbytes(gap - P)
        j2 = rng.randbytes(len(j1) + SKEW)
        S = B + rng.randbytes(300)
        first += j1 + S
        second += j2 + S
    first, second = bytes(first), bytes(second)
    return (second, first) if blocker_in_v else (first, second)   # (R, V)


def _diagonal(rng, q, gap):
    """R = pre + jR + B + tail and V = pre + jV + B + tail per collision,
    |jR| = |jV| = gap: A1 in jR and A2 in jV (different offsets) are the first
    writers of B's slot in the two tables, so at the first equal window after
    the mismatch run neither B is stored and both lookups find another
    window."""
    R = bytearray(rng.randbytes(64))
    V = bytearray(R)
    for A1, A2, B in collisions(q)[1]:
        o1 = rng.randrange(0, gap - P)        # (the last byte of j stays filler)
        o2 = rng.choice([o for o in range(0, gap - P) if o != o1])
        jr, jv = bytearray(rng.randbytes(gap)), bytearray(rng.randbytes(gap))
        jr[o1:o1 + P] = A1
        jv[o2:o2 + P] = A2
        if jr[gap - 1] == jv[gap - 1]:        # B is the first equal window
            jv[gap - 1] ^= 0x55
        tail = rng.randbytes(rng.randrange(200, 300))
        R += bytes(jr) + B + tail
        V += bytes(jv) + B + tail
    return bytes(R), bytes(V)


def _diagonal_short(rng, q, k):
    """The diagonal family with a mismatch run of only k bytes (an epoch of
    k + 1 steps): R = pre + X1 + P + Y + tail and V = pre + X2 + P + Y + tail
    per collision (short_triples).  The window chain resolves such short
    epochs by its lane-shift first-writer search (dg_onepass.hip diag_batch,
    epochs of at most 32 steps), the one whose key packing stops at q = 2^25;
    the gaps of the other families are all longer than that."""
    Pb, triples = short_triples(q, k)
    R = bytearray(rng.randbytes(64))
    V = bytearray(R)
    for X1, X2, Y in triples:
        tail = rng.randbytes(rng.randrange(200, 300))
        R += X1 + Pb + Y + tail
        V += X2 + Pb + Y + tail
    return bytes(R), bytes(V)


@functools.lru_cache(maxsize=None)
def onepass_cases(q: int):
    """[(name, R, V)] for every family and gap, collisions planted for q."""
    out = []
    for k in SHORT_RUNS:
        R, V = _diagonal_short(random.Random(q * 64 + k), q, k)
        out.append((f"diagonal_short{k}_q{q}", R, V))
    for fi, fam in enumerate(FAMILIES):
        for gap in GAPS:
            rng = random.Random((q * 8 + fi) * 4096 + gap)
            if fam == "diagonal":
                R, V = _diagonal(rng, q, gap)
            else:
                R, V = _offdiag(rng, q, gap, fam == "offdiag_v")
            out.append((f"{fam}_gap{gap}_q{q}", R, V))
    return tuple(out)


def n_planted(name: str) -> int:
    return N_TRIPLES if name.startswith("diagonal") else N_PAIRS


@functools.lru_cache(maxsize=None)
def _boundary_pair(r_len: int):
    import oracle as O
    orc = O.Oracle()
    R, E = orc.synth_pair(0x7AB1E000 + (r_len & 0xFFF), r_len, r_len // 100)
    cuts = [r_len * k // 8 for k in range(9)]
    blocks = [E[a:b] for a, b in zip(cuts, cuts[1:])]
    random.Random(8).shuffle(blocks)
    return R, b"".join(blocks)


def correcting_boundary_pair(r_len: int):
    """R: the oracle's synthetic reference of r_len bytes; V: its 1 %-edited
    version cut into 8 blocks and shuffled (fixed seed), so correcting has to
    find every block through the R index."""
    return _boundary_pair(r_len)


def natural_pair(orc):
    """The 128 MiB + 4 KiB pair (1 % edits) whose own q is NATURAL_Q."""
    return orc.synth_pair(NATURAL_SEED, NATURAL_LEN, NATURAL_LEN // 100)
