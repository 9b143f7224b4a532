"""Batches for tests/test_gpu_stale_index.py: a plan is indexed on batch A, the
delta arena is overwritten in place with batch B of the same layout, and the
plan runs without another index pass (the containment contract of
dg_read_plan_run and dg_lineage_plan_run in include/delta_gpu.h).

B holds valid streams or a constant fill, never random bytes.  A_i and B_i have
one length: the shorter one is padded after its END byte, which both index
passes ignore.  The families:

  payload    B_i is A_i with ADD payload bytes changed: the index depends on the
             framing alone, so it is not stale and every result is exact;
  framing    the same version from other commands (another encoder's, and every
             command split until the stream is strides longer: reframe);
  smaller, larger   another version_size: the stale head's vsize sizes requests;
  unordered  A_i is sequential, B_i is one of read_cases.nonsequential_cases
             ("exchanged", "overlapping", "gap"): the stale sequential flag
             sends the range-entry path into a stream that does not tile;
  fills      the arena filled with 0x00, 0x01, 0xFF.

index_cases.serial_index is the index model: equal for payload, different for
every case of the other families (the generators are stale by construction and
assert it; each family has 20 streams or more: tests/test_stale_cases_cpu.py).  Lineage
forests of depth 1, 3 and 8 (lineage_cases) have one level replaced at a time.
Nothing here needs a GPU.
"""
from __future__ import annotations

import random

import high_offset_cases as hc
import index_cases as ic
import lineage_cases as lc
import read_cases as rc

FILLS = [0x00, 0x01, 0xFF]
MIN_STREAMS = 20


def pad(d, n):
    """d with zeros after its END byte, n bytes in all."""
    assert len(d) <= n and d[-1:] == b"\0"
    return d + bytes(n - len(d))


def pair(a, b):
    n = max(len(a), len(b))
    return pad(a, n), pad(b, n)


def gen(rng, n_cmds, rlen, add=(1, 20)):
    """A sequential stream of n_cmds commands over a reference of rlen bytes: COPYs of 1..90 bytes, ADDs between them."""
    return [("C", rng.randrange(0, rlen - 90), rng.randint(1, 90)) if k % 2 else ("A", rng.randbytes(rng.randint(*add)))
            for k in range(n_cmds)]


def split(rng, cmds):
    """The same version from other commands: every command of two bytes or more in two."""
    out = []
    for c in cmds:
        n = c[2] if c[0] == "C" else len(c[1])
        if n < 2:
            out.append(c)
            continue
        k = rng.randrange(1, n)
        out += [("C", c[1], k), ("C", c[1] + k, n - k)] if c[0] == "C" else [("A", c[1][:k]), ("A", c[1][k:])]
    return out


def reframe(rng, d, grow=1):
    """The version of the sequential stream d from other commands, stale by construction: every command is
    split in two until the stream is `grow` index strides and more longer than d.  A stream inside one
    stride has one index however it is framed; here a stride where d, padded, has nothing left (the index
    says "nothing follows") holds commands."""
    st, _, cmds = rc.parse(1 << 32, d)
    assert st == rc.OK
    cmds = [("C", s, n) if kind == 1 else ("A", d[s:s + n]) for _, kind, s, _, n in cmds]
    target = (len(d) // ic.STRIDE + 1 + grow) * ic.STRIDE
    while True:
        out = hc.sstream(cmds)
        if len(out) >= target:
            return out
        finer = split(rng, cmds)
        assert len(finer) > len(cmds), "the version is too short to be framed that finely"
        cmds = finer


def other_payload(rng, d):
    """d with every ADD payload byte changed."""
    out = bytearray(d)
    st, _, cmds = rc.parse(1 << 32, d)
    assert st == rc.OK
    for _, kind, at, _, n in cmds:
        if kind == 2:
            for k in range(at, at + n):
                out[k] ^= rng.randrange(1, 256)
    return bytes(out)


def index_of(ref_len, d):
    return ic.serial_index(ref_len, d)


def stale(ref_len, a, b):
    return index_of(ref_len, a) != index_of(ref_len, b)


SIZES = [6, 40, 200, 200, 400, 700, 1500, 3000]   # commands: from one window of 4 KiB to more than 40 KiB of stream


def read_families(orc):
    """{family: [(name, R, A_i, B_i)]}, A_i and B_i of one length; fills: B_i is None (the arena is filled)."""
    import oracle as O
    rng = random.Random(0x57A1E)
    out = {k: [] for k in ("payload", "framing", "smaller", "larger", "unordered", "fills")}
    for k in range(24):
        R = rng.randbytes(3000 + 97 * k)
        cmds = gen(rng, SIZES[k % len(SIZES)], len(R))
        a = hc.sstream(cmds)
        out["payload"].append((f"payload_{k}", R, a, other_payload(rng, a)))
        out["fills"].append((f"fill_{k}", R, a, None))
        if k % 2:
            b = reframe(rng, a, 1 + k % 3)
        else:   # two encoders on one pair; the second one's commands split further, past the first one's strides
            V = lc.step(rng, lc.step(rng, R, "ins"), "sub")
            a, b = orc.encode(O.ONEPASS, R, V, p=8, q=1), orc.encode(O.CORRECTING, R, V, p=8, q=1)
            b = reframe(rng, b, max(len(a) // ic.STRIDE - len(b) // ic.STRIDE, 0) + 1)
        out["framing"].append((f"framing_{k}", R) + pair(a, b))
        a = hc.sstream(cmds)
        out["smaller"].append((f"smaller_{k}", R) + pair(a, hc.sstream(gen(rng, max(len(cmds) // 2, 2), len(R)))))
        out["larger"].append((f"larger_{k}", R) + pair(a, hc.sstream(gen(rng, len(cmds) + len(cmds) // 2 + 2, len(R)))))
    lost = [c for c in rc.nonsequential_cases(orc) if c[0] in ("exchanged", "overlapping", "gap")]
    assert len(lost) == 3
    for k in range(24):
        name, R, b, _ = lost[k % 3]
        a = hc.sstream(gen(rng, [4, 12, 30, 80, 200, 400, 900, 2000][k // 3], len(R), add=(1, 6)))
        out["unordered"].append((f"unordered_{name}_{k}", R) + pair(a, b))
    # a case that is not stale proves nothing: every generator above is stale by construction, and this holds them to it
    for fam in ("framing", "smaller", "larger", "unordered"):
        for c in out[fam]:
            assert stale(len(c[1]), c[2], c[3]), c[0]
    for c in out["fills"]:
        assert all(stale(len(c[1]), c[2], bytes([f]) * len(c[2])) for f in FILLS), c[0]
    return out


def requests(rng, vs):
    """(off, length) for a version of vs bytes: its edges, a few short ranges, one of up to 16 KiB."""
    rs = [(0, 300), (max(vs - 100, 0), 300), (vs // 2, 4096), (0, min(vs + 5, 1 << 14)), (vs, 7)]
    return rs + [(rng.randrange(0, max(vs, 1)), rng.choice([1, 17, 300, 3000])) for _ in range(5)]


# ── lineages ──

FORESTS = ["history_depth1", "history_depth3", "history_depth8"]
VARIANTS = 4   # per replaced level and family (unordered: the three streams of read_cases)


def lineage_families(dg, orc):
    """{family: [(name, nodes_a, nodes_b)]}: forests of depth 1, 3 and 8 with the top, the middle and the base
    level replaced in turn; nodes as lineage_cases has them, every ref_len stated as the plan made for A
    states it, A's and B's delta of one length.  fills: (name, nodes_a, the level to fill)."""
    import oracle as O
    rng = random.Random(0x57A1F)
    out = {k: [] for k in ("payload", "framing", "smaller", "larger", "unordered", "fills")}
    lost = [c for c in rc.nonsequential_cases(orc) if c[0] in ("exchanged", "overlapping", "gap")]
    for fname in FORESTS:
        f, per = lc.by_name(dg, orc, fname)
        nodes = [(R, d, p, lc.stated_ref_len(f["nodes"], i)) for i, (R, d, p, _) in enumerate(f["nodes"])]
        depth = len(nodes)
        below = lambda j: nodes[0][0] if j == 0 else per[j - 1][1]   # the version level j's delta applies to
        for j in sorted({depth - 1, depth // 2, 0}):
            src, V = below(j), per[j][1]
            enc = lambda algo, p_, v: orc.encode(algo, src, v, p=p_, q=1)
            other = {}
            for k, (algo, p_) in enumerate([(O.CORRECTING, 8), (O.ONEPASS, 4), (O.CORRECTING, 16), (O.ONEPASS, 8)][:VARIANTS]):
                other[f"payload{k}"] = other_payload(rng, nodes[j][1])
                # another encoder's stream of the same version, its commands split past the strides of A's stream
                b = enc(algo, p_, V)
                other[f"framing{k}"] = reframe(rng, b, max(len(nodes[j][1]) // ic.STRIDE - len(b) // ic.STRIDE, 0) + 1 + k % 2)
                other[f"smaller{k}"] = enc(O.ONEPASS, 8, V[:len(V) * (k + 1) // 5])
                other[f"larger{k}"] = enc(O.ONEPASS, 8, V + rng.randbytes(len(V) * (k + 1) // 5 + 50))
            for k, (_, _, b, _) in enumerate(lost):
                other[f"unordered{k}"] = b
            for fam, b in other.items():
                a2, b2 = pair(nodes[j][1], b)
                na = [n if i != j else (n[0], a2, n[2], n[3]) for i, n in enumerate(nodes)]
                nb = [n if i != j else (n[0], b2, n[2], n[3]) for i, n in enumerate(nodes)]
                if fam.startswith("payload"):
                    if a2 == b2:   # (a level without an ADD has no other payload: not a case)
                        continue
                else:   # stale by construction: a case that is not fails here, before any GPU
                    assert stale(nodes[j][3], a2, b2), (fname, j, fam)
                out[fam.rstrip("0123")].append((f"{fname}_level{j}_{fam}", na, nb))
            out["fills"].append((f"{fname}_level{j}_fill", nodes, j))
    return out


def lineage_streams(cases):
    """The streams a family's GPU run replaces: (stated ref_len, A_i, B_i) per replaced level."""
    out = []
    for _, na, nb in cases:
        out += [(a[3], a[1], b[1]) for a, b in zip(na, nb) if a[1] != b[1]]
    return out
