"""Inputs of tests/test_lineage_cpu.py, tests/test_lineage_sanitize_cpu.py and
tests/test_gpu_lineage.py, and the Python model of a lineage read.

A lineage is a base buffer R = V_0 and standard deltas d_1 .. d_k with
V_j = apply(V_{j-1}, d_j).  The model of a read is rc.model_version level by
level, then rc.model_read (model_lineage_read).  The status of a failing
lineage is the first that applies when walking from the requested delta
towards the base (include/delta_gpu.h): per delta its index status with the
stated ref_len, then UNSUPPORTED if it is valid but not sequential, then
INVALID_ARG if its ref_len is not its parent's version_size (node_status).

A forest is {"name", "nodes": [(R or None, delta, parent or BASE, ref_len)]}:
the shape the device takes.  ref_len is what the stream's descriptor states:
len(R) on a base, else the parent's header version_size (2^32 - 1 when the
parent has no readable header), unless a case states another on purpose
("host": False then: the host function cannot express it).  Nothing here
needs a GPU.
"""
from __future__ import annotations

import bisect
import random
import struct

import greedy_cases as gc
import read_cases as rc

OK, INVALID_ARG, UNSUPPORTED, MALFORMED = rc.OK, rc.INVALID_ARG, rc.UNSUPPORTED, rc.MALFORMED
BASE = 0xFFFFFFFF
NO_LIMIT = 0xFFFFFFFF
MAX_COPIES_PER_WINDOW = rc.WINDOW // 13


# ── the model ──

def model_lineage_read(R, deltas, off, length):
    """(status, bytes): rc.model_version applied level by level (every level
    sequential), then rc.model_read."""
    V = R
    for d in deltas:
        st, V, cmds = rc.model_version(V, d)
        if st:
            return st, b""
        if not is_sequential(cmds, len(V)):
            return UNSUPPORTED, b""
    return OK, rc.model_read(V, off, length)


def header_size(d):
    return struct.unpack(">I", d[5:9])[0] if len(d) >= 25 and d[:4] == b"DLT\x03" else None


def is_sequential(cmds, vs):
    end = 0
    for _, _, _, dst, n in cmds:
        if dst != end:
            return False
        end = dst + n
    return end == vs


def stated_ref_len(nodes, i):
    R, _, parent, ref_len = nodes[i]
    if ref_len is not None:
        return ref_len
    if parent == BASE:
        return len(R)
    hs = header_size(nodes[parent][1])
    return NO_LIMIT if hs is None else hs


def node_status(nodes, i):
    """The status of a read of node i's version, in the contract's order."""
    s = i
    while True:
        st, vs, cmds = rc.parse(stated_ref_len(nodes, s), nodes[s][1])
        if st:
            return st                                   # a
        if not is_sequential(cmds, vs):
            return UNSUPPORTED                          # b
        p = nodes[s][2]
        if p == BASE:
            return OK
        pst, pvs, _ = rc.parse(stated_ref_len(nodes, p), nodes[p][1])
        if not pst and stated_ref_len(nodes, s) != pvs:
            return INVALID_ARG                          # c
        s = p


def path(nodes, i):
    """(R, [d_1 .. d_k]) of node i."""
    ds = []
    while True:
        ds.append(nodes[i][1])
        if nodes[i][2] == BASE:
            return nodes[i][0], ds[::-1]
        i = nodes[i][2]


def depth(nodes, i):
    return len(path(nodes, i)[1])


def resolve(forest):
    """Per node (status, V or None, boundaries): the model's view of a forest."""
    nodes = forest["nodes"]
    out = []
    for i in range(len(nodes)):
        st = node_status(nodes, i)
        V, bounds = None, []
        if st == OK:
            R, ds = path(nodes, i)
            V = R
            for d in ds:
                mst, V, cmds = rc.model_version(V, d)
                assert mst == OK, (forest["name"], i)
                # the boundaries of the level below, carried through this level's COPYs
                carried = []
                if forest.get("dense", True):
                    for _, kind, src, dst, n in cmds:
                        if kind == 1:
                            carried += [dst + (b - src) for b in bounds[bisect.bisect_right(bounds, src):
                                                                          bisect.bisect_left(bounds, src + n)]]
                bounds = sorted(set([c[3] for c in cmds] + carried))
        elif forest.get("host", True):
            R, ds = path(nodes, i)
            assert model_lineage_read(R, ds, 0, 1)[0] == st, (forest["name"], i)   # one fault: the orders agree
        out.append((st, V, bounds))
    return out


def ranges(V, bounds, rng, dense=True):
    """(off, length) list: the edges of V, around command boundaries of every level, a tiling."""
    vs = len(V)
    out = [(0, vs), (0, 0), (vs, 5), (max(vs - 3, 0), 10), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (max(vs - 1, 0), 1)]
    if not dense:
        return out + [(vs // 3, 1), (vs // 2, 4096)]
    pick = bounds if len(bounds) <= 16 else bounds[:4] + bounds[-4:] + rng.sample(bounds[4:-4], 8)
    for b in pick:
        out += [(max(b - 1, 0), 2), (b, 1), (max(b - 17, 0), 34), (b, 4096)]
    return out + rc.tiling(vs, 16)


# ── building blocks ──

def chain_forest(name, R, deltas, **kw):
    return dict(name=name, nodes=[(R if j == 0 else None, d, BASE if j == 0 else j - 1, None)
                                  for j, d in enumerate(deltas)], **kw)


def seq_stream(orc, R, cmds):
    placed, vs = rc.sequential(cmds)
    return rc.stream(orc, R, placed, version_size=vs)


def step(rng, V, kind):
    b = bytearray(V)
    if not b or kind == "grow":
        return bytes(b + rng.randbytes(len(b) // 2 + 1500))
    if kind == "sub":
        for _ in range(max(1, len(b) // 100)):
            b[rng.randrange(len(b))] ^= rng.randrange(1, 256)
    elif kind == "ins":
        for _ in range(3):
            at = rng.randrange(len(b))
            b[at:at] = rng.randbytes(rng.randint(1, 300))
    elif kind == "del":
        for _ in range(3):
            at = rng.randrange(len(b))
            del b[at:at + rng.randint(1, 200)]
    elif kind == "transpose":
        x, y = sorted(rng.sample(range(len(b)), 2))
        b = b[y:] + b[x:y] + b[:x]
    elif kind == "shrink":
        b = b[:len(b) // 2]
    elif kind == "empty":
        b = bytearray()
    return bytes(b)


def encode(orc, algo, R, V, p):
    import oracle as O
    if algo == "greedy":
        return gc.model_delta(orc, R, V, p)
    return orc.encode(O.ONEPASS if algo == "onepass" else O.CORRECTING, R, V, p=p, q=1)


def block_permutation(orc, rng, R, block):
    """A stream of block-byte COPYs that permutes the blocks of R."""
    order = list(range(len(R) // block))
    rng.shuffle(order)
    return seq_stream(orc, R, [("C", k * block, block) for k in order])


def rotation(orc, R, block, shift):
    """V = R rotated left by shift, as COPYs that end at multiples of block."""
    n, cmds = len(R), []
    for dst in range(0, n, block):
        src, ln = (dst + shift) % n, min(block, n - dst)
        first = min(ln, n - src)
        cmds.append(("C", src, first))
        if first < ln:
            cmds.append(("C", 0, ln - first))
    return seq_stream(orc, R, cmds)


# ── the corpus ──

def history_forests(dg, orc):
    kinds = ["sub", "ins", "del", "transpose", "grow", "shrink", "sub", "ins"]
    algos = [("onepass", 8), ("correcting", 8), ("greedy", 4), ("onepass", 4), ("correcting", 4), ("greedy", 8)]
    out = []
    for n, (k, size) in enumerate([(1, 2048), (2, 38 << 10), (3, 9000), (5, 20000), (8, 5000)]):
        rng = random.Random(0x11EA + n)
        V = [rng.randbytes(size)]
        for j in range(k):
            kind = kinds[(j + n) % len(kinds)]
            if k == 5 and j == 2:
                kind = "empty"
            V.append(step(rng, V[-1], kind))
        ds = [encode(orc, *algos[(j + n) % len(algos)][:1], V[j], V[j + 1], algos[(j + n) % len(algos)][1]) for j in range(k)]
        out.append(chain_forest(f"history_depth{k}", V[0], ds))
    # the store: the newest version whole, backward deltas made by invert
    rng = random.Random(0x11EB)
    V = [rng.randbytes(12000)]
    for kind in ["ins", "sub", "del", "transpose"]:
        V.append(step(rng, V[-1], kind))
    fwd = [encode(orc, "onepass", V[j], V[j + 1], 8) for j in range(4)]
    back = [dg.invert(V[j], fwd[j]) for j in range(4)]   # delta(V[j + 1] -> V[j])
    out.append(chain_forest("store_backward", V[4], back[::-1]))
    # a composed delta (V0 -> V2) below a plain one
    out.append(chain_forest("composed_below", V[0], [dg.compose(fwd[0], fwd[1]), fwd[2], fwd[3]]))
    return out


def tree_forest(orc):
    """Streams 1, 2 share parent 0; streams 3, 4, 5 share parent 1; 6 lies on 4."""
    rng = random.Random(0x11EC)
    R = rng.randbytes(6000)
    V = {-1: R}
    nodes = []
    for i, (parent, kind) in enumerate([(BASE, "ins"), (0, "sub"), (0, "del"), (1, "transpose"), (1, "ins"), (1, "shrink"),
                                        (4, "sub")]):
        src = V[-1 if parent == BASE else parent]
        V[i] = step(rng, src, kind)
        nodes.append((R if parent == BASE else None, encode(orc, ["onepass", "correcting"][i % 2], src, V[i], 8), parent, None))
    return [dict(name="tree", nodes=nodes)]


def window_forests(orc):
    import encode_plan_cases as epc
    import oracle as O
    out = []
    # an inner level of many windows wholly inside a range: continuations
    R, V1 = epc.dense_pair(random.Random(71), epc.DENSE_STEP, n=epc.DENSE_MIN)
    d1 = orc.encode(O.ONEPASS, R, V1, p=16, q=1)
    rng = random.Random(0x11ED)
    V2 = step(rng, V1, "sub")
    V3 = step(rng, V2, "ins")
    out.append(chain_forest("inner_windows", R, [d1, encode(orc, "onepass", V1, V2, 16), encode(orc, "onepass", V2, V3, 16)]))
    # an ADD payload longer than a window at an inner level
    _, LR, ld, _ = rc.long_add_case(orc)[0]
    LV = rc.model_version(LR, ld)[1]
    R0 = step(rng, LR, "sub")
    V2 = step(rng, LV, "sub")
    out.append(chain_forest("inner_long_add", R0, [encode(orc, "onepass", R0, LR, 8), ld, encode(orc, "onepass", LV, V2, 8),
                                                   encode(orc, "correcting", V2, step(rng, V2, "del"), 8)]))
    return out


def dense_depth(cap):
    """Levels of 16-byte COPYs whose COPYs of one window, summed, come to 4x the stack's capacity."""
    k = -(-4 * cap // MAX_COPIES_PER_WINDOW)
    assert k <= 64, "the capacity is too large: depth 64 cannot reach 4x of it"
    return k


def dense_forest(orc, cap):
    rng = random.Random(0x11EE)
    R = rng.randbytes(16 << 10)
    ds, V = [], R
    for _ in range(dense_depth(cap)):
        d = block_permutation(orc, rng, V, 16)
        ds.append(d)
        V = rc.model_version(V, d)[1]
    return [chain_forest("dense", R, ds, dense=False)]


FANOUT_TOP, FANOUT_BLOCK = 300, 256


def fanout_forest(orc, cap):
    """The stack's overflow: a window of FANOUT_TOP children, the one on top of
    which (the last in stream order) fans out into FANOUT_BLOCK one-byte
    children one level down, over four more levels of 16-byte COPYs."""
    assert FANOUT_TOP <= MAX_COPIES_PER_WINDOW
    rng = random.Random(0x11EF)
    S = FANOUT_TOP * FANOUT_BLOCK
    R = rng.randbytes(S)
    ds, V = [], R
    for _ in range(4):
        d = block_permutation(orc, rng, V, 16)
        ds.append(d)
        V = rc.model_version(V, d)[1]
    # the last block byte by byte, the rest in 4 KiB COPYs
    mid = [("C", (a + 4096) % (S - FANOUT_BLOCK - 4096), min(4096, S - FANOUT_BLOCK - a)) for a in range(0, S - FANOUT_BLOCK, 4096)]
    mid += [("C", rng.randrange(S), 1) for _ in range(FANOUT_BLOCK)]
    d = seq_stream(orc, V, mid)
    ds.append(d)
    V = rc.model_version(V, d)[1]
    order = list(range(FANOUT_TOP - 1))
    rng.shuffle(order)
    d = seq_stream(orc, V, [("C", k * FANOUT_BLOCK, FANOUT_BLOCK) for k in order + [FANOUT_TOP - 1]])
    ds.append(d)
    return [chain_forest("fanout", R, ds, dense=False)]


def fragmenting_forest(orc):
    rng = random.Random(0x11F0)
    R = rng.randbytes(2048)
    ds, V = [], R
    for block, shift in [(4, 1), (8, 3), (16, 5), (32, 7), (64, 9)]:
        d = rotation(orc, V, block, shift)
        ds.append(d)
        V = rc.model_version(V, d)[1]
    return [chain_forest("fragmenting", R, ds)]


def zero_length_forest(orc):
    """Runs of zero-length COPYs longer than a parse window, in sequence (each starts where the one before it
    ends): whole windows that hold no byte of the version, at the requested level and at an inner one.  A
    range that spans a run is served through continuations that move on in the stream and not in the version."""
    rng = random.Random(0x11F3)
    R = rng.randbytes(3000)
    d1 = block_permutation(orc, rng, R, 100)
    V1 = rc.model_version(R, d1)[1]
    cmds = [("C", 5, 100), ("A", rng.randbytes(7))] + [("C", k % 50, 0) for k in range(1000)] + [("C", 900, 300)]
    cmds += [("A", b"")] * 700 + [("A", rng.randbytes(9)), ("C", 0, 64)] + [("C", 3000, 0)] * 330 + [("C", 1200, 50)]
    d2 = seq_stream(orc, V1, cmds)
    V2 = rc.model_version(V1, d2)[1]
    assert len(d2) > 5 * rc.WINDOW and MAX_COPIES_PER_WINDOW < 330
    d3 = seq_stream(orc, V2, [("C", 50, 400), ("A", rng.randbytes(3)), ("C", 0, len(V2))])
    return [chain_forest("zero_length_windows", R, [d1, d2, d3])]


def failing_forests(orc):
    """Lineages of three deltas in which one, at each level in turn, fails."""
    rng = random.Random(0x11F1)
    faults = [(n, R, d) for n, R, d, _ in rc.damaged_cases(orc)]
    faults += [(n, R, d) for n, R, d, _ in rc.nonsequential_cases(orc) if n in ("exchanged", "overlapping", "gap")]
    out = []
    for name, FR, fd in faults:
        for level in (1, 2, 3):
            nodes, below = [], step(rng, FR, "sub")
            # good deltas up to the faulty one's reference ...
            for j in range(1, level):
                target = FR if j == level - 1 else step(rng, below, "ins")
                nodes.append((below if j == 1 else None, encode(orc, "onepass", below, target, 8), BASE if j == 1 else j - 2, None))
                below = target
            nodes.append((FR if level == 1 else None, fd, BASE if level == 1 else level - 2, None))
            # ... and sequential streams above it, inside what its header states
            for j in range(level + 1, 4):
                hs = header_size(nodes[-1][1])
                vs = 64 if hs is None else hs
                cmds = [("C", 0, vs // 2), ("A", rng.randbytes(5)), ("C", vs // 2, vs - vs // 2)]
                nodes.append((None, seq_stream(orc, bytes(vs), cmds), j - 2, None))
            out.append(dict(name=f"fail_{name}_at{level}", nodes=nodes, dense=False))
    # a stated ref_len that is not the parent's size (the device's descriptors only)
    V = [rng.randbytes(3000)]
    for kind in ["ins", "sub", "del"]:
        V.append(step(rng, V[-1], kind))
    ds = [encode(orc, "onepass", V[j], V[j + 1], 8) for j in range(3)]
    for level in (2, 3):
        for delta in (1, -1, 1000):
            f = chain_forest(f"fail_ref_len{delta:+d}_at{level}", V[0], ds, dense=False, host=False)
            R_, d_, p_, _ = f["nodes"][level - 1]
            f["nodes"][level - 1] = (R_, d_, p_, len(V[level - 1]) + delta)
            out.append(f)
    return out


_cache = {}


def corpus(dg, orc):
    """[(forest, [(status, V, [(off, length)])] per node)], built once per session."""
    if "all" not in _cache:
        cap = dg.lineage_work_items()
        forests = history_forests(dg, orc) + tree_forest(orc) + window_forests(orc) + dense_forest(orc, cap)
        forests += fanout_forest(orc, cap) + fragmenting_forest(orc) + zero_length_forest(orc) + failing_forests(orc)
        rng = random.Random(0x11F2)
        out = []
        for f in forests:
            per = []
            for st, V, bounds in resolve(f):
                rs = ranges(V, bounds, rng, f.get("dense", True)) if st == OK else [(0, 16), (3, 1), (0, 0)]
                per.append((st, V, rs))
            out.append((f, per))
        _cache["all"] = out
    return _cache["all"]


def by_name(dg, orc, name):
    return next(c for c in corpus(dg, orc) if c[0]["name"] == name)
