"""Named CRWI graphs for the in-place conversion tests (not a test module).

Each graph is a recipe: a random R (seeded) and a command list whose placed,
standard delta has the stated read/write-interval structure.  The reference's
`delta inplace` output for every graph and both policies is pinned in
tests/golden/golden_inplace_graphs.json (make_golden_inplace_graphs.py); the
CPU test holds dg_make_inplace to it, the GPU test the device converter.

Edge i -> j: copy i reads bytes copy j writes.  Copies are numbered in command
(= destination) order, ADDs not counted.
"""
from __future__ import annotations

import random

POLICIES = ("localmin", "constant")
PERM_SIZES = (63, 64, 65, 127, 128, 129, 4095, 4096, 4097)


def _r(seed: int, n: int) -> bytes:
    return random.Random(0x1A9E0000 + seed).randbytes(n)


def _blocks(order, sizes):
    """Copies of R's consecutive blocks (sizes) in the given order."""
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return [("copy", off[b], sizes[b]) for b in order]


def named_graphs():
    """[(name, params, R, cmds)]; cmds: ("copy", src, len) | ("add", bytes)."""
    out = []

    def g(name, seed, r_len, cmds, **params):
        out.append((name, dict(seed=seed, r_len=r_len, **params), _r(seed, r_len), cmds))

    g("empty", 1, 4096, [])
    g("adds_only", 2, 4096, [("add", b"hello, world"), ("add", _r(102, 300))])
    g("identity_copy", 3, 4096, [("copy", 0, 4096)])
    # two 64-byte blocks exchanged: equal lengths, the tie goes to the lower index
    g("swap_equal", 4, 4096, [("copy", 64, 64), ("copy", 0, 64)])
    # V = R[100:400] + R[0:100]: localmin converts the 100-byte copy, constant copy 0
    g("swap_unequal", 5, 4096, [("copy", 100, 300), ("copy", 0, 100)])
    for k in (3, 8):   # blocks rotated left by one: one cycle, one victim
        g(f"rotate_{k}", 6 + k, 4096, _blocks(list(range(1, k)) + [0], [64] * k), blocks=k)
    # eight blocks of distinct lengths, reversed: several victims, multi-edge SCCs
    g("reverse_8", 20, 4096, _blocks(list(range(7, -1, -1)), [40, 72, 56, 104, 88, 24, 120, 136]))
    # copy 1 reads [99, 109): 1 byte of copy 0's write [0, 100) (edge through the
    # lo - 1 predecessor) and its own write (no self edge); copy 2 reads
    # [100, 105), starting exactly where copy 0's write ends (no edge to it)
    g("pred_touch", 21, 4096, [("copy", 2000, 100), ("copy", 99, 10), ("copy", 100, 5)])
    # copy 2 reads [50, 100), ending exactly at copy 1's write [100, 200) (no
    # edge); copy 3 reads [50, 101), 1 byte into it (edge)
    g("hi_touch", 22, 4096, [("copy", 3000, 100), ("copy", 3100, 100), ("copy", 50, 50), ("copy", 50, 51)])
    # src = dst + 5: the copy reads its own write only
    g("self_overlap", 23, 4096, [("add", b"0123456789"), ("copy", 15, 200), ("add", b"tail")])
    # copy 0 (2048 bytes) reads [2048, 4096), where 130 8-byte copies write;
    # each of them reads copy 0's destination: 130 two-cycles through copy 0
    g("wide_fan", 24, 4096, [("copy", 2048, 2048)] + [("copy", 8 * i, 8) for i in range(130)], fan=130)
    # swap A = copies 0, 1; copy 2 reads A's writes; swap B = copies 3, 4, and
    # copy 4 also reads copy 2's write: B -> 2 -> A, so B is the source component
    # although A has the lower indices
    g("two_sccs_linked", 25, 4096,
      [("copy", 64, 64), ("copy", 0, 64), ("copy", 32, 64), ("copy", 256, 64), ("copy", 160, 64)])
    # copy 0 (128) <-> copy 1 (100) and copy 0 <-> copy 2 (28): the first cycle
    # found is 0 -> 1 -> 0, which does not hold copy 2, the shortest of all
    g("figure_eight", 26, 4096, [("copy", 128, 128), ("copy", 0, 100), ("copy", 100, 28)])
    # permutations of 4-byte blocks: bitmap and scan word boundaries.  R has
    # 4096 blocks; the 4097-copy graph repeats one block at the end
    for n in PERM_SIZES:
        rng = random.Random(0x9E3700 + n)
        nb = min(n, 4096)
        perm = list(range(nb))
        rng.shuffle(perm)
        if n > nb:
            perm += [rng.randrange(nb) for _ in range(n - nb)]
        g(f"perm_{n}", 100 + n, 4096 if n <= 1024 else 16384, [("copy", 4 * b, 4) for b in perm], copies=n)
    return out


SEAM_SIZES = (2047, 2048, 2049, 65535, 65536, 65537)


def seam_graphs():
    """Graphs at the storage seams of the device's order kernel, kept apart from named_graphs() because they
    are larger: the dst column is cached in LDS up to 2048 copies, and the ready bitmap lies in LDS up to 2048
    words, 65536 copies (kLdsWords of dg_inplace_dev.hip).  Pinned in tests/golden/golden_inplace_seams.json."""
    out = []

    def g(name, seed, r_len, cmds, **params):
        out.append((name, dict(seed=seed, r_len=r_len, **params), _r(seed, r_len), cmds))

    for n in SEAM_SIZES:   # permutations of 4-byte blocks, one block repeated where R has one too few
        rng = random.Random(0x9E3700 + n)
        r_len = 16384 if n < 4096 else 1 << 18
        nb = min(n, r_len // 4)
        perm = list(range(nb))
        rng.shuffle(perm)
        if n > nb:
            perm += [rng.randrange(nb) for _ in range(n - nb)]
        g(f"perm_{n}", 100 + n, r_len, [("copy", 4 * b, 4) for b in perm], copies=n)
    # lengths on both sides of 2^8 and 2^16, so three radix passes, on the Kahn path and with victims: six
    # blocks rotated left by one, then two exchanges of neighbours; then six copies that read the rotation's
    # blocks and that nothing reads: ready from the start, they pop in rank order before all others
    sizes = [65536, 255, 65537, 256, 65535, 257, 256, 65536, 65535, 257]
    g("radix_edges", 30, 400 * 1024, _blocks([1, 2, 3, 4, 5, 0, 7, 6, 9, 8], sizes) +
      [("copy", 100 * k, n) for k, n in enumerate([257, 65536, 255, 65537, 256, 65535])])
    return out


def build(dg, orc, R, cmds):
    """(standard delta, V) of a recipe: place_commands + encode_delta."""
    cl = [dg.CopyCmd(c[1], c[2]) if c[0] == "copy" else dg.AddCmd(c[1]) for c in cmds]
    V = b"".join(R[c[1]:c[1] + c[2]] if c[0] == "copy" else c[1] for c in cmds)
    d = dg.encode_delta(dg.place_commands(cl), inplace=False, version_size=len(V),
                        src_crc=orc.crc64_xz(R), dst_crc=orc.crc64_xz(V))
    return d, V
