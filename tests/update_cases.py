"""Inputs of tests/test_gpu_update.py: in-place command lists, the deltas made of
them, and ways to damage a delta.

The order kinds restate those of tests/test_gpu_decode_order.py (c5 shape,
reversed ADDs, ADDs overwriting within a batch of 64 commands and across
batches, a shuffled tail, moving COPYs, zero-length commands, grow) and add
shrink (version_size < |R|).  The moving families are block rotations (every
COPY overwrites the bytes the one before it read), whole-buffer shifts (one
COPY onto an overlapping range, forward and backward) and blocks swapped
through an ADD (a broken cycle).  Expected bytes always come from the oracle's
sequential replay.
"""
from __future__ import annotations

ORDER_KINDS = ["c5_shape", "reversed", "overlap_batch", "overlap_cross", "shuffled_tail", "moving", "zero", "grow",
               "shrink"]
ROTATE_BLOCKS = [16, 100, 1000, 4096]
SHIFTS = [1, 15, 16, 17, 300]
MOVE_KINDS = ([f"rotate{b}" for b in ROTATE_BLOCKS] + [f"shift_fwd{k}" for k in SHIFTS] +
              [f"shift_back{k}" for k in SHIFTS] + ["swap"])
WINDOW = 4096   # bytes of the command stream the kernel parses at a time


def order_case(dg, rng, kind, n_r=20000, n_cmds=1500):
    """(R, cmds, version_size): COPYs first (no-ops on the diagonal, some moving),
    then ADDs, as the in-place format lists them (inplace.c:711-725)."""
    R = rng.randbytes(n_r)
    vsize = n_r + 3000 if kind == "grow" else n_r - n_r // 4 if kind == "shrink" else n_r
    cap = max(n_r, vsize)
    top = min(n_r, vsize)   # commands of a shrinking update stay inside V
    cmds = []
    pos = 0
    while pos < top and len(cmds) < n_cmds // 2:
        ln = rng.randint(1, 40)
        if pos + ln > top:
            break
        if kind == "moving" and rng.random() < 0.02:
            src = rng.randrange(0, n_r - ln)
            cmds.append(dg.PlacedCopy(src=src, dst=pos, length=ln))
        elif kind == "zero" and rng.random() < 0.05:
            cmds.append(dg.PlacedCopy(src=pos, dst=pos, length=0))
        else:
            cmds.append(dg.PlacedCopy(src=pos, dst=pos, length=ln))
        pos += ln + rng.randint(0, 12)
    adds = []
    p = 0
    lim = (vsize if kind == "shrink" else cap) - 64
    while p < lim and len(adds) < n_cmds // 2:
        ln = rng.randint(1, 24)
        adds.append((p, ln))
        p += ln + rng.randint(0, 30)
    if kind == "reversed":
        adds.reverse()
    elif kind == "overlap_batch":   # an ADD overwriting the one 5 commands before
        for k in range(10, len(adds), 97):
            d0, _ = adds[k - 5]
            adds[k] = (d0 + 1, 8)
    elif kind == "overlap_cross":   # an ADD overwriting one ~200 commands earlier
        for k in range(300, len(adds), 211):
            d0, _ = adds[k - 200]
            adds[k] = (d0, 4)
    elif kind == "shuffled_tail":   # victim-style ADDs appended out of order
        adds += [(rng.randrange(0, lim), rng.randint(1, 40)) for _ in range(40)]
    for d0, ln in adds:
        if kind == "zero" and rng.random() < 0.05:
            ln = 0
        cmds.append(dg.PlacedAdd(dst=d0, data=rng.randbytes(ln)))
    return R, cmds, vsize


def moves_case(dg, rng, kind, n):
    """(R, cmds, version_size) of one moving family over a buffer of about n bytes."""
    if kind.startswith("rotate"):
        bs = int(kind[6:])
        nb = max(n // bs, 2)
        R = rng.randbytes(nb * bs + rng.randint(0, 9))
        cmds = [dg.PlacedCopy(src=(b + 1) * bs, dst=b * bs, length=bs) for b in range(nb - 1)]   # V[b] = R[b + 1]
        cmds.append(dg.PlacedAdd(dst=(nb - 1) * bs, data=R[:bs]))
        return R, cmds, len(R)
    R = rng.randbytes(n)
    if kind.startswith("shift_fwd"):    # V = R[k:] + tail: dst < src, overlapping
        k = int(kind[9:])
        return R, [dg.PlacedCopy(src=k, dst=0, length=n - k), dg.PlacedAdd(dst=n - k, data=rng.randbytes(k))], n
    if kind.startswith("shift_back"):   # V = head + R[:-k]: dst > src, overlapping
        k = int(kind[10:])
        return R, [dg.PlacedCopy(src=0, dst=k, length=n - k), dg.PlacedAdd(dst=0, data=rng.randbytes(k))], n
    assert kind == "swap"               # neighbours a, b: b's bytes saved in an ADD, a copied over b, the ADD over a
    cmds, pos = [], 0
    while pos + 2 * 40 < n:
        ln = rng.randint(1, 40)
        if rng.random() < 0.5:
            cmds.append(dg.PlacedCopy(src=pos, dst=pos + ln, length=ln))
            cmds.append(dg.PlacedAdd(dst=pos, data=R[pos + ln:pos + 2 * ln]))
        else:
            cmds.append(dg.PlacedCopy(src=pos, dst=pos, length=2 * ln))
        pos += 2 * ln + rng.randint(0, 7)
    return R, cmds, n


def pad_noops(dg, rng, cmds, n_r, count):
    """`count` COPYs of a range onto itself in front of cmds: they write nothing
    and read nothing, and make the stream 13 bytes longer each."""
    pre = []
    for _ in range(count):
        ln = rng.randint(1, 40)
        at = rng.randrange(0, max(n_r - ln, 1))
        pre.append(dg.PlacedCopy(src=at, dst=at, length=min(ln, n_r - at)))
    return pre + cmds


def make_delta(dg, orc, R, cmds, vsize):
    """(in-place delta of cmds with the CRCs the oracle's replay implies, V)."""
    z = b"\0" * 8
    d0 = dg.encode_delta(cmds, inplace=True, version_size=vsize, src_crc=z, dst_crc=z)
    rc, V = orc.decode(R, d0, ignore_hash=True)
    assert rc == 0 and len(V) == vsize
    d = dg.encode_delta(cmds, inplace=True, version_size=vsize, src_crc=orc.crc64_xz(R), dst_crc=orc.crc64_xz(V))
    return d, V


def version_size(d):
    return int.from_bytes(d[5:9], "big") if len(d) >= 25 else 0


def commands_at(d):
    """[(offset, type, header bytes, payload bytes)] of a well-formed stream, END last."""
    out, x = [], 25
    while x < len(d):
        t = d[x]
        if t == 0:
            out.append((x, 0, 1, 0))
            break
        hdr = 13 if t == 1 else 9
        pay = 0 if t == 1 else int.from_bytes(d[x + 5:x + 9], "big")
        out.append((x, t, hdr, pay))
        x += hdr + pay
    return out


def three_window_stream(dg, orc, rng):
    """(R, delta, V): a c5-shaped stream of three parse windows whose last command
    before END is a COPY of a range onto itself (a COPY in the last window)."""
    R, cmds, vsize = order_case(dg, rng, "c5_shape", n_r=20000, n_cmds=600)
    cmds.append(dg.PlacedCopy(src=19000, dst=19000, length=500))
    d, V = make_delta(dg, orc, R, cmds, vsize)
    assert 2 * WINDOW + 25 < len(d) <= 3 * WINDOW, len(d)
    return R, d, V


DAMAGES = ["cut_window1", "cut_window3", "cut_last_payload", "unknown_window3", "copy_src_past", "add_dst_past",
           "bad_magic", "flag_cleared", "cap_short", "src_crc"]
# the damages decode calls malformed too: the status must be decode's
DECODE_AGREES = DAMAGES[:7]


def damage(d, R, how):
    """(damaged stream, buf_cap or None for the exact one, expected status)."""
    cm = commands_at(d)
    bsz = max(len(R), version_size(d))
    b = bytearray(d)
    in_w1 = next(c for c in cm if c[0] > 2000)
    in_w3 = next(c for c in cm if c[0] > 2 * WINDOW + 600)
    if how == "cut_window1":          # three bytes into a command header
        return bytes(b[:in_w1[0] + 3]), None, 8
    if how == "cut_window3":
        return bytes(b[:in_w3[0] + 3]), None, 8
    if how == "cut_last_payload":     # the last ADD loses its last payload byte (and what follows it)
        x, _, hdr, pay = [c for c in cm if c[1] == 2 and c[3] >= 2][-1]
        assert x > 2 * WINDOW + 25
        return bytes(b[:x + hdr + pay - 1]), None, 8
    if how == "unknown_window3":
        b[in_w3[0]] = 7
        return bytes(b), None, 8
    if how == "copy_src_past":        # the last COPY (in the last window) reads one byte past bsz
        x, _, _, _ = [c for c in cm if c[1] == 1][-1]
        assert x > 2 * WINDOW + 25
        ln = int.from_bytes(b[x + 9:x + 13], "big")
        b[x + 1:x + 5] = (bsz - ln + 1).to_bytes(4, "big")
        return bytes(b), None, 8
    if how == "add_dst_past":
        x, _, _, pay = [c for c in cm if c[1] == 2 and c[3] >= 2][-1]
        b[x + 1:x + 5] = (bsz - pay + 1).to_bytes(4, "big")
        return bytes(b), None, 8
    if how == "bad_magic":
        b[0] ^= 1
        return bytes(b), None, 8
    if how == "flag_cleared":         # a well-formed standard delta
        b[4] = 0
        return bytes(b), None, 2
    if how == "cap_short":
        return bytes(b), bsz - 1, 7
    assert how == "src_crc"
    b[9] ^= 0x40
    return bytes(b), None, 9
