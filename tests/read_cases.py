"""Inputs of tests/test_read_cpu.py, tests/test_read_sanitize_cpu.py and
tests/test_gpu_read.py, and the Python model of a range read.

The model is the reference's replay (src/c/apply.c:229-249), sliced: a zeroed
buffer of version_size bytes, the commands in stream order, later writes over
earlier ones; a read of (off, length) is bytes [off, off + n) of it with
n = 0 if off >= version_size else min(length, version_size - off).  It parses
the stream itself and reports the statuses of include/delta_gpu.h.

A case is (name, R, delta, status): status 0 for every stream that must be
served, the expected failure otherwise.  Nothing here needs a GPU.
"""
from __future__ import annotations

import random
import struct

import encode_plan_cases as epc
import window_cases as wc

OK, INVALID_ARG, UNSUPPORTED, MALFORMED = 0, 1, 2, 8
STRIDE = 1024   # stream bytes per index entry (csrc/dg_read_dev.h)
WINDOW = 4096   # stream bytes per parse window of the read kernels


# ── streams from command lists: ("C", src, dst, len) or ("A", dst, bytes), in stream order ──

def stream(orc, R, cmds, *, version_size, end=True, flags=0):
    out = bytearray(b"DLT\x03" + bytes([flags]) + struct.pack(">I", version_size))
    _, V = replay(R, cmds, version_size)
    out += orc.crc64_xz(R) + orc.crc64_xz(V)
    for c in cmds:
        if c[0] == "C":
            out += b"\x01" + struct.pack(">III", c[1], c[2], c[3])
        else:
            out += b"\x02" + struct.pack(">II", c[1], len(c[2])) + c[2]
    if end:
        out += b"\x00"
    return bytes(out)


def replay(R, cmds, version_size):
    """(ok, V): the commands over zeros; not ok when one leaves V or R."""
    V = bytearray(version_size)
    for c in cmds:
        if c[0] == "C":
            _, src, dst, n = c
            if src + n > len(R) or dst + n > version_size:
                return False, bytes(V)
            V[dst:dst + n] = R[src:src + n]
        else:
            _, dst, data = c
            if dst + len(data) > version_size:
                return False, bytes(V)
            V[dst:dst + len(data)] = data
    return True, bytes(V)


def sequential(cmds):
    """("C", src, len) / ("A", bytes) placed one after the other."""
    out, dst = [], 0
    for c in cmds:
        if c[0] == "C":
            out.append(("C", c[1], dst, c[2]))
            dst += c[2]
        else:
            out.append(("A", dst, bytes(c[1])))
            dst += len(c[1])
    return out, dst


# ── the model ──

def parse(R_len, delta):
    """(status, version_size, [(stream offset, kind, src or payload offset, dst, len)])."""
    if len(delta) < 25 or delta[:4] != b"DLT\x03":
        return MALFORMED, 0, []
    if delta[4] & 1:
        return UNSUPPORTED, 0, []
    vs = struct.unpack(">I", delta[5:9])[0]
    pos, cmds = 25, []
    while pos < len(delta):
        t = delta[pos]
        if t == 0:
            break
        if t == 1:
            if pos + 13 > len(delta):
                return MALFORMED, vs, []
            src, dst, n = struct.unpack(">III", delta[pos + 1:pos + 13])
            if src + n > R_len or dst + n > vs:
                return MALFORMED, vs, []
            cmds.append((pos, 1, src, dst, n))
            pos += 13
        elif t == 2:
            if pos + 9 > len(delta):
                return MALFORMED, vs, []
            dst, n = struct.unpack(">II", delta[pos + 1:pos + 9])
            if pos + 9 + n > len(delta) or dst + n > vs:
                return MALFORMED, vs, []
            cmds.append((pos, 2, pos + 9, dst, n))
            pos += 9 + n
        else:
            return MALFORMED, vs, []
    return OK, vs, cmds


def model_version(R, delta):
    """(status, V, commands): the whole replay."""
    st, vs, cmds = parse(len(R), delta)
    if st:
        return st, None, []
    V = bytearray(vs)
    for _, kind, s, dst, n in cmds:
        V[dst:dst + n] = R[s:s + n] if kind == 1 else delta[s:s + n]
    return OK, bytes(V), cmds


def model_read(V, off, length):
    n = 0 if off >= len(V) else min(length, len(V) - off)
    return V[off:off + n]


# ── ranges ──

def ranges(V, cmds, delta_len):
    """The (off, length) list of a stream: around command boundaries of V (the
    first and last 10, and the commands nearest each multiple of 1024 and 4096
    stream bytes, 40 at the most), the edges of V, and 64 ranges that tile V."""
    vs = len(V)
    bs = [c[3] for c in cmds[:10]] + [c[3] for c in cmds[-10:]]
    if cmds:
        for m in list(range(WINDOW, delta_len, WINDOW)) + list(range(STRIDE, delta_len, STRIDE)):
            bs.append(min(cmds, key=lambda c: abs(c[0] - m))[3])
    seen, bl = set(), []
    for b in bs:
        if b not in seen and len(bl) < 40:
            seen.add(b)
            bl.append(b)
    out = []
    for b in bl:
        for o, n in ((b - 1, 2), (b, 1), (b, 15), (b, 16), (b, 17), (b - 17, 34)):
            out.append((max(o, 0), n))
    out += [(0, vs), (0, 0), (max(vs - 1, 0), 1), (vs, 5), (max(vs - 3, 0), 10), (0xFFFFFFFF, 0xFFFFFFFF)]
    return out + tiling(vs)


def tiling(vs, parts=64):
    cuts = [vs * k // parts for k in range(parts + 1)]
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]


# ── the corpus ──

def encoder_cases(orc):
    import oracle as O
    out = []
    R, V = orc.synth_pair(0x5EAD0001, 64 << 10, 655)   # 1 % edits: about 13 KiB of stream, 4 windows
    out.append(("onepass_1pct", R, orc.encode(O.ONEPASS, R, V, p=16, q=1), OK))
    R, V = epc.dense_pair(random.Random(71), epc.DENSE_STEP, n=epc.DENSE_MIN)   # an edit every 24 bytes
    out.append(("onepass_dense24", R, orc.encode(O.ONEPASS, R, V, p=16, q=1), OK))
    R, V = orc.synth_transpose(0x5EAD0002, 24, 600)
    out.append(("correcting_transpose", R, orc.encode(O.CORRECTING, R, V, p=16, q=1), OK))
    return out


def long_add_case(orc):
    rng = random.Random(72)
    R = rng.randbytes(900)
    cmds, vs = sequential([("C", 10, 300), ("A", rng.randbytes(20000)), ("C", 400, 200), ("C", 0, 77)])
    return [("long_add", R, stream(orc, R, cmds, version_size=vs), OK)]


def nonsequential_cases(orc):
    rng = random.Random(73)
    R = rng.randbytes(2000)
    lit = rng.randbytes
    out = []
    base, vs = sequential([("C", 100, 60), ("A", lit(33)), ("C", 0, 90), ("A", lit(5)), ("C", 700, 400)])
    sw = [base[1], base[0]] + base[2:]
    out.append(("exchanged", R, stream(orc, R, sw, version_size=vs), OK))
    out.append(("descending", R, stream(orc, R, base[::-1], version_size=vs), OK))
    ov = [("A", 0, lit(100)), ("C", 5, 50, 100), ("A", 120, lit(30)), ("C", 900, 40, 20), ("A", 45, lit(10))]
    out.append(("overlapping", R, stream(orc, R, ov, version_size=150), OK))
    out.append(("gap", R, stream(orc, R, [("C", 0, 0, 40), ("A", 100, lit(20))], version_size=150), OK))
    out.append(("nothing_written", R, stream(orc, R, [], version_size=70), OK))
    zl = [("C", 7, 0, 0), ("C", 0, 0, 30), ("A", 30, b""), ("C", 30, 30, 30), ("C", 99, 60, 0), ("A", 60, lit(5)),
          ("A", 65, b"")]
    out.append(("zero_lengths_in_sequence", R, stream(orc, R, zl, version_size=65), OK))
    zo = [("C", 0, 0, 30), ("A", 5, b""), ("C", 30, 30, 35), ("C", 1, 65, 0)]
    out.append(("zero_length_out_of_sequence", R, stream(orc, R, zo, version_size=65), OK))
    # several windows of commands: 700 short ones, then with two exchanged, reversed, and with every tenth written twice
    many, vm = sequential([("C", rng.randrange(0, 1900), rng.randint(1, 40)) if k % 3 else ("A", lit(rng.randint(1, 25)))
                           for k in range(700)])
    out.append(("many_in_sequence", R, stream(orc, R, many, version_size=vm), OK))
    out.append(("many_exchanged", R, stream(orc, R, [many[1], many[0]] + many[2:], version_size=vm), OK))
    out.append(("many_descending", R, stream(orc, R, many[::-1], version_size=vm), OK))
    twice = []
    for k, c in enumerate(many):
        if k % 10 == 0 and c[0] == "C":
            twice.append(("A", c[2], lit(c[3])))   # overwritten by the command itself
        twice.append(c)
        if k % 97 == 0 and k:
            twice.append(("A", many[k - 1][2] if many[k - 1][0] == "C" else many[k - 1][1], lit(1)))   # over an earlier one
    out.append(("many_overlapping", R, stream(orc, R, twice, version_size=vm), OK))
    return out


def edge_cases(orc):
    rng = random.Random(74)
    R = rng.randbytes(300)
    cmds, vs = sequential([("C", 10, 50), ("A", rng.randbytes(30)), ("C", 200, 40)])
    return [
        ("version_size_0", R, stream(orc, R, [("C", 5, 0, 0)], version_size=0), OK),
        ("end_only", R, stream(orc, R, [], version_size=0), OK),
        ("end_only_empty_r", b"", stream(orc, b"", [], version_size=0), OK),
        ("missing_end", R, stream(orc, R, cmds, version_size=vs, end=False), OK),
        ("header_only", R, stream(orc, R, [], version_size=0, end=False), OK),
    ]


def damaged_cases(orc):
    rng = random.Random(75)
    R = rng.randbytes(300)
    cmds, vs = sequential([("C", 10, 50), ("A", rng.randbytes(30)), ("C", 200, 40)])
    d = stream(orc, R, cmds, version_size=vs)

    def patch(at, val):
        return d[:at] + bytes(val) + d[at + len(val):]

    past_r, vp = sequential([("C", 10, 50), ("C", len(R) - 49, 50)])
    return [
        ("truncated_header", R, d[:24], MALFORMED),
        ("empty", R, b"", MALFORMED),
        ("bad_magic", R, patch(0, b"X"), MALFORMED),
        ("unknown_command", R, patch(25 + 13, b"\x07"), MALFORMED),
        ("payload_past_end", R, d[:25 + 13 + 9 + 4], MALFORMED),
        ("copy_header_cut", R, d[:25 + 13 + 9 + 30 + 6], MALFORMED),
        ("dst_past_version", R, patch(5, struct.pack(">I", vs - 1)), MALFORMED),
        ("copy_past_ref", R, stream(orc, R + b"\0", past_r, version_size=vp), MALFORMED),
        ("inplace_flag", R, patch(4, b"\x01"), UNSUPPORTED),
        ("inplace_flag_and_damage", R, patch(4, b"\x01")[:25 + 13 + 9 + 4], UNSUPPORTED),
    ]


_cache = {}


def corpus(dg, orc):
    """Every case, built once per session; each damaged stream between good neighbours."""
    if "all" not in _cache:
        good = encoder_cases(orc) + long_add_case(orc) + nonsequential_cases(orc) + edge_cases(orc)
        good += [(n, R, d, OK) for n, R, _, d, _ in wc.standard_cases(dg, orc)]
        bad = damaged_cases(orc)
        out = []
        for k, c in enumerate(good):
            out.append(c)
            if k < len(bad):
                out.append(bad[k])
        _cache["all"] = out
    return _cache["all"]


def with_ranges(dg, orc):
    """[(name, R, delta, status, V or None, [(off, length)])] over the corpus."""
    if "ranges" not in _cache:
        out = []
        for name, R, d, st in corpus(dg, orc):
            mst, V, cmds = model_version(R, d)
            assert mst == st, (name, mst, st)
            rs = ranges(V, cmds, len(d)) if st == OK else [(0, 16), (3, 1), (0, 0)]
            out.append((name, R, d, st, V, rs))
        _cache["ranges"] = out
    return _cache["ranges"]
