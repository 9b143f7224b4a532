"""Inputs of tests/test_index_model_cpu.py, tests/test_gpu_index_chunked.py and
tests/test_gpu_decode_large.py, and two Python models of a stream's index
(csrc/dg_read_dev.h): the one-block pass's and the chunked pass's.

An index is (head, entries): head = dict(status, vsize, seq, n_ent, dl) as the
32-byte head holds them, entries = [(stream offset, dst)] * n_ent for a stream
whose status is 0 and [] otherwise (a failed stream's entries are unspecified).

serial_index states what dg_read_index_kernel leaves, from read_cases.parse.
chunked_index restates the three stages of csrc/dg_index_dev.hip: exit for
every offset of every chunk (framing only), the walk over the chunks, and the
per-chunk fill from the chunk's true entry with the stride rule.  Both must
agree on every stream; the streams below are made to sit badly on chunk edges.

A case is (name, R, delta, status) as in read_cases.  Nothing here needs a GPU.
"""
from __future__ import annotations

import random
import struct

import read_cases as rc

OK, UNSUPPORTED, MALFORMED = rc.OK, rc.UNSUPPORTED, rc.MALFORMED
STRIDE = rc.STRIDE
CHUNK = 4096          # the chunk size the streams are laid out for
END, BAD = 0xFFFFFFFF, 0xFFFFFFFE   # exit codes (csrc/dg_index_dev.h)
NONE = 0xFFFFFFFF     # dst of an entry after the last command


# ── the one-block pass ──

def _early(delta):
    """The statuses taken before parsing: (status, vsize)."""
    if len(delta) < 25 or delta[:4] != b"DLT\x03":
        return MALFORMED, 0
    if delta[4] & 1:
        return UNSUPPORTED, 0
    return OK, struct.unpack(">I", delta[5:9])[0]


def _head(st, vs, seq, n_ent, dl):
    return dict(status=st, vsize=vs, seq=int(bool(seq) and not st), n_ent=n_ent, dl=0 if st else dl)


def serial_index(ref_len, delta):
    dl = len(delta)
    est, vs = _early(delta)
    if est:
        return _head(est, 0, 0, 0, dl), []
    n_ent = dl // STRIDE + 1
    st, _, cmds = rc.parse(ref_len, delta)
    if st:
        return _head(st, vs, 0, n_ent, dl), []
    ents, j = [], 0
    for k in range(n_ent):
        while j < len(cmds) and cmds[j][0] < STRIDE * k:
            j += 1
        ents.append((cmds[j][0], cmds[j][3]) if j < len(cmds) else (dl, NONE))
    seq, run_end = True, 0
    for _, _, _, dst, n in cmds:
        seq = seq and dst == run_end
        run_end = dst + n
    return _head(OK, vs, seq and run_end == vs, n_ent, dl), ents


# ── the chunked pass ──

def exit_table(delta, chunk_bytes):
    """exit[x] for every stream offset: where the chain that starts at x leaves
    x's chunk (the first command at or after the chunk's end; len(delta) when it
    runs off the stream), END or BAD.  Framing only: type byte, header complete,
    payload inside the stream."""
    dl = len(delta)
    ex = [BAD] * dl
    for c0 in range(0, dl, chunk_bytes):
        c1 = min(c0 + chunk_bytes, dl)
        for x in range(c1 - 1, c0 - 1, -1):
            t = delta[x]
            if t > 2:
                continue
            if t == 0:
                ex[x] = END
                continue
            hdr = 13 if t == 1 else 9
            if x + hdr > dl:
                continue
            end = x + hdr + (0 if t == 1 else struct.unpack(">I", delta[x + 5:x + 9])[0])
            if end > dl:
                continue
            ex[x] = end if end >= c1 else ex[end]
    return ex


def walk(delta, ex, chunk_bytes):
    """Per chunk (entry, live), and whether the chain meets bad framing."""
    dl = len(delta)
    nch = max(1, -(-dl // chunk_bytes))
    cur, mode, out = 25, 0, []
    if cur >= dl:
        mode = 1
    for k in range(nch):
        c0, cend = k * chunk_bytes, (k + 1) * chunk_bytes
        live = mode == 0 and c0 < dl
        out.append((cur if live else dl, live))
        if live and cur < cend:
            nx = ex[cur]
            if nx == END:
                mode = 1
            elif nx == BAD:
                mode = 2
            else:
                cur = nx
                if cur >= dl:
                    mode = 1
    return out, mode == 2


def _command(ref_len, delta, vs, pos):
    """The real window step on one command at pos < len(delta): ("end",), ("bad",) or (next pos, dst, len)."""
    dl = len(delta)
    t = delta[pos]
    if t == 0:
        return ("end",)
    if t == 1:
        if pos + 13 > dl:
            return ("bad",)
        src, dst, n = struct.unpack(">III", delta[pos + 1:pos + 13])
        if src + n > ref_len or dst + n > vs:
            return ("bad",)
        return pos + 13, dst, n
    if t == 2:
        if pos + 9 > dl:
            return ("bad",)
        dst, n = struct.unpack(">II", delta[pos + 1:pos + 9])
        if pos + 9 + n > dl or dst + n > vs:
            return ("bad",)
        return pos + 9 + n, dst, n
    return ("bad",)


def fill(ref_len, delta, vs, chunk_bytes, k, entry, live, ents):
    """Chunk k writes the entries whose strides lie in it; returns (failed, any, first dst, last end, break inside)."""
    dl = len(delta)
    c0, cend = k * chunk_bytes, (k + 1) * chunk_bytes
    n_ent = dl // STRIDE + 1
    klo = c0 // STRIDE
    khi = n_ent - 1 if cend >= dl else cend // STRIDE - 1
    nxt = klo            # the next stride to write
    any_own, first, run_end, brk = False, 0, 0, False
    pos = entry
    while live and pos < dl:
        c = _command(ref_len, delta, vs, pos)
        if c == ("bad",):
            return (True, any_own, first, run_end, brk)
        if c == ("end",):
            break
        # the command is the first at or after every stride up to its own
        while nxt <= min(pos // STRIDE, khi):
            ents[nxt] = (pos, c[1])
            nxt += 1
        if pos >= cend:
            break        # it starts in a later chunk: that chunk's own
        if any_own and c[1] != run_end:
            brk = True
        if not any_own:
            first = c[1]
        any_own, run_end = True, c[1] + c[2]
        pos = c[0]
    while nxt <= khi:
        ents[nxt] = (dl, NONE)
        nxt += 1
    return (False, any_own, first, run_end, brk)


def chunked_index(ref_len, delta, chunk_bytes):
    dl = len(delta)
    est, vs = _early(delta)
    if est:
        return _head(est, 0, 0, 0, dl), []
    n_ent = dl // STRIDE + 1
    ex = exit_table(delta, chunk_bytes)
    chunks, walk_bad = walk(delta, ex, chunk_bytes)
    ents = [None] * n_ent
    recs = []
    for k, (entry, live) in enumerate(chunks):
        if k * chunk_bytes < dl:
            recs.append((live, fill(ref_len, delta, vs, chunk_bytes, k, entry, live, ents)))
    failed = walk_bad or any(live and r[0] for live, r in recs)
    if failed:
        return _head(MALFORMED, vs, 0, n_ent, dl), []
    seq, run_end = True, 0
    for live, (_, any_own, first, last_end, brk) in recs:
        if live and any_own:
            seq = seq and not brk and first == run_end
            run_end = last_end
    assert None not in ents, "a stride no chunk wrote"
    return _head(OK, vs, seq and run_end == vs, n_ent, dl), ents


# ── the index as dg_read_plan_index_get returns it ──

def unpack_index(raw):
    doff, dl, vsize, status, flags, n_ent, _ = struct.unpack("<QIIiIII", raw[:32])
    ents = [struct.unpack("<II", raw[32 + 8 * k:40 + 8 * k]) for k in range((len(raw) - 32) // 8)]
    return dict(status=status, vsize=vsize, seq=flags & 1, n_ent=n_ent, dl=dl), ents, doff


# ── the streams ──

def _tail(rng, n, rlen=3000):
    """n short commands: two COPYs, then an ADD, and so on."""
    return [("C", rng.randrange(0, rlen - 100), rng.randint(1, 40)) if k % 3 else ("A", rng.randbytes(rng.randint(1, 25)))
            for k in range(n)]


def _payload(rng, n):
    """n bytes none of which is a command type."""
    return bytes(rng.randrange(3, 256) for _ in range(n))


FAKES = {
    "end": b"\x00",
    "copy_out_of_bounds": b"\x01" + struct.pack(">III", 0xFFFFFF00, 0, 0x1000),
    "add_past_stream": b"\x02" + struct.pack(">II", 0, 0x7FFFFFFF),
    "zero_adds": (b"\x02" + struct.pack(">II", 0, 0)) * 6,
}


def fake_command_cases(orc):
    """One ADD payload across two chunk edges; at each edge the payload spells a fake command."""
    rng = random.Random(81)
    R = rng.randbytes(3000)
    out = []
    for a, b in (("end", "copy_out_of_bounds"), ("add_past_stream", "zero_adds"), ("zero_adds", "end"),
                 ("copy_out_of_bounds", "add_past_stream")):
        head = [("C", 10, 300), ("A", rng.randbytes(40))]
        p0 = 25 + 13 + 9 + 40 + 9          # the long payload's first stream offset
        pay = bytearray(_payload(rng, 9500))
        for edge, kind in ((CHUNK, a), (2 * CHUNK, b)):
            f = FAKES[kind]
            pay[edge - p0:edge - p0 + len(f)] = f
        cmds, vs = rc.sequential(head + [("A", bytes(pay))] + _tail(rng, 60))
        d = rc.stream(orc, R, cmds, version_size=vs)
        assert p0 < CHUNK and p0 + len(pay) > 2 * CHUNK + 64
        out.append((f"fake_{a}_then_{b}", R, d, OK))
    return out


def filled_payload_cases(orc):
    rng = random.Random(82)
    R = rng.randbytes(3000)
    out = []
    for b in (0, 1, 2):
        cmds, vs = rc.sequential([("C", 5, 100), ("A", bytes([b]) * 10000), ("C", 700, 50)] + _tail(rng, 40))
        out.append((f"payload_all_{b:02x}", R, rc.stream(orc, R, cmds, version_size=vs), OK))
    return out


def _shifted(orc, rng, R, first_at, body, **kw):
    """A leading ADD of the length that puts the next command at stream offset first_at, then body."""
    lead = first_at - 25 - 9
    cmds, vs = rc.sequential([("A", _payload(rng, lead))] + body)
    d = rc.stream(orc, R, cmds, version_size=vs, **kw)
    assert rc.parse(len(R), d)[2][1][0] == first_at
    return d


def edge_placement_cases(orc):
    rng = random.Random(83)
    R = rng.randbytes(3000)
    out = []
    body = [("C", 100, 77)] + _tail(rng, 600)
    out.append(("command_at_chunk_edge", R, _shifted(orc, rng, R, CHUNK, body), OK))
    for i in range(1, 13):   # a COPY header with i of its 13 bytes before the edge
        out.append((f"copy_header_cut_at_{i}", R, _shifted(orc, rng, R, CHUNK - i, body), OK))
    # (at chunk_bytes 8192 the edge at 4096 is a window edge inside chunk 0)
    out.append(("copy_header_cut_by_window_edge", R, _shifted(orc, rng, R, CHUNK - 5, [("C", 3, 9)] + _tail(rng, 900)), OK))
    add_body = [("A", rng.randbytes(30))] + _tail(rng, 500)
    for i in (1, 4, 8):
        out.append((f"add_header_cut_at_{i}", R, _shifted(orc, rng, R, 2 * CHUNK - i, add_body), OK))
    return out


def end_and_length_cases(orc):
    rng = random.Random(84)
    R = rng.randbytes(3000)
    out = []
    cmds, vs = rc.sequential(_tail(rng, 300))
    d = rc.stream(orc, R, cmds, version_size=vs)
    assert CHUNK < len(d) < 2 * CHUNK
    d = bytearray(d + rng.randbytes(5 * CHUNK + 300 - len(d)))   # garbage after END, malformed commands on the later edges
    d[2 * CHUNK:2 * CHUNK + 9] = FAKES["add_past_stream"]
    d[3 * CHUNK + 7:3 * CHUNK + 20] = FAKES["copy_out_of_bounds"]
    d[4 * CHUNK] = 7
    out.append(("end_in_chunk_1_then_garbage", R, bytes(d), OK))
    cmds, vs = rc.sequential(_tail(rng, 800))
    out.append(("missing_end_many_chunks", R, rc.stream(orc, R, cmds, version_size=vs, end=False), OK))
    out.append(("stream_of_25_bytes", R, rc.stream(orc, R, [], version_size=0, end=False), OK))
    # exactly one chunk: the last ADD's length makes the stream 4096 bytes
    body = _tail(rng, 200)
    cmds, vs = rc.sequential(body)
    short = len(rc.stream(orc, R, cmds, version_size=vs))
    assert short + 9 < CHUNK
    cmds, vs = rc.sequential(body + [("A", rng.randbytes(CHUNK - short - 9))])
    d = rc.stream(orc, R, cmds, version_size=vs)
    assert len(d) == CHUNK
    out.append(("exactly_one_chunk", R, d, OK))
    cmds, vs = rc.sequential(body + [("A", rng.randbytes(2 * CHUNK - short - 9))])
    d = rc.stream(orc, R, cmds, version_size=vs, end=False)
    assert len(d) == 2 * CHUNK - 1
    out.append(("one_byte_short_of_two_chunks_no_end", R, d, OK))
    return out


def malformed_cases(orc):
    """A truly malformed command in chunk 0, in a middle chunk and in the last chunk."""
    rng = random.Random(85)
    R = rng.randbytes(3000)
    cmds, vs = rc.sequential(_tail(rng, 1100))
    d = rc.stream(orc, R, cmds, version_size=vs)
    _, _, parsed = rc.parse(len(R), d)
    nch = -(-len(d) // CHUNK)
    assert nch >= 4
    out = []

    def pick(chunk, kind):
        return next(c for c in parsed if c[0] // CHUNK == chunk and c[1] == kind and c[4] > 1 and
                    c[0] % CHUNK < CHUNK - 40)

    for where, chunk in (("chunk_0", 0), ("middle", nch // 2), ("last", nch - 1)):
        copy, add = pick(chunk, 1), pick(chunk, 2)

        def patched(at, val):
            return d[:at] + val + d[at + len(val):]

        out.append((f"bad_type_{where}", R, patched(copy[0], b"\x07"), MALFORMED))
        out.append((f"payload_past_end_{where}", R, patched(add[0] + 5, struct.pack(">I", 0x7FFFFFFF)), MALFORMED))
        out.append((f"dst_past_version_{where}", R, patched(copy[0] + 5, struct.pack(">I", vs - 1)), MALFORMED))
        out.append((f"copy_out_of_r_{where}", R, patched(copy[0] + 1, struct.pack(">I", len(R) - 1)), MALFORMED))
    return out


def nonsequential_cases(orc):
    """read_cases.nonsequential_cases' many_* families at several chunks, and a break exactly on a chunk edge."""
    rng = random.Random(86)
    R = rng.randbytes(2000)
    lit = rng.randbytes
    out = []
    many, vm = rc.sequential([("C", rng.randrange(0, 1900), rng.randint(1, 40)) if k % 3 else ("A", lit(rng.randint(1, 25)))
                              for k in range(1500)])
    out.append(("many_in_sequence_x", R, rc.stream(orc, R, many, version_size=vm), OK))
    out.append(("many_exchanged_x", R, rc.stream(orc, R, [many[1], many[0]] + many[2:], version_size=vm), OK))
    out.append(("many_exchanged_late_x", R, rc.stream(orc, R, many[:-2] + [many[-1], many[-2]], version_size=vm), OK))
    out.append(("many_descending_x", R, rc.stream(orc, R, many[::-1], version_size=vm), OK))
    twice = []
    for k, c in enumerate(many):
        if k % 10 == 0 and c[0] == "C":
            twice.append(("A", c[2], lit(c[3])))
        twice.append(c)
        if k % 97 == 0 and k:
            twice.append(("A", many[k - 1][2] if many[k - 1][0] == "C" else many[k - 1][1], lit(1)))
    out.append(("many_overlapping_x", R, rc.stream(orc, R, twice, version_size=vm), OK))
    out.append(("short_of_version_x", R, rc.stream(orc, R, many, version_size=vm + 3), OK))
    # the one break of the stream is between the last command of chunk 0 and the first of chunk 1
    lead = CHUNK - 25 - 9
    body, n = rc.sequential(_tail(rng, 500, 2000))
    gap = 5
    cmds = [("A", 0, _payload(rng, lead))] + [(c[0], c[1], c[2] + lead + gap, c[3]) if c[0] == "C" else
                                              (c[0], c[1] + lead + gap, c[2]) for c in body]
    d = rc.stream(orc, R, cmds, version_size=lead + gap + n)
    assert rc.parse(len(R), d)[2][1][0] == CHUNK
    out.append(("break_on_chunk_edge", R, d, OK))
    return out


_cache = {}


def new_cases(orc):
    """The streams of this file, each damaged one between good neighbours."""
    if "new" not in _cache:
        good = (fake_command_cases(orc) + filled_payload_cases(orc) + rc.long_add_case(orc) + edge_placement_cases(orc) +
                end_and_length_cases(orc) + nonsequential_cases(orc))
        bad = malformed_cases(orc)
        out = []
        for k, c in enumerate(good):
            out.append(c)
            if k < len(bad):
                out.append(bad[k])
        assert len(bad) < len(good)
        _cache["new"] = out
    return _cache["new"]


def all_cases(dg, orc):
    """new_cases, then read_cases.corpus unchanged."""
    if "all" not in _cache:
        _cache["all"] = new_cases(orc) + list(rc.corpus(dg, orc))
    return _cache["all"]


def models(dg, orc):
    """[(name, R, delta, status, serial_index)] over all_cases, built once."""
    if "models" not in _cache:
        _cache["models"] = [(n, R, d, st, serial_index(len(R), d)) for n, R, d, st in all_cases(dg, orc)]
    return _cache["models"]
