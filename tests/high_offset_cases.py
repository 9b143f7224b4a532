"""Command streams whose offsets and sizes sit in the upper half of the u32
range, for tests/test_high_offset_cpu.py and tests/test_gpu_high_offset.py.

The transforms are pure functions of the command streams, and a stream of 60
bytes can describe a 4 GiB version, so nothing here is large: the streams are
built with struct.pack, the one reference R is a SparseBytes, and every expected
result comes from tests/sparse_model.py (pinned to the dense models by
tests/test_sparse_model_cpu.py).  Nothing here needs a GPU or the library.

E = {2^31 - 1, 2^31, 2^31 + 1, 2^32 - 2, 2^32 - 1}.  Every operator's cases put
each of src, dst, src + len, dst + len, version_size and ref_len on every member
of E that its limits allow; reach() computes what the accepted cases reach and
ALLOWED states what they must (tests/test_high_offset_cpu.py compares the two,
so a family that silently shrinks fails).  What a limit excludes:

  * R is RLEN = 2^32 - 1 - 2^20 bytes, the largest reference the encode and
    splice plans accept (tests/test_plan_cpu.py, tests/test_splice_cpu.py), so
    wherever a stream is checked against R (read, decode, update, invert) src,
    src + len and ref_len reach 2^31 - 1, 2^31 and 2^31 + 1 only: 2^32 - 2 and
    2^32 - 1 are past R's end.
  * splice: whole.r_len and whole.v_len are below 2^32 - 2^20, so every
    quantity of a spliced delta reaches the three low members only.
  * compose never sees R: it has no ref_len.  A's src + len may reach 2^32
    itself (the contract refuses "> 2^32" only), which is pinned as accepted.
  * decode and update: versions stay below 64 KiB (one block moves and, with CRC
    checks on, checksums a whole stream, and R's CRC over 4 GiB by one block
    would take seconds: these cases run with ignore_hash), so dst, dst + len and
    version_size are small; only src, src + len and ref_len are high.

No case asks a one-block kernel to move more than 1 MiB: outputs of compose,
invert and splice carry a few KiB of literals, every read request is at most
1 MiB after clipping (checked when the corpus is built).

  * lineage: a level on R is bound as read is.  A level on another version has
    that version's size as its ref_len, up to 2^32 - 1, so its src, src + len
    and ref_len reach all of E ("inner" rows of ALLOWED): the one consumer that
    takes a COPY's end, and a work item's hi, to 0xFFFFFFFF.  No level between R
    and the requested one is ever built, on the host or the device.  Every
    request is at most 1 MiB after clipping, resolves to at most 4096 leaf
    pieces (sm.lineage_pieces) and lies at most 64 levels above R: bounds on
    work, asserted when the corpus is built.
  * inplace: the victims read R, so src, src + len and ref_len are bound as invert's are.  The expected bytes
    are the reference's own (tests/golden/golden_inplace_high.json) and dg_make_inplace's, not the model's; no
    expected output holds more than 1 MiB of victim payload under the policy it is listed for (asserted when the
    corpus is built, from the CRWI digraph of each stream), but for the capacity cases, which nothing converts.
"""
from __future__ import annotations

import random
import struct

import sparse_model as sm

OK, INVALID_ARG, UNSUPPORTED, TOO_LARGE, MALFORMED = sm.OK, sm.INVALID_ARG, sm.UNSUPPORTED, sm.TOO_LARGE, sm.MALFORMED
H = 1 << 31
U32 = 1 << 32
E = [H - 1, H, H + 1, U32 - 2, U32 - 1]
LOW = E[:3]
RLEN = U32 - 1 - (1 << 20)
WINDOW_BYTES = 64
EDGES = [1024, 4096, 65536]            # index stride / one-wave parse window, decode's window and the chunk, a large chunk
QUANTITIES = ["src", "dst", "src+len", "dst+len", "version_size", "ref_len"]
CRC_R, CRC_1, CRC_2 = b"R-crc64.", b"V1crc64.", b"V2crc64."   # nothing checks them: these cases run without CRC checks

ALLOWED = {
    "compose": {"src": E, "dst": E, "src+len": E + [U32], "dst+len": E, "version_size": E, "ref_len": []},
    "invert": {"src": LOW, "dst": E, "src+len": LOW, "dst+len": E, "version_size": E, "ref_len": LOW},
    "read": {"src": LOW, "dst": E, "src+len": LOW, "dst+len": E, "version_size": E, "ref_len": LOW},
    "inplace": {"src": LOW, "dst": E, "src+len": LOW, "dst+len": E, "version_size": E, "ref_len": LOW},
    "splice": {"src": LOW, "dst": LOW, "src+len": LOW, "dst+len": LOW, "version_size": LOW, "ref_len": LOW},
    "decode": {"src": LOW, "dst": [], "src+len": LOW, "dst+len": [], "version_size": [], "ref_len": LOW},
    "update": {"src": LOW, "dst": [], "src+len": LOW, "dst+len": [], "version_size": [], "ref_len": LOW},
    # src, src+len, ref_len: of the levels on R; "inner ...": of the levels on another version, whose ref_len is the
    # parent's version_size and so not bound by R; off, off+n: of the requests, on the requested level, n clipped
    "lineage": {"src": LOW, "dst": E, "src+len": LOW, "dst+len": E, "version_size": E, "ref_len": LOW,
                "inner src": E, "inner src+len": E, "inner ref_len": E, "off": E, "off+n": E,
                # off of a request of at least one byte on a level whose index has "nothing follows" entries
                "off beside dst 0xFFFFFFFF entries": E[:4]},
}


# ── the one reference ──

def _reference():
    rng = random.Random(0x2331)
    at = [12345, H // 2 + 7, H - 33, H + 100001, 3 * (1 << 30) + 5, RLEN - WINDOW_BYTES]
    assert all(o % 2 for o in at) and at[2] <= H - 1 and H + 1 < at[2] + WINDOW_BYTES and at[-1] + WINDOW_BYTES == RLEN
    return sm.SparseBytes(RLEN, {o: rng.randbytes(WINDOW_BYTES) for o in at})


R = _reference()


# ── streams ──

def seq(cmds, at=0):
    """("C", src, len) / ("A", bytes) placed one after the other from `at`: (placed, end)."""
    out = []
    for c in cmds:
        if c[0] == "C":
            out.append(("C", c[1], at, c[2]))
            at += c[2]
        else:
            out.append(("A", at, bytes(c[1])))
            at += len(c[1])
    return out, at


def stream(placed, version_size, *, src_crc=CRC_R, dst_crc=CRC_1, flags=0, end=True):
    """placed: ("C", src, dst, len) / ("A", dst, bytes) in stream order; fields are taken mod 2^32."""
    out = bytearray(b"DLT\x03" + bytes([flags]) + struct.pack(">I", version_size % U32) + src_crc + dst_crc)
    for c in placed:
        if c[0] == "C":
            out += b"\x01" + struct.pack(">III", c[1] % U32, c[2] % U32, c[3] % U32)
        else:
            out += b"\x02" + struct.pack(">II", c[1] % U32, len(c[2]) % U32) + c[2]
    return bytes(out + (b"\x00" if end else b""))


def sstream(cmds, **kw):
    placed, size = seq(cmds)
    return stream(placed, size, **kw)


def edges_full(rng):
    """A version of 2^32 - 1 bytes whose command boundaries are every member of E,
    closed by a zero-length COPY at dst = 0xFFFFFFFF (the value the index keeps
    for "after the last command").  Sources stay inside R."""
    cmds = [("C", 1, H - 1), ("A", rng.randbytes(1)), ("C", H, 1), ("A", rng.randbytes(1)), ("C", 5, U32 - 2 - (H + 2)),
            ("A", rng.randbytes(1)), ("C", 7, 0)]
    placed, size = seq(cmds)
    assert size == U32 - 1 and [c[1 if c[0] == "A" else 2] for c in placed] == [0, H - 1, H, H + 1, H + 2, U32 - 2, U32 - 1]
    return placed, size


def covering(rng, ref_len, target=None, n_small=420, top=H):
    """A sequentially placed stream that reads nearly all of R[0, ref_len): what
    invert needs to keep its literals small, and a fair stream for every other
    operator.  One COPY up to V offset 2^31 exactly; then n_small short commands,
    all with dst >= 2^31, COPYs of 3..9 bytes whose sources run on from 2^31 in
    shuffled order with gaps of 0..3 bytes, an ADD after some; then one COPY to
    one byte before R's end.  With target, the first command at dst 2^31 starts at
    that stream offset: 1-byte COPYs of consecutive sources (which merge) and one
    ADD pad the stream in front of the long COPY.  n_small = 1000 makes a stream
    of more than three 4 KiB chunks.  top: another V offset than 2^31 for the
    long COPY's end, for a ref_len too short for sources above 2^31."""
    n_pad, fine = 0, 3
    if target is not None:
        n_pad = (target - 47 - 1) // 13
        fine = target - 47 - 13 * n_pad
        assert 1 <= fine <= 13
    cmds = [("C", k, 1) for k in range(n_pad)] + [("A", rng.randbytes(fine)), ("C", n_pad, top - n_pad - fine)]
    at_r = top - fine                      # R is read up to here
    small = []
    for k in range(n_small):
        at_r += rng.randint(0, 3) if k % 5 else 0
        n = rng.randint(3, 9)
        small.append(("C", at_r, n))
        at_r += n
    rng.shuffle(small)
    body = []
    for k, c in enumerate(small):
        body.append(c)
        if k % 9 == 4:
            body.append(("A", rng.randbytes(rng.randint(1, 4))))
    cmds += body + [("C", at_r, ref_len - 1 - at_r)]
    placed, size = seq(cmds)
    d = stream(placed, size)
    if target is not None:
        first_high = next(k for k, c in enumerate(placed) if c[1 if c[0] == "A" else 2] >= top)
        assert len(stream(placed[:first_high], 0, end=False)) == target and placed[first_high][2] == top
    assert size < U32 and at_r < ref_len - 1
    return d, placed, size


def edge_targets():
    """Stream offsets 4 bytes before each boundary, counted from the stream's start
    (chunks, index stride) and from byte 25 (the parse windows)."""
    return [w - 4 + b for w in EDGES for b in (0, 25)]


# ── compose: (name, A, B, status) ──

def compose_cases():
    rng = random.Random(0x2332)
    out = []

    def add(name, a, b, status=OK):
        a = a if isinstance(a, bytes) else sstream(a, src_crc=CRC_R, dst_crc=CRC_1)
        b = b if isinstance(b, bytes) else sstream(b, src_crc=CRC_1, dst_crc=CRC_2)
        out.append((name, a, b, status))

    # long single commands: one COPY of A that ends at R offset 2^32 itself, read whole by B
    for e in E:
        add(f"long_copy_{e:#x}", [("C", U32 - e, e)], [("C", 0, e)])
    add("long_copy_src_fffffffe", [("C", U32 - 2, 2)], [("C", 1, 1), ("C", 0, 2)])
    add("long_copy_src_ffffffff", [("A", b"ab"), ("C", U32 - 1, 1)], [("C", 2, 1), ("C", 0, 3)])
    # B copies whole, from 1 and from a piece boundary a version whose boundaries are all of E
    pf, size = edges_full(rng)
    af = stream(pf, size, src_crc=CRC_R, dst_crc=CRC_1)
    add("edges_whole", af, [("C", 0, U32 - 1)])
    add("edges_from_1", af, [("C", 1, U32 - 2)])
    add("edges_from_boundary", af, [("A", b"x"), ("C", H - 1, H), ("C", 0, H - 2)])
    add("edges_across_each", af, [("C", e - 1, 2) for e in E[:4]] + [("C", e, 1) for e in E[:4]] + [("C", H - 2, 5)])
    # merges: pieces below 2^31 each, above it together: inside A, across commands of B, across both
    add("merge_inside_a", [("C", 0, H - 1), ("C", H - 1, 2), ("C", H + 1, H - 3)], [("C", 0, U32 - 2)])
    add("merge_across_b", [("C", 9, U32 - 10)], [("C", 0, H - 1), ("C", H - 1, 1), ("C", H, H - 10)])
    add("merge_across_both", [("C", 1, H - 1), ("C", H, H - 1)], [("C", 1, H - 2), ("C", H - 1, H - 2)])
    add("no_merge_gap_of_one", [("C", 1, H - 1), ("C", H + 1, H - 2)], [("C", 0, U32 - 3)])
    # table searches: 400 and more commands in both streams, A's pieces on both sides of V1 offset 2^31,
    # B's COPYs inside, at and across them, every dst of B's short commands above 2^31
    a_cmds = [("C", 7, H - 600)]
    for k in range(420):
        a_cmds.append(("A", rng.randbytes(rng.randint(1, 3))) if k % 4 == 3 else ("C", rng.randrange(H - 99, H + 99), rng.randint(2, 6)))
    a_cmds.append(("C", H + 500, 4000))
    pa, va = seq(a_cmds)
    bounds = [c[1 if c[0] == "A" else 2] for c in pa[1:]]
    assert bounds[0] < H < bounds[-1] and va > H + 600
    b_cmds = [("C", 0, H)]
    for k, x in enumerate(bounds):
        n = pa[1 + k][3] if pa[1 + k][0] == "C" else len(pa[1 + k][2])
        b_cmds.append([("C", x - 2, 4), ("C", x, n), ("C", x + 1, 1), ("C", x - 3, 3)][k % 4])
        if k % 50 == 49:
            b_cmds.append(("A", rng.randbytes(2)))
    add("table_search", a_cmds, b_cmds)
    assert len(a_cmds) >= 400 and len(b_cmds) >= 400
    # window and chunk edges: the first command at dst 2^31 four bytes before a boundary, as A and as B
    for t in edge_targets():
        d, _, vs = covering(rng, RLEN, target=t, n_small=1000)
        add(f"edge_{t}_as_a", d, [("C", H - 40, 90), ("C", 0, vs)])
        add(f"edge_{t}_as_b", [("C", 3, RLEN)], d[:9] + CRC_1 + CRC_2 + d[25:])
    # refusals by wrap, each the only defect of its pair
    add("a_src_len_2p32_plus_16", stream([("C", U32 - 1, 0, 17)], 17), [("C", 0, 17)], MALFORMED)
    for e in E:
        add(f"b_src_len_past_v1_{e:#x}", [("C", 0, e)], stream([("C", 1, 0, e)], e, src_crc=CRC_1, dst_crc=CRC_2), MALFORMED)
    add("b_src_len_2p32_plus_16", [("C", 0, U32 - 1)], stream([("C", U32 - 1, 0, 17)], 17, src_crc=CRC_1, dst_crc=CRC_2), MALFORMED)
    two = [("C", 0, 0, H), ("C", H, H, H)]
    add("a_sum_2p32_version_size_0", stream(two, 0), stream([], 0, src_crc=CRC_1, dst_crc=CRC_2), UNSUPPORTED)
    add("a_sum_2p32_plus_16", stream(two + [("C", 0, U32, 16)], 16), [("C", 0, 16)], UNSUPPORTED)
    add("b_sum_2p32_plus_16", [("C", 0, U32 - 1)],
        stream([("C", 0, 0, H), ("C", 0, H, H), ("C", 0, U32, 16)], 16, src_crc=CRC_1, dst_crc=CRC_2), UNSUPPORTED)
    add("a_add_dst_len_wraps", stream([("C", 0, 0, U32 - 8), ("A", U32 - 8, rng.randbytes(24))], 16), [("C", 0, 16)], UNSUPPORTED)
    return out


# ── invert: (name, ref_len, A, status), against R.head(ref_len) ──

def invert_cases():
    rng = random.Random(0x2333)
    out = []

    def add(name, ref_len, a, status=OK):
        out.append((name, ref_len, a if isinstance(a, bytes) else sstream(a), status))

    for e in LOW:
        add(f"long_copy_ref_{e:#x}", e, [("C", 0, e)])
        add(f"tail_copy_ref_{e:#x}", e, [("C", e - 1, 1), ("C", 0, e - 1)])
    add("long_copy_whole_r", RLEN, [("C", 3, RLEN - 5)])
    # V of 2^32 - 1 bytes: the second COPY is shadowed by the first and vanishes; dst and dst + len on 2^32 - 2 and 2^32 - 1
    add("version_ffffffff", RLEN, [("C", 0, RLEN), ("C", 5, (1 << 20) - 1), ("A", b"z"), ("C", 9, 0)])
    # command boundaries of V on every member of E, R covered up to its last byte (the fifth COPY is shadowed)
    add("version_fffffffe", RLEN, [("C", 0, RLEN), ("C", 5, U32 - 2 - RLEN)])
    add("edges", RLEN, [("C", 0, H - 1), ("A", b"p"), ("C", H - 1, 1), ("A", b"q"), ("C", H, RLEN - H - 1),
                        ("C", 0, U32 - 2 - (RLEN + 1)), ("A", b"r"), ("C", 7, 0)])
    # keys on both sides of 2^31, not in key order: a signed compare would put the high ones first
    add("unsorted_across_2p31", RLEN, [("C", H + 1, RLEN - H - 1), ("C", H, 1), ("C", H - 1, 1), ("C", 0, H - 1)])
    add("unsorted_equal_src", H + 1, [("C", H - 1, 1), ("C", H - 1, 2), ("C", 0, H - 1)])
    # merges: two COPYs below 2^31 each whose inverse is one COPY above it; and the same with a gap in V
    add("merge", RLEN, [("C", 0, H - 1), ("C", H - 1, RLEN - 3 - (H - 1))])
    add("no_merge_dst_gap", RLEN, [("C", 0, H - 1), ("A", b"q"), ("C", H - 1, RLEN - 3 - (H - 1))])
    # table searches and window edges
    add("table_search", RLEN, covering(rng, RLEN, n_small=520)[0])
    add("table_search_ref_2p31_plus_4000", H + 4000, covering(rng, H + 4000)[0])
    for t in edge_targets():
        add(f"edge_{t}", RLEN, covering(rng, RLEN, target=t, n_small=1000)[0])
    # refusals
    for e in LOW:
        add(f"src_len_past_ref_{e:#x}", e, stream([("C", 0, 0, e - 1), ("C", e - 1, e - 1, 2)], e + 1), MALFORMED)
    add("src_len_2p32", RLEN, stream([("C", U32 - 16, 0, 16)], 16), MALFORMED)
    add("src_len_2p32_plus_16", RLEN, stream([("C", U32 - 16, 0, 32)], 32), MALFORMED)
    two = [("C", 0, 0, H), ("C", 5, H, H)]
    add("sum_2p32_version_size_0", RLEN, stream(two, 0), UNSUPPORTED)
    add("sum_2p32_plus_16", RLEN, stream(two + [("C", 0, U32, 16)], 16), UNSUPPORTED)
    add("add_dst_len_wraps", RLEN,
        stream([("C", 0, 0, RLEN), ("C", 0, RLEN, U32 - 8 - RLEN), ("A", U32 - 8, rng.randbytes(24))], 16), UNSUPPORTED)
    return out


# ── read: (name, ref_len, delta, status, [(off, len)]) ──

def _requests(d, ref_len):
    st = sm.Stream.of(d)
    vs = st.version_size
    high = [c[2] for c in st.cmds if c[2] >= H]
    picked = high[:10] + high[-10:] + high[len(high) // 2:len(high) // 2 + 4]
    seen, rs = set(), []
    for b in picked:
        if b not in seen:
            seen.add(b)
            rs += [(max(o, 0), n) for o, n in ((b - 1, 2), (b, 1), (b, 15), (b, 16), (b, 17), (b - 17, 34))]
    rs += [(e, 40) for e in E] + [(e - 40, 81) for e in E]
    rs += [(vs, 5), (max(vs - 1, 0), 1), (max(vs - 3, 0), 10), (max(vs - 100, 0), 0xFFFFFFFF), (U32 - 5, 100), (U32 - 1, 1),
           (0xFFFFFFFF, 0xFFFFFFFF), (0, 0), (0, 64), (H - 4096, 8192)]
    for off, n in rs:   # the condition of the module docstring
        assert (0 if off >= vs else min(n, vs - off)) <= sm.SLICE_MAX
    return rs


def read_cases():
    rng = random.Random(0x2334)
    out = []

    def add(name, ref_len, d, status=OK):
        d = d if isinstance(d, bytes) else sstream(d)
        out.append((name, ref_len, d, status, _requests(d, ref_len) if status == OK else [(0, 16), (H, 1), (0, 0)]))

    pf, size = edges_full(rng)
    add("edges", RLEN, stream(pf, size))
    add("edges_add_at_ffffffff", RLEN, stream(pf[:-1] + [("A", U32 - 1, b"")], size))
    add("edges_descending", RLEN, stream(pf[::-1], size))              # not sequential: the whole-stream path
    add("edges_exchanged", RLEN, stream([pf[1], pf[0]] + pf[2:], size))
    for e in E:   # version_size on every member; the last byte an ADD
        add(f"version_{e:#x}", RLEN, [("C", 3, H - 2), ("C", 3, e - 1 - (H - 2)), ("A", rng.randbytes(1))])
    for e in LOW:
        add(f"ref_len_{e:#x}", e, [("A", rng.randbytes(2)), ("C", e - 40, 40), ("C", 0, e), ("C", e - 1, 1)])
    add("long_copy_from_window", RLEN, [("C", 3, H + 9), ("A", rng.randbytes(5)), ("C", H - 33, 100), ("C", H + 1, 7), ("C", H - 1, 2)])
    add("gap_above_2p31", RLEN, stream([("C", 0, 0, H - 10), ("A", H + 10, rng.randbytes(7)), ("C", H - 33, H + 100, 64)], U32 - 1))
    add("overwrite_above_2p31", RLEN, stream([("C", 4, 0, RLEN - 4), ("A", H - 2, rng.randbytes(5)), ("C", RLEN - 64, H, 64)], U32 - 2))
    add("table_search", RLEN, covering(rng, RLEN)[0])
    for t in edge_targets():
        add(f"edge_{t}", RLEN, covering(rng, RLEN, target=t, n_small=1000)[0])
    # refusals, each the only defect of its stream
    for e in LOW:
        add(f"src_len_past_ref_{e:#x}", e, stream([("C", e - 1, 0, 2)], 2), MALFORMED)
    add("src_len_2p32", RLEN, stream([("C", U32 - 16, 0, 16)], 16), MALFORMED)
    add("src_len_2p32_plus_16", RLEN, stream([("C", U32 - 16, 0, 32)], 32), MALFORMED)
    for e in E:
        add(f"dst_len_past_version_{e:#x}", RLEN, stream([("C", 0, e - 1, 2)], e), MALFORMED)
    add("dst_len_2p32", RLEN, stream([("C", 0, U32 - 16, 16)], U32 - 1), MALFORMED)
    add("dst_len_2p32_plus_16", RLEN, stream([("C", 0, U32 - 16, 32)], U32 - 1), MALFORMED)
    add("add_dst_len_wraps", RLEN, stream([("A", U32 - 8, rng.randbytes(24))], U32 - 1), MALFORMED)
    return out


# ── splice: (name, whole, segments, deltas, src_crc, status) ──

def _tile(v_len, n):
    cuts = [v_len * k // n for k in range(n + 1)]
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]


def splice_cases():
    rng = random.Random(0x2335)
    out = []

    def seg_stream(cmds, **kw):
        return sstream(cmds, src_crc=rng.randbytes(8), dst_crc=rng.randbytes(8), **kw)

    def add(name, whole, segs, deltas, status=OK):
        out.append((name, whole, segs, deltas, rng.randbytes(8), status))

    top = sm.PLAN_LIMIT - 1   # == RLEN: the largest r_len and v_len
    # geometry: 1, 2, 64 and 65 segments that tile a V just under the limit; every segment one COPY of its own
    # span of R through a window that is all of R, so the splice is one COPY through every seam: pieces below 2^31
    # each (from 2 segments on), 2^32 - 2^20 - 1 together; the CRC weights cover |Y| up to about 4 GiB
    for n in (1, 2, 64, 65):
        segs = [(16, top, 48 + a, b) for a, b in _tile(top, n)]
        add(f"one_copy_{n}", (16, top, 48, top), segs, [seg_stream([("C", a - 48, b)]) for _, _, a, b in segs])
    # the same through empty segments, and with a literal at one seam
    cuts = [0, 0, H - 1, H - 1, H - 1, H, H + 1, top, top]
    segs = [(0, top, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    add("one_copy_through_empty_segments", (0, top, 0, top), segs,
        [seg_stream([("C", a, b)] if b else []) for _, _, a, b in segs])
    deltas = [seg_stream([("C", a, b - 1), ("A", b"!")] if k == 1 else [("C", a, b)] if b else [])
              for k, (_, _, a, b) in enumerate(segs)]
    add("literal_at_seam_2p31", (0, top, 0, top), segs, deltas)
    # windows whose offset in R rebases a src across 2^31; neighbours that merge after rebasing and ones that do not
    segs = [(H - 10, 100, 0, 30), (H + 20, 1000, 30, 70), (H - 1, 2, 100, 2), (0, top, 102, H + 1 - 102), (H + 1, 7, H + 1, 6)]
    deltas = [seg_stream([("A", b"ab"), ("C", 2, 28)]), seg_stream([("C", 0, 60), ("C", 70, 10)]), seg_stream([("C", 0, 2)]),
              seg_stream([("C", 3, H + 1 - 102)]), seg_stream([("C", 1, 6)])]
    add("rebase_across_2p31", (0, top, 0, H + 7), segs, deltas)
    for e in LOW:   # whole.r_len, whole.v_len, a rebased src + len and dst + len on e
        segs = [(5, e - 5, 0, e - 7), (e - 2, 2, e - 7, 7)]
        add(f"ends_at_{e:#x}", (0, e, 0, e), segs, [seg_stream([("C", 0, e - 7)]), seg_stream([("A", b"12345"), ("C", 0, 2)])])
        segs = [(0, e + 9, 0, e), (e, 9, e, 4)]   # a rebased src and a dst on e; the seam's COPYs merge
        add(f"starts_at_{e:#x}", (0, e + 9, 0, e + 4), segs, [seg_stream([("A", b"xy"), ("C", 2, e - 2)]), seg_stream([("C", 0, 4)])])
    # 400 and more commands in one segment whose window starts at 2^31 - 600: every rebased src near or above 2^31
    cmds = []
    for k in range(430):
        cmds.append(("A", rng.randbytes(rng.randint(1, 3))) if k % 4 == 3 else ("C", rng.randrange(500, 700), rng.randint(2, 6)))
    _, n0 = seq(cmds)
    segs = [(0, top, 0, H - 7), (H - 600, 2000, H - 7, n0), (H + 100001, 64, H - 7 + n0, 64)]
    add("table_search_in_a_window", (0, top, 0, H - 7 + n0 + 64), segs,
        [seg_stream([("C", 0, H - 7)]), seg_stream(cmds), seg_stream([("C", 0, 64)])])
    for t in edge_targets()[:4]:   # the 1 KiB and 4 KiB edges (one wave parses a segment: no chunks)
        d, _, vs = covering(rng, RLEN, target=t, n_small=1000)
        add(f"edge_{t}", (0, top, 0, vs + 5), [(0, top, 0, vs), (RLEN - 64, 64, vs, 5)], [d, seg_stream([("C", 59, 5)])])
    # refusals: the bound of a segment's COPY is its window, seg[j].r_len
    for e in LOW:
        add(f"src_len_past_window_{e:#x}", (0, top, 0, 10), [(0, 50, 0, 4), (7, e, 4, 6)],
            [seg_stream([("C", 0, 4)]), seg_stream([("C", e - 5, 6)])], MALFORMED)
    add("src_len_2p32", (0, top, 0, 16), [(0, top, 0, 16)], [stream([("C", U32 - 16, 0, 16)], 16)], MALFORMED)
    add("src_len_2p32_plus_16", (0, top, 0, 32), [(0, top, 0, 32)], [stream([("C", U32 - 16, 0, 32)], 32)], MALFORMED)
    two = [("C", 0, 0, H), ("C", 5, H, H)]
    add("sum_2p32_version_size_0", (0, top, 0, 4), [(0, top, 0, 0), (0, 9, 0, 4)],
        [stream(two, 0), seg_stream([("C", 1, 4)])], UNSUPPORTED)
    add("sum_2p32_plus_16", (0, top, 0, 16), [(0, top, 0, 16)], [stream(two + [("C", 0, U32, 16)], 16)], UNSUPPORTED)
    add("add_dst_len_wraps", (0, top, 0, 16), [(0, top, 0, 16)],
        [stream([("C", 0, 0, RLEN), ("C", 0, RLEN, U32 - 8 - RLEN), ("A", U32 - 8, rng.randbytes(24))], 16)], UNSUPPORTED)
    add("r_len_at_the_limit", (0, top + 1, 0, 4), [(0, 9, 0, 4)], [seg_stream([("C", 1, 4)])], TOO_LARGE)
    add("v_len_at_the_limit", (0, top, 0, top + 1), [(0, top, 0, top + 1)], [seg_stream([("C", 0, top + 1)])], TOO_LARGE)
    return out


# ── decode and update: (name, ref_len, delta, status); versions of at most 64 KiB from R's windows above 2^31 ──

def _window_copies(ref_len):
    """(src, len) inside R's windows, with src and src + len on what fits of E."""
    picks = [(H - 33, 32), (H - 2, 1), (H - 1, 1), (H - 1, 2), (H, 1), (H + 1, 20), (H - 20, 40), (H + 100001, 64),
             (3 * (1 << 30) + 5, 64), (RLEN - 64, 64), (RLEN - 1, 1)]
    return [(s, n) for s, n in picks if s + n <= ref_len]


def decode_cases():
    rng = random.Random(0x2336)
    out = []
    for ref_len in LOW + [RLEN]:
        cmds = []
        for s, n in _window_copies(ref_len):
            cmds += [("C", s, n), ("A", rng.randbytes(rng.randint(1, 17)))]
        cmds.append(("C", ref_len - 9, 9))                       # src + len == ref_len
        out.append((f"windows_ref_{ref_len:#x}", ref_len, sstream(cmds), OK))
    cmds = []
    for k in range(1200):   # more than three 4 KiB windows of commands, every src in a window of R around or above 2^31
        cmds.append(("A", rng.randbytes(rng.randint(1, 9))) if k % 3 == 2 else
                    ("C", rng.choice([H - 33, H + 100001, RLEN - 64]) + rng.randrange(0, 40), rng.randint(1, 24)))
    out.append(("three_windows", RLEN, sstream(cmds), OK))
    assert len(out[-1][2]) > 3 * 4096
    placed, size = seq(cmds[:60])
    out.append(("gap_and_overwrite", RLEN, stream(placed[::-1] + [("C", RLEN - 64, 10, 64)], size + 100), OK))
    for e in LOW:
        out.append((f"src_len_past_ref_{e:#x}", e, stream([("C", H - 33, 0, 8), ("C", e - 1, 8, 2)], 10), MALFORMED))
    out.append(("src_len_2p32", RLEN, stream([("C", U32 - 16, 0, 16)], 16), MALFORMED))
    out.append(("src_len_2p32_plus_16", RLEN, stream([("C", U32 - 16, 0, 32)], 32), MALFORMED))
    out.append(("dst_len_2p32_plus_16", RLEN, stream([("C", H, U32 - 16, 32)], 16), MALFORMED))
    out.append(("add_dst_len_wraps", RLEN, stream([("A", U32 - 8, rng.randbytes(24))], 16), MALFORMED))
    assert all(sm.Stream.of(c[2]).version_size <= 65536 for c in out)
    return out


def update_cases():
    """In-place streams, hand-made: the buffer holds R (buf_cap covers it), the
    version is its first bytes.  Later COPYs read what earlier commands stored
    (memmove order), one range stays as R left it, one COPY overlaps itself."""
    rng = random.Random(0x2337)
    out = []
    for ref_len in LOW + [RLEN]:
        placed, at = [], 0
        for s, n in _window_copies(ref_len):
            placed.append(("C", s, at, n))
            at += n + 3                                          # three bytes of R (zeros) stay between them
        placed += [("C", ref_len - 9, at, 9), ("C", 5, at + 9, 40), ("C", at + 20, at + 25, 20), ("C", at + 25, at + 21, 20),
                   ("A", at + 60, rng.randbytes(11)), ("C", H - 33, 2, 3), ("C", 0, at + 71, 12)]
        out.append((f"windows_ref_{ref_len:#x}", ref_len, stream(placed, at + 90, flags=1), OK))
    placed, at = [], 0
    for k in range(1000):   # more than three 4 KiB windows: COPYs from around and above 2^31 to increasing dst, then ADDs
        n = rng.randint(1, 24)
        placed.append(("C", rng.choice([H - 33, H + 100001, RLEN - 64]) + rng.randrange(0, 40), at, n))
        at += n + rng.randint(0, 5)
    placed += [("A", rng.randrange(0, at - 9), rng.randbytes(rng.randint(1, 9))) for _ in range(40)]
    out.append(("three_windows", RLEN, stream(placed, at, flags=1), OK))
    assert len(out[-1][2]) > 3 * 4096
    # bsz = max(ref_len, version_size) bounds both dst + len and a COPY's src + len
    for e in LOW:
        out.append((f"src_len_past_bsz_{e:#x}", e, stream([("C", H - 33, 0, 8), ("C", e - 1, 8, 2)], 10, flags=1), MALFORMED))
        out.append((f"dst_len_past_bsz_{e:#x}", e, stream([("C", 0, e - 1, 2)], 10, flags=1), MALFORMED))
    out.append(("src_len_2p32", RLEN, stream([("C", U32 - 16, 0, 16)], 16, flags=1), MALFORMED))
    out.append(("src_len_2p32_plus_16", RLEN, stream([("C", U32 - 16, 0, 32)], 32, flags=1), MALFORMED))
    out.append(("dst_len_2p32_plus_16", RLEN, stream([("C", 0, U32 - 16, 32)], 16, flags=1), MALFORMED))
    out.append(("add_dst_len_wraps", RLEN, stream([("A", U32 - 8, rng.randbytes(24))], 16, flags=1), MALFORMED))
    out.append(("standard_flag", RLEN, stream([("C", H - 33, 0, 8)], 8), UNSUPPORTED))
    assert all(sm.Stream.of(c[2]).version_size <= 65536 for c in out)
    return out


# ── lineage: (name, nodes, requests, statuses) ──
#
# nodes: (ref_len or None, delta, parent or BASE, stated ref_len or None): a base level reads R.head(ref_len), any
# other the version of nodes[parent]; a stated ref_len is what a device descriptor claims instead of the parent's
# size (such a case has no host form).  requests: (node, off, length).  statuses: per node, as the contract of
# include/delta_gpu.h gives them; the model must arrive at the same ones on its own.

BASE = 0xFFFFFFFF
S = U32 - 1                  # the largest version_size, and the largest ref_len of an inner level
WORK_ITEMS = 256             # dg_lineage_work_items(): the fan-out cases overflow a stack of that many
LINEAGE_MAX_PIECES = 4096
LINEAGE_MAX_DEPTH = 64


def stated_ref_len(nodes, i):
    """What stream i's descriptor states: as lineage_cases.stated_ref_len."""
    ref_len, _, parent, stated = nodes[i]
    if stated is not None:
        return stated
    if parent == BASE:
        return ref_len
    below = sm.Stream.of(nodes[parent][1])
    return below.version_size if below.header else sm.NO_LIMIT


def lineage_path(nodes, i):
    """(ref_len of the base, [d_1 .. d_k], [stated ref_len or None per level]) of node i."""
    chain = [i]
    while nodes[chain[-1]][2] != BASE:
        chain.append(nodes[chain[-1]][2])
    chain.reverse()
    assert len(chain) <= LINEAGE_MAX_DEPTH
    return nodes[chain[0]][0], [nodes[k][1] for k in chain], [nodes[k][3] for k in chain]


def host_expressible(case):
    return all(n[3] is None for n in case[1])


_heads = {}


def r_head(ref_len):
    if ref_len not in _heads:
        _heads[ref_len] = R.head(ref_len)
    return _heads[ref_len]


def lineage_model(nodes, i, off, n):
    """(status, leaf pieces) of one request, from the sparse model."""
    ref_len, ds, stated = lineage_path(nodes, i)
    return sm.lineage_leaves(r_head(ref_len), ds, off, n, stated)


def base_tiling(e, size=S):
    """A version of `size` bytes tiled with COPYs of R.head(e): R[0, e) first (src + len == ref_len), then
    short COPYs whose src and src + len are the members of LOW that e allows, then long ones from R's first window."""
    cmds = [("C", 0, e)] + [("C", x - 7, 7) for x in LOW if x <= e] + [("C", x, min(9, e - x)) for x in LOW if x < e]
    at = seq(cmds)[1]
    while at < size:
        n = min(size - at, e - 12340)
        cmds.append(("C", 12340, n))
        at += n
    return sstream(cmds)


def shift_level(rng, k, size=S, m=3):
    """One ADD of m bytes and one long COPY: the ADD in front for even k (src + len == size - m), behind for odd
    k (src + len == size, the parent's last byte)."""
    return sstream([("A", rng.randbytes(m)), ("C", 0, size - m)] if k % 2 == 0 else [("C", m, size - m), ("A", rng.randbytes(m))])


def inner_edges(rng):
    """A version of 2^32 - 1 bytes whose COPYs put src and src + len on every member of E, against a parent of
    2^32 - 1 bytes; a zero-length COPY reads at src = 0xFFFFFFFF."""
    cmds = [("C", H - 1, 1), ("A", rng.randbytes(2)), ("C", H, 1), ("C", H + 1, 1), ("C", U32 - 2, 1), ("C", U32 - 1, 0),
            ("C", U32 - 9, 7), ("A", rng.randbytes(1)), ("C", 0, H - 1)]
    at = seq(cmds)[1]
    cmds.append(("C", H - 40, S - at))
    placed, size = seq(cmds)
    srcs, ends = {c[1] for c in placed if c[0] == "C"}, {c[1] + c[3] for c in placed if c[0] == "C"}
    assert size == S and set(E) <= srcs and set(E) <= ends and max(ends) == S
    return stream(placed, size)


def has_sentinel(d):
    """The stream's index ends with entries for "nothing follows" (stream offset, dst = 0xFFFFFFFF): a stride of
    1024 stream bytes begins after the last command's first byte."""
    at = last = 25
    for kind, _, _, n in sm.Stream.of(d).cmds:
        last = at
        at += 13 if kind == 1 else 9 + n
    return len(d) // 1024 > last // 1024


def _carried(nodes, i, memo):
    """The command boundaries of node i's version: its own, and those of the levels below carried through its COPYs."""
    if i not in memo:
        import bisect
        st = sm.Stream.of(nodes[i][1])
        out = {c[2] for c in st.cmds}
        if nodes[i][2] != BASE and st.header:
            below = _carried(nodes, nodes[i][2], memo)
            for kind, src, dst, n in st.cmds:
                if kind == 1:
                    out.update(dst + (b - src) for b in below[bisect.bisect_right(below, src):bisect.bisect_left(below, src + n)])
        memo[i] = sorted(out)
    return memo[i]


def carried_bounds(nodes, i):
    return _carried(nodes, i, {})


def _lineage_requests(nodes, i, memo, extra=()):
    """Around command boundaries of node i's version, its own and the carried ones (all of them up to 64, else
    the first few, and the first, last and middle ones at or above 2^31 - 1), on E, and at the version's edges."""
    vs = sm.Stream.of(nodes[i][1]).version_size
    bounds = _carried(nodes, i, memo)
    high = [b for b in bounds if b >= H - 1]
    picked = bounds if len(bounds) <= 64 else bounds[1:4] + high[:10] + high[-10:] + high[len(high) // 2:len(high) // 2 + 4]
    seen, rs = set(), list(extra)
    for b in picked:
        if b not in seen:
            seen.add(b)
            rs += [(max(o, 0), n) for o, n in ((b - 1, 2), (b, 1), (b, 17), (b - 17, 34))]
    rs += [(e, 40) for e in E] + [(e - 40, 81) for e in E] + [(e - 40, 40) for e in E]
    rs += [(0, 64), (vs, 5), (max(vs - 1, 0), 1), (max(vs - 3, 0), 10), (max(vs - 100, 0), 0xFFFFFFFF), (U32 - 5, 100),
           (0xFFFFFFFF, 0xFFFFFFFF), (0, 0), (H - 4096, 8192)]
    return [(i, off, n) for off, n in rs]


FAILING_REQUESTS = [(0, 16), (H, 1), (0, 0)]
LINEAGE_EXPECTED = {}   # name: per request (status, bytes, leaf pieces), from the sparse model


def lineage_cases():
    rng = random.Random(0x2339)
    out = []

    def add(name, nodes, want, statuses=None, extra=None):
        """want: the nodes that are requested; statuses: per node, OK unless stated."""
        statuses = statuses or [OK] * len(nodes)
        memo, reqs = {}, []
        for i in want:
            if statuses[i] == OK:
                reqs += _lineage_requests(nodes, i, memo, (extra or {}).get(i, ()))
            else:
                reqs += [(i, off, n) for off, n in FAILING_REQUESTS]
        out.append((name, nodes, reqs, statuses))

    def chain(ref_len, deltas):
        return [(ref_len if j == 0 else None, d, BASE if j == 0 else j - 1, None) for j, d in enumerate(deltas)]

    # tall: every level's version is 2^32 - 1 bytes, one piece per level and request
    for depth, e in zip((2, 4, 64), LOW):
        nodes = chain(e, [base_tiling(e)] + [shift_level(rng, k) for k in range(1, depth)])
        add(f"tall_{depth}", nodes, sorted({0, 1, depth // 2, depth - 1}))
    # edges at every level: the closing zero-length COPY at dst 0xFFFFFFFF below and above other levels
    pf, size = edges_full(rng)
    pg, _ = edges_full(rng)
    nodes = chain(RLEN, [base_tiling(RLEN), stream(pf, size), inner_edges(rng), shift_level(rng, 2), stream(pg, size),
                         shift_level(rng, 3), inner_edges(rng)])
    add("edges_at_every_level", nodes, range(7))
    # the index's "nothing follows" entries (dst = 0xFFFFFFFF) beside requests above 2^31: strides of bytes after
    # END, and the strides inside a last ADD's payload
    tail = sstream([("C", 0, S - 3000), ("A", rng.randbytes(3000))])
    nodes = chain(RLEN, [base_tiling(RLEN) + bytes(1500), stream(pf, size) + bytes(2100), tail, inner_edges(rng) + bytes(1024),
                         shift_level(rng, 2) + bytes(5000)])
    assert all(has_sentinel(n[1]) for n in nodes)
    add("sentinel_entries", nodes, range(5))
    # version_size, and with it the ref_len of the level above, on every member of E
    for e in E:
        mid = sstream([("C", 3, H - 2), ("C", 3, e - 1 - (H - 2)), ("A", rng.randbytes(1))])
        add(f"version_{e:#x}", chain(RLEN, [base_tiling(RLEN), mid, sstream([("A", rng.randbytes(2)), ("C", 2, e - 2)])]), [1, 2])
    # fan-out above 2^31: the first command at dst 2^31 on an index stride, a window edge, a chunk edge; node 1 is
    # requested (its COPYs are children one level down) and node 2 reads through it (children of a child)
    for t, n_small in ((EDGES[0], 420), (EDGES[1], 1000), (EDGES[2], 420), (25 + EDGES[1], 1000)):
        d, _, vs = covering(rng, S, target=t, n_small=n_small)
        nodes = chain(RLEN, [base_tiling(RLEN), d, shift_level(rng, 2, size=vs), shift_level(rng, 3, size=vs)])
        wide = [(H - 40, 8192), (H, 8192), (H + 3, 1 << 14)]
        add(f"fanout_{t}_{n_small}", nodes, [1, 2, 3], extra={1: wide, 2: wide, 3: wide})
    # inner ref_len at the limit
    top_s = sstream([("C", S - 1, 1), ("A", rng.randbytes(2)), ("C", 0, S - 3)])           # src + len == ref_len == 2^32 - 1
    add("limit_served", chain(RLEN, [base_tiling(RLEN), top_s, sstream([("C", S - 2, 2), ("C", 0, S - 2)])]), [1, 2])
    faulty = stream([("C", U32 - 16, 0, 16)], 16)                                          # src + len == 2^32
    up16 = sstream([("C", 8, 8), ("C", 0, 8)])
    add("limit_2p32_at1", chain(RLEN, [faulty, up16, up16]), [0, 1, 2], [MALFORMED] * 3)
    add("limit_2p32_at2", chain(RLEN, [base_tiling(RLEN), faulty, up16]), [0, 1, 2], [OK, MALFORMED, MALFORMED])
    add("limit_2p32_at3", chain(RLEN, [base_tiling(RLEN), shift_level(rng, 1), faulty]), [0, 1, 2], [OK, OK, MALFORMED])
    add("limit_src_ffffffff_len_1", chain(RLEN, [base_tiling(RLEN), stream([("C", U32 - 1, 0, 1)], 1)]), [1], [OK, MALFORMED])
    unordered = stream([("C", 0, 8, 8), ("C", 8, 0, 8)], 16)                               # valid, not sequential
    add("limit_unordered_above_2p32", chain(RLEN, [base_tiling(RLEN), faulty, unordered]), [2], [OK, MALFORMED, UNSUPPORTED])
    add("limit_2p32_above_unordered", chain(RLEN, [sstream([("C", H - 8, 16)]), unordered, faulty]), [1, 2],
        [OK, UNSUPPORTED, MALFORMED])
    short = sstream([("A", rng.randbytes(2)), ("C", 0, S - 3)])                            # a version of 2^32 - 2 bytes
    nodes = chain(RLEN, [base_tiling(RLEN), short, shift_level(rng, 1, size=S - 1)])
    nodes[1] = nodes[1][:3] + (S - 1,)                                                     # the parent has 2^32 - 1
    add("limit_stated_one_below", nodes, [0, 1, 2], [OK, INVALID_ARG, INVALID_ARG])
    nodes = chain(RLEN, [base_tiling(RLEN, size=S - 1), sstream([("C", 0, S - 1)])])
    nodes[1] = nodes[1][:3] + (S,)                                                         # the parent has 2^32 - 2
    add("limit_stated_one_above", nodes, [0, 1], [OK, INVALID_ARG])
    for name, junk in (("other_magic", b"XLT\x03" + bytes(40)), ("ten_bytes", b"DLT\x03\x00\x00\x00\x00\x10\x00")):
        reads_all = sstream([("C", U32 - 9, 8), ("C", U32 - 1, 0)])                        # inside 2^32 - 1: "no limit"
        add(f"limit_no_header_{name}", chain(RLEN, [junk, reads_all]), [0, 1], [MALFORMED, MALFORMED])
        add(f"limit_no_header_{name}_2p32", chain(RLEN, [junk, stream([("C", U32 - 8, 0, 8)], 8)]), [1], [MALFORMED, MALFORMED])
    # trees: lineages that share a high inner level, requested in one launch
    d, _, vs = covering(rng, S, target=EDGES[0], n_small=420)
    nodes = chain(RLEN, [base_tiling(RLEN), stream(pf, size)])
    nodes += [(None, d, 1, None), (None, shift_level(rng, 3), 1, None), (None, shift_level(rng, 2, size=vs), 2, None),
              (None, inner_edges(rng), 1, None), (None, shift_level(rng, 2), 5, None)]
    add("tree_on_edges", nodes, range(2, 7), extra={2: [(H - 40, 8192)], 4: [(H - 40, 8192)]})
    # the bounds on work of the module docstring; what the model gives is kept for the tests
    for name, nodes, reqs, statuses in out:
        LINEAGE_EXPECTED[name] = exp = []
        for i, off, n in reqs:
            st, leaves = lineage_model(nodes, i, off, n)
            assert st == statuses[i], (name, i, st)
            assert sum(len(x) for x in leaves) <= sm.SLICE_MAX and len(leaves) <= LINEAGE_MAX_PIECES, (name, i, off, n)
            exp.append((st, b"".join(leaves), len(leaves)))
    return out


def window_children(d, pos):
    """The non-empty COPYs of the 4 KiB parse window of stream d that starts at the command at stream offset pos:
    the children of one step of the lineage walk when d is not the level on the base."""
    at, kids, seen = 25, 0, False
    for kind, ref, dst, n in sm.Stream.of(d).cmds:
        seen = seen or at == pos
        if at >= pos and at + (13 if kind == 1 else 9) <= pos + 4096:
            kids += kind == 1 and n > 0
        at += 13 if kind == 1 else 9 + n
    assert seen, "no command starts there"
    return kids


# ── in-place conversion: (name, ref_len, standard delta, statuses) ──
#
# statuses: {"localmin": ..., "constant": ..., "host": ...}: what the device plan gives under each policy, and
# what dg_make_inplace returns.  A case without a policy's key is not in that policy's list: the constant policy
# converts the lowest-index pending copy whatever its length, which in a covering() stream is the one of 2 GiB.
# The expected bytes are not computed here: they are the reference's own (tests/golden/golden_inplace_high.json)
# and, as a second comparator, dg_make_inplace's.  What is computed here is the CRWI digraph of a stream, as
# dg_inplace.cpp builds it, for the bounds on work and for the sizes of the capacity cases.

POLICIES = ("localmin", "constant")
IP_LENGTHS = [1, 7, 255, 256, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, 1 << 24, (1 << 24) + 1,
              (1 << 24) + 256, 3 << 24, 1 << 30, H - (1 << 20) - 1]      # both sides of every radix byte, with ties
IP_WINDOWS = [H - 33, H + 100001, 3 * (1 << 30) + 5]                     # the windows of R the cycles' blocks read
IP_VICTIM_MAX = 1 << 20
IP_VICTIMS = {}              # name of a touching case: the victims it was built for (the same under both policies)


def copies_of(d):
    return [(src, dst, n) for kind, src, dst, n in sm.Stream.of(d).cmds if kind == 1]


def crwi_ranges(copies):
    """Per copy i the index range [a, b) of the copies whose writes its read interval meets (i itself may lie
    inside and is no neighbour): dg_inplace.cpp step 3, for commands placed sequentially (dst non-decreasing)."""
    import bisect
    starts = [c[1] for c in copies]
    assert starts == sorted(starts)
    out = []
    for i, (src, _, n) in enumerate(copies):
        lo = bisect.bisect_left(starts, src)
        hi = bisect.bisect_left(starts, src + n, lo)
        if lo > 0 and lo - 1 != i and copies[lo - 1][1] + copies[lo - 1][2] > src:
            lo -= 1
        out.append((lo, hi))
    return out


def has_edges(copies):
    return any(b - a > (1 if a <= i < b else 0) for i, (a, b) in enumerate(crwi_ranges(copies)))


def crwi_sccs(copies):
    """The non-trivial strongly connected components of the CRWI digraph (Tarjan, iterative)."""
    n, rs = len(copies), crwi_ranges(copies)
    index, low, on, stack, comps, counter = [None] * n, [0] * n, [False] * n, [], [], 0
    for s in range(n):
        if index[s] is not None:
            continue
        index[s] = low[s] = counter
        counter += 1
        on[s] = True
        stack.append(s)
        call = [[s, rs[s][0]]]
        while call:
            v, x = call[-1]
            if x == v:
                x += 1
            if x < rs[v][1]:
                call[-1][1] = x + 1
                if index[x] is None:
                    index[x] = low[x] = counter
                    counter += 1
                    on[x] = True
                    stack.append(x)
                    call.append([x, rs[x][0]])
                elif on[x]:
                    low[v] = min(low[v], index[x])
                continue
            call.pop()
            if call:
                low[call[-1][0]] = min(low[call[-1][0]], low[v])
            if low[v] == index[v]:
                comp = []
                while True:
                    x = stack.pop()
                    on[x] = False
                    comp.append(x)
                    if x == v:
                        break
                if len(comp) > 1:
                    comps.append(comp)
    return comps


def constant_victims(copies):
    """The copies the constant policy converts, in conversion order: Kahn's order, and at a stall the lowest-index
    pending copy.  (The set does not depend on which ready copy pops first.)"""
    n, rs = len(copies), crwi_ranges(copies)
    indeg = [0] * n
    for i, (a, b) in enumerate(rs):
        for x in range(a, b):
            indeg[x] += x != i
    ready, done, victims, low_ptr, left = [i for i in range(n) if indeg[i] == 0], [False] * n, [], 0, n
    while left:
        if ready:
            v = ready.pop()
        else:
            while done[low_ptr]:
                low_ptr += 1
            v = low_ptr
            victims.append(v)
        done[v] = True
        left -= 1
        for x in range(*rs[v]):
            if x != v and not done[x]:
                indeg[x] -= 1
                if indeg[x] == 0:
                    ready.append(x)
    return victims


def victim_bound(d, policy):
    """An upper bound of the victims' payload bytes: exact under the constant policy; under localmin a victim is
    the smallest copy of a cycle, so of a component every copy but its one longest may be converted."""
    copies = copies_of(d)
    if policy == "constant":
        return sum(copies[v][2] for v in constant_victims(copies))
    total = 0
    for comp in crwi_sccs(copies):
        lens = sorted(copies[v][2] for v in comp)
        total += sum(lens) - (lens[-1] if lens[-1] > lens[-2] else 0)
    return total


def in_window(src, n):
    """R[src, src + n) lies wholly inside one of R's windows of random bytes."""
    return n > 0 and any(o <= src and src + n <= o + len(b) for o, b in R.windows())


def inplace_size(d, victims):
    """The size of the in-place form of standard delta d when the copies `victims` (indices) are converted."""
    st, copies = sm.Stream.of(d), copies_of(d)
    adds = [n for kind, _, _, n in st.cmds if kind == 2]
    return 25 + 13 * (len(copies) - len(victims)) + sum(9 + n for n in adds) + sum(9 + copies[v][2] for v in victims) + 1


def _identity(lengths, at=0):
    """COPYs with src == dst, one after the other from `at`: each reads only what it writes itself."""
    cmds = []
    for n in lengths:
        cmds.append(("C", at, n))
        at += n
    return cmds


def inplace_cases():
    rng = random.Random(0x233A)
    out, refusals = [], []

    def add(name, ref_len, d, status=OK, host=None, only=POLICIES, into=None):
        d = d if isinstance(d, bytes) else sstream(d)
        st = {p: status for p in only}
        st["host"] = status if host is None else host
        (out if into is None else into).append((name, ref_len, d, st))

    def shuffled(ls):
        ls = list(ls)
        rng.shuffle(ls)
        return ls

    # refusals, each the only defect of its stream; each goes between two good streams (below)
    for e in LOW:
        add(f"refuse_src_len_past_ref_{e:#x}", e, stream([("C", 0, 0, e - 1), ("C", e - 1, e - 1, 2)], e + 1), MALFORMED,
            into=refusals)
    add("refuse_src_len_2p32", RLEN, stream([("C", U32 - 16, 0, 16)], 16), MALFORMED, into=refusals)
    add("refuse_src_len_2p32_plus_16", RLEN, stream([("C", U32 - 16, 0, 32)], 32), MALFORMED, into=refusals)
    # the host converter takes no dst field as it is: it sorts the commands by dst and places them itself
    add("refuse_dst_off_by_one", RLEN, stream([("C", 0, 0, H), ("C", 5, H + 1, 8)], H + 9), UNSUPPORTED, host=OK, into=refusals)
    # every dst field is the running sum mod 2^32: a 32-bit compare accepts it.  The host converter sorts the
    # third command in front of the second, places all three and answers DG_OK (include/delta_gpu.h)
    add("refuse_sum_2p32_plus_16", RLEN, stream([("C", 0, 0, H), ("C", 5, H, H), ("C", 0, U32, 16)], 16), UNSUPPORTED, host=OK,
        into=refusals)

    # identity tilings: no edge, the output order is the rank.  One with every length of IP_LENGTHS (4 radix
    # passes), one of 128 copies (two lane batches), and one each whose longest copy needs 1, 2 and 3 passes
    assert sum(IP_LENGTHS) == 3354592519 < RLEN
    add("identity_4_passes", RLEN, _identity(shuffled(IP_LENGTHS)))
    add("identity_4_passes_128", RLEN, _identity(shuffled(IP_LENGTHS + [rng.randrange(1, 1 << 20) for _ in range(111)])))
    for (passes, base), e in zip(((1, [1, 7, 255, 255, 254, 128]),
                                  (2, [1, 7, 255, 256, 256, 257, 65535, 65535, 0x0134, 0x0234, 0xFF00, 0x00FF]),
                                  (3, [255, 256, 257, 65535, 65536, 65536, 65537, (1 << 24) - 1, 0x010203, 0x020203, 0xFF0000])), LOW):
        ls = base + [rng.randrange(1, 1 << (8 * passes)) for _ in range(70 - len(base))]
        assert 1 << (8 * passes - 8) <= max(ls) < 1 << (8 * passes)
        add(f"identity_{passes}_passes", e, _identity(shuffled(ls)))

    # the same lengths followed by a short tail whose COPYs read what the tiling writes: edges, so the lengths go
    # through the Kahn loop; dst, dst + len and version_size on every member of E
    for e in E:
        ls = shuffled(IP_LENGTHS[:-1])                            # below 2^31 together
        at = sum(ls)
        if e in LOW:
            cmds = _identity(ls) + [("C", at, e - 64 - at), ("C", 12345, 20), ("A", rng.randbytes(3)), ("C", 5, 40),
                                    ("C", H // 2 + 7, 1)]
        else:
            cmds = _identity(ls) + [("C", at, H - 1 - at), ("C", H - 1, 1), ("C", H, 1), ("C", H + 1, RLEN - 4 - (H + 1))]
            at = RLEN - 4 + (1 << 19) + 5 + 64
            cmds += [("C", 12345, 1 << 19), ("A", rng.randbytes(5)), ("C", H - 33, 64), ("C", 3, e - 1 - at), ("C", H // 2 + 7, 1)]
            if e == U32 - 1:
                cmds.append(("C", 7, 0))                          # dst = 0xFFFFFFFF
        assert seq(cmds)[1] == e
        add(f"tail_{e:#x}", min(e, RLEN), cmds)
        if e in LOW:
            out.append(refusals.pop(0))

    # covering() streams: localmin only
    for e in LOW:
        add(f"covering_ref_{e:#x}", e, covering(rng, e, top=e - 8000)[0], only=("localmin",))
    add("covering_whole_r", RLEN, covering(rng, RLEN)[0], only=("localmin",))
    for t in edge_targets():   # the first command at dst 2^31 behind an edge of the 1 KiB parse window (and of the others)
        add(f"edge_{t}", RLEN, covering(rng, RLEN, target=t, n_small=1000 if t < 5000 else 420)[0], only=("localmin",))
    out.append(refusals.pop(0))

    # cycles above 2^31: tests/inplace_graphs.py's, scaled to fit a window of R; the blocks at dst >= 2^31 behind
    # one identity COPY, every source inside the window, so a victim's payload is random bytes
    shapes = {
        "swap_equal": [(8, 8), (0, 8)],
        "swap_unequal": [(10, 20), (0, 10)],
        "rotate_3": [(8, 8), (16, 8), (0, 8)],
        "rotate_8": [(3 * ((k + 1) % 8), 3) for k in range(8)],
        "reverse_8": [(27, 3), (22, 5), (18, 4), (11, 7), (5, 6), (3, 2), (1, 2), (0, 1)],
        "two_sccs_linked": [(4, 4), (0, 4), (2, 4), (16, 4), (10, 4)],
        "figure_eight": [(15, 15), (0, 11), (11, 4)],
    }
    for k, (name, blocks) in enumerate(shapes.items()):
        for w in (IP_WINDOWS[k % 3], IP_WINDOWS[(k + 1) % 3]):
            base = max(w, H)                                      # (the window at 2^31 - 33: from 2^31 on)
            assert sum(n for _, n in blocks) <= 30
            cmds = [("C", 0, base)] + [("C", base + o, n) for o, n in blocks]
            assert all(in_window(c[1], c[2]) for c in cmds[1:])
            add(f"{name}_at_{base:#x}", RLEN, cmds)
        if k in (1, 4):
            out.append(refusals.pop(0))

    # touching intervals: a two-cycle that exists only with the one-byte overlap
    for w in LOW:
        for ov in (0, 1):
            # hi: A writes [w - 10, w) and reads up to w (+ 1: into B's write); B writes from w and reads A's write
            add(f"hi_touch_{w:#x}_{ov}", RLEN, [("C", 0, w - 10), ("C", w - 10 + ov, 10), ("C", w - 8, 5)])
            # pred: A writes [w - 10, w) and reads B's write; B writes from w and reads from w (- 1: the last byte A writes)
            add(f"pred_touch_{w:#x}_{ov}", RLEN, [("C", 0, w - 10), ("C", w, 10), ("C", w - ov, 5)])
            IP_VICTIMS[f"hi_touch_{w:#x}_{ov}"] = IP_VICTIMS[f"pred_touch_{w:#x}_{ov}"] = ov
    for ov in (0, 1):   # J, the last copy, writes [RLEN - 100, 2^32 - 1); A reads up to RLEN - 100 (+ 1); J reads A's write
        add(f"end_touch_{ov}", RLEN, [("C", 0, H), ("C", RLEN - 110 + ov, 10), ("C", H + 10, RLEN - 100 - (H + 10)),
                                      ("C", H, U32 - 1 - (RLEN - 100))])
        IP_VICTIMS[f"end_touch_{ov}"] = ov
        # the same with J's write ending at 2^32 itself, and A reading from one byte behind J's first: J is then the
        # write that starts before A's read interval and reaches into it, which dst[j] + len[j] decides, a sum that
        # no longer fits 32 bits.  The lengths sum to 2^32, which no command follows, so every dst is in place; the
        # header's version_size is the sum mod 2^32, 0.  The device plan, dg_make_inplace and the reference convert it
        add(f"end_touch_2p32_{ov}", RLEN, [("C", 0, H), ("C", RLEN - 110 + 11 * ov, 10), ("C", H + 10, RLEN - 100 - (H + 10)),
                                           ("C", H, U32 - (RLEN - 100))])
        IP_VICTIMS[f"end_touch_2p32_{ov}"] = ov
    out.append(refusals.pop(0))
    add("closing_swap", RLEN, [("C", 0, IP_WINDOWS[1]), ("C", IP_WINDOWS[1] + 5, 5), ("C", IP_WINDOWS[1], 5)])
    assert not refusals and out[0][3]["host"] == OK == out[-1][3]["host"]

    # the bounds on work, and the victims that read random bytes
    in_windows = 0
    for name, ref_len, d, st in out:
        if st["host"] != OK or UNSUPPORTED in st.values():
            continue
        copies = copies_of(d)
        for p in POLICIES:
            assert p not in st or victim_bound(d, p) <= IP_VICTIM_MAX, (name, p)
        # a component all of whose copies read inside a window gives at least one such victim, whichever it is
        in_windows += sum(1 for comp in crwi_sccs(copies) if all(in_window(copies[v][0], copies[v][2]) for v in comp))
    assert in_windows >= 12, in_windows
    return out


def inplace_list(policy):
    """The cases of one policy's batch, in corpus order: a refusal always lies between two accepted streams."""
    cases = [c for c in corpus()["inplace"] if policy in c[3]]
    for k, c in enumerate(cases):
        assert c[3][policy] == OK or (0 < k < len(cases) - 1 and cases[k - 1][3][policy] == OK == cases[k + 1][3][policy]), c[0]
    return cases


def inplace_capacity_cases():
    """(name, ref_len, standard delta, {policy: size}): streams with one victim of about 2^31 bytes, which
    nothing here converts: they run last in a batch whose out_cap ends a few KiB behind the good outputs, get
    DG_ERR_CAPACITY, and their sizes still count in the packed offsets.  size: of the in-place form, from the
    command list.  Two such sizes stay below 2^32 together, so there are three exchanges, for the offsets to
    pass 2^32 under either policy: V = R[RLEN - a, RLEN) + R[0, b), a two-cycle whose victim is the shorter
    copy, the first of equals (localmin), or the first (constant).  The covering() stream is the constant
    policy's alone: its lowest-index pending copy is the one of 2 GiB, which lies on no cycle."""
    out = []
    for name, a, b in (("exchange_short_first", RLEN - H, H), ("exchange_long_first", H, H - 1), ("exchange_equal", H - 1, H - 1)):
        d = sstream([("C", RLEN - a, a), ("C", 0, b)])
        assert crwi_sccs(copies_of(d)) == [[1, 0]] and constant_victims(copies_of(d)) == [0]
        out.append((name, RLEN, d, {"localmin": inplace_size(d, [0 if a <= b else 1]), "constant": inplace_size(d, [0])}))
    d = covering(random.Random(0x233B), RLEN)[0]
    copies, victims = copies_of(d), constant_victims(copies_of(d))
    assert sum(1 for v in victims if copies[v][2] > IP_VICTIM_MAX) == 1 and copies[victims[0]][2] == H - 3
    out.append(("covering_constant", RLEN, d, {"constant": inplace_size(d, victims)}))
    for p in POLICIES:
        assert all(H - (1 << 21) < c[3][p] < H + (1 << 16) for c in out if p in c[3])
        assert sum(c[3][p] for c in out if p in c[3]) > U32
    return out



_cache = {}


def corpus():
    if not _cache:
        _cache.update(compose=compose_cases(), invert=invert_cases(), read=read_cases(), splice=splice_cases(),
                      decode=decode_cases(), update=update_cases(), lineage=lineage_cases(), inplace=inplace_cases())
    return _cache


def _fields(d, into, rebase=0):
    st = sm.Stream.of(d)
    into["version_size"].add(st.version_size)
    for kind, ref, dst, n in st.cmds:
        into["dst"].add(dst)
        into["dst+len"].add(dst + n)
        if kind == 1:
            into["src"].add(ref + rebase)
            into["src+len"].add(ref + rebase + n)


def reach():
    """Per operator and quantity, the values the accepted cases take."""
    c = corpus()
    out = {op: {q: set() for q in ALLOWED[op]} for op in c}
    for _, a, b, st in c["compose"]:
        if st == OK:
            _fields(a, out["compose"])
            _fields(b, out["compose"])
    for op in ("invert", "read", "decode", "update"):
        for case in c[op]:
            if case[3] == OK:
                _fields(case[2], out[op])
                out[op]["ref_len"].add(case[1])
    for _, ref_len, d, st in c["inplace"]:
        if OK in (st.get("localmin"), st.get("constant")):
            _fields(d, out["inplace"])
            out["inplace"]["ref_len"].add(ref_len)
    for _, whole, segs, deltas, _, st in c["splice"]:
        if st == OK:   # of the spliced delta: sources rebased, dst in the whole V
            into = out["splice"]
            into["ref_len"].add(whole[1])
            into["version_size"].add(whole[3])
            for (sro, _, svo, _), d in zip(segs, deltas):
                for kind, ref, dst, n in sm.Stream.of(d).cmds:
                    into["dst"].add(svo - whole[2] + dst)
                    into["dst+len"].add(svo - whole[2] + dst + n)
                    if kind == 1:
                        into["src"].add(ref + sro - whole[0])
                        into["src+len"].add(ref + sro - whole[0] + n)
    into = out["lineage"]
    for _, nodes, reqs, statuses in c["lineage"]:
        for i, (ref_len, d, parent, _) in enumerate(nodes):
            if statuses[i] == OK:   # (every level below an accepted one is accepted)
                mine = {q: set() for q in QUANTITIES}
                _fields(d, mine)
                mine["ref_len"].add(stated_ref_len(nodes, i))
                for q in QUANTITIES:
                    into[q if parent == BASE or q.startswith(("dst", "version")) else "inner " + q].update(mine[q])
        for i, off, n in reqs:
            if statuses[i] == OK:
                vs = sm.Stream.of(nodes[i][1]).version_size
                into["off"].add(off)
                into["off+n"].add(off + (0 if off >= vs else min(n, vs - off)))
                if off < vs and n and has_sentinel(nodes[i][1]):
                    into["off beside dst 0xFFFFFFFF entries"].add(off)
    return out
