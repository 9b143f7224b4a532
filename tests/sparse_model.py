"""A model of the delta transforms that never materialises a version or a
reference: plain Python, int arithmetic, nothing sized by a buffer.

The dense models (compose_cases.model_compose, invert_cases.model_invert,
splice_cases.model_splice, read_cases.model_version) build an array of
version_size entries, so they cannot follow an offset past a few MiB.  Every
field of the DLT\\x03 format is a u32 and the kernels keep src, dst and len in
32-bit registers; this model is the reference for the upper half of that range.
tests/test_sparse_model_cpu.py pins it to the dense models on all their corpora.

  SparseBytes   a buffer of any length, zero except for a few windows;
  pieces        a version as [(dst, len, "lit", bytes) | (dst, len, "ref", src)],
                sequential and non-empty; compose, invert, splice and read work
                on pieces by interval arithmetic and emit the normal forms of
                include/delta_gpu.h (maximal merging, no zero-length command,
                sequential dst);
  replay        bytes [a, b) of what decode or update makes of R, standard and
                in-place streams (memmove order, zeros in an uncovered tail:
                src/c/apply.c:271-284, as update_cases.py restates it), by
                tracing each byte back through the commands that wrote it;
  lineage       a byte range of a version k deltas away from R, by recursion
                over pieces: no level between R and the requested one is built;
  crc64 combine crc(X || Y) from crc(X), crc(Y) and |Y| in Python ints;
  statuses      each operator's contract, with every sum in unbounded ints.

Every function returns (status, bytes); the bytes are empty on a failure.
"""
from __future__ import annotations

import bisect
import struct

OK, INVALID_ARG, UNSUPPORTED, TOO_LARGE, CAPACITY, MALFORMED, SRC_CRC, DST_CRC = 0, 1, 2, 3, 7, 8, 9, 10
SLICE_MAX = 1 << 20
U32 = 1 << 32
PLAN_LIMIT = U32 - (1 << 20)   # the encode and splice plans refuse an r_len or v_len at or above this


# ── sparse buffers ──

class SparseBytes:
    """`length` bytes, zero everywhere but in the windows {offset: bytes}."""

    def __init__(self, length, windows=None):
        self.length = int(length)
        items = sorted((int(o), bytes(b)) for o, b in dict(windows or {}).items() if len(b))
        for (o, b), (o2, _) in zip(items, items[1:]):
            assert o + len(b) <= o2, "windows overlap"
        assert all(o >= 0 and o + len(b) <= self.length for o, b in items), "a window outside the buffer"
        self.starts = [o for o, _ in items]
        self.data = [b for _, b in items]

    @classmethod
    def of(cls, b):
        return b if isinstance(b, SparseBytes) else cls(len(b), {0: bytes(b)})

    def __len__(self):
        return self.length

    def head(self, n):
        """The first n bytes as a buffer of their own (a shorter ref_len of the same R)."""
        assert 0 <= n <= self.length
        return SparseBytes(n, {o: b[:n - o] for o, b in zip(self.starts, self.data) if o < n})

    def windows(self):
        return list(zip(self.starts, self.data))

    def __getitem__(self, s):
        assert isinstance(s, slice) and s.step in (None, 1)
        a, b = s.indices(self.length)[:2]
        b = max(a, b)
        assert b - a <= SLICE_MAX, "a slice of more than 1 MiB of a sparse buffer"
        out = bytearray(b - a)
        k = max(bisect.bisect_right(self.starts, a) - 1, 0)
        while k < len(self.starts) and self.starts[k] < b:
            o, d = self.starts[k], self.data[k]
            lo, hi = max(a, o), min(b, o + len(d))
            if lo < hi:
                out[lo - a:hi - a] = d[lo - o:hi - o]
            k += 1
        return bytes(out)


# ── CRC-64/XZ in Python ints (reflected, polynomial 0xC96C5795D7870F42) ──

_POLY = 0xC96C5795D7870F42
_M64 = (1 << 64) - 1
_table = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ _POLY if _c & 1 else _c >> 1
    _table.append(_c)


def crc64(data: bytes) -> int:
    c = _M64
    for x in data:
        c = _table[(c ^ x) & 0xFF] ^ (c >> 8)
    return c ^ _M64


def _mul(a: int, b: int) -> int:
    """a * b in GF(2)[x] mod P, bit 63 the coefficient of x^0."""
    p = 0
    for k in range(63, -1, -1):
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ _POLY if b & 1 else b >> 1
    return p


def _xpow(n: int) -> int:
    """x^n mod P."""
    r, sq = 1 << 63, 1 << 62
    while n:
        if n & 1:
            r = _mul(r, sq)
        sq = _mul(sq, sq)
        n >>= 1
    return r


def crc64_combine(crc_x: int, crc_y: int, len_y: int) -> int:
    """crc(X || Y): the init and final inversions cancel, so it is crc(X) x^(8 |Y|) + crc(Y)."""
    return _mul(crc_x, _xpow(8 * len_y)) ^ crc_y


def crc64_repeat(crc_b: int, len_b: int, k: int) -> int:
    """crc of a block repeated k times, by doubling."""
    out, have = 0, 0                      # crc of the empty string
    for bit in range(k.bit_length() - 1, -1, -1):
        out = crc64_combine(out, out, have * len_b)
        have *= 2
        if (k >> bit) & 1:
            out = crc64_combine(out, crc_b, len_b)
            have += 1
    return out


def crc64_sparse(buf: SparseBytes) -> int:
    """crc of a sparse buffer: the windows' CRCs joined over runs of zeros."""
    zero = crc64(b"\0")
    out, at = 0, 0
    for o, d in buf.windows() + [(buf.length, b"")]:
        out = crc64_combine(out, crc64_repeat(zero, 1, o - at), o - at)
        out = crc64_combine(out, crc64(d), len(d))
        at = o + len(d)
    return out


# ── streams ──

class Stream:
    """A parsed DLT\\x03 stream.  header: the 25 bytes and the magic are there;
    framing: every command header and payload is inside the stream and every
    type is known (a missing END is the end of input; bytes after END are
    ignored).  cmds: (kind, src or payload offset, dst, len), 1 COPY, 2 ADD, up
    to the first framing error."""

    _memo = {}

    @classmethod
    def of(cls, d):
        """Parsed once per bytes object (a stream is read at many ranges)."""
        if isinstance(d, Stream):
            return d
        if d not in cls._memo:
            if len(cls._memo) >= 256:
                cls._memo.clear()
            cls._memo[d] = cls(d)
        return cls._memo[d]

    def __init__(self, d: bytes):
        self.data = d
        self.bounds, self.monotone, self.tiles_v, self.tiles = {}, None, None, None
        self.header = len(d) >= 25 and d[:4] == b"DLT\x03"
        self.framing = self.header
        self.inplace, self.version_size, self.cmds = False, 0, []
        self.src_crc = self.dst_crc = bytes(8)
        if not self.header:
            return
        self.inplace = bool(d[4] & 1)
        self.version_size = struct.unpack(">I", d[5:9])[0]
        self.src_crc, self.dst_crc = d[9:17], d[17:25]
        pos = 25
        while pos < len(d):
            t = d[pos]
            if t == 0:
                break
            if t == 1 and pos + 13 <= len(d):
                src, dst, n = struct.unpack(">III", d[pos + 1:pos + 13])
                self.cmds.append((1, src, dst, n))
                pos += 13
            elif t == 2 and pos + 9 <= len(d) and pos + 9 + struct.unpack(">I", d[pos + 5:pos + 9])[0] <= len(d):
                dst, n = struct.unpack(">II", d[pos + 1:pos + 9])
                self.cmds.append((2, pos + 9, dst, n))
                pos += 9 + n
            else:
                self.framing = False
                break

    def placed(self) -> bool:
        """Every dst is the sum of the earlier lengths, and they sum to version_size."""
        if self.tiles_v is None:
            at, self.tiles_v = 0, True
            for _, _, dst, n in self.cmds:
                if dst != at:
                    self.tiles_v = False
                    break
                at += n
            self.tiles_v = self.tiles_v and at == self.version_size
        return self.tiles_v

    def pieces(self):
        """The non-empty commands as pieces."""
        return [(dst, n, "ref", ref) if kind == 1 else (dst, n, "lit", self.data[ref:ref + n])
                for kind, ref, dst, n in self.cmds if n]

    def copy_past(self, limit) -> bool:
        return any(kind == 1 and ref + n > limit for kind, ref, _, n in self.cmds)


def merge(pieces):
    """Maximal merging: literal neighbours join; "ref" neighbours join when the
    second starts in the source where the first ends.  dst is recomputed."""
    out = []
    at = 0
    for _, n, kind, x in pieces:
        if not n:
            continue
        if out and out[-1][2] == kind == "lit":
            out[-1][3].append(x)
            out[-1][1] += n
        elif out and out[-1][2] == kind == "ref" and out[-1][3] + out[-1][1] == x:
            out[-1][1] += n
        else:
            out.append([at, n, kind, [x] if kind == "lit" else x])
        at += n
    return [(d, n, k, b"".join(x) if k == "lit" else x) for d, n, k, x in out]


def emit(pieces, version_size, src_crc, dst_crc):
    """(status, the standard delta of the merged pieces)."""
    runs = merge(pieces)
    size = 26 + sum(13 if k == "ref" else 9 + n for _, n, k, _ in runs)
    if size >= U32:
        return TOO_LARGE, b""
    assert all(max(d, n, d + n) < U32 and (k == "lit" or x < U32) for d, n, k, x in runs), "a field the format cannot hold"
    out = bytearray(b"DLT\x03\x00" + struct.pack(">I", version_size) + bytes(src_crc) + bytes(dst_crc))
    for d, n, k, x in runs:
        out += (b"\x01" + struct.pack(">III", x, d, n)) if k == "ref" else (b"\x02" + struct.pack(">II", d, n) + x)
    out += b"\x00"
    assert len(out) == size
    return OK, bytes(out)


def cut(pieces, starts, s, e):
    """The pieces of a tiling (starts[k] = pieces[k][0]) inside [s, e), clipped."""
    out = []
    k = bisect.bisect_right(starts, s) - 1
    while s < e:
        d, n, kind, x = pieces[k]
        lo, hi = max(s, d), min(e, d + n)
        out.append((lo, hi - lo, kind, x[lo - d:hi - d] if kind == "lit" else x + (lo - d)))
        s = hi
        k += 1
    return out


# ── compose ──

def compose(A: bytes, B: bytes, ignore_hash=False):
    a, b = Stream.of(A), Stream.of(B)
    if not a.framing or not b.framing:
        return MALFORMED, b""
    if a.copy_past(U32) or b.copy_past(a.version_size):   # "a COPY of A with src + len > 2^32", read literally
        return MALFORMED, b""
    if a.inplace or b.inplace or not a.placed() or not b.placed():
        return UNSUPPORTED, b""
    if not ignore_hash and a.dst_crc != b.src_crc:
        return SRC_CRC, b""
    pa = a.pieces()
    starts = [p[0] for p in pa]
    out = []
    for p in b.pieces():
        out += [p] if p[2] == "lit" else cut(pa, starts, p[3], p[3] + p[1])
    return emit(out, b.version_size, a.src_crc, b.dst_crc)


# ── invert ──

def invert(R, A: bytes):
    R = SparseBytes.of(R)
    a = Stream.of(A)
    n = len(R)
    if not a.framing or a.copy_past(n):
        return MALFORMED, b""
    if a.inplace or not a.placed():
        return UNSUPPORTED, b""
    # owner of a position: smallest src, then longest, then first in the stream.
    # Painted in reverse key order, so that the first in key order stays on top.
    keyed = sorted(((src, -ln, k, dst) for k, (kind, src, dst, ln) in enumerate(a.cmds) if kind == 1 and ln), reverse=True)
    iv, starts = [], []   # disjoint (start, end, offset of V at start) in order, and their starts
    for src, nl, _, dst in keyed:
        s, e = src, src - nl
        i = bisect.bisect_right(starts, s) - 1
        if i < 0 or iv[i][1] <= s:
            i += 1
        j = bisect.bisect_left(starts, e)
        new = []
        if i < j and iv[i][0] < s:
            new.append((iv[i][0], s, iv[i][2]))
        new.append((s, e, dst))
        if i < j and iv[j - 1][1] > e:
            lo, hi, v = iv[j - 1]
            new.append((e, hi, v + (e - lo)))
        iv[i:j] = new
        starts[i:j] = [x[0] for x in new]
    out, at = [], 0
    for lo, hi, v in iv:
        if lo > at:
            out.append((at, lo - at, "lit", R[at:lo]))
        out.append((lo, hi - lo, "ref", v))
        at = hi
    if at < n:
        out.append((at, n - at, "lit", R[at:n]))
    return emit(out, n, a.dst_crc, a.src_crc)


# ── splice ──

def splice_geometry(whole, segs):
    """The status dg_splice and dg_splice_plan_create give the geometry alone."""
    ro, rl, vo, vl = whole
    if not segs:
        return INVALID_ARG
    if rl >= PLAN_LIMIT or vl >= PLAN_LIMIT:
        return TOO_LARGE
    at = vo
    for sro, srl, svo, svl in segs:
        if svo != at or at + svl > vo + vl:
            return INVALID_ARG
        at += svl
        if sro < ro or sro + srl > ro + rl:
            return INVALID_ARG
    return OK if at == vo + vl else INVALID_ARG


def splice(whole, segs, deltas, src_crc: bytes, seg_status=None):
    g = splice_geometry(whole, segs)
    if g:
        return g, b""
    for s in seg_status or []:
        if s:
            return s, b""
    ro, rl, vo, vl = whole
    streams = [Stream.of(d) for d in deltas]
    if any(not st.framing or st.copy_past(seg[1]) for st, seg in zip(streams, segs)):
        return MALFORMED, b""
    if any(st.inplace or not st.placed() or st.version_size != seg[3] for st, seg in zip(streams, segs)):
        return UNSUPPORTED, b""
    out, crc = [], 0
    for st, (sro, _, svo, svl) in zip(streams, segs):
        for d, n, kind, x in st.pieces():
            out.append((svo - vo + d, n, kind, x if kind == "lit" else x + (sro - ro)))
        crc = crc64_combine(crc, int.from_bytes(st.dst_crc, "big"), svl)
    return emit(out, vl, src_crc, crc.to_bytes(8, "big"))


# ── replay: decode, update and range reads ──

def _bounds_ok(st: Stream, ref_len: int) -> bool:
    """Every command inside its limits: a standard delta reads R and writes V; an
    in-place delta does both in a buffer of bsz = max(ref_len, version_size)."""
    if ref_len not in st.bounds:
        bsz = max(ref_len, st.version_size)
        lim_dst, lim_src = (bsz, bsz) if st.inplace else (st.version_size, ref_len)
        st.bounds[ref_len] = all(dst + n <= lim_dst and (kind == 2 or ref + n <= lim_src) for kind, ref, dst, n in st.cmds)
    return st.bounds[ref_len]


def _writers(st: Stream, lo, hi, k):
    """The commands before k that may write into [lo, hi), last first."""
    if st.monotone is None:
        st.dsts = [c[2] for c in st.cmds]
        st.ends = [c[2] + c[3] for c in st.cmds]
        st.monotone = st.dsts == sorted(st.dsts) and st.ends == sorted(st.ends)
    if st.monotone:
        return range(min(bisect.bisect_left(st.dsts, hi), k) - 1, bisect.bisect_right(st.ends, lo) - 1, -1)
    return range(k - 1, -1, -1)


def replay(R, delta, window):
    """Bytes [a, b) of the buffer after every command of a well-formed stream.
    A standard delta starts from zeros and reads R; an in-place delta starts from
    R followed by zeros up to bsz and reads the buffer as the commands before it
    left it (memmove: a COPY reads all of its source before it stores).  Each
    byte is traced back to the last command that wrote it."""
    R = SparseBytes.of(R)
    st = Stream.of(delta)
    a, b = window
    assert 0 <= a <= b and b - a <= SLICE_MAX
    out = bytearray(b - a)
    cmds = st.cmds
    todo = [(a, b, len(cmds), 0)]   # bytes [lo, hi) of the buffer before command k go to out[pos:]
    while todo:
        lo, hi, k, pos = todo.pop()
        for j in _writers(st, lo, hi, k):
            kind, ref, dst, n = cmds[j]
            s, e = max(lo, dst), min(hi, dst + n)
            if s < e:
                break
        else:                                     # nothing wrote it: the initial buffer
            if st.inplace and lo < len(R):
                m = min(hi, len(R))
                out[pos:pos + m - lo] = R[lo:m]
            continue
        if lo < s:
            todo.append((lo, s, j, pos))
        if e < hi:
            todo.append((e, hi, j, pos + (e - lo)))
        if kind == 2:
            out[pos + (s - lo):pos + (e - lo)] = st.data[ref + (s - dst):ref + (e - dst)]
        elif st.inplace:
            todo.append((ref + (s - dst), ref + (e - dst), j, pos + (s - lo)))
        else:
            out[pos + (s - lo):pos + (e - lo)] = R[ref + (s - dst):ref + (e - dst)]
    return bytes(out)


def decode_status(ref_len: int, delta: bytes, out_cap=None):
    """dg_decode_plan_run with ignore_hash: DG_ERR_MALFORMED or DG_ERR_CAPACITY."""
    st = Stream.of(delta)
    if not st.framing or not _bounds_ok(st, ref_len):
        return MALFORMED
    need = max(ref_len, st.version_size) if st.inplace else st.version_size
    return CAPACITY if out_cap is not None and need > out_cap else OK


def update_status(ref_len: int, delta: bytes, buf_cap: int):
    """dg_update_plan_run with ignore_hash, for a stream with one defect at most."""
    st = Stream.of(delta)
    if not st.header:
        return MALFORMED
    if max(ref_len, st.version_size) > buf_cap:
        return CAPACITY
    if not st.framing or not _bounds_ok(st, ref_len):
        return MALFORMED
    return OK if st.inplace else UNSUPPORTED


def inplace_status(ref_len: int, delta: bytes):
    """dg_inplace_plan_run's per-stream status for a standard delta of at most one defect: malformed framing or a
    COPY past R, then commands that are not placed one after the other (the sum taken in 64 bits)."""
    st = Stream.of(delta)
    if not st.framing or st.copy_past(ref_len):
        return MALFORMED
    at = 0
    for _, _, dst, n in st.cmds:
        if dst != at:
            return UNSUPPORTED
        at += n
    return OK


def read(R, delta: bytes, off: int, length: int):
    """dg_read: (status, bytes [off, off + n)) with pread's n."""
    R = SparseBytes.of(R)
    st = Stream.of(delta)
    if not st.header:
        return MALFORMED, b""
    if st.inplace:
        return UNSUPPORTED, b""
    if not st.framing or not _bounds_ok(st, len(R)):
        return MALFORMED, b""
    n = 0 if off >= st.version_size else min(length, st.version_size - off)
    return OK, replay(R, delta, (off, off + n))


# ── lineage reads ──

NO_LIMIT = U32 - 1   # ref_len of a level whose parent has no readable header


def index_status(st: Stream, ref_len: int):
    """What the read plan's index pass reports for a stream with that ref_len."""
    if not st.header:
        return MALFORMED
    if st.inplace:
        return UNSUPPORTED
    return OK if st.framing and _bounds_ok(st, ref_len) else MALFORMED


def lineage_ref_lens(base_len: int, deltas, stated=None):
    """ref_len per level (index 0: the delta on R): what a descriptor states where
    stated[j] is not None, else len(R) for the first and the header version_size
    of the level below for the others (NO_LIMIT below a level without a header)."""
    out = []
    for j, d in enumerate(deltas):
        if stated is not None and stated[j] is not None:
            out.append(stated[j])
        elif j == 0:
            out.append(base_len)
        else:
            below = Stream.of(deltas[j - 1])
            out.append(below.version_size if below.header else NO_LIMIT)
    return out


def lineage_status(base_len: int, deltas, stated=None):
    """The contract's order (include/delta_gpu.h): from the requested level
    towards R, per level a. its index status with its ref_len, b. UNSUPPORTED if
    it is not sequential, c. INVALID_ARG if its ref_len is not the version_size
    of a level below whose own index status is 0 (stated descriptors only)."""
    streams = [Stream.of(d) for d in deltas]
    ref = lineage_ref_lens(base_len, deltas, stated)
    for j in range(len(deltas) - 1, -1, -1):
        st = index_status(streams[j], ref[j])
        if st:
            return st
        if not streams[j].placed():
            return UNSUPPORTED
        if j and index_status(streams[j - 1], ref[j - 1]) == OK and ref[j] != streams[j - 1].version_size:
            return INVALID_ARG
    return OK


def _tiling(st: Stream):
    if st.tiles is None:
        st.tiles = st.pieces()
        st.tile_starts = [p[0] for p in st.tiles]
    return st.tiles, st.tile_starts


def _lineage_leaves(R, streams, j, lo, hi, out):
    """Bytes [lo, hi) of V_j, lo < hi, as leaf pieces appended to out: an ADD
    yields its payload, a COPY becomes [src, src + len) one level down, level 0
    slices R."""
    if j == 0:
        out.append(R[lo:hi])
        return
    for _, n, kind, x in cut(*_tiling(streams[j - 1]), lo, hi):
        if kind == "lit":
            out.append(x)
        else:
            _lineage_leaves(R, streams, j - 1, x, x + n, out)


def lineage_leaves(R, deltas, off: int, length: int, stated=None):
    """(status, the leaf pieces of the request in output order: ADD payloads and slices of R)."""
    R = SparseBytes.of(R)
    status = lineage_status(len(R), deltas, stated)
    if status:
        return status, []
    streams = [Stream.of(d) for d in deltas]
    vs = streams[-1].version_size if streams else len(R)
    n = 0 if off >= vs else min(length, vs - off)
    out = []
    if n:
        _lineage_leaves(R, streams, len(streams), off, off + n, out)
    return OK, out


def lineage_read(R, deltas, off: int, length: int, stated=None):
    """dg_read_lineage and dg_lineage_plan_run: (status, bytes [off, off + n) of
    V_k) with pread's n; deltas[0] is the delta on R."""
    status, leaves = lineage_leaves(R, deltas, off, length, stated)
    return status, b"".join(leaves)


def lineage_pieces(R, deltas, off: int, length: int, stated=None):
    """The leaf pieces (ADD payloads and slices of R) the request resolves to."""
    return len(lineage_leaves(R, deltas, off, length, stated)[1])
