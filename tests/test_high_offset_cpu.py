"""CPU: the HIP-free host code (dg_compose, dg_invert, dg_read, dg_splice) on
the high-offset corpus of tests/high_offset_cases.py, against the sparse model:
exact bytes, exact statuses.

The corpus puts src, dst, src + len, dst + len, version_size and ref_len on
2^31 - 1, 2^31, 2^31 + 1, 2^32 - 2 and 2^32 - 1; the first test checks that it
still does.  R is one zeroed numpy buffer of 2^32 - 1 - 2^20 bytes with the
corpus's few windows written in (untouched pages cost nothing); the functions
are called through ctypes on it.  dg_decode and dg_update have no host form
(both need a context and a device): their cases run in
tests/test_gpu_high_offset.py only, and here the model's statuses for them are
compared with the ones the corpus states.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import high_offset_cases as hc
import sparse_model as sm

U8P = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def host_r():
    buf = np.zeros(hc.RLEN, dtype=np.uint8)
    for o, b in hc.R.windows():
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return buf


def _take(dg, rc_, out):
    got = C.string_at(out.data, out.len) if out.len else b""
    dg.lib.dg_buffer_free(C.byref(out))
    return rc_, b"" if rc_ else got


def test_corpus_reaches_what_it_is_for():
    got = hc.reach()
    for op, want in hc.ALLOWED.items():
        for q in hc.QUANTITIES:
            missing = [hex(x) for x in want[q] if x not in got[op][q]]
            assert not missing, (op, q, missing)
    c = hc.corpus()
    assert all(len(c[k]) >= n for k, n in dict(compose=39, invert=30, read=35, splice=28, decode=13, update=16).items())
    # the families: long single commands, merges above 2^31, 400 commands and more, the window and chunk edges
    big = [sm.Stream.of(x[1]) for x in c["compose"]] + [sm.Stream.of(x[2]) for x in c["invert"] + c["read"]]
    assert sum(1 for s in big if any(n >= hc.H for _, _, _, n in s.cmds)) >= 20
    assert sum(1 for s in big if len(s.cmds) >= 400) >= 22
    edge = [sm.Stream.of(x[2]) for x in c["invert"] + c["read"] if x[0].startswith("edge_")]
    assert len(edge) == 12 and all(len(s.data) > 3 * 4096 and len(s.cmds) >= 1000 for s in edge)
    for op in ("compose", "invert", "read", "splice"):
        names = [x[0] for x in c[op]]
        assert all(any(n.startswith(f"edge_{t}") for n in names) for t in hc.edge_targets()[:4]), op
    merged = sm.Stream.of(sm.invert(hc.R, next(x[2] for x in c["invert"] if x[0] == "merge"))[1])
    assert [(k, n) for k, _, _, n in merged.cmds] == [(1, hc.RLEN - 3), (2, 3)]
    one = next(x for x in c["splice"] if x[0] == "one_copy_65")
    assert [(k, n) for k, _, _, n in sm.Stream.of(sm.splice(*one[1:5])[1]).cmds] == [(1, hc.RLEN)]
    assert all(seg[3] < hc.H for seg in one[2])
    # R: windows at and around 2^31, at odd offsets, and at the last byte
    assert all(o % 2 for o, _ in hc.R.windows()) and hc.R[hc.RLEN - 1:hc.RLEN] != b"\0" and len(hc.R) == sm.PLAN_LIMIT - 1
    assert hc.R[hc.H - 2:hc.H + 2].count(0) < 3


def test_the_model_gives_the_stated_statuses():
    """The statuses the corpus states come from reading each contract in
    include/delta_gpu.h; the model must arrive at the same ones on its own."""
    c = hc.corpus()
    for name, a, b, st in c["compose"]:
        assert sm.compose(a, b)[0] == st, name
    for name, ref_len, a, st in c["invert"]:
        assert sm.invert(hc.R.head(ref_len), a)[0] == st, name
    for name, ref_len, d, st, rs in c["read"]:
        assert {sm.read(hc.R.head(ref_len), d, off, n)[0] for off, n in rs} == {st}, name
        assert sm.decode_status(ref_len, d) == st, name
    for name, whole, segs, deltas, crc, st in c["splice"]:
        assert sm.splice(whole, segs, deltas, crc)[0] == st, name
    for name, ref_len, d, st in c["decode"]:
        assert sm.decode_status(ref_len, d, 65536) == st, name
    for name, ref_len, d, st in c["update"]:
        assert sm.update_status(ref_len, d, hc.RLEN) == st, name
    # no one-block kernel moves more than 1 MiB, and no output exceeds 64 KiB of literals by much
    for name, a, b, st in c["compose"]:
        assert len(sm.compose(a, b)[1]) < 65536 + 4096, name
    for name, ref_len, a, st in c["invert"]:
        assert len(sm.invert(hc.R.head(ref_len), a)[1]) < 65536 + 4096, name


def test_dg_compose(dg):
    for name, a, b, st in hc.corpus()["compose"]:
        try:
            got = (sm.OK, dg.compose(a, b))
        except dg.DeltaError as e:
            got = (e.code, b"")
        assert got == sm.compose(a, b), name
        assert got[0] == st, name


def test_dg_invert(dg, host_r):
    for name, ref_len, a, st in hc.corpus()["invert"]:
        out = dg._lib.Buffer()
        rc_ = dg.lib.dg_invert(host_r.ctypes.data_as(U8P), ref_len, dg._lib._u8(a), len(a), C.byref(out))
        assert _take(dg, rc_, out) == sm.invert(hc.R.head(ref_len), a), name
        assert rc_ == st, name


def test_dg_read(dg, host_r):
    for name, ref_len, d, st, rs in hc.corpus()["read"]:
        ref = hc.R.head(ref_len)
        for off, n in rs:
            out = dg._lib.Buffer()
            rc_ = dg.lib.dg_read(host_r.ctypes.data_as(U8P), ref_len, dg._lib._u8(d), len(d), off, n, C.byref(out))
            assert _take(dg, rc_, out) == sm.read(ref, d, off, n), (name, off, n)
            assert rc_ == st, name


def test_dg_splice(dg):
    for name, whole, segs, deltas, crc, st in hc.corpus()["splice"]:
        try:
            got = (sm.OK, dg.splice(segs, deltas, whole, crc))
        except dg.DeltaError as e:
            got = (e.code, b"")
        assert got == sm.splice(whole, segs, deltas, crc), name
        assert got[0] == st, name


def test_dg_read_refuses_4_gib(dg):
    """r_len or delta_len of 4 GiB: refused before a byte is read."""
    d = hc.sstream([("C", 0, 4)])
    small = C.cast((C.c_uint8 * 8)(), U8P)
    out = dg._lib.Buffer()
    assert dg.lib.dg_read(small, 1 << 32, dg._lib._u8(d), len(d), 0, 4, C.byref(out)) == sm.TOO_LARGE
    assert dg.lib.dg_read(small, 8, dg._lib._u8(d), 1 << 32, 0, 4, C.byref(out)) == sm.TOO_LARGE
    assert dg.lib.dg_read(small, 8, dg._lib._u8(d), len(d), 0, 4, C.byref(out)) == sm.OK and out.len == 4
    dg.lib.dg_buffer_free(C.byref(out))
