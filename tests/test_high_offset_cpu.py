"""CPU: the HIP-free host code (dg_compose, dg_invert, dg_make_inplace, dg_read, dg_read_lineage, dg_splice) on
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

In-place conversion has no model of its bytes here: dg_make_inplace is held to
tests/golden/golden_inplace_high.json, minted from the reference's own
`delta inplace` on a sparse file (tests/golden/make_golden_inplace_graphs.py),
and to the CLI itself where oracle/_ref/delta exists; what the sparse model
adds is the meaning: the in-place stream replays to the same bytes as the
standard one.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import high_offset_cases as hc
import sparse_model as sm

U8P = C.POINTER(C.c_uint8)
HERE = os.path.dirname(os.path.abspath(__file__))
REF_CLI = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "delta")
GOLD_INPLACE = {(c["name"], c["policy"]): c
                for c in json.load(open(os.path.join(HERE, "golden", "golden_inplace_high.json")))["cases"]}


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
        for q in want:
            missing = [hex(x) for x in want[q] if x not in got[op][q]]
            assert not missing, (op, q, missing)
    c = hc.corpus()
    assert all(len(c[k]) >= n for k, n in dict(compose=39, invert=30, read=35, splice=28, decode=13, update=16, lineage=28,
                                                         inplace=58).items())
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
    # the lineage families
    lin = {x[0]: x for x in c["lineage"]}
    for depth in (2, 4, 64):   # tall: every level 2^32 - 1 bytes, the top one requested
        _, nodes, reqs, sts = lin[f"tall_{depth}"]
        assert len(nodes) == depth and sts == [sm.OK] * depth and any(i == depth - 1 for i, _, _ in reqs)
        assert all(sm.Stream.of(n[1]).version_size == hc.S for n in nodes)
        assert len(hc.lineage_path(nodes, depth - 1)[1]) == depth
    _, nodes, reqs, sts = lin["edges_at_every_level"]
    closing = [i for i, n in enumerate(nodes) if sm.Stream.of(n[1]).cmds[-1] == (1, 7, hc.S, 0)]
    assert len(closing) == 2 and all(0 < i < len(nodes) - 1 for i in closing) and {i for i, _, _ in reqs} == set(range(7))
    for i in range(7):   # every boundary straddled at the level that has it and, carried through the COPYs, from every level above
        bounds = hc.carried_bounds(nodes, i)
        assert i not in closing or set(hc.E) <= set(bounds)
        assert i < closing[0] or sum(1 for b in bounds if b >= hc.H - 4) >= 5, i   # edges_full's, carried
        assert all((i, b - 1, 2) in reqs and (i, b - 17, 34) in reqs for b in bounds if b >= 17), i
    fan = [x for x in c["lineage"] if x[0].startswith("fanout_")]
    assert sorted(int(x[0].split("_")[1]) for x in fan) == sorted(hc.EDGES + [25 + 4096]) and len(fan) == 4
    for name, nodes, reqs, sts in fan:
        t, n_small = (int(w) for w in name.split("_")[1:])
        st = sm.Stream.of(nodes[1][1])
        assert t % 1024 == 0 or (t - 25) % 4096 == 0, name
        assert len(hc.stream([], 0, end=False)) == 25 and sum(1 for c_ in st.cmds if c_[2] >= hc.H) > n_small
        kids = hc.window_children(nodes[1][1], t)   # the window the index enters for lo = 2^31
        assert kids > hc.WORK_ITEMS, (name, kids)   # more children than the stack has slots: the item is cut above 2^31
        assert all((i, hc.H, 8192) in reqs for i in (1, 2, 3)), name
    assert {n_small for n_small in (420, 1000)} == {int(x[0].split("_")[2]) for x in fan}
    limit = [x for x in c["lineage"] if x[0].startswith("limit_")]
    assert len(limit) >= 13 and sum(1 for x in limit if not hc.host_expressible(x)) == 2
    assert [lin[f"limit_2p32_at{k}"][3].index(sm.MALFORMED) for k in (1, 2, 3)] == [0, 1, 2]
    assert lin["limit_served"][3] == [sm.OK] * 3
    _, nodes, reqs, sts = lin["tree_on_edges"]
    assert [n[2] for n in nodes].count(1) == 3 and {i for i, _, _ in reqs} == {2, 3, 4, 5, 6} and sts == [sm.OK] * 7
    assert max(e[2] for v in hc.LINEAGE_EXPECTED.values() for e in v) > 1000   # (leaf pieces of one request)
    # the in-place families: identity tilings of every pass count, the tails, covering() at every ref_len and
    # window edge, the cycles at the three windows, the touching pairs, the refusals between good streams
    ip = {x[0]: x for x in c["inplace"]}
    assert len(ip) == len(c["inplace"])
    for passes in (1, 2, 3, 4):
        longest = max(n for _, _, n in hc.copies_of(ip[f"identity_{passes}_passes"][2]))
        assert 1 << (8 * passes - 8) <= longest < 1 << (8 * passes)
    for name in ["identity_4_passes", "identity_4_passes_128"] + [f"tail_{e:#x}" for e in hc.E]:
        lens = sorted(n for _, _, n in hc.copies_of(ip[name][2]))
        assert all(lens.count(n) >= hc.IP_LENGTHS[:-1].count(n) for n in hc.IP_LENGTHS[:-1]), name
        assert name.startswith("identity") == (not hc.has_edges(hc.copies_of(ip[name][2]))), name
    assert len(hc.copies_of(ip["identity_4_passes_128"][2])) == 128
    assert [ip[f"tail_{e:#x}"][1] for e in hc.E] == hc.LOW + [hc.RLEN] * 2
    cov = [x for x in c["inplace"] if x[0].startswith(("covering_", "edge_"))]
    assert len(cov) == 10 and sorted(x[1] for x in cov)[:3] == hc.LOW and all(set(x[3]) == {"localmin", "host"} for x in cov)
    assert sum(1 for x in cov if len(x[2]) > 3 * 4096) >= 4
    for t in hc.edge_targets():   # the command at dst 2^31 starts 4 bytes before the edge
        st = sm.Stream.of(ip[f"edge_{t}"][2])
        at = 25 + sum(13 if k == 1 else 9 + n for k, _, dst, n in st.cmds if dst < hc.H)
        assert at == t and any(dst == hc.H for _, _, dst, _ in st.cmds)
    cyc = [x for x in c["inplace"] if "_at_0x" in x[0]]
    assert len(cyc) == 14 and {int(x[0].split("_at_")[1], 16) for x in cyc} == {max(w, hc.H) for w in hc.IP_WINDOWS}
    assert all(dst >= hc.H and hc.in_window(src, n) for x in cyc for src, dst, n in hc.copies_of(x[2])[1:])
    assert len(hc.IP_VICTIMS) == 16 and sorted(hc.IP_VICTIMS.values()) == [0] * 8 + [1] * 8
    assert any(dst + n == hc.U32 - 1 and n > 1 << 20 for src, dst, n in hc.copies_of(ip["end_touch_1"][2]))
    assert any(dst + n == hc.U32 and n > 1 << 20 for src, dst, n in hc.copies_of(ip["end_touch_2p32_1"][2]))
    for name in ("identity_4_passes", "identity_4_passes_128", "tail_0xffffffff"):   # three radix passes would not do
        cp = hc.copies_of(ip[name][2])
        assert sorted(range(len(cp)), key=lambda i: (cp[i][2], i)) != sorted(range(len(cp)), key=lambda i: (cp[i][2] & 0xFFFFFF, i)), name
    refused = [x for x in c["inplace"] if x[3]["localmin"] != sm.OK]
    assert sorted(x[3]["localmin"] for x in refused) == [sm.UNSUPPORTED] * 2 + [sm.MALFORMED] * 5
    assert [x[3]["host"] for x in refused if x[3]["localmin"] == sm.UNSUPPORTED] == [sm.OK] * 2
    assert all(x[3]["localmin"] == x[3]["constant"] for x in refused)
    for pol in hc.POLICIES:   # (asserts that every refusal lies between two accepted streams)
        assert len(hc.inplace_list(pol)) == {"localmin": 58, "constant": 48}[pol]
    cap = hc.inplace_capacity_cases()
    assert [sorted(x[3]) for x in cap] == [["constant", "localmin"]] * 3 + [["constant"]]
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
    for name, nodes, reqs, sts in c["lineage"]:
        for i in {i for i, _, _ in reqs}:
            ref_len, ds, stated = hc.lineage_path(nodes, i)
            assert sm.lineage_status(ref_len, ds, stated) == sts[i], (name, i)
    for name, ref_len, d, sts in c["inplace"]:
        assert {sts[p] for p in hc.POLICIES if p in sts} == {sm.inplace_status(ref_len, d)}, name
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


@pytest.fixture(scope="module")
def host_inplace(dg, host_r):
    """dg_make_inplace of every case under every policy of its list: (rc, bytes, stats), computed once."""
    out = {}
    for name, ref_len, d, sts in hc.corpus()["inplace"]:
        for pol in hc.POLICIES:
            if pol in sts:
                buf, stats = dg._lib.Buffer(), dg._lib.InplaceStats()
                rc_ = dg.lib.dg_make_inplace(host_r.ctypes.data_as(U8P), ref_len, dg._lib._u8(d), len(d), dg._lib.POLICIES[pol],
                                             C.byref(buf), C.byref(stats))
                out[(name, pol)] = _take(dg, rc_, buf) + ({k: getattr(stats, k) for k, _ in dg._lib.InplaceStats._fields_},)
    return out


def test_dg_make_inplace_equals_reference_golden(host_inplace):
    cases = hc.corpus()["inplace"]
    assert set(GOLD_INPLACE) == {(name, pol) for name, _, _, sts in cases for pol in hc.POLICIES if sts.get(pol) == sm.OK}
    for name, ref_len, d, sts in cases:
        for pol in hc.POLICIES:
            if pol not in sts:
                continue
            rc_, got, _ = host_inplace[(name, pol)]
            assert rc_ == sts["host"], (name, pol)
            if sts[pol] == sm.OK:
                g = GOLD_INPLACE[(name, pol)]
                assert g["std_sha256"] == hashlib.sha256(d).hexdigest(), name
                assert (len(got), hashlib.sha256(got).hexdigest()) == (g["len"], g["sha256"]), (name, pol)
                assert len(got) <= len(d) + hc.IP_VICTIM_MAX + 4 * len(d) // 13, (name, pol)   # (the bound on work)


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="oracle/_ref/delta not built")
def test_dg_make_inplace_equals_reference_cli(host_inplace, tmp_path):
    files = {}
    for name, ref_len, d, sts in hc.corpus()["inplace"]:
        for pol in hc.POLICIES:
            if sts.get(pol) != sm.OK:
                continue
            if ref_len not in files:
                files[ref_len] = tmp_path / f"r_{ref_len:x}"
                with open(files[ref_len], "wb") as f:   # sparse: the length, then the windows
                    f.truncate(ref_len)
                    for o, b in hc.R.head(ref_len).windows():
                        f.seek(o)
                        f.write(b)
            (tmp_path / "d").write_bytes(d)
            subprocess.run([REF_CLI, "inplace", str(files[ref_len]), str(tmp_path / "d"), str(tmp_path / "o"), "--policy", pol],
                           check=True, capture_output=True)
            assert host_inplace[(name, pol)][1] == (tmp_path / "o").read_bytes(), (name, pol)


def _replay_windows(vs):
    ws = [(0, min(64, vs)), (max(vs - 100, 0), vs)] + [(max(e - 40, 0), min(e + 41, vs)) for e in hc.E if e - 40 < vs]
    return [w for w in ws if w[0] < w[1]]


def test_inplace_streams_mean_what_the_standard_ones_do(host_inplace):
    """Replayed in memmove order inside a buffer that holds R, the converted stream gives the version's bytes."""
    seen = 0
    for name, ref_len, d, sts in hc.corpus()["inplace"]:
        ref = hc.R.head(ref_len)
        for pol in hc.POLICIES:
            if sts.get(pol) != sm.OK:
                continue
            got = host_inplace[(name, pol)][1]
            st = sm.Stream.of(got)
            assert st.inplace and st.framing and st.version_size == sm.Stream.of(d).version_size
            for w in _replay_windows(st.version_size):
                assert sm.replay(ref, got, w) == sm.replay(ref, d, w), (name, pol, w)
                seen += 1
    assert seen > 400


def test_inplace_corpus_orders_and_victims(host_inplace):
    c = {x[0]: x for x in hc.corpus()["inplace"]}
    # an identity tiling has no edge: the output lists its copies by (length, index), under either policy
    for name in [n for n in c if n.startswith("identity_")]:
        copies = hc.copies_of(c[name][2])
        want = [copies[i] for i in sorted(range(len(copies)), key=lambda i: (copies[i][2], i))]
        assert want != copies
        for pol in hc.POLICIES:
            _, got, stats = host_inplace[(name, pol)]
            assert hc.copies_of(got) == want and stats["num_adds"] == 0, (name, pol)
    # the touching pairs: a victim only with the one-byte overlap
    for name, victims in hc.IP_VICTIMS.items():
        for pol in hc.POLICIES:
            assert host_inplace[(name, pol)][2]["num_adds"] == victims, (name, pol)
    # at least 12 victims whose payload is random bytes: an ADD of the output that the input does not have, whose
    # payload has no zero run of 8 bytes and equals R at the source of the COPY it replaces
    random_victims = 0
    for name, ref_len, d, sts in c.values():
        if sts.get("localmin") != sm.OK:
            continue
        srcs = {(dst, n): src for src, dst, n in hc.copies_of(d)}
        out = sm.Stream.of(host_inplace[(name, "localmin")][1])
        for kind, at, dst, n in out.cmds:
            if kind == 2 and (dst, n) in srcs and hc.in_window(srcs[(dst, n)], n):
                assert out.data[at:at + n] == hc.R[srcs[(dst, n)]:srcs[(dst, n)] + n] and (n < 8 or bytes(8) not in out.data[at:at + n])
                random_victims += 1
    assert random_victims >= 12, random_victims
    # the constant policy's victims are the model's (hc.constant_victims), which the capacity cases' sizes rest on
    for name, ref_len, d, sts in c.values():
        if sts.get("constant") == sm.OK:
            copies = hc.copies_of(d)
            assert host_inplace[(name, "constant")][2]["num_adds"] - sum(1 for k, *_ in sm.Stream.of(d).cmds if k == 2) == \
                len(hc.constant_victims(copies)), name
            assert len(host_inplace[(name, "constant")][1]) == hc.inplace_size(d, hc.constant_victims(copies)), name


def test_dg_read(dg, host_r):
    for name, ref_len, d, st, rs in hc.corpus()["read"]:
        ref = hc.R.head(ref_len)
        for off, n in rs:
            out = dg._lib.Buffer()
            rc_ = dg.lib.dg_read(host_r.ctypes.data_as(U8P), ref_len, dg._lib._u8(d), len(d), off, n, C.byref(out))
            assert _take(dg, rc_, out) == sm.read(ref, d, off, n), (name, off, n)
            assert rc_ == st, name


def test_dg_read_lineage(dg, host_r):
    """Every case the host can express (no stated ref_len), every request: the status and the bytes of the model."""
    assert dg.lineage_work_items() == hc.WORK_ITEMS   # the fan-out cases are sized for it
    ran = 0
    for case in hc.corpus()["lineage"]:
        name, nodes, reqs, sts = case
        if not hc.host_expressible(case):
            continue
        for (i, off, n), (st, exp, _) in zip(reqs, hc.LINEAGE_EXPECTED[name]):
            ref_len, ds, _ = hc.lineage_path(nodes, i)
            k = len(ds)
            dp = (U8P * k)(*[dg._lib._u8(d) for d in ds])
            dl = (C.c_size_t * k)(*[len(d) for d in ds])
            out = dg._lib.Buffer()
            rc_ = dg.lib.dg_read_lineage(host_r.ctypes.data_as(U8P), ref_len, dp, dl, k, off, n, C.byref(out))
            assert _take(dg, rc_, out) == (st, exp), (name, i, off, n)
            assert rc_ == sts[i], (name, i)
            ran += 1
    assert ran > 3500


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
