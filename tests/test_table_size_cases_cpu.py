"""CPU: the table-size cases (tests/table_size_cases.py) test what they claim.

* the planted windows share a slot at their q and at no other q under test;
* every onepass case is sensitive to the slot: its oracle delta at the planted
  q differs from the oracle's delta at each of the other four q, so a kernel
  whose slot is wrong at that q (and sends the planted windows apart) cannot
  give the expected bytes;
* the deltas decode, the speculative member model (oracle/spec_model.c)
  equals the oracle on the diagonal cases and leaves the planted members
  unverified (check (B));
* the geometry is the intended one: q as given, |F| on both sides of 2^23,
  the 4096-slot rows in the LDS build and the others in the global build;
* the reference's own encoder gives the oracle's bytes, and the committed
  goldens (read by the GPU tests, where the reference is absent) are those.
"""
from __future__ import annotations

import hashlib
import shutil

import pytest

import table_size_cases as T
from test_plan_cpu import MAX_TABLE, driver, geom, one  # noqa: F401  (driver: a fixture)
from test_spec_model import sm, spec  # noqa: F401  (sm: a fixture)

ONEPASS, CORRECTING = 1, 2
LDS_BYTES = 160 << 10   # one workgroup's LDS on gfx950
N_CASES = len(T.FAMILIES) * len(T.GAPS) + len(T.SHORT_RUNS)   # per q


@pytest.fixture(scope="module")
def deltas(orc):
    """oracle delta of a case at any q, computed once"""
    cache = {}

    def get(case, q):
        name, R, V = case
        if (name, q) not in cache:
            cache[name, q] = orc.encode(ONEPASS, R, V, 16, q)
        return cache[name, q]
    return get


def test_fingerprint_is_the_oracles(orc):
    for A, B in T.collisions(T.Q_DEFAULT)[0]:
        for w in (A, B, A[3:] + B[:3]):
            assert T.fingerprint(w) == orc.fingerprint(w, 0, 16)
            assert T.fingerprint(w) == sum(b * 263 ** (15 - i) for i, b in enumerate(w)) % T.M61


@pytest.mark.parametrize("q", T.QS)
def test_planted_windows_share_a_slot_only_at_q(q):
    pairs, triples = T.collisions(q)
    assert len(pairs) == T.N_PAIRS and len(triples) == T.N_TRIPLES
    short = []
    for k in T.SHORT_RUNS:
        Pb, trs = T.short_triples(q, k)
        assert len(Pb) == 16 - k and len(trs) == T.N_TRIPLES
        for X1, X2, Y in trs:
            assert len(X1) == len(X2) == len(Y) == k and X1[0] != X2[0] and X1[-1] != X2[-1]
            short.append((X1 + Pb, X2 + Pb, Pb + Y))
    for ws in pairs + triples + tuple(short):
        assert all(len(w) == 16 for w in ws) and len(set(ws)) == len(ws)
        fps = [T.fingerprint(w) for w in ws]
        assert len({f % q for f in fps}) == 1
        for o in T.QS:
            if o != q:
                assert len({f % o for f in fps}) == len(fps), (q, o)


@pytest.mark.parametrize("q", T.QS)
def test_every_case_is_sensitive_to_the_slot(orc, deltas, q):
    cases = T.onepass_cases(q)
    assert len(cases) == N_CASES
    for case in cases:
        name, R, V = case
        assert orc.onepass_q(len(R), 16, q) == q, name   # the pair is too small to raise q
        d = deltas(case, q)
        assert orc.decode(R, d) == (0, V), name
        for o in T.QS:
            if o != q:
                # a planted collision costs one byte of delta (the COPY starts a
                # byte later); a long epoch at a small q can hold one of its own,
                # hence no exact count
                assert d != deltas(case, o), (name, o)
                assert 0 < len(d) - len(deltas(case, o)) <= T.n_planted(name), (name, o)


@pytest.mark.parametrize("q", T.QS)
def test_spec_model_on_the_diagonal_cases(orc, sm, q):
    for name, R, V in T.onepass_cases(q):
        got, st = spec(orc, sm, R, V, q)
        assert got == orc.diff_onepass(R, V, p=16, q=q), name
        if name.startswith("diagonal"):
            assert st.members - st.verified >= T.N_TRIPLES, (name, st.members, st.verified)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_geometry(driver, orc):
    lines = []
    for q in T.QS:
        for _, R, V in T.onepass_cases(q):
            lines.append(geom(ONEPASS, [(0, len(R), 0, len(V))], q=q, lds=LDS_BYTES))
    lines.append(geom(ONEPASS, [(0, T.NATURAL_LEN, 0, T.NATURAL_LEN)], q=1, lds=LDS_BYTES))
    # the generic chain's plan: odd pair offsets
    name, R, V = T.onepass_cases(T.Q_ABOVE_25)[0]
    lines.append(geom(ONEPASS, [(1, len(R), 3, len(V))], q=T.Q_ABOVE_25, lds=LDS_BYTES))
    for r_len, q, mt, _ in T.CORRECTING_ROWS:
        lines.append(geom(CORRECTING, [(0, r_len, 0, r_len)], q=q, max_table=mt, lds=LDS_BYTES))
    got = driver(lines)
    assert all(g["rc"] == 0 for g in got)
    k = 0
    for q in T.QS:
        for _ in T.onepass_cases(q):
            assert got[k]["pp"][0]["q"] == q and got[k]["aligned16"] == 1
            k += 1
    assert got[k]["pp"][0]["q"] == orc.onepass_q(T.NATURAL_LEN, 16, 1) == T.NATURAL_Q
    assert (1 << 23) < T.NATURAL_Q < (1 << 25)
    assert got[k + 1]["pp"][0]["q"] == T.Q_ABOVE_25 and got[k + 1]["aligned16"] == 0
    k += 2
    for (r_len, q, mt, want), g in zip(T.CORRECTING_ROWS, got[k:]):
        assert orc.correcting_params(r_len, 16, q, mt) == want
        x = g["pp"][0]
        assert (x["q"], x["f_size"], x["m"]) == want
        # |F| = 8388581 takes the FP64 checkpoint test, 8388617 the Barrett one
        assert (want[1] < (1 << 23)) == (r_len == 4194304)
        # the LDS build where the table fits one block's LDS, else the global build
        assert (x["q"] <= g["corr_lds_cap"]) == (mt == 4096)
    assert MAX_TABLE == T.MAX_TABLE


def _check(c, algo, q, mt, d):
    assert (c["algo"], c["q"], c["max_table"]) == (algo, q, mt), c["name"]
    assert sorted(c) == ["algo", "delta_len", "delta_sha256", "max_table", "name", "q"]
    assert len(d) == c["delta_len"], c["name"]
    assert hashlib.sha256(d).hexdigest() == c["delta_sha256"], c["name"]


def test_goldens_are_the_oracles_onepass(orc, deltas):
    gold = T.golden()
    n = 0
    for q in T.QS:
        for case in T.onepass_cases(q):
            _check(gold[case[0]], ONEPASS, q, T.MAX_TABLE, deltas(case, q))
            n += 1
    assert n == N_CASES * len(T.QS) and len(gold) == n + 1 + len(T.CORRECTING_ROWS) + 1


def test_goldens_are_the_oracles_correcting(orc):
    gold = T.golden()
    for r_len, q, mt, _ in T.CORRECTING_ROWS:
        R, V = T.correcting_boundary_pair(r_len)
        d = orc.encode(CORRECTING, R, V, 16, q, 256, mt)
        assert orc.decode(R, d) == (0, V)
        _check(gold[T.correcting_name(r_len, q, mt)], CORRECTING, q, mt, d)
    r_len, q, mt = T.BUF_CAP_1_ROW
    R, V = T.correcting_boundary_pair(r_len)
    _check(gold[T.correcting_name(r_len, q, mt, 1)], CORRECTING, q, mt, orc.encode(CORRECTING, R, V, 16, q, 1, mt))


def test_reference_equals_the_oracle_onepass(orc, ref, deltas):
    for q in T.QS:
        for case in T.onepass_cases(q):
            assert ref.encode(ONEPASS, case[1], case[2], p=16, q=q) == deltas(case, q), case[0]


def test_reference_equals_the_oracle_correcting(orc, ref):
    rows = [(r, q, mt, 256) for r, q, mt, _ in T.CORRECTING_ROWS] + [T.BUF_CAP_1_ROW + (1,)]
    for r_len, q, mt, bc in rows:
        R, V = T.correcting_boundary_pair(r_len)
        assert ref.encode(CORRECTING, R, V, p=16, q=q, buf_cap=bc, max_table=mt) == \
            orc.encode(CORRECTING, R, V, 16, q, bc, mt), (r_len, q, mt, bc)


def test_reference_equals_the_oracle_at_the_natural_size(orc, ref):
    """The 128 MiB + 4 KiB pair, whose own q = 8388881 passes 2^23 (the
    longest step here: a few seconds for each encoder)."""
    R, V = T.natural_pair(orc)
    d = orc.encode(ONEPASS, R, V, 16, 1)
    assert ref.encode(ONEPASS, R, V, p=16, q=1) == d
    _check(T.golden()["natural_128MiB"], ONEPASS, 1, T.MAX_TABLE, d)
