"""The encoders at table sizes on both sides of 2^23 and 2^25.

Every encoder kernel turns a fingerprint into a table slot, and the code that
does it changes at two sizes: `slot_of` (dg_devutil.h) and the correcting
kernels' checkpoint test leave the FP64 path for the 64-bit Barrett reduction
at 2^23, and the window chain's first-writer search stops packing
(slot + 1 | member << 25) into a dword at 2^25.  On random data a wrong but
deterministic slot goes unseen at such sizes, so the onepass pairs here carry
planted slot collisions for the q they run at (tests/table_size_cases.py;
tests/test_table_size_cases_cpu.py proves that each delta depends on them).
Every comparison is exact: the oracle's bytes and the reference-minted hashes
of tests/golden/golden_table_size.json.

Which test reaches which call site at q (or |F|) >= 2^23 and >= 2^25:

* window chain, dg_onepass.hip diag_batch `slot_of` and the first-writer search
  (packed keys below 2^25, the plain loop from there; taken for epochs of at
  most 32 steps, which only the diagonal_short cases have), and the member
  kernel (dg_members.hip) with its check (B): test_onepass_planted_collisions,
  modes chain / members / auto, q = 8388617 (>= 2^23), 33554467 (>= 2^25);
* the table tier in HBM (epochs past the register history): the same test,
  gaps 900 and 3000;
* the generic chain (pair offsets not 16-byte aligned, dg_onepass.hip
  `slot_of` at the generic window refill and step): test_onepass_generic_chain
  at the same q;
* onepass at a q it chose itself: test_onepass_natural_size, q = 8388881.
  The natural crossing of 2^25 needs a pair of 512 MiB and is left to the
  planted cases;
* correcting, |F| = 8388617 >= 2^23, `checkpoint_slot` in the global build
  (cap 524287, 1048573), the LDS build (cap 4099) and the scan (every row):
  test_correcting_around_2_23.  |F| >= 2^25 would need |R| > 16 MiB and a
  second of one-wave scan per pair; test_arith_model.py pins the arithmetic
  there;
* `checkpoint_only` (--verbose): test_gpu_verbose.py, |F| = 8388617.
"""
from __future__ import annotations

import hashlib

import pytest

import table_size_cases as T

pytestmark = pytest.mark.gpu

ONEPASS, CORRECTING = 1, 2
MODES = ("members", "chain", "auto")


@pytest.fixture(scope="module")
def gold():
    return T.golden()


@pytest.fixture(scope="module")
def want(orc):
    """{q: the oracle's deltas of onepass_cases(q)}, computed once"""
    cache = {}

    def get(q):
        if q not in cache:
            cache[q] = [orc.encode(ONEPASS, R, V, 16, q) for _, R, V in T.onepass_cases(q)]
        return cache[q]
    return get


def _context(dg, q, mode="auto"):
    """A context of the test's own whose table pool holds 8 tables of q slots
    (4 GiB at 2^25: not something to keep for the session)."""
    c = dg.Context(0)
    c.set_limit(dg.LIMIT_TABLE_POOL_BYTES, 8 * 16 * q)
    c.set_limit(dg.LIMIT_ONEPASS_MEMBERS, {"members": dg.MEMBERS_ON, "chain": dg.MEMBERS_OFF,
                                           "auto": dg.MEMBERS_AUTO}[mode])
    return c


def _check_golden(gold, name, d):
    g = gold[name]
    assert len(d) == g["delta_len"], name
    assert hashlib.sha256(d).hexdigest() == g["delta_sha256"], name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("q", T.QS)
def test_onepass_planted_collisions(dg, orc, gold, want, q, mode):
    """All families and gaps in one batch of 16-byte aligned pairs: the window
    chain, the member kernel and the table tier."""
    cases = T.onepass_cases(q)
    ctx = _context(dg, q, mode)
    try:
        got = dg.encode_batch([(R, V) for _, R, V in cases], "onepass", p=16, q=q, ctx=ctx)
        for (name, R, V), d, w in zip(cases, got, want(q)):
            assert d == w, (name, mode)
            _check_golden(gold, name, d)
        for (name, R, V), d in zip(cases, got):
            if name.startswith(("diagonal_short9", "offdiag_v_gap3000")):
                assert dg.decode(R, d, ctx=ctx) == V, name
    finally:
        ctx.close()


def _odd_layout(cases):
    """(layout, R arena, V arena): every pair at an odd offset of both arenas"""
    lay, ra, va = [], bytearray(b"\xEE"), bytearray(b"\xEE" * 3)
    for _, R, V in cases:
        lay.append((len(ra), len(R), len(va), len(V)))
        ra += R + b"\xEE" * (2 - len(R) % 2)
        va += V + b"\xEE" * (2 - len(V) % 2)
    assert all(ro % 2 == 1 and vo % 2 == 1 for ro, _, vo, _ in lay)
    return lay, bytes(ra) + bytes(64), bytes(va) + bytes(64)


@pytest.mark.parametrize("q", T.QS)
def test_onepass_generic_chain(dg, orc, gold, want, torch_cuda, q):
    """The same cases through a plan whose pair offsets are odd: not the
    16-byte aligned LDS-window chain but the generic one."""
    torch = torch_cuda
    cases = T.onepass_cases(q)
    lay, ra, va = _odd_layout(cases)
    n = len(cases)
    ctx = _context(dg, q)
    try:
        plan = dg.EncodePlan(ctx, "onepass", lay, p=16, q=q)
        assert plan.table_size(0) == q and not plan.members
        ref = torch.frombuffer(bytearray(ra), dtype=torch.uint8).cuda()
        ver = torch.frombuffer(bytearray(va), dtype=torch.uint8).cuda()
        out = torch.empty(plan.output_bound, dtype=torch.uint8, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run(ref.data_ptr(), ver.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(),
                 st.data_ptr(), ctx.stream)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n
        offs, outc = off.cpu().tolist(), bytes(out.cpu().numpy())
        for i, ((name, R, V), w) in enumerate(zip(cases, want(q))):
            d = outc[offs[i]:offs[i + 1]]
            assert d == w, name
            _check_golden(gold, name, d)
        plan.close()
    finally:
        ctx.close()


def test_onepass_natural_size(dg, orc, gold):
    """One pair of 128 MiB + 4 KiB at --table-size 1: q = next_prime(seeds / 16)
    = 8388881 passes 2^23 with no user input.  (The natural crossing of 2^25
    needs a pair of 512 MiB; the planted cases above cover that branch.)  The
    oracle's encode of this pair, about 3 s, is the longest step."""
    R, V = T.natural_pair(orc)
    assert len(R) == len(V) == T.NATURAL_LEN
    ctx = _context(dg, T.NATURAL_Q)
    try:
        plan = dg.EncodePlan(ctx, "onepass", [(0, len(R), 0, len(V))], p=16, q=1)
        assert plan.table_size(0) == T.NATURAL_Q == orc.onepass_q(len(R), 16, 1)
        plan.close()
        d = dg.encode_batch([(R, V)], "onepass", p=16, q=1, ctx=ctx)[0]
        assert d == orc.encode(ONEPASS, R, V, 16, 1)
        _check_golden(gold, "natural_128MiB", d)
        assert d[9:17] == dg.crc64_xz(R, ctx=ctx) and d[17:25] == dg.crc64_xz(V, ctx=ctx)
        assert dg.decode(R, d, ctx=ctx) == V      # (verifies both CRCs)
    finally:
        ctx.close()


@pytest.mark.parametrize("q,max_table", [(1, T.MAX_TABLE), (1048573, T.MAX_TABLE), (1, 4096)])
def test_correcting_around_2_23(dg, ctx, orc, gold, q, max_table):
    """|F| = next_prime(2 seeds) is 8388581 < 2^23 at |R| = 4194304 and
    8388617 > 2^23 at |R| = 4194312: the FP64 checkpoint test and the Barrett
    one, side by side in one batch.  Tables of 524287 and 1048573 slots are
    past one block's LDS and take the global build; max_table = 4096 (4099
    slots, m = 2047) takes the LDS build, and there about 2049 passing seeds
    fall into 4099 slots and the delta is most of V, so each stored seed
    decides a match."""
    rows = [r for r in T.CORRECTING_ROWS if (r[1], r[2]) == (q, max_table)]
    assert [r[0] for r in rows] == [4194304, 4194312]
    pairs = [T.correcting_boundary_pair(r[0]) for r in rows]
    for (r_len, _, _, prm), (R, _) in zip(rows, pairs):
        assert len(R) == r_len and orc.correcting_params(r_len, 16, q, max_table) == prm
    got = dg.encode_batch(pairs, "correcting", p=16, q=q, max_table=max_table, ctx=ctx)
    for (r_len, _, _, _), (R, V), d in zip(rows, pairs, got):
        assert d == orc.encode(CORRECTING, R, V, 16, q, 256, max_table), r_len
        _check_golden(gold, T.correcting_name(r_len, q, max_table), d)
        assert dg.decode(R, d, ctx=ctx) == V, r_len


def test_correcting_around_2_23_buffer_of_one(dg, ctx, orc, gold):
    r_len, q, max_table = T.BUF_CAP_1_ROW
    R, V = T.correcting_boundary_pair(r_len)
    d = dg.encode(R, V, "correcting", p=16, q=q, buf_cap=1, max_table=max_table, ctx=ctx)
    assert d == orc.encode(CORRECTING, R, V, 16, q, 1, max_table)
    _check_golden(gold, T.correcting_name(r_len, q, max_table, 1), d)
    assert dg.decode(R, d, ctx=ctx) == V
