"""The library's plan arithmetic against the oracle, on the CPU under ASan + UBSan.

dg_plan.cpp (table sizes, buffer geometry, CRC constant tables, the --verbose
report) contains no HIP, so it is compiled here with g++
-fsanitize=address,undefined together with tests/sanitize/plan_check.cpp and
dg_format.cpp.  The driver prints what the library computes; this module
compares it with the oracle's formulas (onepass_q, correcting_params,
crc64_xz, encode) and with identities that follow from the CRC register's own
step, not with a copy of the construction.
"""
from __future__ import annotations

import json
import os
import random
import shutil
import subprocess

import pytest

from cases import small_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "delta-compression_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

ONEPASS, CORRECTING = 1, 2
OK, INVALID_ARG, UNSUPPORTED, TOO_LARGE = 0, 1, 2, 3
DEFAULT_Q, BUF_CAP, MAX_TABLE = 1048573, 256, 1073741827
M64 = (1 << 64) - 1
X0 = 1 << 63   # x^0 in the reflected representation


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_check") / "plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "sanitize", "plan_check.cpp"),
           os.path.join(CSRC, "dg_plan.cpp"), os.path.join(CSRC, "dg_format.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)

    def run(lines):
        p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env,
                           timeout=600)
        assert p.returncode == 0, p.stdout[-500:] + p.stderr[-4000:]
        out = [json.loads(l) for l in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def geom(algo, pairs, p=16, q=DEFAULT_Q, buf_cap=BUF_CAP, max_table=MAX_TABLE, flags=0, n_cu=256,
         lds=65536, pool=0, members=0):
    """pairs: (r_off, r_len, v_off, v_len)"""
    w = [algo, p, q, buf_cap, max_table, flags, n_cu, lds, pool, members, len(pairs)]
    for d in pairs:
        w += list(d)
    return "geom " + " ".join(str(x) for x in w)


def one(algo, r_len, v_len=0, **kw):
    return geom(algo, [(0, r_len, 0, v_len)], **kw)


# ── sizing against the reference's formulas ──

def test_sizing_matches_the_oracle(driver, orc):
    lines, want = [], []
    for p in (1, 4, 16, 64):
        for r_len in (0, 1, p - 1, p, p + 1, 4096, 65536, 262144, 1 << 20):
            for q in (1, 4099, DEFAULT_Q):
                lines.append(one(ONEPASS, r_len, p=p, q=q))
                want.append((orc.onepass_q(r_len, p, q), None, None))
                for mt in (MAX_TABLE, 1000):   # 1000 clamps every table but the smallest
                    lines.append(one(CORRECTING, r_len, p=p, q=q, max_table=mt))
                    want.append(orc.correcting_params(r_len, p, q, mt))
    for g, (q, f, m) in zip(driver(lines), want):
        assert g["rc"] == OK
        x = g["pp"][0]
        assert x["q"] == q and x["q_magic"] == M64 // q
        if f is not None:
            assert (x["f_size"], x["m"]) == (f, m)
            assert (x["f_magic"], x["m_magic"]) == (M64 // f, M64 // m)


def test_sizing_pinned_triples(driver, orc):
    # the values tests/test_oracle.py pins for the oracle
    got = driver([one(ONEPASS, 65536, q=1), one(ONEPASS, 262144, q=1), one(ONEPASS, 1 << 20, q=1),
                  one(ONEPASS, 65536, q=DEFAULT_Q), one(CORRECTING, 65536, q=1),
                  one(CORRECTING, 262144, q=1), one(CORRECTING, 1 << 20, q=1)])
    assert [g["pp"][0]["q"] for g in got[:4]] == [4099, 16411, 65537, 1048573]
    assert [(g["pp"][0]["q"], g["pp"][0]["f_size"], g["pp"][0]["m"]) for g in got[4:]] == \
        [(8191, 131059, 17), (32771, 524261, 16), (131071, 2097131, 16)]


def test_output_bound_covers_the_reference_delta(driver, orc):
    lines, sizes = [], []
    for name, R, V, _, q in small_cases():
        for algo in (ONEPASS, CORRECTING):
            for p in (1, 4, 16):
                lines.append(one(algo, len(R), len(V), p=p, q=q))
                sizes.append((name, algo, p, len(orc.encode(algo, R, V, p=p, q=q))))
    for g, (name, algo, p, size) in zip(driver(lines), sizes):
        assert g["rc"] == OK and g["out_bound"] >= size, (name, algo, p, g["out_bound"], size)


# ── layout invariants on a mixed batch ──

LENS = (0, 15, 16, 2047, 2048, 2049, 300000)


def mixed_batch(aligned):
    pairs, r, v = [], 0, 0
    for i, n in enumerate(LENS):
        m = LENS[(i + 3) % len(LENS)]
        pairs.append((r, n, v, m))
        r += (n + 15) & ~15
        v += (m + 15) & ~15
        if not aligned and i == 2:
            r += 4
            v += 9
    return pairs


def check_spans(g, pairs, with_r):
    """two spans per pair (R then V; R only for the pairs in with_r), their
    CRCs at 2i and 2i + 1, segments of 64 KiB over the 16-byte padded range"""
    spans, segs = [], []
    for i, (r_off, r_len, v_off, v_len) in enumerate(pairs):
        for which, off, n in ((0, r_off, r_len), (1, v_off, v_len)):
            if which == 0 and i not in with_r:
                continue
            nseg = 0 if n < 8 else (((off + n + 15) & ~15) - (off & ~15) + 65535) // 65536
            spans.append([off, n, len(segs), nseg, which, 2 * i + which])
            segs += [[len(spans) - 1, j] for j in range(nseg)]
    assert g["spans"] == spans and g["segs"] == segs


@pytest.mark.parametrize("aligned", [True, False])
def test_layout_invariants(driver, aligned):
    pairs = mixed_batch(aligned)
    n = len(pairs)
    on, on_m, co, co_g = driver([geom(ONEPASS, pairs, q=1), geom(ONEPASS, pairs, q=1, members=1),
                                 geom(CORRECTING, pairs, q=1), geom(CORRECTING, pairs, q=1, lds=0)])
    for g in (on, on_m, co, co_g):
        assert g["rc"] == OK
        assert bool(g["aligned16"]) == aligned
        base = 0
        for x, d in zip(g["pp"], pairs):
            assert x["rec_base"] == base and x["rec_cap"] == d[3] // 16 + 1
            base += x["rec_cap"]
        assert g["total_rec"] == base
        assert g["v_total"] == sum(d[3] for d in pairs)
        assert (g["qmin"], g["qmax"]) == (min(x["q"] for x in g["pp"]), max(x["q"] for x in g["pp"]))
        assert g["table_bytes"] == 16 * g["qmax"]
        # the automatic pool (>= 1 GiB) holds 8 of these tables: a multiple of 8
        assert g["n_tables"] >= 8 and g["n_tables"] % 8 == 0
    # a pool of 5 tables: one per pair at most, no rounding; of 20: 8 (7 pairs, at least 8)
    five, twenty = driver([geom(ONEPASS, pairs, q=1, pool=5 * on["table_bytes"]),
                           geom(ONEPASS, pairs, q=1, pool=20 * on["table_bytes"])])
    assert five["n_tables"] == 5 and twenty["n_tables"] == 8

    # member mode: only over 16-byte aligned pairs
    assert not on["members"] and bool(on_m["members"]) == aligned
    assert on["route_min"] == 2 and on_m["route_min"] == 0
    if aligned:
        chunks, slots, jobs = 0, 0, []
        for i, (x, d) in enumerate(zip(on_m["pp"], pairs)):
            nch = min(d[1], d[3]) // 2048 + 1
            assert (x["n_chunks"], x["chunk_base"], x["mem_base"]) == (nch, chunks, slots)
            jobs += [w for c in range(nch) for w in (i, c)]
            chunks += nch
            slots += nch * (2048 // 16 + 1)
        assert (on_m["n_chunks"], on_m["mem_slots"], on_m["jobs"]) == (chunks, slots, jobs)
    else:
        assert on_m["n_chunks"] == 0 and on_m["jobs"] == []

    # CRC spans: onepass and an all-global correcting plan hash every R and V
    # on the side stream; a fused correcting plan only the R's it cannot build in LDS
    for g in (on, on_m, co_g):
        check_spans(g, pairs, set(range(n)))
    cap = (65536 - (2048 + 10240 + 128 + 256)) // 4
    assert co["corr_lds_cap"] == cap and co["crc_fused"] and not co_g["crc_fused"]
    big = [i for i, x in enumerate(co["pp"]) if x["q"] > cap]
    assert big == [LENS.index(300000)] and co["gpairs"] == big
    assert co_g["gpairs"] == list(range(n))
    check_spans(co, pairs, set(big))
    base = 0
    for x in co["pp"]:
        assert x["tab_base"] == base
        base += x["q"]
    assert co["ctab_entries"] == base


def test_error_exits(driver):
    got = driver([one(ONEPASS, (1 << 32) - (1 << 20)), one(ONEPASS, 16, (1 << 32) - (1 << 20)),
                  one(CORRECTING, 65536, q=(1 << 32) - 1, max_table=1 << 33),
                  one(CORRECTING, 65536, q=1 << 32, max_table=1 << 33),
                  one(ONEPASS, 100, p=0), one(ONEPASS, 100, p=65537),
                  one(ONEPASS, 100, flags=1 << 1), one(CORRECTING, 100, buf_cap=4096),
                  one(CORRECTING, 100, buf_cap=4095), one(ONEPASS, 100, p=65536), one(0, 100, flags=1 << 1)])
    assert [g["rc"] for g in got] == [TOO_LARGE, TOO_LARGE, TOO_LARGE, TOO_LARGE, INVALID_ARG, INVALID_ARG,
                                      UNSUPPORTED, UNSUPPORTED, OK, OK, OK]
    assert got[0]["err"] == "pair 0: buffers of 4 GiB or more do not fit the u32 format"
    assert got[2]["err"].startswith("table size ") and got[2]["err"].endswith(" too large")
    assert got[4]["err"] == "--seed-len must be >= 1"
    assert got[5]["err"] == "--seed-len above 65536 is not supported"
    assert got[6]["err"] == "--splay is not supported (hash-table path only)"
    assert got[7]["err"] == "--buffer-size above 4095 is not supported (LDS lookback ring)"


# ── CRC tables, tied to the oracle's CRC ──

class Crc:
    def __init__(self, d):
        self.d = d
        self.tab = [int(w, 16) for w in d["tab"]]
        self.xinv = [int(w, 16) for w in d["xinv"]]
        self.k32 = [int(w, 16) for w in d["k32"]]
        self.kseg = int(d["kseg"], 16)
        T = self.tab
        # Z: one zero byte through the raw register, by tab[0..255]; as a
        # linear map, the images of the 64 register bits
        self.z1 = [((1 << i) >> 8) ^ T[(1 << i) & 0xff] for i in range(64)]
        self._pow = {}

    @staticmethod
    def apply(cols, z):
        r, i = 0, 0
        while z:
            if z & 1:
                r ^= cols[i]
            z >>= 1
            i += 1
        return r

    def zn(self, n):
        """the map Z^n (square and multiply on the 64 columns)"""
        if n not in self._pow:
            res, base, e = [1 << i for i in range(64)], self.z1, n
            while e:
                if e & 1:
                    res = [self.apply(base, c) for c in res]
                base = [self.apply(base, c) for c in base]
                e >>= 1
            self._pow[n] = res
        return self._pow[n]

    def Z(self, n, z):
        return self.apply(self.zn(n), z)

    def nib(self, first, z):
        """the product the kernels form from a nibble table: 16 look-ups of z"""
        r = 0
        for j in range(16):
            r ^= self.tab[first + 16 * j + ((z >> (4 * j)) & 15)]
        return r

    def crc64(self, data):
        T, c, i = self.tab, M64, 0
        while len(data) - i >= 8:
            w = int.from_bytes(data[i:i + 8], "little") ^ c
            c = 0
            for k in range(8):
                c ^= T[(7 - k) * 256 + ((w >> (8 * k)) & 0xff)]
            i += 8
        for b in data[i:]:
            c = (c >> 8) ^ T[(c ^ b) & 0xff]
        return (c ^ M64).to_bytes(8, "big")


@pytest.fixture(scope="module")
def crc(driver):
    return Crc(driver(["crc"])[0])


ZS = [X0, 1, 0x0123456789ABCDEF, 0xFEDCBA9876543210, M64, 0x8000000000000001]


def test_crc_slice_tables_compute_crc64_xz(crc, orc):
    assert len(crc.tab) == crc.d["tab_words"]
    for data in (b"", b"123456789", random.Random(11).randbytes(1024), random.Random(12).randbytes(1021)):
        assert crc.crc64(data) == orc.crc64_xz(data)
    # the register step really is the byte table (the basis of every identity below)
    r = z = 0x0123456789ABCDEF
    for _ in range(3):
        r = (r >> 8) ^ crc.tab[r & 0xff]
    assert crc.Z(3, z) == r


def test_crc_nibble_tables_multiply(crc):
    d = crc.d
    first = lambda c: 8 * 256 + c * d["nib_words"]
    for lv in range(d["levels"]):
        for z in ZS:
            assert crc.nib(first(lv), z) == crc.Z(1024 << lv, z)
    fin = lambda c: first(d["levels"] + c)
    seg = d["seg_bytes"]
    shifts = {0: seg, 17: 2 * seg, 18: 3 * seg, 19: 4 * seg, d["fin_x256"]: 256, d["fin_x512"]: 512,
              d["fin_x48k"]: 48 * 1024}
    assert len(shifts) + 16 == d["fin_tabs"]
    for c, n in shifts.items():
        for z in ZS:
            assert crc.nib(fin(c), z) == crc.Z(n, z)
    assert crc.kseg == crc.Z(seg, X0)
    # the pad inverses invert: Z^t of the product with x^(-8t) gives z back
    for t in range(16):
        assert crc.nib(fin(1 + t), X0) == crc.xinv[t]
        for z in ZS:
            assert crc.Z(t, crc.nib(fin(1 + t), z)) == z


def test_crc_row_tables(crc):
    d, T = crc.d, crc.tab
    for base, pb in ((d["rows16"], 16), (d["rows8"], 8)):
        for j in range(pb):
            cols = crc.zn(64 * pb - 1 - j)
            for i in (0, 1, 2, 0x55, 0x80, 0xff):
                assert T[base + 256 * j + i] == crc.apply(cols, T[i])
            assert all(T[base + 256 * j + i] == crc.apply(cols, T[i]) for i in range(0, 256, 7))
    for base, pb in ((d["rowk16"], 16), (d["rowk8"], 8)):
        for l in range(64):
            assert crc.Z(pb * l, T[base + l]) == X0
    for base, n in ((d["r5_8"], 512), (d["r5_16"], 1024), (d["r5_16"] + 32 * 13, 1016)):
        cols = crc.zn(n)
        for k in range(13):
            for v in range(32):
                assert T[base + 32 * k + v] == crc.apply(cols, (v << (5 * k)) & M64)
    assert d["r5_16"] + 32 * 26 == d["tab_words"]


def test_crc_k32_and_unpad(crc, driver):
    step = crc.zn(32)
    assert crc.k32[0] == X0
    for t in range(1, 1024):
        assert crc.k32[t] == crc.apply(step, crc.k32[t - 1])
    assert crc.k32[1023] == crc.Z(32 * 1023, X0)
    lens = (1, 32767, 32768, 100000)
    got = driver([one(CORRECTING, n, 100, q=1) for n in lens])
    for g, n in zip(got, lens):
        assert g["crc_fused"]
        assert crc.Z(-n % 32768, g["pp"][0]["crc_unpad"]) == X0


# ── --verbose over the golden deltas and their truncations ──

def test_verbose_report_is_memory_safe(driver):
    cases = [c for c in json.load(open(os.path.join(HERE, "golden", "golden.json")))["cases"]
             if "delta_hex" in c and len(c["delta_hex"]) < 40000]
    assert len(cases) > 50
    by_size = sorted(cases, key=lambda c: len(c["delta_hex"]))
    # every truncation of the largest onepass and correcting deltas and of a short one
    cut = [next(c for c in reversed(by_size) if c["algo"] == a) for a in (ONEPASS, CORRECTING)]
    cut.append(next(c for c in by_size if len(c["delta_hex"]) > 2 * 60))
    lines = ["verbose %d %d 0 %d %d %d %s" % (c["algo"], c["p"], c["r_len"], c["v_len"], t, c["delta_hex"])
             for cs, t in ((cases, 0), (cut, 1)) for c in cs]
    assert all(g["ok"] == 1 for g in driver(lines))
