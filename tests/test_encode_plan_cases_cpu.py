"""The inputs of tests/test_gpu_encode_plan.py do what they claim (no GPU).

Every pair of tests/encode_plan_cases.py is encoded by the oracle with the
options the GPU test uses and parsed with the host-only decode_delta; the shapes
the GPU test relies on (record counts on the tile boundaries, the ADD payload
classes, chunks with more members than one tile, tiles over the stages, the
chunk edges) are asserted on the parsed commands.  These are conditions on the
inputs: a generator that stops producing a shape fails here and does not thin
out the GPU test silently.
"""
from __future__ import annotations

import collections

import pytest

import encode_plan_cases as C

ONEPASS, CORRECTING = 1, 2
OPTIONS = [(ONEPASS, 1), (ONEPASS, 257), (ONEPASS, 1048573), (CORRECTING, 1)]
ONEPASS_OPTIONS = OPTIONS[:3]


def _id(o):
    return ("onepass" if o[0] == ONEPASS else "correcting") + f"_q{o[1]}"


def plan_pair_bound(algo, v_len, p=C.P):
    """The plan's per-pair share of output_bound (dg_plan.cpp pair_out_bound)."""
    if algo == CORRECTING:
        return 57 + v_len + 22 * (v_len // p)
    return 35 + v_len + (v_len // p) * max(0, 22 - p)


class Parsed:
    """One delta's commands as the serialisers see them: the COPY records
    (src, dst, length, gap = the ADD before it) and the trailing ADD."""

    def __init__(self, dg, delta, v_len):
        cmds, inplace, vs, _, _ = dg.decode_delta(delta)
        assert not inplace and vs == v_len
        self.records, self.tail, at = [], 0, 0
        gap = 0
        for c in cmds:
            assert c.dst == at, "commands in V order, without holes"
            if isinstance(c, dg.PlacedAdd):
                assert gap == 0
                gap = len(c.data)
                at += gap
            else:
                self.records.append((c.src, c.dst, c.length, gap))
                gap = 0
                at += c.length
        self.tail = gap
        assert at == v_len

    @property
    def n(self):
        return len(self.records)

    @property
    def gaps(self):
        return [r[3] for r in self.records if r[3]]

    def plain_tiles(self):
        """Bytes of each tile of 64 records of the plain serialiser (serialize_run)."""
        sz = [13 + (9 + g if g else 0) for _, _, _, g in self.records]
        return [sum(sz[k:k + 64]) for k in range(0, len(sz), 64)]

    def members(self):
        """chunk -> the diagonal COPYs (src == dst) that start in it, in order."""
        out = collections.defaultdict(list)
        for s, d, ln, g in self.records:
            if s == d:
                out[d // C.CHUNK].append((d, ln, g))
        return out

    def member_tiles(self):
        """Bytes of each chunk's tiles of 64 members (member_serialize_pipe)."""
        out = []
        for ms in self.members().values():
            sz = [13 + (9 + g if g else 0) for _, _, g in ms]
            out += [sum(sz[k:k + 64]) for k in range(0, len(sz), 64)]
        return out


_PARSED = {}


@pytest.fixture(scope="module")
def parsed(dg, orc):
    def get(opt):
        if opt not in _PARSED:
            algo, q = opt
            _PARSED[opt] = {name: (Parsed(dg, orc.encode(algo, R, V, p=C.P, q=q), len(V)), R, V)
                            for name, R, V in C.small_layout_cases()}
        return _PARSED[opt]
    return get


def test_sizes_and_names():
    cases = C.small_layout_cases()
    assert 35 <= len(cases) <= 64
    assert len({c[0] for c in cases}) == len(cases)
    assert all(len(R) <= C.MAX_LEN and len(V) <= C.MAX_LEN for _, R, V in cases)
    for align in (16, 1):
        lay = C.layout([(R, V) for _, R, V in cases], align)
        assert lay.r_size <= C.MAX_ARENA and lay.v_size <= C.MAX_ARENA


@pytest.mark.parametrize("opt", OPTIONS, ids=_id)
def test_every_delta_within_the_plan_bound(parsed, orc, opt):
    algo, q = opt
    closest = 0.0
    for name, R, V in C.small_layout_cases():
        d = orc.encode(algo, R, V, p=C.P, q=q)
        b = plan_pair_bound(algo, len(V))
        assert len(d) <= b, name
        closest = max(closest, len(d) / b)
    if algo == ONEPASS:   # command_dense: 23 delta bytes per 17 of V against the bound's 22 per 16
        p = parsed(opt)["command_dense"][0]
        assert p.n == 1000 and set(p.gaps) == {1} and all(r[2] == 16 for r in p.records)
        assert closest >= 0.98


@pytest.mark.parametrize("opt", ONEPASS_OPTIONS, ids=_id)
def test_stream_edges(parsed, opt):
    ps = parsed(opt)
    by = {name: (len(R), len(V)) for name, (p, R, V) in ps.items()}
    assert by["v_empty"][1] == 0 and by["v_empty"][0] > 0
    assert by["r_empty"] == (0, 100) and by["both_empty"] == (0, 0)
    assert 0 < by["v_lt5"][1] < 5 and 5 <= by["v_lt_p"][1] < C.P and by["v_eq_p"][1] == C.P
    assert by["r_longer"][0] > by["r_longer"][1] and by["v_longer"][0] < by["v_longer"][1]
    for name in ("v_empty", "r_empty", "both_empty", "v_lt5", "v_lt_p"):
        assert ps[name][0].n == 0
    assert ps["v_eq_p"][0].records == [(0, 0, 16, 0)]
    assert ps["r_longer"][0].n == 2 and ps["v_longer"][0].n == 2


@pytest.mark.parametrize("opt", ONEPASS_OPTIONS, ids=_id)
def test_chunk_edges(parsed, opt):
    """min(|R|, |V|) on and around the chunk and piece boundaries, with a
    diagonal COPY that ends at min(|R|, |V|): the last chunk's last member."""
    ps = parsed(opt)
    E = []
    for n in C.CHUNK_EDGE_LENGTHS:
        p, R, V = ps[f"edge_{n}"]
        e = min(len(R), len(V))
        assert e == n
        E.append(e)
        assert any(s == d and d + ln == e for s, d, ln, g in p.records), n
        assert set(p.members()) >= set(range(e // C.CHUNK))   # members start in every whole chunk
    assert {2032, 2047, 2048, 2049, 2064, 4095, 4096, 4097} <= set(E)
    assert sum(e % 16 != 0 for e in E) >= 5
    rel = [(len(ps[f"edge_{n}"][1]) > len(ps[f"edge_{n}"][2])) - (len(ps[f"edge_{n}"][1]) < len(ps[f"edge_{n}"][2]))
           for n in C.CHUNK_EDGE_LENGTHS]
    assert rel.count(1) >= 3 and rel.count(-1) >= 3 and rel.count(0) >= 3


@pytest.mark.parametrize("opt", ONEPASS_OPTIONS, ids=_id)
def test_record_counts(parsed, opt):
    ps = parsed(opt)
    assert ps["no_records"][0].n == 0 and ps["no_records"][0].tail == 7000
    for n in C.COPY_COUNTS:
        p = ps[f"copies_{n}"][0]
        assert p.n == n and all(s == d for s, d, _, _ in p.records)            # members, where members run
    for n in (63, 64, 65, 129):
        p = ps[f"copies_{n}_shift"][0]
        assert p.n == n and all(s != d for s, d, _, _ in p.records)            # plain records in every mode
    counts = {p.n for p, _, _ in ps.values()}
    assert {0, 1, 63, 64, 65, 128, 129} <= counts
    # the tile test's pairs: whatever the one-pass scan finds of their scattered pieces
    for name in ("records_64_mixed", "records_129", "direct_tiles", "all_direct"):
        assert ps[name][0].n >= 1, name


@pytest.mark.parametrize("opt", OPTIONS, ids=_id)
def test_plain_tiles_over_the_stage(parsed, opt):
    """A tile of the plain serialiser over its 4096-byte stage is written unstaged."""
    ps = parsed(opt)
    for name in ("direct_tiles", "all_direct", "direct_tile_shift"):
        assert max(ps[name][0].plain_tiles()) > 4096, name
    if opt[0] == ONEPASS:
        p = ps["direct_tile_shift"][0]   # 64 records of 102 bytes, then a staged tile
        t = p.plain_tiles()
        assert p.n > 64 and t[0] > 4096 and 0 < t[1] <= 4096
        assert any(0 < max(q.plain_tiles(), default=0) <= 4096 and q.n > 64 for q, _, _ in ps.values())


def _classes(lengths):
    return {"1-4": sorted({g for g in lengths if 1 <= g <= 4}),
            "5-32": sorted({g for g in lengths if 5 <= g <= 32}),
            "33-255": sorted({g for g in lengths if 33 <= g <= 255}),
            "256+": sorted({g for g in lengths if g >= 256})}


@pytest.mark.parametrize("opt", OPTIONS, ids=_id)
def test_add_payload_classes(parsed, opt):
    ps = parsed(opt)
    gaps, tails, shifted = [], [], []
    for name, (p, R, V) in ps.items():
        gaps += p.gaps
        tails.append(p.tail)
        if name.endswith("_shift"):
            shifted += p.gaps
    g, t, s = _classes(gaps), _classes(tails), _classes(shifted)
    for cls in ("1-4", "5-32", "33-255", "256+"):
        assert g[cls] and t[cls] and s[cls], cls
    assert max(g["256+"]) > 512 and max(t["256+"]) > 512 and max(s["256+"]) > 512   # more than one pass of 256 bytes
    if opt[0] == ONEPASS:
        assert {1, 2, 3, 4} <= set(g["1-4"]) and {5, 32} <= set(g["5-32"]) and {33, 255} <= set(g["33-255"])
        assert {1, 4} <= set(t["1-4"]) and {5, 32} <= set(t["5-32"]) and {33, 255} <= set(t["33-255"])
        assert 256 in g["256+"] or 257 in g["256+"]
        # the same classes among the members' gaps (put_bulk: <= 4, < 16, <= 64, wave-wide)
        m = [x[2] for ms in ps["gaps_small"][0].members().values() for x in ms]
        m += [x[2] for ms in ps["gaps_large"][0].members().values() for x in ms]
        assert {1, 4} <= set(m) and max(m) > 1024
        assert any(5 <= x < 16 for x in m) and any(16 <= x <= 64 for x in m) and any(64 < x < 256 for x in m)


@pytest.mark.parametrize("opt", ONEPASS_OPTIONS, ids=_id)
def test_payload_window_crosses_the_end_of_v(parsed, opt):
    ps = parsed(opt)
    for name in ("window_5_16", "window_9_20", "window_15_16"):
        p, R, V = ps[name]
        s, d, ln, g = p.records[-1]
        assert d + ln == len(V) and p.tail == 0
        assert 5 <= g <= 32 and d >= len(V) - 32 and (d - g) + 32 > len(V), name


@pytest.mark.parametrize("opt", ONEPASS_OPTIONS, ids=_id)
def test_member_density(parsed, opt):
    ps = parsed(opt)
    most = {}
    for k in C.DENSE_K:
        p, R, V = ps[f"dense_{k}"]
        assert len(V) // C.CHUNK == 3
        most[k] = max(len(ms) for ms in p.members().values())
    assert all(most[k] >= 65 for k in (17, 20, 24, 31)), most   # a second tile of members
    assert most[17] >= 120                                        # near the 129 slots
    assert most[32] == 64 and most[33] in (62, 63), most          # and the counts at one full tile
    for name in ("alternating_18_30", "alternating_17_34"):
        p = ps[name][0]
        assert max(p.member_tiles()) > 2048, name                 # the member serialiser's unstaged tile
        assert max(len(ms) for ms in p.members().values()) <= 64
    assert max(ps["dense_17"][0].member_tiles()) <= 2048


def test_layouts():
    cases = [(R, V) for _, R, V in C.small_layout_cases()]
    for align in (16, 1):
        lay = C.layout(cases, align)
        r, v = C.arenas(lay, cases)
        assert len(r) == lay.lay[-1][0] + lay.lay[-1][1] and len(v) == lay.lay[-1][2] + lay.lay[-1][3]
        ends = [0, 0]
        for (ro, rl, vo, vl), (R, V) in zip(lay.lay, cases):
            assert r[ro:ro + rl] == R and v[vo:vo + vl] == V
            assert ro >= ends[0] and vo >= ends[1]
            ends = [ro + rl, vo + vl]
            if align == 16:
                assert ro % 16 == 0 and vo % 16 == 0
            else:
                assert ro % 2 == 1 and vo % 2 == 1


def test_datasets(dg, orc):
    small, auto = C.rerun_lengths(), C.auto_lengths()
    assert len(small) >= 12 and sum(a != b for a, b in small) >= 4
    assert {n for n in C.CHUNK_EDGE_LENGTHS} <= {min(a, b) for a, b in small}
    assert len(auto) == 8 and sum(v for _, v in auto) // 8 >= (128 << 10)
    ds = C.datasets(small, seed=1)
    assert set(ds) == set(C.DATASETS)
    for name, pairs in ds.items():
        assert [(len(R), len(V)) for R, V in pairs] == small
        # the unmatched stretch of more than 4096 bytes, then a match
        R, V = pairs[-1]
        for q in (1, 257, 1048573):
            p = Parsed(dg, orc.encode(ONEPASS, R, V, p=C.P, q=q), len(V))
            assert p.n >= 1 and p.records[0][3] > 4096, (name, q)
    # the densely edited pair: thousands of matches too short to be found from
    # another seed, in an index (q = 65537 < 2 x seeds) that is half full
    dense = small.index((C.DENSE_MIN, C.DENSE_MIN))
    assert 2 * (C.DENSE_MIN - C.P + 1) > 65537
    for name in ("edits", "shift"):
        R, V = ds[name][dense]
        p = Parsed(dg, orc.encode(CORRECTING, R, V, p=C.P, q=65537), len(V))
        assert sum(ln < C.DENSE_STEP for _, _, ln, _ in p.records) >= 1000, name
    assert ds["edits"] != ds["same"] and all(R != S for (R, _), (S, _) in zip(ds["edits"], ds["shift"]))
    # shift: the matches leave the diagonal; same and edits: they stay on it
    for name, diag in (("shift", False), ("same", True), ("edits", True)):
        R, V = ds[name][5]
        p = Parsed(dg, orc.encode(ONEPASS, R, V, p=C.P, q=1), len(V))
        assert p.n >= 1 and all((s == d) == diag for s, d, _, _ in p.records), name
    R, V = ds["unrelated"][5]
    assert Parsed(dg, orc.encode(ONEPASS, R, V, p=C.P, q=1), len(V)).n == 0
