"""CPU: the resemblance sketch and the base selection on the host (dg_sketch,
dg_sketch_match, csrc/dg_sketch.cpp), `delta pick`, and the sketch plan's work
list (sketch_plan_geometry, csrc/dg_plan.cpp), against the Python model of
tests/sketch_cases.py, which states the definition of include/delta_gpu.h in
plain integers.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

import sketch_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "delta-compression_amd", "csrc")
CLI = os.path.join(ROOT, "delta-compression_amd", "bin", "delta")

INVALID_ARG, TOO_LARGE = 1, 3
CHUNK = 16384   # dg_sketch_plan_chunk_bytes of this build (test_plan_geometry reads it back)

X512 = bytes(range(256)) * 2
KNOWN_P16_K16 = [
    0x00f5a4e541b4808b, 0x1053f43b7b2357d0, 0x2006400bac80ab1c, 0x306c3ccc939b6560,
    0x4168f46b76fbb901, 0x50080798295d5d68, 0x609f87c0d89e2a7d, 0x724a6e4f3a1899c5,
    0x84ccf1d00f6d14d5, 0x90018597505e716d, 0xa0aeb49b40f4dfbb, 0xb16186b26de3f9a1,
    0xc0c012a2fb0ee35d, 0xd06789287c29b00f, 0xe1810a7a3ac1357f, 0xf0cbf95857deb4db,
]


def test_model_fingerprints_match_the_oracle(orc):
    assert sc.check_fingerprints(orc) >= 300


def test_known_answers(dg):
    for f in (sc.sketch, dg.sketch):
        assert f(X512, 16, 16) == KNOWN_P16_K16
        s = f(X512, 4, 16)
        assert s[0] == 0x01498ab6281f1ac7 and s[15] == 0xf0850489bf42ee83 and sc.EMPTY not in s


def test_sketch_equals_model_over_the_sweep(dg):
    for p in sc.SEEDS:
        for name, buf in sc.sweep_buffers(p, CHUNK):
            for k in sc.BINS:
                assert dg.sketch(buf, p, k) == sc.sketch(buf, p, k), (p, k, name)


def test_sketch_properties(dg):
    p, k = 16, 256
    by = dict(sc.sweep_buffers(p, CHUNK))
    assert dg.sketch(by["random_15"], p, k) == [sc.EMPTY] * k   # n < p: every bin empty
    for name in ("zeros_%d" % (CHUNK + 1), "period1_65"):   # one distinct window: exactly one bin
        assert sum(w != sc.EMPTY for w in dg.sketch(by[name], p, k)) == 1, name
    assert sum(w != sc.EMPTY for w in dg.sketch(by["period256_300"], p, k)) <= 256
    # every byte offset is a feature: three bytes in front move nothing
    eq, us = sc.score(dg.sketch(by["base"], p, k), dg.sketch(by["shifted"], p, k))
    assert eq >= us - 3 and us == k
    assert dg.SKETCH_EMPTY == sc.EMPTY and dg.SKETCH_BINS == 256 and dg.SEED_LEN == 16


def test_match_equals_model(dg):
    for name, T, Cd, k, mode, base, min_equal in sc.match_cases():
        assert dg.match_sketches(T, Cd, k, mode, base, min_equal) == sc.select(T, Cd, mode, base, min_equal), name


def test_match_rules(dg):
    by = {c[0]: c for c in sc.match_cases()}
    run = lambda n: dg.match_sketches(*by[n][1:])
    assert run("duplicates_k256")[0][0] == 2                  # of equal candidates the smallest index
    assert run("tie_k16") == [(1, 1, 2)]                      # 1/2 first, 2/4 later: the earlier stays
    assert run("tie_swapped_k16") == [(1, 2, 4)]              # and the other way round
    assert run("tie_min2_k16") == [(3, 2, 4)]                 # min_equal 2 leaves only the 2/4
    assert run("nothing_k16") == [(dg.MATCH_NONE, 0, 0)] * 2
    assert run("first_of_set_k256") == [(dg.MATCH_NONE, 0, 0)]
    assert run("min5_k16") == [(dg.MATCH_NONE, 0, 0)]
    got = run("self_k16_mode2")                               # earlier: an acyclic assignment
    assert all(b == dg.MATCH_NONE or b < t for t, (b, _, _) in enumerate(got))
    got = run("window_k256_mode1")                            # not self, in a window at 40
    assert all(b != 40 + t for t, (b, _, _) in enumerate(got))
    assert [g[0] for g in run("self_k256_mode0")] == list(range(70))   # all: everything picks itself
    assert dg.match_sketches([], [[0] * 16], 16) == [] and dg.match_sketches([[0] * 16], [], 16) == [(dg.MATCH_NONE, 0, 0)]
    assert dg.match_sketches([[5] * 16], [[5] * 16], 16, mode="all") == [(0, 16, 16)]
    assert (dg.MATCH_ALL, dg.MATCH_NOT_SELF, dg.MATCH_EARLIER) == (sc.ALL, sc.NOT_SELF, sc.EARLIER)


def test_argument_errors(dg):
    import ctypes as C
    out = (C.c_uint64 * 2048)()
    data = (C.c_uint8 * 64)()
    for p, k in [(0, 256), (65, 256), (16, 0), (16, 8), (16, 2048), (16, 48), (16, 255)]:
        assert dg.lib.dg_sketch(data, 64, p, k, out) == INVALID_ARG, (p, k)
        with pytest.raises(dg.DeltaError):
            dg.sketch(b"x" * 64, p, k)
    assert dg.lib.dg_sketch(data, 64, 16, 256, None) == INVALID_ARG
    assert dg.lib.dg_sketch(None, 64, 16, 256, out) == INVALID_ARG
    assert dg.lib.dg_sketch(None, 0, 16, 256, out) == 0 and list(out[:256]) == [sc.EMPTY] * 256
    assert dg.lib.dg_sketch(data, 1 << 32, 16, 256, out) == TOO_LARGE   # refused before a byte is read
    assert dg.lib.dg_sketch(data, (1 << 32) - 1, 0, 256, out) == INVALID_ARG
    m = (dg._lib.Match * 1)()
    sk = (C.c_uint64 * 16)()
    ok = dict(n_t=1, n_c=1, k=16, mode=0, base=0, min_equal=1)
    for bad in [dict(k=8), dict(k=24), dict(k=2048), dict(mode=3), dict(mode=-1), dict(min_equal=0)]:
        a = {**ok, **bad}
        assert dg.lib.dg_sketch_match(sk, a["n_t"], sk, a["n_c"], a["k"], a["mode"], a["base"], a["min_equal"], m) == INVALID_ARG, bad
    assert dg.lib.dg_sketch_match(sk, 1, sk, 1, 16, 0, 0, 1, None) == INVALID_ARG
    assert dg.lib.dg_sketch_match(sk, 1, sk, 1, 16, 0, 0, 1, m) == 0
    with pytest.raises(ValueError):
        dg.match_sketches([], [], 16, mode="later")


# ── the plan's work list (dg_plan.cpp, no HIP), in a stand-alone program ──

@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_plan_geometry(tmp_path):
    exe = tmp_path / "sketch_geometry_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           os.path.join(HERE, "sanitize", "sketch_geometry_check.cpp"),
           os.path.join(CSRC, "dg_plan.cpp"), os.path.join(CSRC, "dg_format.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    for p in sc.SEEDS:
        _, spans = sc.pack([b for _, b in sc.sweep_buffers(p, CHUNK)], first=3)
        spans += [(7, 5 * CHUNK + 1), (0, 0)]
        arg = [str(p), "256"] + ["%d:%d" % s for s in spans]
        r = subprocess.run([str(exe)] + arg, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln.split() for ln in r.stdout.splitlines()]
        assert lines[0] == ["ok", str(CHUNK), str(64 - 8)]
        items = [(int(a), int(b)) for a, b in lines[1:]]
        assert items == sorted(items) and len(set(items)) == len(items)   # span by span, chunk by chunk
        # every window of every span belongs to exactly one chunk: chunk k holds the
        # window starts [k c, min((k + 1) c, windows)), and those ranges tile [0, windows)
        for i, (off, ln) in enumerate(spans):
            windows = max(ln - p + 1, 0)
            chunks = [k for s, k in items if s == i]
            assert chunks == list(range(-(-windows // CHUNK))), (p, i)
            covered = sum(min((k + 1) * CHUNK, windows) - k * CHUNK for k in chunks)
            assert covered == windows
            if chunks:   # the last window of the last chunk ends with the span, none reads past it
                last = min((chunks[-1] + 1) * CHUNK, windows) - 1
                assert last + p == ln
    for arg, want in [(["0", "256", "0:10"], INVALID_ARG), (["65", "256", "0:10"], INVALID_ARG),
                      (["16", "8", "0:10"], INVALID_ARG), (["16", "2048", "0:10"], INVALID_ARG),
                      (["16", "96", "0:10"], INVALID_ARG), (["16", "256", "0:%d" % (1 << 32)], TOO_LARGE),
                      (["16", "256", "%d:32" % ((1 << 64) - 16)], INVALID_ARG)]:
        r = subprocess.run([str(exe)] + arg, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.split()[:2] == ["fail", str(want)], (arg, r.stdout, r.stderr[-2000:])
    r = subprocess.run([str(exe), "16", "1024"], capture_output=True, text=True, timeout=60)   # no span: an empty plan
    assert r.stdout.split() == ["ok", str(CHUNK), str(64 - 10)]


# ── the CLI ──

def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True)


def test_cli_pick(dg, tmp_path):
    bases, versions = sc.family()
    paths = []
    for i, b in enumerate(bases[:4]):
        paths.append(tmp_path / ("base%d.bin" % i))
        paths[-1].write_bytes(b)
    pv = tmp_path / "version.bin"
    pv.write_bytes(versions[2])
    for opts, p, k in [((), 16, 256), (("--seed-len", "4", "--bins", "64"), 4, 64)]:
        r = run_cli("pick", *opts, str(pv), *map(str, paths))
        assert r.returncode == 0, r.stderr
        sv = sc.sketch(versions[2], p, k)
        want = ["%d/%d\t%s" % (*sc.score(sv, sc.sketch(b, p, k)), path) for b, path in zip(bases, paths)]
        assert r.stdout.splitlines() == want + ["best: %s" % paths[2]]
        assert int(want[2].split("/")[0]) > 0
    # nothing resembles: every candidate 0/used, no best
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    r = run_cli("pick", str(empty), str(paths[0]), str(empty))
    assert r.returncode == 0 and r.stdout.splitlines() == ["0/256\t%s" % paths[0], "0/0\t%s" % empty, "best: none"]
    r = run_cli("pick", str(pv), str(paths[0]), str(tmp_path / "missing.bin"))
    assert r.returncode == 1 and "missing.bin" in r.stderr
    for opts in [("--bins", "100"), ("--bins", "8"), ("--seed-len", "0"), ("--seed-len", "65"), ("--seed-len", "x"), ("--nope",)]:
        r = run_cli("pick", *opts, str(pv), str(paths[0]))
        assert r.returncode == 1 and r.stderr, opts
    assert run_cli("pick", str(pv)).returncode == 1
    assert "pick" in run_cli().stderr


def test_header_declares_and_library_exports(dg):
    names = ["dg_sketch", "dg_sketch_match", "dg_sketch_plan_create", "dg_sketch_plan_chunk_bytes", "dg_sketch_plan_run",
             "dg_sketch_plan_set_timing", "dg_sketch_plan_stage_times", "dg_sketch_plan_destroy",
             "dg_sketch_match_device", "dg_sketch_batch"]
    hdr = open(os.path.join(ROOT, "include", "delta_gpu.h")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, hdr), n
        assert hasattr(dg.lib, n), n
    assert "dg_match_t" in hdr and "dg_sketch_plan_t" in hdr and "O(n_t n_c K)" in hdr
    assert re.search(r"#define\s+DG_ABI_VERSION\s+3\b", hdr) and dg.lib.dg_abi_version() == 3
    assert {"SketchPlan", "sketch", "sketch_batch", "match_sketches", "pick_bases", "MATCH_ALL", "MATCH_NOT_SELF",
            "MATCH_EARLIER", "MATCH_NONE"} <= set(dg.__all__)
