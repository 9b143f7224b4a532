"""CPU: named CRWI graphs (tests/inplace_graphs.py) through the host converter
and through the serial core the device converter shares.

* dg_make_inplace equals tests/golden/golden_inplace_graphs.json, minted from
  the reference's `delta inplace`, for every graph and both policies; where
  oracle/_ref/delta exists the reference is also run directly.
* The graphs mean what their names say (stats of the conversion).
* dg_inplace_core.h (neighbour ranges, Tarjan, the resumable cycle search, the
  stall policy) with lane width 1, compiled with g++ -fsanitize=address,
  undefined into a stand-alone program together with dg_inplace.cpp and
  dg_format.cpp (no HIP, nothing loaded into Python), prints the same bytes as
  dg_make_inplace over the same graphs and 200 random ones, over the seam
  graphs (2047..2049 and 65535..65537 copies, three radix passes with victims)
  and over the accepted streams of the high-offset corpus
  (tests/high_offset_cases.py), whose R of 4 GiB is a sparse record.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import struct
import subprocess

import pytest

import high_offset_cases as hc
import sparse_model as sm
from inplace_graphs import POLICIES, SEAM_SIZES, build, named_graphs, seam_graphs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "delta-compression_amd", "csrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "delta")
GOLD = {(c["name"], c["policy"]): c
        for c in json.load(open(os.path.join(HERE, "golden", "golden_inplace_graphs.json")))["cases"]}
SEAM_GOLD = {(c["name"], c["policy"]): c
             for c in json.load(open(os.path.join(HERE, "golden", "golden_inplace_seams.json")))["cases"]}
GRAPHS = named_graphs()
SEAMS = seam_graphs()


@pytest.fixture(scope="module")
def built(dg, orc):
    return {name: (R, *build(dg, orc, R, cmds)) for name, _, R, cmds in GRAPHS}


@pytest.fixture(scope="module")
def built_seams(dg, orc):
    return {name: (R, *build(dg, orc, R, cmds)) for name, _, R, cmds in SEAMS}


def test_goldens_cover_every_graph():
    assert set(GOLD) == {(name, pol) for name, _, _, _ in GRAPHS for pol in POLICIES}
    assert set(SEAM_GOLD) == {(name, pol) for name, _, _, _ in SEAMS for pol in POLICIES}
    assert [name for name, *_ in SEAMS] == [f"perm_{n}" for n in SEAM_SIZES] + ["radix_edges"]
    assert SEAM_SIZES == (2047, 2048, 2049, 65535, 65536, 65537)   # kLdsWords = 2048 copies, and 2048 words of 32 ready bits
    for gold, graphs in ((GOLD, GRAPHS), (SEAM_GOLD, SEAMS)):
        for name, params, R, _ in graphs:
            for pol in POLICIES:
                assert gold[(name, pol)]["params"] == params
                assert gold[(name, pol)]["r_sha256"] == hashlib.sha256(R).hexdigest()


@pytest.mark.parametrize("name", [g[0] for g in SEAMS])
def test_host_converter_equals_reference_golden_at_the_seams(dg, built_seams, name):
    R, std, V = built_seams[name]
    n_copies = sum(c[0] == "copy" for c in next(g[3] for g in SEAMS if g[0] == name))
    for pol in POLICIES:
        c = SEAM_GOLD[(name, pol)]
        assert c["std_sha256"] == hashlib.sha256(std).hexdigest()
        got, stats = dg.make_inplace(R, std, pol, stats=True)
        assert len(got) == c["len"] and hashlib.sha256(got).hexdigest() == c["sha256"]
        assert dg.info(got)["version_size"] == len(V) == c["v_len"]
        assert stats["num_adds"] > 0 and stats["num_copies"] + stats["num_adds"] == n_copies   # cycles: the Kahn path
    if name == "radix_edges":   # lengths on both sides of 2^8 and 2^16 among the kept copies and among the victims
        cmds = sm.Stream(dg.make_inplace(R, std, "localmin")).cmds
        for kind in (1, 2):
            lens = [n for k, _, _, n in cmds if k == kind]
            assert min(lens) < 256 and max(lens) >= 65535, kind


@pytest.mark.parametrize("name", [g[0] for g in GRAPHS])
def test_host_converter_equals_reference_golden(dg, built, name):
    R, std, V = built[name]
    for pol in POLICIES:
        c = GOLD[(name, pol)]
        assert c["std_sha256"] == hashlib.sha256(std).hexdigest()
        got = dg.make_inplace(R, std, pol)
        assert len(got) == c["len"] and hashlib.sha256(got).hexdigest() == c["sha256"]
        if "hex" in c:
            assert got == bytes.fromhex(c["hex"])
        assert dg.info(got)["version_size"] == len(V) == c["v_len"]


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="oracle/_ref/delta not built")
def test_host_converter_equals_reference_cli(dg, built, tmp_path):
    for name, (R, std, _) in built.items():
        (tmp_path / "r").write_bytes(R)
        (tmp_path / "d").write_bytes(std)
        for pol in POLICIES:
            subprocess.run([REF_CLI, "inplace", str(tmp_path / "r"), str(tmp_path / "d"), str(tmp_path / "o"),
                            "--policy", pol], check=True, capture_output=True)
            assert dg.make_inplace(R, std, pol) == (tmp_path / "o").read_bytes(), (name, pol)


def test_graphs_mean_what_they_say(dg, built):
    def conv(name, pol):
        R, std, _ = built[name]
        return dg.make_inplace(R, std, pol, stats=True)

    n_adds = {name: sum(c[0] == "add" for c in cmds) for name, _, _, cmds in GRAPHS}
    victims = lambda name, pol: conv(name, pol)[1]["num_adds"] - n_adds[name]   # noqa: E731
    assert conv("swap_unequal", "localmin")[0] != conv("swap_unequal", "constant")[0]
    assert victims("wide_fan", "localmin") > 100
    assert victims("reverse_8", "localmin") > 1 and victims("reverse_8", "constant") > 1
    for name in ("identity_copy", "pred_touch", "hi_touch", "self_overlap", "empty", "adds_only"):
        assert victims(name, "localmin") == 0 == victims(name, "constant"), name   # acyclic
    for name in ("rotate_3", "rotate_8", "swap_equal"):
        assert victims(name, "localmin") == 1 == victims(name, "constant"), name
    # sources first: the victims' conversion order differs between the policies
    assert conv("two_sccs_linked", "localmin")[0] != conv("two_sccs_linked", "constant")[0]
    assert conv("figure_eight", "localmin")[0] != conv("figure_eight", "constant")[0]


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="oracle/_ref/delta not built")
def test_host_converter_equals_reference_cli_at_the_seams(dg, built_seams, tmp_path):
    for name, (R, std, _) in built_seams.items():
        (tmp_path / "r").write_bytes(R)
        (tmp_path / "d").write_bytes(std)
        for pol in POLICIES:
            subprocess.run([REF_CLI, "inplace", str(tmp_path / "r"), str(tmp_path / "d"), str(tmp_path / "o"),
                            "--policy", pol], check=True, capture_output=True)
            assert dg.make_inplace(R, std, pol) == (tmp_path / "o").read_bytes(), (name, pol)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_shared_core_under_asan_ubsan(built, built_seams, tmp_path):
    exe = tmp_path / "inplace_core_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "sanitize", "inplace_core_driver.cpp"),
           os.path.join(CSRC, "dg_format.cpp"), os.path.join(CSRC, "dg_inplace.cpp"),
           "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    corpus, runs = bytearray(), 0
    for R, std, _ in list(built.values()) + list(built_seams.values()):
        corpus += struct.pack("<II", 0, len(R)) + R + struct.pack("<I", len(std)) + std + struct.pack("<I", 3)
        runs += 2
    # the high-offset corpus: a sparse R, and each stream under the policies whose list accepts it
    for name, ref_len, d, sts in hc.corpus()["inplace"]:
        mask = sum(1 << p for p, pol in enumerate(POLICIES) if sts.get(pol) == hc.OK)
        if mask:
            ws = hc.R.head(ref_len).windows()
            corpus += struct.pack("<IQI", 1, ref_len, len(ws)) + b"".join(struct.pack("<QI", o, len(b)) + b for o, b in ws)
            corpus += struct.pack("<I", len(d)) + d + struct.pack("<I", mask)
            runs += bin(mask).count("1")
    assert runs == 2 * (len(built) + len(built_seams)) + 92
    (tmp_path / "corpus.bin").write_bytes(bytes(corpus))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), "200"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"checked {runs + 2 * 200} failures 0" in p.stdout
