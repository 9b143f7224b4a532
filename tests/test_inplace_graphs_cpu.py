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
  dg_make_inplace over the same graphs and 200 random ones.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import struct
import subprocess

import pytest

from inplace_graphs import POLICIES, build, named_graphs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "delta-compression_amd", "csrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "delta")
GOLD = {(c["name"], c["policy"]): c
        for c in json.load(open(os.path.join(HERE, "golden", "golden_inplace_graphs.json")))["cases"]}
GRAPHS = named_graphs()


@pytest.fixture(scope="module")
def built(dg, orc):
    return {name: (R, *build(dg, orc, R, cmds)) for name, _, R, cmds in GRAPHS}


def test_goldens_cover_every_graph():
    assert set(GOLD) == {(name, pol) for name, _, _, _ in GRAPHS for pol in POLICIES}
    for name, params, R, _ in GRAPHS:
        for pol in POLICIES:
            assert GOLD[(name, pol)]["params"] == params
            assert GOLD[(name, pol)]["r_sha256"] == hashlib.sha256(R).hexdigest()


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


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_shared_core_under_asan_ubsan(built, tmp_path):
    exe = tmp_path / "inplace_core_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "sanitize", "inplace_core_driver.cpp"),
           os.path.join(CSRC, "dg_format.cpp"), os.path.join(CSRC, "dg_inplace.cpp"),
           "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    corpus = bytearray()
    for R, std, _ in built.values():
        corpus += struct.pack("<I", len(R)) + R + struct.pack("<I", len(std)) + std
    (tmp_path / "corpus.bin").write_bytes(bytes(corpus))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), "200"], capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"checked {2 * (len(built) + 200)} failures 0" in p.stdout
