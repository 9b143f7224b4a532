"""CPU: dg_compose under ASan + UBSan, in a stand-alone program.

tests/sanitize/compose_check.cpp drives the host composer over the builders'
corpus (tests/compose_cases.py), over truncations of it at every length and
over single-byte damage.  It is compiled here together with dg_compose.cpp and
dg_format.cpp, with the sanitizers' static runtimes, and run as its own process
with the environment as it is.
"""
from __future__ import annotations

import os
import shutil
import struct
import subprocess

import pytest

import compose_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "delta-compression_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_compose_under_sanitizers(dg, orc, tmp_path):
    corpus = tmp_path / "corpus.bin"
    cases = cc.all_cases(dg, orc)
    _, bad = cc.damaged(dg, orc)
    with open(corpus, "wb") as f:
        for a, b in [(c[4], c[5]) for c in cases] + [(x[1], x[2]) for x in bad]:
            f.write(struct.pack("<I", len(a)) + a + struct.pack("<I", len(b)) + b)
    exe = tmp_path / "compose_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           os.path.join(HERE, "sanitize", "compose_check.cpp"),
           os.path.join(CSRC, "dg_compose.cpp"), os.path.join(CSRC, "dg_format.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-4000:]
    words = p.stdout.split()
    got = dict(zip(words[0::2], map(int, words[1::2])))
    assert got["pairs"] == len(cases) + len(bad)
    assert got["corpus_failures"] == len(bad)   # every built case composes, every damaged one is refused
    assert got["ok"] > len(cases) and got["failed"] > 10 * len(cases)
