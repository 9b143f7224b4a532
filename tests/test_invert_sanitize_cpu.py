"""CPU: dg_invert under ASan + UBSan, in a stand-alone program.

tests/sanitize/invert_check.cpp drives the host inverter over the builders'
corpus (tests/invert_cases.py), over truncations of it at every length and over
single-byte damage.  It is compiled here together with dg_invert.cpp and
dg_format.cpp, with the sanitizers' static runtimes, and run as its own process
with the environment as it is.
"""
from __future__ import annotations

import os
import shutil
import struct
import subprocess

import pytest

import invert_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "delta-compression_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_invert_under_sanitizers(dg, orc, tmp_path):
    corpus = tmp_path / "corpus.bin"
    cases = ic.all_cases(dg, orc)
    (R, _, _), bad = ic.damaged(dg, orc)
    with open(corpus, "wb") as f:
        for r, a in [(c[1], c[3]) for c in cases] + [(R, x[1]) for x in bad]:
            f.write(struct.pack("<I", len(r)) + r + struct.pack("<I", len(a)) + a)
    exe = tmp_path / "invert_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           os.path.join(HERE, "sanitize", "invert_check.cpp"),
           os.path.join(CSRC, "dg_invert.cpp"), os.path.join(CSRC, "dg_format.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-4000:]
    words = p.stdout.split()
    got = dict(zip(words[0::2], map(int, words[1::2])))
    assert got["cases"] == len(cases) + len(bad)
    assert got["corpus_failures"] == len(bad)   # every built case inverts, every damaged one is refused
    assert got["ok"] > len(cases) and got["failed"] > 10 * len(cases)
