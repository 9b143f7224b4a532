"""CPU: dg_sketch and dg_sketch_match under ASan + UBSan, in a stand-alone program.

tests/sanitize/sketch_check.cpp drives the host functions over the sweep corpus
(tests/sketch_cases.py) at every (p, K) of the sweep, whole and cut short, and
matches the sketches against each other in every mode.  It is compiled here
together with dg_sketch.cpp, with the sanitizers' static runtimes, and run as
its own process with the environment as it is.
"""
from __future__ import annotations

import functools
import operator
import os
import shutil
import struct
import subprocess

import pytest

import sketch_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "delta-compression_amd", "csrc")
CHUNK = 16384

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_sketch_under_sanitizers(tmp_path):
    corpus = tmp_path / "corpus.bin"
    bufs = [b for _, b in sc.sweep_buffers(16, CHUNK)]
    with open(corpus, "wb") as f:
        for b in bufs:
            f.write(struct.pack("<I", len(b)) + b)
    exe = tmp_path / "sketch_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           os.path.join(HERE, "sanitize", "sketch_check.cpp"), os.path.join(CSRC, "dg_sketch.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-4000:]
    words = p.stdout.split()
    got = dict(zip(words[0::2], map(int, words[1::2])))
    combos = len(sc.SEEDS) * len(sc.BINS)
    assert got["buffers"] == len(bufs)
    assert got["sketches"] > 4 * combos * len(bufs)
    assert got["matches"] == combos * 6 * (len(bufs) - len(bufs) // 3)
    want = functools.reduce(operator.xor, (w for p_ in sc.SEEDS for k in sc.BINS for b in bufs for w in sc.sketch(b, p_, k)))
    assert got["digest"] == want
