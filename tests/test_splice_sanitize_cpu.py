"""CPU: dg_splice and dg_segment_pairs under ASan + UBSan, in a stand-alone program.

tests/sanitize/splice_check.cpp drives the host splice over the corpus of
tests/splice_cases.py and its damaged groups, and over every segment stream cut
at every length up to 64 bytes.  It is compiled here together with
dg_splice.cpp, dg_plan.cpp and dg_format.cpp, with the sanitizers' static
runtimes, and run as its own process with the environment as it is.  Its digest
of the uncut cases must be the model's.
"""
from __future__ import annotations

import os
import shutil
import struct
import subprocess

import pytest

import splice_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "delta-compression_amd", "csrc")
SRC_CRC = bytes(range(1, 9))   # what splice_check.cpp passes

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _fnv(h, data):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_splice_under_sanitizers(dg, orc, tmp_path):
    cases = sc.all_cases(dg, orc)
    (R, V, whole, segs, good), bad = sc.damaged(dg, orc)
    items = [(c[3], c[4], c[5], None, 0, sc.model_splice(dg, orc, c[4], c[5], c[3], SRC_CRC, c[2])) for c in cases]
    items += [(whole, sg, ds, st, code, b"") for _, sg, ds, st, code in bad]
    corpus = tmp_path / "corpus.bin"
    want, cuts = 0xcbf29ce484222325, 0
    with open(corpus, "wb") as f:
        for wh, sg, ds, st, code, exp in items:
            f.write(struct.pack("<4QI", *wh, len(sg)))
            for j, (s, d) in enumerate(zip(sg, ds)):
                f.write(struct.pack("<4QiI", *s, st[j] if st else 0, len(d)) + d)
                cuts += min(64, len(d))
            want = _fnv(want, bytes([code]) + exp)
    exe = tmp_path / "splice_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           os.path.join(HERE, "sanitize", "splice_check.cpp"), os.path.join(CSRC, "dg_splice.cpp"),
           os.path.join(CSRC, "dg_plan.cpp"), os.path.join(CSRC, "dg_format.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-4000:]
    words = p.stdout.split()
    got = dict(zip(words[0::2], map(int, words[1::2])))
    assert got["cases"] == len(items)
    assert got["ok"] + got["failed"] == len(items) + cuts
    assert got["failed"] > 25 * len(items)   # the cut streams
    assert got["segments"] > 0
    assert got["digest"] == want
