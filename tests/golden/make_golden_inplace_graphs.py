#!/usr/bin/env python3
"""Regenerate tests/golden/golden_inplace_graphs.json from the REFERENCE itself.

For every named graph of tests/inplace_graphs.py and both cycle policies, the
crafted standard delta is converted by the reference's own CLI
(`oracle/_ref/delta inplace`, compiled from the reference's src/c by
oracle/Makefile).  Stored per case: the recipe parameters, the sha256 of R and
of the standard delta, and the length and sha256 of the reference's output,
plus its hex when under 4 KiB.  Run in the dev container:

    make -C oracle ref && python tests/golden/make_golden_inplace_graphs.py
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, TESTS)

import oracle as O  # noqa: E402
from conftest import load_product  # noqa: E402
from inplace_graphs import POLICIES, build, named_graphs  # noqa: E402

REF_CLI = os.path.join(ROOT, "oracle", "_ref", "delta")
INLINE_MAX = 4096


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def ref_inplace(R: bytes, std: bytes, policy: str, tmp: str) -> bytes:
    fr, fd, fo = (os.path.join(tmp, x) for x in ("r", "d", "o"))
    open(fr, "wb").write(R)
    open(fd, "wb").write(std)
    subprocess.run([REF_CLI, "inplace", fr, fd, fo, "--policy", policy], check=True, capture_output=True)
    return open(fo, "rb").read()


def main():
    dg = load_product()
    orc = O.Oracle()
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, params, R, cmds in named_graphs():
            std, V = build(dg, orc, R, cmds)
            for policy in POLICIES:
                out = ref_inplace(R, std, policy, tmp)
                e = {"name": name, "policy": policy, "params": params, "r_sha256": sha(R),
                     "std_sha256": sha(std), "v_len": len(V), "len": len(out), "sha256": sha(out)}
                if len(out) < INLINE_MAX:
                    e["hex"] = out.hex()
                cases.append(e)
    doc = {"generator": "reference src/c via oracle/_ref/delta inplace", "cases": cases}
    path = os.path.join(HERE, "golden_inplace_graphs.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
